// LDS-DMA (global_load_lds_dwordx4 with a scalar base) and the counted waits that go with it.
#pragma once
#include "common.hpp"

namespace shasta {

// One global_load_lds_dwordx4 of 16 bytes per lane: global base + voff -> LDS at lds_dst + 16 lane (M0 holds lds_dst).
// Why asm and not the builtin: hipcc only emits the 64-bit-VGPR-address form for the LDS-DMA builtin (two v_lshl_add_u64 per
// instruction: measured 2560 instead of 2048 cycles per tile at 64 rows in anchor_l1_mfma_kernel).  Here the uniform base stays in
// scalar registers (the tile advance is a scalar add) and the per-lane 32-bit offset goes into the instruction's VGPR-offset field.
//
// M0: the asm writes M0 and names it in its clobber list, but the compiler treats M0 as a reserved register - it does not honour
// that clobber and only warns (-Winline-asm, silenced here, nowhere else).  These helpers are therefore correct only as long as no
// compiler-generated instruction of the same kernel relies on M0 keeping a value across the call - e.g. the LDS-DMA builtin, whose M0
// setup the compiler may share between instructions.  Saving and restoring M0 here would add instructions to every DMA.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void lds_dma_x4(uint32_t voff, const char* base, uint32_t lds_dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(base), "s"(lds_dst) : "memory", "m0");
}
// the same, non-temporal: for streams read once (weights), so that what the following kernels read stays in L2 / Infinity Cache
__device__ __forceinline__ void lds_dma_x4_nt(uint32_t voff, const char* base, uint32_t lds_dst) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1 nt" ::"v"(voff), "s"(base), "s"(lds_dst) : "memory", "m0");
}
#pragma clang diagnostic pop

// wait until at most N vector-memory instructions of this wave are in flight (LDS-DMA counts like a load)
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// a pointer the compiler should keep in scalar registers (the base operand of lds_dma_x4)
__device__ __forceinline__ const char* uniform_ptr(const char* p) {
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return reinterpret_cast<const char*>(((uint64_t)hi << 32) | lo);
}

}  // namespace shasta
