// Exclusive scans and stable, atomic-free compaction for workgroups of 256 threads (four wavefronts): the one copy of what the
// voxelisers, the sparse index, the sweep assembly and the head decode share.  Everything here is integer arithmetic on flags and
// counts, so a result depends on the flags alone - never on timing - and is the same on every run.
//   compaction : count (block_place(...).count per block) -> scan of the block counts (scan_sums_kernel, or scan_with_carry in a kernel
//                of the caller's) -> write (the flag recomputed, place = the block's offset + block_place(...).place).
//   long scan  : scan_blocks_kernel (1024 values per workgroup: prefix inside the block + the block's total) -> scan_sums_kernel over
//                the totals; scan_prefix() reads the result.
// Every function that takes s_wave contains barriers: ALL 256 threads of the workgroup call it, in uniform control flow.
#pragma once
#include "common.hpp"

namespace shasta {

constexpr int SCAN_THREADS = 256;   // threads per workgroup of everything below
constexpr int SCAN_VALUES = 1024;   // values per workgroup of scan_blocks_kernel (256 threads x 4)

// exclusive scan of 256 values, one per thread of a 256-thread block; *total = their sum
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* s_wave, uint32_t* total) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    __syncthreads();  // (s_wave may still be read from the previous call)
    if (lane == 63) s_wave[wv] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int j = 0; j < wv; ++j) base += s_wave[j];
    *total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    return base + inc - v;
}

// The ballot step of a compaction.  place = kept elements of lower waves + of lower lanes of this wave (the element's rank among the
// block's kept ones, in thread order); count = the block's kept elements.  s_wave: four words of LDS.
// Barrier contract: exactly one __syncthreads(), after the write of s_wave - every thread of the block calls this, so a thread
// that has nothing to write returns AFTER the call, never before it; s_wave is not read or written by the caller, and a second call
// in one kernel needs a barrier of the caller's in between.
struct BlockPlace {
    int place, count;
};
__device__ __forceinline__ BlockPlace block_place(bool keep, int* s_wave) {
    const unsigned long long ballot = __ballot(keep);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) s_wave[wv] = __popcll(ballot);
    __syncthreads();
    BlockPlace r;
    r.place = __popcll(ballot & ((1ull << lane) - 1ull));
    for (int j = 0; j < wv; ++j) r.place += s_wave[j];
    r.count = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    return r;
}

// One workgroup scans in[0 .. n) in trips of 256 with a carry: emit(j, exclusive prefix of in[j]) for every j < n, by the thread that
// read in[j] (so emit may overwrite in[j]); returns the sum of all n values, in every thread.
template <typename Emit>
__device__ __forceinline__ uint32_t scan_with_carry(const uint32_t* in, int n, uint32_t* s_wave, Emit emit) {
    uint32_t carry = 0;
    for (int base = 0; base < n; base += SCAN_THREADS) {
        const int j = base + threadIdx.x;
        const uint32_t v = j < n ? in[j] : 0u;
        uint32_t total;
        const uint32_t ex = block_scan(v, s_wave, &total);
        if (j < n) emit(j, carry + ex);
        carry += total;
    }
    return carry;
}

// One workgroup per segment of nblk block sums (grid.x segments, back to back): the segment -> its exclusive scan in place.  The
// segment's total goes to count[segment] where count is given and, with TOTAL_PAST, to the word behind the segment (one segment only).
// (A template, as scan_blocks_kernel: only the files that launch it carry a copy.)
template <bool TOTAL_PAST>
static __global__ __launch_bounds__(256) void scan_sums_kernel(uint32_t* __restrict__ sums, int nblk, int32_t* __restrict__ count) {
    __shared__ uint32_t s_wave[4];
    uint32_t* c = sums + (size_t)blockIdx.x * nblk;
    const uint32_t total = scan_with_carry(c, nblk, s_wave, [c](int j, uint32_t ex) { c[j] = ex; });
    if (threadIdx.x == 0) {
        if (TOTAL_PAST) c[nblk] = total;
        if (count) count[blockIdx.x] = (int32_t)total;
    }
}

// Per block of 1024 values: pre[i] = sum of the block's values before i, sums[block] = the block's total.  The value of a word is its
// number of set bits (POPC: a bitmap) or the word itself.  The arrays are whole blocks long.
template <bool POPC>
static __global__ __launch_bounds__(256) void scan_blocks_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ pre,
                                                                 uint32_t* __restrict__ sums) {
    __shared__ uint32_t s_wave[4];
    const size_t w0 = (size_t)blockIdx.x * SCAN_VALUES + 4 * threadIdx.x;
    u32x4 v = *reinterpret_cast<const u32x4*>(in + w0);
    if (POPC) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = __popc(v[q]);
    }
    uint32_t total;
    const uint32_t ex = block_scan(v[0] + v[1] + v[2] + v[3], s_wave, &total);
    u32x4 o;
    o[0] = ex, o[1] = ex + v[0], o[2] = ex + v[0] + v[1], o[3] = ex + v[0] + v[1] + v[2];
    *reinterpret_cast<u32x4*>(pre + w0) = o;
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sum of the values before value i, after scan_blocks_kernel and scan_sums_kernel
__device__ __forceinline__ uint32_t scan_prefix(const uint32_t* __restrict__ pre, const uint32_t* __restrict__ sums, size_t i) {
    return sums[i / SCAN_VALUES] + pre[i];
}

}  // namespace shasta
