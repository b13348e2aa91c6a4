// Index of a set of cells of a dense grid: a bitmap, prefix counts of its set bits, and the rank of a cell among the set ones in
// linear order.  Shared by sparse_conv.hip (the index of a level of the sparse backbone) and dynvox.hip (the sorted unique voxels of a
// point cloud).  Setting the bits is the caller's business (integer atomicOr); everything here only reads them, so the result depends on
// the set of cells alone, never on the order the bits were set in.
#pragma once
#include "common.hpp"

namespace shasta {

constexpr int SC_SCAN = 1024;    // bitmap words per scan block (256 threads x 4)

// Workspace of one index.  words: the bitmap rounded up to whole scan blocks (the tail stays zero).
struct SpIndex {
    uint32_t* bits;   // [words]
    uint32_t* pre;    // [words]  set bits before this word inside its scan block
    uint32_t* sums;   // [nblk + 1] set bits before this scan block; [nblk] = the level's row count
    int* perm;        // [rows]
    size_t words;
    int nblk;
    size_t bytes;
    SpIndex(void* ws, int B, int D, int H, int W, int rows) {
        const size_t cells = (size_t)B * D * H * W;
        words = align_up((cells + 31) / 32, SC_SCAN);
        nblk = (int)(words / SC_SCAN);
        char* p = static_cast<char*>(ws);
        size_t off = 0;
        bits = reinterpret_cast<uint32_t*>(p + off), off += align_up(words * 4, 256);
        pre = reinterpret_cast<uint32_t*>(p + off), off += align_up(words * 4, 256);
        sums = reinterpret_cast<uint32_t*>(p + off), off += align_up(((size_t)nblk + 1) * 4, 256);
        perm = reinterpret_cast<int*>(p + off), off += align_up((size_t)(rows > 0 ? rows : 1) * 4, 256);
        bytes = off;
    }
};

__device__ __forceinline__ int sp_rank(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ pre,
                                       const uint32_t* __restrict__ sums, int lin) {
    const int w = lin >> 5;
    const uint32_t word = bits[w], bit = 1u << (lin & 31);
    if (!(word & bit)) return -1;
    return (int)(sums[w / SC_SCAN] + pre[w] + __popc(word & (bit - 1)));
}

// exclusive scan of 256 values, one per thread of a 256-thread block; *total = their sum
__device__ __forceinline__ uint32_t sp_block_scan(uint32_t v, uint32_t* s_wave, uint32_t* total) {
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

static __global__ __launch_bounds__(256) void sp_scan_words_kernel(const uint32_t* __restrict__ bits, uint32_t* __restrict__ pre,
                                                                   uint32_t* __restrict__ sums) {
    __shared__ uint32_t s_wave[4];
    const size_t w0 = (size_t)blockIdx.x * SC_SCAN + 4 * threadIdx.x;
    const u32x4 v = *reinterpret_cast<const u32x4*>(bits + w0);
    const uint32_t c0 = __popc(v[0]), c1 = __popc(v[1]), c2 = __popc(v[2]), c3 = __popc(v[3]);
    uint32_t total;
    const uint32_t ex = sp_block_scan(c0 + c1 + c2 + c3, s_wave, &total);
    u32x4 o;
    o[0] = ex, o[1] = ex + c0, o[2] = ex + c0 + c1, o[3] = ex + c0 + c1 + c2;
    *reinterpret_cast<u32x4*>(pre + w0) = o;
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums[] -> its exclusive scan in place, sums[nblk] = the count (also to *count where given)
static __global__ __launch_bounds__(256) void sp_scan_sums_kernel(uint32_t* __restrict__ sums, int nblk, int* __restrict__ count) {
    __shared__ uint32_t s_wave[4];
    uint32_t carry = 0;
    for (int base = 0; base < nblk; base += 256) {
        const int j = base + threadIdx.x;
        const uint32_t v = j < nblk ? sums[j] : 0u;
        uint32_t total;
        const uint32_t ex = sp_block_scan(v, s_wave, &total);
        if (j < nblk) sums[j] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        sums[nblk] = carry;
        if (count) *count = (int)carry;
    }
}

static int sp_scan(const SpIndex& ix, int* count, hipStream_t st) {
    hipLaunchKernelGGL(sp_scan_words_kernel, dim3(ix.nblk), dim3(256), 0, st, ix.bits, ix.pre, ix.sums);
    hipLaunchKernelGGL(sp_scan_sums_kernel, dim3(1), dim3(256), 0, st, ix.sums, ix.nblk, count);
    return check_launch("spconv index scan");
}

}  // namespace shasta
