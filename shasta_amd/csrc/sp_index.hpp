// Index of a set of cells of a dense grid: a bitmap, prefix counts of its set bits, and the rank of a cell among the set ones in
// linear order.  Users: sparse_conv.hip (the index of a level of the sparse backbone) and dynvox.hip (the sorted unique voxels of a
// point cloud).  Setting the bits is the caller's business (integer atomicOr); everything here only reads them, so the result depends on
// the set of cells alone, never on the order the bits were set in.  The scans themselves are scan.hpp's (shared with the compactions
// of sweeps.hip, head.hip and voxelize.hip, which need no index).
#pragma once
#include "scan.hpp"

namespace shasta {

constexpr int SC_SCAN = SCAN_VALUES;  // bitmap words per scan block

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

// set cells below cell `lin` in linear order, given `word` = bits[lin >> 5]: the rank of `lin` if its bit is set
__device__ __forceinline__ int sp_rank_below(uint32_t word, const uint32_t* __restrict__ pre, const uint32_t* __restrict__ sums, int lin) {
    return (int)(scan_prefix(pre, sums, (size_t)(lin >> 5)) + __popc(word & ((1u << (lin & 31)) - 1u)));
}

// rank of cell `lin` among the set ones, -1 if its bit is not set
__device__ __forceinline__ int sp_rank(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ pre,
                                       const uint32_t* __restrict__ sums, int lin) {
    const uint32_t word = bits[lin >> 5];
    if (!((word >> (lin & 31)) & 1u)) return -1;
    return sp_rank_below(word, pre, sums, lin);
}

// one thread per bitmap word: the (b, z, y, x) of its set bits at their ranks; perm (where given) = identity.  Rows >= capacity are
// not written.
static __global__ void sp_index_emit_kernel(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ pre,
                                            const uint32_t* __restrict__ sums, size_t words, int D, int H, int W, int capacity,
                                            int* __restrict__ coords, int* __restrict__ perm) {
    const size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= words) return;
    uint32_t word = bits[w];
    if (!word) return;
    int rank = (int)scan_prefix(pre, sums, w);
    while (word && rank < capacity) {
        const int bit = __ffs(word) - 1;
        word &= word - 1;
        int lin = (int)(w * 32) + bit;
        const int x = lin % W;
        lin /= W;
        const int y = lin % H;
        lin /= H;
        const int z = lin % D, b = lin / D;
        int* c = coords + 4 * (size_t)rank;
        c[0] = b, c[1] = z, c[2] = y, c[3] = x;
        if (perm) perm[rank] = rank;
        ++rank;
    }
}

// bits -> pre, sums (sums[nblk] = the number of set cells, also to *count where given)
static int sp_scan(const SpIndex& ix, int* count, hipStream_t st) {
    hipLaunchKernelGGL(scan_blocks_kernel<true>, dim3(ix.nblk), dim3(256), 0, st, ix.bits, ix.pre, ix.sums);
    hipLaunchKernelGGL(scan_sums_kernel<true>, dim3(1), dim3(256), 0, st, ix.sums, ix.nblk, count);
    return check_launch("spconv index scan");
}

}  // namespace shasta
