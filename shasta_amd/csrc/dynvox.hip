// Dynamic voxelisation (+ per-voxel mean of ALL points), bit-identical to the reference's reader on the CPU.
// Restates det3d/models/readers/dynamic_voxel_encoder.py:8-17 (voxelization) and :83-102 (the batch loop of DynamicVoxelEncoder.forward):
//   * a point is kept iff lo_j <= p_j <= hi_j on x, y, z (fp32 compares, both ends inclusive; NaN and +-inf drop out);
//   * its integer coordinate is trunc((p_j - lo_j) / vs_j), a true fp32 division; a point on an upper face gets coordinate == extent,
//     one past the grid, and the reference keeps that voxel - so does this file: the cell space of a cloud is
//     (gz + 1) x (gy + 1) x (gx + 1);
//   * the voxels of a cloud are the unique coordinates in lexicographic (z, y, x) order (torch.unique(dim=0) sorts), clouds in batch
//     order; there is no cap on the points of a voxel and none on the number of voxels;
//   * voxels[v] = (sum of the kept points of v, added one by one in ascending point index, starting from 0) / count.  That is what
//     scatter_mean computes on the CPU; a tree-shaped or atomic sum gives other bits.
// Parallel formulation (integer atomics only; every float is added in a fixed order -> the same bits on every run):
//   1. key   : lin = ((c (gz+1) + z)(gy+1) + y)(gx+1) + x per kept point, -1 per dropped one; bit `lin` of a bitmap of all clouds' cells
//              is set (atomicOr).  The linear order of that space IS the order of the output rows.
//   2. scan  : prefix counts of the set bits (sp_index.hpp, the index of the sparse backbone's levels); rank(lin) = the voxel's row.
//   3. emit  : every set bit writes its (cloud, z, y, x) at its rank; the ranks of the cells c * S give the per-cloud prefix of V.
//   4. count : row[i] = rank(lin_i); slot[i] = atomicAdd(cnt[row], 1) - the point's (arbitrary but unique) place in its voxel's list.
//   5. scan  : cnt -> segment starts.   6. fill: seg[start(row[i]) + slot[i]] = i.
//   7. sum   : a voxel of up to DV_THREAD_MAX points: one thread per (voxel, channel) walks the list in ascending order by selection
//              (next = the smallest index above the last one: n^2 / 2 cached loads, n is typically below 5).
//              A longer list goes onto a worklist; one wavefront per entry sorts the list (stable LSD radix sort on 8-bit digits,
//              O(n) per pass, ping-pong between seg and a second buffer) and then adds its points one by one, lanes = channels.
// No host read anywhere: every launch is sized by the number of points (an upper bound of V) and bounded by counts read on the device.
#include "common.hpp"
#include "sp_index.hpp"
#include <limits.h>
#include <math.h>

namespace shasta {

constexpr int DV_MAX_CLOUDS = 32;
constexpr int DV_THREAD_MAX = 32;    // longest list the thread-per-(voxel, channel) kernel sums itself
constexpr int DV_LONG_BLOCKS = 2048; // wavefronts that share the worklist of longer lists

struct DvGrid {
    float lo[3], hi[3], vs[3];
    int g[3];  // x, y, z extents as the reader's `shape` has them; coordinates run 0 .. g[j] inclusive
};

struct DvBatch {
    int n;
    int off[DV_MAX_CLOUDS + 1];  // first point of every cloud, relative to the first cloud (+ the total)
};

// Everything but the bitmap index; P points.
struct DvWs {
    SpIndex ix;
    int *row, *slot, *cnt, *nlong, *cpre, *seg, *tmp, *longlist;
    uint32_t* csum;
    size_t cnt_words;  // cnt rounded up to whole scan blocks
    int cblk;
    size_t zero_bytes;  // cnt and nlong lie back to back: one memset
    size_t bytes;
    DvWs(void* ws, int n, const DvGrid& G, long P) : ix(ws, n, G.g[2] + 1, G.g[1] + 1, G.g[0] + 1, 0) {
        const size_t p = P > 0 ? (size_t)P : 1;
        cnt_words = align_up(p, SC_SCAN);
        cblk = (int)(cnt_words / SC_SCAN);
        char* base = static_cast<char*>(ws);
        size_t off = ix.bytes;
        auto take = [&](size_t b) {
            char* q = base + off;
            off += align_up(b, 256);
            return q;
        };
        row = reinterpret_cast<int*>(take(p * 4));
        slot = reinterpret_cast<int*>(take(p * 4));
        cnt = reinterpret_cast<int*>(take(cnt_words * 4));
        nlong = reinterpret_cast<int*>(take(4));
        zero_bytes = (size_t)(reinterpret_cast<char*>(nlong) - reinterpret_cast<char*>(cnt)) + 4;
        cpre = reinterpret_cast<int*>(take(cnt_words * 4));
        csum = reinterpret_cast<uint32_t*>(take(((size_t)cblk + 1) * 4));
        seg = reinterpret_cast<int*>(take(p * 4));
        tmp = reinterpret_cast<int*>(take(p * 4));
        longlist = reinterpret_cast<int*>(take((p / (DV_THREAD_MAX + 1) + 1) * 4));
        bytes = off;
    }
};

static bool dv_shape_ok(int n, int gx, int gy, int gz) {
    return n >= 1 && n <= DV_MAX_CLOUDS && gx >= 1 && gy >= 1 && gz >= 1 &&
           (double)n * ((double)gz + 1) * ((double)gy + 1) * ((double)gx + 1) < 2147483648.0;
}

__global__ __launch_bounds__(256) void dv_key_kernel(const float* __restrict__ pts, DvBatch B, int ndim, DvGrid G,
                                                     int* __restrict__ keys, uint32_t* __restrict__ bits) {
    const long gi = (long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= B.off[B.n]) return;
    int c = 0;
    while (c + 1 < B.n && gi >= B.off[c + 1]) ++c;
    int cc[3];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float p = pts[(size_t)gi * ndim + j];
        ok = ok && p >= G.lo[j] && p <= G.hi[j];  // false for a NaN
        const float f = __fdiv_rn(__fsub_rn(p, G.lo[j]), G.vs[j]);
        cc[j] = ok ? (int)f : 0;
        ok = ok && cc[j] <= G.g[j];  // (holds for every kept point: the entry point checked the largest coordinate of the range)
    }
    int lin = -1;
    if (ok) {
        lin = ((c * (G.g[2] + 1) + cc[2]) * (G.g[1] + 1) + cc[1]) * (G.g[0] + 1) + cc[0];
        atomicOr(&bits[lin >> 5], 1u << (lin & 31));
    }
    keys[gi] = lin;
}

// num_voxels[c] = voxels of the clouds before c (the set bits below cell c * S), num_voxels[n] = V
__global__ void dv_prefix_kernel(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ pre, const uint32_t* __restrict__ sums,
                                 int n, int cells_per_cloud, int nblk, int* __restrict__ num_voxels) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n) return;
    if (c == n) {
        num_voxels[n] = (int)sums[nblk];
        return;
    }
    const int lin = c * cells_per_cloud;
    num_voxels[c] = sp_rank_below(bits[lin >> 5], pre, sums, lin);
}

// keys[i]: linear cell -> row of the voxel; slot[i] = the point's place in its voxel's list (arrival order: any permutation)
__global__ __launch_bounds__(256) void dv_count_kernel(int* __restrict__ keys, long P, const uint32_t* __restrict__ bits,
                                                       const uint32_t* __restrict__ pre, const uint32_t* __restrict__ sums,
                                                       int* __restrict__ slot, int* __restrict__ cnt) {
    const long gi = (long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= P) return;
    const int lin = keys[gi];
    if (lin < 0) return;
    const int r = sp_rank(bits, pre, sums, lin);  // (the bit is set: this point set it; r < V <= P)
    keys[gi] = r;
    if (r >= 0 && r < P) slot[gi] = atomicAdd(&cnt[r], 1);
}

// first entry of voxel v's list in seg: the points of the voxels before it (cnt scanned into cpre, csum by scan.hpp's two kernels)
__device__ __forceinline__ int dv_start(const int* __restrict__ cpre, const uint32_t* __restrict__ csum, int v) {
    return (int)scan_prefix(reinterpret_cast<const uint32_t*>(cpre), csum, (size_t)v);
}

__global__ __launch_bounds__(256) void dv_fill_kernel(const int* __restrict__ row, const int* __restrict__ slot, long P,
                                                      const int* __restrict__ cpre, const uint32_t* __restrict__ csum,
                                                      int* __restrict__ seg) {
    const long gi = (long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= P) return;
    const int r = row[gi];
    if (r < 0) return;
    const long at = (long)dv_start(cpre, csum, r) + slot[gi];
    if (at < P) seg[at] = (int)gi;  // (always: the lists of all voxels hold the kept points, once each)
}

// One thread per (voxel, channel).  Lists of up to DV_THREAD_MAX points are summed here, in ascending point index; longer ones are
// handed to dv_sum_long_kernel.  The lanes of a voxel read the same list words (one fetch) and consecutive floats of a point.
__global__ __launch_bounds__(256) void dv_sum_kernel(const float* __restrict__ pts, int ndim, const int* __restrict__ cnt,
                                                     const int* __restrict__ cpre, const uint32_t* __restrict__ csum,
                                                     const int* __restrict__ seg, const uint32_t* __restrict__ sums, int nblk, int capacity,
                                                     float* __restrict__ voxels, int* __restrict__ num_points, int* __restrict__ longlist,
                                                     int* __restrict__ nlong) {
    const long id = (long)blockIdx.x * 256 + threadIdx.x;
    const int V = min((int)sums[nblk], capacity);
    if (id >= (long)V * ndim) return;
    const int v = (int)(id / ndim), k = (int)(id - (long)v * ndim);
    const int n = cnt[v];
    if (k == 0 && num_points) num_points[v] = n;
    if (n > DV_THREAD_MAX) {
        if (k == 0) longlist[atomicAdd(nlong, 1)] = v;  // (at most P / (DV_THREAD_MAX + 1) such voxels: the list's size)
        return;
    }
    const int* list = seg + dv_start(cpre, csum, v);
    float s = 0.0f;
    int last = -1;
    for (int t = 0; t < n; ++t) {
        int m = INT_MAX;
        for (int j = 0; j < n; ++j) {
            const int e = list[j];
            if (e > last && e < m) m = e;
        }
        s = __fadd_rn(s, pts[(size_t)m * ndim + k]);
        last = m;
    }
    voxels[id] = __fdiv_rn(s, (float)n);
}

// One wavefront (a workgroup of 64 threads) per long list: sort it, then add its points in order.
//   sort: LSD radix sort, `passes` digits of 8 bits (the point indices are below 2^(8 passes)), each pass stable: a histogram of the
//         digit in LDS, its exclusive scan, then the list goes through in tiles of 64 - a lane's place is the digit's running offset plus
//         the number of lower lanes of the tile with the same digit (eight ballots), and the last lane of every digit moves the offset.
//   sum : lane k < ndim owns channel k; 64 indices are loaded at a time, the points are fetched eight at a time and added one by one.
__global__ __launch_bounds__(64) void dv_sum_long_kernel(const float* __restrict__ pts, int ndim, const int* __restrict__ cnt,
                                                         const int* __restrict__ cpre, const uint32_t* __restrict__ csum, int* seg,
                                                         int* tmp, int passes, const int* __restrict__ longlist,
                                                         const int* __restrict__ nlong, float* __restrict__ voxels) {
    __shared__ int hist[256];
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int todo = *nlong;
    for (int item = blockIdx.x; item < todo; item += gridDim.x) {
        const int v = longlist[item];
        const int n = cnt[v], start = dv_start(cpre, csum, v);
        int* src = seg + start;
        int* dst = tmp + start;
        for (int pass = 0; pass < passes; ++pass) {
            const int shift = 8 * pass;
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) hist[4 * lane + q] = 0;
            __syncthreads();
            for (int i = lane; i < n; i += 64) atomicAdd(&hist[(src[i] >> shift) & 255], 1);
            __syncthreads();
            {
                const int c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
                const int mine = c0 + c1 + c2 + c3;
                int inc = mine;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const int o = __shfl_up(inc, off, 64);
                    if (lane >= off) inc += o;
                }
                const int ex = inc - mine;
                hist[4 * lane] = ex, hist[4 * lane + 1] = ex + c0, hist[4 * lane + 2] = ex + c0 + c1, hist[4 * lane + 3] = ex + c0 + c1 + c2;
            }
            __syncthreads();
            for (int base = 0; base < n; base += 64) {
                const int i = base + lane;
                const bool valid = i < n;
                const int key = valid ? src[i] : 0;
                const int d = (key >> shift) & 255;
                unsigned long long peers = __ballot(valid);
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const bool one = (d >> b) & 1;
                    const unsigned long long bal = __ballot(one);
                    peers &= one ? bal : ~bal;
                }
                if (valid) dst[hist[d] + __popcll(peers & below)] = key;
                __syncthreads();
                if (valid && (peers >> lane) == 1ull) hist[d] += __popcll(peers);  // the highest lane of the digit
                __syncthreads();
            }
            int* t = src;
            src = dst;
            dst = t;
        }
        __syncthreads();  // the last pass's stores are visible to the whole wavefront
        float s = 0.0f;
        const int k = lane < ndim ? lane : 0;
        for (int base = 0; base < n; base += 64) {
            const int mine = base + lane < n ? src[base + lane] : 0;
            const int m = min(64, n - base);
            for (int j0 = 0; j0 < m; j0 += 8) {
                float val[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int idx = __shfl(mine, (j0 + u) & 63, 64);
                    val[u] = j0 + u < m ? pts[(size_t)idx * ndim + k] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (j0 + u < m) s = __fadd_rn(s, val[u]);
            }
        }
        if (lane < ndim) voxels[(size_t)v * ndim + lane] = __fdiv_rn(s, (float)n);
    }
}

static int dv_memset(void* p, int value, size_t bytes, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(p, value, bytes, st);
    if (e != hipSuccess) {
        set_error("dynvox: memset", e);
        return SHASTA_E_LAUNCH;
    }
    return SHASTA_OK;
}

static bool dv_offsets_ok(const int* h_offsets, int n) {
    if (!h_offsets || h_offsets[0] < 0) return false;
    for (int c = 0; c < n; ++c)
        if (h_offsets[c + 1] < h_offsets[c]) return false;
    return true;
}

}  // namespace shasta

using namespace shasta;

extern "C" size_t shasta_dynvox_workspace_bytes(const int* h_offsets, int num_clouds, int gx, int gy, int gz) {
    if (!dv_shape_ok(num_clouds, gx, gy, gz) || !dv_offsets_ok(h_offsets, num_clouds)) return 0;
    DvGrid G = {};
    G.g[0] = gx, G.g[1] = gy, G.g[2] = gz;
    return DvWs(nullptr, num_clouds, G, (long)h_offsets[num_clouds] - h_offsets[0]).bytes;
}

extern "C" int shasta_dynvox_mean_f32(const float* points, const int* h_offsets, int num_clouds, int ndim, const float* h_range6,
                                      const float* h_voxel3, int gx, int gy, int gz, float* voxels, int32_t* coors,
                                      int32_t* num_points, int capacity, int32_t* num_voxels, void* workspace, size_t workspace_bytes,
                                      shasta_stream_t stream) {
    SHASTA_REQUIRE(h_offsets && h_range6 && h_voxel3 && num_voxels && workspace, "dynvox: null pointer");
    if (ndim < 3 || ndim > 32 || !dv_shape_ok(num_clouds, gx, gy, gz)) {
        set_error_msg("dynvox: 3 to 32 floats per point, 1 to 32 clouds, num_clouds * (gz+1)(gy+1)(gx+1) cells below 2^31");
        return SHASTA_E_UNSUPPORTED;
    }
    SHASTA_REQUIRE(dv_offsets_ok(h_offsets, num_clouds), "dynvox: offsets must start at >= 0 and not decrease");
    SHASTA_REQUIRE(capacity >= 0 && (capacity == 0 || (voxels && coors)), "dynvox: null outputs or negative capacity");
    const long P = (long)h_offsets[num_clouds] - h_offsets[0];
    SHASTA_REQUIRE(P == 0 || points, "dynvox: null points");
    DvGrid G;
    G.g[0] = gx, G.g[1] = gy, G.g[2] = gz;
    for (int j = 0; j < 3; ++j) {
        G.lo[j] = h_range6[j], G.hi[j] = h_range6[3 + j], G.vs[j] = h_voxel3[j];
        SHASTA_REQUIRE(isfinite(G.lo[j]) && isfinite(G.hi[j]) && isfinite(G.vs[j]) && G.vs[j] > 0.0f && G.lo[j] <= G.hi[j],
                       "dynvox: the range must be finite and ordered, the voxel size positive");
        // subtraction and division are monotonic: no kept point has a larger coordinate than the upper face
        const float top = (G.hi[j] - G.lo[j]) / G.vs[j];
        SHASTA_REQUIRE(top < 2147483648.0f && (int)top <= G.g[j], "dynvox: the grid is smaller than (hi - lo) / voxel_size");
    }
    if ((uintptr_t)workspace % 16) {
        set_error_msg("dynvox: workspace must be 16-byte aligned");
        return SHASTA_E_ALIGN;
    }
    const DvWs L(workspace, num_clouds, G, P);
    if (workspace_bytes < L.bytes) {
        set_error_msg("dynvox: workspace too small");
        return SHASTA_E_WORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    int rc;
    if (P == 0) return dv_memset(num_voxels, 0, ((size_t)num_clouds + 1) * sizeof(int32_t), st);
    DvBatch B;
    B.n = num_clouds;
    for (int c = 0; c <= DV_MAX_CLOUDS; ++c) B.off[c] = h_offsets[c < num_clouds ? c : num_clouds] - h_offsets[0];
    const float* pts = points + (size_t)h_offsets[0] * ndim;
    const SpIndex& ix = L.ix;
    const unsigned pblocks = (unsigned)((P + 255) / 256);
    const int D = gz + 1, H = gy + 1, W = gx + 1;
    if ((rc = dv_memset(ix.bits, 0, ix.words * 4, st))) return rc;
    if ((rc = dv_memset(L.cnt, 0, L.zero_bytes, st))) return rc;
    hipLaunchKernelGGL(dv_key_kernel, dim3(pblocks), dim3(256), 0, st, pts, B, ndim, G, L.row, ix.bits);
    if ((rc = check_launch("dv_key"))) return rc;
    if ((rc = sp_scan(ix, nullptr, st))) return rc;
    hipLaunchKernelGGL(dv_prefix_kernel, dim3(1), dim3(64), 0, st, ix.bits, ix.pre, ix.sums, num_clouds, D * H * W, ix.nblk, num_voxels);
    if (capacity > 0)
        hipLaunchKernelGGL(sp_index_emit_kernel, dim3((unsigned)((ix.words + 255) / 256)), dim3(256), 0, st, ix.bits, ix.pre, ix.sums, ix.words,
                           D, H, W, capacity, coors, (int*)nullptr);
    if ((rc = check_launch("sp_index_emit"))) return rc;
    if (capacity == 0) return SHASTA_OK;
    hipLaunchKernelGGL(dv_count_kernel, dim3(pblocks), dim3(256), 0, st, L.row, P, ix.bits, ix.pre, ix.sums, L.slot, L.cnt);
    hipLaunchKernelGGL(scan_blocks_kernel<false>, dim3(L.cblk), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(L.cnt),
                       reinterpret_cast<uint32_t*>(L.cpre), L.csum);
    hipLaunchKernelGGL(scan_sums_kernel<true>, dim3(1), dim3(256), 0, st, L.csum, L.cblk, (int32_t*)nullptr);
    hipLaunchKernelGGL(dv_fill_kernel, dim3(pblocks), dim3(256), 0, st, L.row, L.slot, P, L.cpre, L.csum, L.seg);
    if ((rc = check_launch("dv_fill"))) return rc;
    const long rows = P < capacity ? P : capacity;  // V <= P
    hipLaunchKernelGGL(dv_sum_kernel, dim3((unsigned)((rows * ndim + 255) / 256)), dim3(256), 0, st, pts, ndim, L.cnt, L.cpre, L.csum, L.seg,
                       ix.sums, ix.nblk, capacity, voxels, num_points, L.longlist, L.nlong);
    if ((rc = check_launch("dv_sum"))) return rc;
    if (P > DV_THREAD_MAX) {
        int passes = 1;
        while (passes < 4 && (P - 1) >> (8 * passes)) ++passes;
        const long lists = P / (DV_THREAD_MAX + 1);
        hipLaunchKernelGGL(dv_sum_long_kernel, dim3((unsigned)(lists < DV_LONG_BLOCKS ? lists : DV_LONG_BLOCKS)), dim3(64), 0, st, pts, ndim,
                           L.cnt, L.cpre, L.csum, L.seg, L.tmp, passes, L.longlist, L.nlong, voxels);
        if ((rc = check_launch("dv_sum_long"))) return rc;
    }
    return SHASTA_OK;
}
