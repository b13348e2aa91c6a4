// Multi-sweep cloud assembly, bit-identical to the reference's loader on the CPU.
// Restates det3d/datasets/pipelines/loading.py:23-69 (read_file, remove_close, read_sweep) and :111-148 (LoadPointCloudFromFile, the
// nuScenes branch), and the point half of det3d/datasets/pipelines/preprocess.py:126-136 (det3d/core/sampler/preprocess.py:771-839,
// 940-962: random_flip_both, global_rotation, global_scaling_v2, global_translate_).  A segment is one file; per segment:
//   * close test : a row is dropped iff fabs((double)x) < radius && fabs((double)y) < radius.  Strict: |x| == radius stays; a NaN
//                  coordinate makes its comparison false, so the row stays.  The key frame's flag is off: it is never filtered.
//   * transform  : r_i = ((m[i][0] x + m[i][1] y) + m[i][2] z) + m[i][3] for i = 0, 1, 2: the three products are formed in float64
//                  from the fp32 coordinates and rounded each (__dmul_rn), then added LEFT TO RIGHT in the order written, the
//                  translation last (__dadd_rn: no fused multiply-add), and the sum is rounded once to fp32.  The reference leaves the
//                  order to its BLAS; for data whose float64 sum is not within a few float64 ulps of an fp32 rounding tie every order
//                  rounds to the same fp32, which is what the golden fixture is built from.
//   * no transform: x, y, z are copied as 32-bit words (-0.0 and NaN payloads survive).
//   * columns 3 .. keep - 1 are copied as words; column `keep` is (float)time_lag.
// Augmentation (optional, per cloud, on every row that is written, in the reference's order):
//   1. flips     : y = -y (SHASTA_AUG_NEG_Y), then x = -x (SHASTA_AUG_NEG_X): sign-bit flips.
//   2. rotation  : x' = fl(fl(x c) + fl(y s)), y' = fl(fl(x (-s)) + fl(y c)) in fp32 with separate roundings, z unchanged.  The
//                  reference multiplies by a 3 x 3 fp32 matrix through its BLAS ([[c, -s, 0], [s, c, 0], [0, 0, 1]]), whose order and
//                  fusing are not fixed: equal within the bound of a three-term fp32 dot product, bit-equal for c = 1, s = 0.
//   3. scale     : fl32((double)v scale) for v = x, y, z: with an fp32-valued scale this is the fp32 multiply the reference makes.
//   4. translate : fl32((double)v + t[j]) (the reference adds a float64 array in place); only with SHASTA_AUG_TRANSLATE, because the
//                  reference skips the step when every std is zero (adding 0.0 would turn -0.0 into +0.0).
// Parallel formulation - a stable compaction with no float atomics, no workgroup that waits on another, and a grid that follows
// from the host's row counts alone:
//   0. tables : the host's segment (and augmentation) arrays are copied into the workspace on the caller's stream.
//   1. plan   : one workgroup: first row and first block of every segment (exclusive scans of rows and of ceil(rows / 256)), first
//               block of every cloud.  A block of SW_ROWS = 256 rows never spans two segments, so a segment's parameters are uniform
//               over a workgroup and live in scalar registers.
//   2. count  : one workgroup per block, one row per thread: keep flag, wave ballot, the block's number of kept rows.
//   3. scan   : one workgroup: exclusive scan of the block counts = every block's first output row; the value at a cloud's first block
//               is prefix[cloud], the total is prefix[num_clouds].
//   4. write  : the block's raw rows come in as contiguous words (coalesced) into LDS; every thread recomputes its row's keep flag,
//               its place = block offset + kept rows of lower waves + kept rows of lower lanes (ballot), assembles the row and puts it
//               at that place in an LDS image of the block's output, which leaves as contiguous words (coalesced; rows are 20 bytes).
//               The row stride in LDS is raw_ndim / keep + 1 words; for the nuScenes widths (5 and 5) the lanes of a half wave hit
//               32 different banks.
#include "common.hpp"
#include "scan.hpp"
#include <limits.h>
#include <math.h>

namespace shasta {

constexpr int SW_ROWS = SHASTA_SWEEPS_BLOCK_ROWS;  // rows per block = threads per workgroup
constexpr int SW_MAX_CLOUDS = SHASTA_SWEEPS_MAX_CLOUDS;
constexpr int SW_MAX_SEGMENTS = SHASTA_SWEEPS_MAX_SEGMENTS;
constexpr int SW_MIN_NDIM = 3, SW_MAX_NDIM = 8;
static_assert(SW_ROWS == SCAN_THREADS, "the kernels below use scan.hpp: 256 threads");
static_assert(sizeof(shasta_sweep_segment) == 120 && sizeof(shasta_sweep_augment) == 48, "table layouts");

struct SwPlan {
    int row0[SW_MAX_SEGMENTS + 1];       // rows before the segment; [S] = total_rows
    int blk0[SW_MAX_SEGMENTS + 1];       // blocks before the segment; [S] = number of blocks
    int cloud_blk[SW_MAX_CLOUDS + 1];    // first block of the first segment of a cloud >= c; [n] = number of blocks
};

struct SwWs {
    shasta_sweep_segment* seg;
    shasta_sweep_augment* aug;
    SwPlan* plan;
    uint32_t *cnt, *off;
    size_t bytes;
    SwWs(void* ws, int S, long total_rows) {
        const size_t blocks = (size_t)total_rows / SW_ROWS + (size_t)S + 1;  // sum of ceil(rows_s / 256) <= total / 256 + S
        char* base = static_cast<char*>(ws);
        size_t at = 0;
        auto take = [&](size_t b) {
            char* q = base + at;
            at += align_up(b, 256);
            return q;
        };
        seg = reinterpret_cast<shasta_sweep_segment*>(take((size_t)S * sizeof(shasta_sweep_segment)));
        aug = reinterpret_cast<shasta_sweep_augment*>(take(SW_MAX_CLOUDS * sizeof(shasta_sweep_augment)));
        plan = reinterpret_cast<SwPlan*>(take(sizeof(SwPlan)));
        cnt = reinterpret_cast<uint32_t*>(take(blocks * 4));
        off = reinterpret_cast<uint32_t*>(take(blocks * 4));
        bytes = at;
    }
};

static bool sw_sizes_ok(int S, long total_rows) { return S >= 1 && S <= SW_MAX_SEGMENTS && total_rows >= 0 && total_rows <= INT_MAX; }

__global__ __launch_bounds__(256) void sw_plan_kernel(const shasta_sweep_segment* __restrict__ seg, int S, int n, SwPlan* __restrict__ plan) {
    __shared__ uint32_t s_wave[4];
    __shared__ int s_blk0[SW_MAX_SEGMENTS + 1];
    const int t = threadIdx.x;
    uint32_t r[4], k[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int s = 4 * t + q;
        r[q] = s < S ? (uint32_t)seg[s].rows : 0u;
        k[q] = (r[q] + SW_ROWS - 1) / SW_ROWS;
    }
    uint32_t rows_total, blk_total;
    uint32_t er = block_scan(r[0] + r[1] + r[2] + r[3], s_wave, &rows_total);
    uint32_t ek = block_scan(k[0] + k[1] + k[2] + k[3], s_wave, &blk_total);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int s = 4 * t + q;
        if (s < S) plan->row0[s] = (int)er, plan->blk0[s] = (int)ek, s_blk0[s] = (int)ek;
        er += r[q], ek += k[q];
    }
    if (t == 0) plan->row0[S] = (int)rows_total, plan->blk0[S] = (int)blk_total, s_blk0[S] = (int)blk_total;
    __syncthreads();
    if (t <= n) {
        int s = 0;
        while (s < S && seg[s].cloud < t) ++s;
        plan->cloud_blk[t] = s_blk0[s];
    }
}

// the segment of block b: blk0[s] <= b < blk0[s + 1] (blk0[0] = 0, blk0[S] = number of blocks > b)
__device__ __forceinline__ int sw_segment_of(const int* __restrict__ blk0, int S, int b) {
    int lo = 0, hi = S;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk0[mid] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool sw_keep(uint32_t xb, uint32_t yb, bool drop, double radius) {
    const bool close = fabs((double)__uint_as_float(xb)) < radius && fabs((double)__uint_as_float(yb)) < radius;
    return !(drop && close);
}

__global__ __launch_bounds__(256) void sw_count_kernel(const uint32_t* __restrict__ raw, int raw_ndim, const shasta_sweep_segment* __restrict__ seg,
                                                       int S, const SwPlan* __restrict__ plan, double radius, uint32_t* __restrict__ cnt) {
    __shared__ int s_wave[4];
    const int b = blockIdx.x, t = threadIdx.x;
    const int s = sw_segment_of(plan->blk0, S, b);
    const int local = (b - plan->blk0[s]) * SW_ROWS + t, rows = seg[s].rows;
    bool keep = false;
    if (local < rows) {
        const uint32_t* p = raw + ((size_t)plan->row0[s] + local) * raw_ndim;
        keep = sw_keep(p[0], p[1], seg[s].flags & SHASTA_SWEEP_DROP_CLOSE, radius);
    }
    const int kept = block_place(keep, s_wave).count;
    if (t == 0) cnt[b] = (uint32_t)kept;
}

// one workgroup: off[b] = kept rows before block b; prefix[c] = kept rows before cloud c, prefix[n] = all kept rows
__global__ __launch_bounds__(256) void sw_scan_kernel(const uint32_t* __restrict__ cnt, int nblk, uint32_t* __restrict__ off,
                                                      const SwPlan* __restrict__ plan, int n, int32_t* __restrict__ prefix) {
    __shared__ uint32_t s_wave[4];
    __shared__ int s_first[SW_MAX_CLOUDS + 1];
    if (threadIdx.x <= n) s_first[threadIdx.x] = plan->cloud_blk[threadIdx.x];
    __syncthreads();
    const uint32_t total = scan_with_carry(cnt, nblk, s_wave, [&](int j, uint32_t ex) {
        off[j] = ex;
        for (int c = 0; c <= n; ++c)
            if (s_first[c] == j) prefix[c] = (int32_t)ex;
    });
    if (threadIdx.x <= n && s_first[threadIdx.x] >= nblk) prefix[threadIdx.x] = (int32_t)total;
}

__global__ __launch_bounds__(256) void sw_write_kernel(const uint32_t* __restrict__ raw, int raw_ndim, const shasta_sweep_segment* __restrict__ seg,
                                                       int S, const SwPlan* __restrict__ plan, double radius, int keep_cols,
                                                       const shasta_sweep_augment* __restrict__ aug, const uint32_t* __restrict__ off,
                                                       uint32_t* __restrict__ out) {
    __shared__ uint32_t s_in[SW_ROWS * SW_MAX_NDIM];
    __shared__ uint32_t s_out[SW_ROWS * (SW_MAX_NDIM + 1)];
    __shared__ int s_wave[4];
    const int b = blockIdx.x, t = threadIdx.x;
    const int s = sw_segment_of(plan->blk0, S, b);
    const int first = (b - plan->blk0[s]) * SW_ROWS, rows = seg[s].rows, flags = seg[s].flags;
    const int nb = min(SW_ROWS, rows - first);  // >= 1: the block exists
    const uint32_t* src = raw + ((size_t)plan->row0[s] + first) * raw_ndim;
    for (int i = t; i < nb * raw_ndim; i += SW_ROWS) s_in[i] = src[i];
    __syncthreads();
    uint32_t v[SW_MAX_NDIM] = {};
    bool keep = false;
    if (t < nb) {
#pragma unroll
        for (int j = 0; j < SW_MAX_NDIM; ++j) v[j] = j < raw_ndim ? s_in[t * raw_ndim + j] : 0u;
        keep = sw_keep(v[0], v[1], flags & SHASTA_SWEEP_DROP_CLOSE, radius);
    }
    const BlockPlace bp = block_place(keep, s_wave);
    const int place = bp.place, kept = bp.count;
    const int ow = keep_cols + 1;
    if (keep) {
        if (flags & SHASTA_SWEEP_TRANSFORM) {
            const double x = (double)__uint_as_float(v[0]), y = (double)__uint_as_float(v[1]), z = (double)__uint_as_float(v[2]);
            const double* m = seg[s].transform;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const double r = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(m[4 * i], x), __dmul_rn(m[4 * i + 1], y)), __dmul_rn(m[4 * i + 2], z)),
                                           m[4 * i + 3]);
                v[i] = __float_as_uint((float)r);
            }
        }
        if (aug) {
            const shasta_sweep_augment& A = aug[seg[s].cloud];
            if (A.flags & SHASTA_AUG_NEG_Y) v[1] ^= 0x80000000u;
            if (A.flags & SHASTA_AUG_NEG_X) v[0] ^= 0x80000000u;
            const float x = __uint_as_float(v[0]), y = __uint_as_float(v[1]);
            float p[3];
            p[0] = __fadd_rn(__fmul_rn(x, A.c), __fmul_rn(y, A.s));
            p[1] = __fadd_rn(__fmul_rn(x, -A.s), __fmul_rn(y, A.c));
            p[2] = __uint_as_float(v[2]);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                p[j] = (float)__dmul_rn((double)p[j], A.scale);
                if (A.flags & SHASTA_AUG_TRANSLATE) p[j] = (float)__dadd_rn((double)p[j], A.translate[j]);
                v[j] = __float_as_uint(p[j]);
            }
        }
        uint32_t* o = s_out + place * ow;
#pragma unroll
        for (int j = 0; j < SW_MAX_NDIM; ++j)
            if (j < keep_cols) o[j] = v[j];
        o[keep_cols] = __float_as_uint((float)seg[s].time_lag);
    }
    __syncthreads();
    uint32_t* dst = out + (size_t)off[b] * ow;  // off[b] + kept <= total_rows <= capacity
    for (int i = t; i < kept * ow; i += SW_ROWS) dst[i] = s_out[i];
}

}  // namespace shasta

using namespace shasta;

extern "C" size_t shasta_sweeps_workspace_bytes(int num_segments, long total_rows) {
    if (!sw_sizes_ok(num_segments, total_rows)) return 0;
    return SwWs(nullptr, num_segments, total_rows).bytes;
}

extern "C" int shasta_sweeps_assemble_f32(const float* raw, long total_rows, int raw_ndim, const shasta_sweep_segment* h_segments,
                                          int num_segments, int num_clouds, int keep, double radius, const shasta_sweep_augment* h_augment,
                                          float* out, long capacity, int32_t* prefix, void* workspace, size_t workspace_bytes,
                                          shasta_stream_t stream) {
    SHASTA_REQUIRE(h_segments && prefix && workspace, "sweeps: null pointer");
    SHASTA_REQUIRE(num_clouds >= 1 && num_clouds <= SW_MAX_CLOUDS, "sweeps: 1 to 32 clouds per call");
    SHASTA_REQUIRE(sw_sizes_ok(num_segments, total_rows), "sweeps: 1 to 1024 segments, 0 to 2^31 - 1 rows per call");
    if (raw_ndim < SW_MIN_NDIM || raw_ndim > SW_MAX_NDIM) {
        set_error_msg("sweeps: 3 to 8 floats per raw row");
        return SHASTA_E_UNSUPPORTED;
    }
    SHASTA_REQUIRE(keep >= 1 && keep <= raw_ndim, "sweeps: keep must be 1 .. raw_ndim");
    SHASTA_REQUIRE(!(radius != radius), "sweeps: the radius is a NaN");
    SHASTA_REQUIRE(capacity >= total_rows, "sweeps: capacity below total_rows, the number of rows that can survive");
    SHASTA_REQUIRE(total_rows == 0 || (raw && out), "sweeps: null rows or output");
    long sum = 0;
    int nblk = 0, last_cloud = 0;
    for (int s = 0; s < num_segments; ++s) {
        const shasta_sweep_segment& g = h_segments[s];
        SHASTA_REQUIRE(g.rows >= 0, "sweeps: a negative row count");
        SHASTA_REQUIRE(g.cloud >= last_cloud && g.cloud < num_clouds, "sweeps: cloud indices must lie in 0 .. num_clouds - 1 and not decrease");
        last_cloud = g.cloud;
        sum += g.rows;
        SHASTA_REQUIRE(sum <= total_rows, "sweeps: the segments hold more rows than total_rows");
        nblk += cdiv(g.rows, SW_ROWS);
    }
    SHASTA_REQUIRE(sum == total_rows, "sweeps: the segments' rows do not sum to total_rows");
    if ((uintptr_t)workspace % 16) {
        set_error_msg("sweeps: workspace must be 16-byte aligned");
        return SHASTA_E_ALIGN;
    }
    const SwWs L(workspace, num_segments, total_rows);
    if (workspace_bytes < L.bytes) {
        set_error_msg("sweeps: workspace too small");
        return SHASTA_E_WORKSPACE;
    }
    hipStream_t st = as_stream(stream);
    hipError_t e;
    if (nblk == 0) {
        if ((e = hipMemsetAsync(prefix, 0, ((size_t)num_clouds + 1) * sizeof(int32_t), st)) != hipSuccess) {
            set_error("sweeps: memset", e);
            return SHASTA_E_LAUNCH;
        }
        return SHASTA_OK;
    }
    if ((e = hipMemcpyAsync(L.seg, h_segments, (size_t)num_segments * sizeof(shasta_sweep_segment), hipMemcpyHostToDevice, st)) != hipSuccess ||
        (h_augment &&
         (e = hipMemcpyAsync(L.aug, h_augment, (size_t)num_clouds * sizeof(shasta_sweep_augment), hipMemcpyHostToDevice, st)) != hipSuccess)) {
        set_error("sweeps: copy of the tables", e);
        return SHASTA_E_LAUNCH;
    }
    int rc;
    const uint32_t* rw = reinterpret_cast<const uint32_t*>(raw);
    hipLaunchKernelGGL(sw_plan_kernel, dim3(1), dim3(256), 0, st, L.seg, num_segments, num_clouds, L.plan);
    hipLaunchKernelGGL(sw_count_kernel, dim3((unsigned)nblk), dim3(SW_ROWS), 0, st, rw, raw_ndim, L.seg, num_segments, L.plan, radius, L.cnt);
    if ((rc = check_launch("sw_count"))) return rc;
    hipLaunchKernelGGL(sw_scan_kernel, dim3(1), dim3(256), 0, st, L.cnt, nblk, L.off, L.plan, num_clouds, prefix);
    hipLaunchKernelGGL(sw_write_kernel, dim3((unsigned)nblk), dim3(SW_ROWS), 0, st, rw, raw_ndim, L.seg, num_segments, L.plan, radius, keep,
                       h_augment ? L.aug : (const shasta_sweep_augment*)nullptr, L.off, reinterpret_cast<uint32_t*>(out));
    return check_launch("sw_write");
}
