// CenterPoint training targets on the device: ground-truth boxes -> heatmaps, anno_box, ind, mask, cat (include/shasta_hip.h has the
// arithmetic, step by step).  Restates the box half of det3d/datasets/pipelines/preprocess.py:126-136, filter_gt_box_outside_range
// (det3d/core/sampler/preprocess.py:108-122) and AssignLabel (det3d/datasets/pipelines/preprocess.py:273-458, the nuScenes branch).
// Parallel formulation:
//   1. ct_assign_kernel : one workgroup of 256 threads per sample.  Loop A walks the sample's boxes in chunks of 256 in input order:
//        augment, range filter, class -> bin g (0 .. 63, the class over all tasks), and the box's stable rank inside its bin = running
//        count of the bin over earlier chunks + counts of the lower waves of this chunk + lower lanes of this wave with the same bin
//        (ballots).  After the loop the running counts are the histogram; slot = boxes of the task's earlier classes + rank.  Loop B
//        (same thread <-> box mapping) computes the slot's targets and leaves one record (x, y, radius, class) per slot.
//   2. ct_draw_kernel   : one wave per slot; the clipped (2r + 1)^2 window, integer atomicMax on the bit patterns of the non-negative
//        fp32 values: a maximum does not depend on order, so every run gives the same bits.  Work follows the drawn pixels (a few
//        hundred per object), not map x objects as a per-pixel gather would; the atomics return nothing and resolve in L2.
// The `h < eps max` cut of gaussian2D is not built: the smallest value of a window is exp(-36 r^2 / (2r + 1)^2) > e^-9, far above
// 2.2e-16 times the maximum 1.
#include "common.hpp"
#include <math.h>

namespace shasta {

constexpr int CT_THREADS = 256;
constexpr int CT_BINS = SHASTA_CENTER_MAX_TASKS * SHASTA_CENTER_MAX_TASK_CLASSES;  // 64
static_assert(sizeof(shasta_box_augment) == 48, "table layout");
static_assert(CT_BINS == 64 && CT_THREADS == 256, "ct_assign_kernel: one thread per bin in a wave, four waves");

struct CtParams {  // by value to the kernels
    int T, max_objs, min_radius, W, H, B;
    int first[SHASTA_CENTER_MAX_TASKS + 1];  // 0-based first bin of a task; [T] = number of bins
    long long hm_off[SHASTA_CENTER_MAX_TASKS];  // first element of a task's block in hm
    float pc_x, pc_y, vx, vy, osf;
    float k1m, k1p, km2, km1, k16;  // fl32 of 1 - o, 1 + o, -2 o, o - 1, 16 o
    int use_filter;
    float xlo, ylo, xhi, yhi;
};

struct CtWs {
    int32_t* off;               // B + 1
    shasta_box_augment* aug;    // B
    int4* obj;                  // T * B * max_objs records (x, y, radius, class); radius < 0: empty
    size_t bytes;
    CtWs(void* base, int B, int T, int max_objs) {
        char* p = static_cast<char*>(base);
        size_t at = 0;
        auto take = [&](size_t n) { char* q = p + at; at += align_up(n, 256); return q; };
        off = reinterpret_cast<int32_t*>(take((SHASTA_CENTER_MAX_BATCH + 1) * sizeof(int32_t)));
        aug = reinterpret_cast<shasta_box_augment*>(take(SHASTA_CENTER_MAX_BATCH * sizeof(shasta_box_augment)));
        obj = reinterpret_cast<int4*>(take((size_t)T * B * max_objs * sizeof(int4)));
        bytes = at;
    }
};

static bool ct_sizes_ok(int B, int T, int max_objs) {
    return B >= 1 && B <= SHASTA_CENTER_MAX_BATCH && T >= 1 && T <= SHASTA_CENTER_MAX_TASKS && max_objs >= 1 && max_objs <= SHASTA_CENTER_MAX_OBJS;
}

__device__ __forceinline__ void ct_rotate(float& a, float& b, float c, float s) {
    const float x = a, y = b;
    a = __fadd_rn(__fmul_rn(x, c), __fmul_rn(y, s));
    b = __fadd_rn(__fmul_rn(x, -s), __fmul_rn(y, c));
}

__device__ __forceinline__ void ct_augment(float* v, const shasta_box_augment& A) {
    if (A.flags & SHASTA_AUG_NEG_Y) {
        v[1] = -v[1];
        v[8] = __fadd_rn(-v[8], 3.14159274101257324f);
        v[7] = -v[7];
    }
    if (A.flags & SHASTA_AUG_NEG_X) {
        v[0] = -v[0];
        v[8] = __fadd_rn(-v[8], 6.28318548202514648f);
        v[6] = -v[6];
    }
    ct_rotate(v[0], v[1], A.c, A.s);
    ct_rotate(v[6], v[7], A.c, A.s);
    v[8] = __fadd_rn(v[8], A.angle);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)__dmul_rn((double)v[j], A.scale);
    if (A.flags & SHASTA_AUG_TRANSLATE) {
#pragma unroll
        for (int j = 0; j < 3; ++j) v[j] = (float)__dadd_rn((double)v[j], A.translate[j]);
    }
}

// points_in_convex_polygon_jit for the rectangle P0 = (xlo, ylo), P1 = (xlo, yhi), P2 = (xhi, yhi), P3 = (xhi, ylo), edge k from P(k-1)
// to P(k): cross = fl32(vec.y fl32(P.x - px)) - fl32(vec.x fl32(P.y - py)) in float64; inside iff every cross < 0 (a NaN passes, as there)
__device__ __forceinline__ bool ct_point_inside(float px, float py, float xlo, float ylo, float xhi, float yhi) {
    const float X[4] = {xlo, xlo, xhi, xhi}, Y[4] = {ylo, yhi, yhi, ylo};
    bool in = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = (k + 3) & 3;
        const float ex = __fsub_rn(X[k], X[j]), ey = __fsub_rn(Y[k], Y[j]);
        const double cross = __dsub_rn((double)__fmul_rn(ey, __fsub_rn(X[k], px)), (double)__fmul_rn(ex, __fsub_rn(Y[k], py)));
        if (cross >= 0.0) in = false;
    }
    return in;
}

__device__ __forceinline__ bool ct_box_in_range(const float* v, float xlo, float ylo, float xhi, float yhi) {
    const float sn = sinf(v[8]), cs = cosf(v[8]);
    const float hx[4] = {-0.5f, -0.5f, 0.5f, 0.5f}, hy[4] = {-0.5f, 0.5f, 0.5f, -0.5f};  // corners_nd: clockwise from the minimum
    bool any = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float a = __fmul_rn(v[3], hx[i]), b = __fmul_rn(v[4], hy[i]);
        const float cx = __fadd_rn(__fadd_rn(__fmul_rn(a, cs), __fmul_rn(b, sn)), v[0]);
        const float cy = __fadd_rn(__fadd_rn(__fmul_rn(a, -sn), __fmul_rn(b, cs)), v[1]);
        any = any || ct_point_inside(cx, cy, xlo, ylo, xhi, yhi);
    }
    return any;
}

__device__ __forceinline__ float ct_radius(float h, float w, const CtParams& P) {
    const float hw = __fadd_rn(h, w);
    const float b1 = hw;
    const float c1 = __fdiv_rn(__fmul_rn(__fmul_rn(w, h), P.k1m), P.k1p);
    const float r1 = __fdiv_rn(__fadd_rn(b1, __fsqrt_rn(__fsub_rn(__fmul_rn(b1, b1), __fmul_rn(4.0f, c1)))), 2.0f);
    const float b2 = __fmul_rn(2.0f, hw);
    const float c2 = __fmul_rn(__fmul_rn(P.k1m, w), h);
    const float r2 = __fdiv_rn(__fadd_rn(b2, __fsqrt_rn(__fsub_rn(__fmul_rn(b2, b2), __fmul_rn(16.0f, c2)))), 2.0f);
    const float b3 = __fmul_rn(P.km2, hw);
    const float c3 = __fmul_rn(__fmul_rn(P.km1, w), h);
    const float r3 = __fdiv_rn(__fadd_rn(b3, __fsqrt_rn(__fsub_rn(__fmul_rn(b3, b3), __fmul_rn(P.k16, c3)))), 2.0f);
    float r = r1;  // Python's min(r1, r2, r3): a later value replaces the minimum only when it is smaller
    if (r2 < r) r = r2;
    if (r3 < r) r = r3;
    return r;
}

static __global__ __launch_bounds__(CT_THREADS) void ct_assign_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ classes,
                                                                      const int32_t* __restrict__ off, const shasta_box_augment* __restrict__ aug,
                                                                      CtParams P, float* __restrict__ boxes_out, uint8_t* __restrict__ keep_out,
                                                                      float* __restrict__ anno_box, long long* __restrict__ ind,
                                                                      uint8_t* __restrict__ mask, long long* __restrict__ cat,
                                                                      float* __restrict__ gtbc, int4* __restrict__ obj) {
    __shared__ int s_run[CT_BINS];
    __shared__ int s_wcnt[4][CT_BINS];
    __shared__ int s_base[CT_BINS];                       // boxes of the task's earlier classes
    __shared__ int s_task_first[SHASTA_CENTER_MAX_TASKS];  // boxes of the earlier tasks
    __shared__ short s_rank[SHASTA_CENTER_MAX_BOXES];
    __shared__ signed char s_bin[SHASTA_CENTER_MAX_BOXES];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int row0 = off[b], n = min(off[b + 1] - row0, SHASTA_CENTER_MAX_BOXES);
    const int nbins = P.first[P.T];
    if (t < CT_BINS) s_run[t] = 0;
    for (int i = t; i < 4 * CT_BINS; i += CT_THREADS) (&s_wcnt[0][0])[i] = 0;
    __syncthreads();
    const unsigned long long lower = (1ull << lane) - 1ull;
    for (int c0 = 0; c0 < n; c0 += CT_THREADS) {  // loop A; n is uniform over the workgroup
        const int i = c0 + t;
        int g = -1;
        if (i < n) {
            float v[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) v[j] = boxes[(size_t)(row0 + i) * 9 + j];
            if (aug) ct_augment(v, aug[b]);
#pragma unroll
            for (int j = 0; j < 9; ++j) boxes_out[(size_t)(row0 + i) * 9 + j] = v[j];
            const bool keep = !P.use_filter || ct_box_in_range(v, P.xlo, P.ylo, P.xhi, P.yhi);
            keep_out[row0 + i] = keep ? 1 : 0;
            const int cls = classes[row0 + i];
            if (keep && cls >= 1 && cls <= nbins) g = cls - 1;
            s_bin[i] = (signed char)g;
        }
        int wrank = 0;
        unsigned long long todo = __ballot(g >= 0);
        while (todo) {  // one round per distinct bin in the wave
            const int src = __ffsll((long long)todo) - 1;
            const int gl = __shfl(g, src, 64);
            const unsigned long long m = __ballot(g == gl);
            if (g == gl) {
                wrank = __popcll(m & lower);
                if (lane == src) s_wcnt[wv][g] = __popcll(m);
            }
            todo &= ~m;
        }
        __syncthreads();
        if (g >= 0) {
            int r = s_run[g] + wrank;
            for (int w = 0; w < wv; ++w) r += s_wcnt[w][g];
            s_rank[i] = (short)r;
        }
        __syncthreads();
        if (t < CT_BINS) {
            s_run[t] += s_wcnt[0][t] + s_wcnt[1][t] + s_wcnt[2][t] + s_wcnt[3][t];
            s_wcnt[0][t] = s_wcnt[1][t] = s_wcnt[2][t] = s_wcnt[3][t] = 0;
        }
        __syncthreads();
    }
    if (t < P.T) {
        int before = 0;
        for (int u = 0; u < t; ++u)
            for (int g = P.first[u]; g < P.first[u + 1]; ++g) before += s_run[g];
        s_task_first[t] = before;
        int acc = 0;
        for (int g = P.first[t]; g < P.first[t + 1]; ++g) {
            s_base[g] = acc;
            acc += s_run[g];
        }
    }
    __syncthreads();
    for (int c0 = 0; c0 < n; c0 += CT_THREADS) {  // loop B
        const int i = c0 + t;
        if (i >= n) continue;
        const int g = s_bin[i];
        if (g < 0) continue;
        int task = 0;
        while (g >= P.first[task + 1]) ++task;  // g < first[T]
        const int k = s_base[g] + s_rank[i];
        float v[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) v[j] = boxes_out[(size_t)(row0 + i) * 9 + j];  // this thread's own stores of loop A
        const float period = 6.28318548202514648f;
        v[8] = __fsub_rn(v[8], __fmul_rn(floorf(__fadd_rn(__fdiv_rn(v[8], period), 0.5f)), period));
        if (gtbc) {
            const int row = s_task_first[task] + k;
            if (row < P.max_objs) {
                float* o = gtbc + ((size_t)b * P.max_objs + row) * 10;
                o[0] = v[0], o[1] = v[1], o[2] = v[2], o[3] = v[3], o[4] = v[4], o[5] = v[5], o[6] = v[8], o[7] = v[6], o[8] = v[7];
                o[9] = (float)(g + 1);
            }
        }
        if (k >= P.max_objs) continue;
        const float w = __fdiv_rn(__fdiv_rn(v[3], P.vx), P.osf), l = __fdiv_rn(__fdiv_rn(v[4], P.vy), P.osf);
        if (!(w > 0.0f && l > 0.0f)) continue;
        const float rf = ct_radius(l, w, P);
        // int(radius): truncation; clamped to the largest window that can matter (a window of 2 x 512 covers every map from every centre)
        const int ri = rf < (float)(2 * SHASTA_CENTER_MAX_MAP) ? (int)rf : 2 * SHASTA_CENTER_MAX_MAP;
        const int radius = max(P.min_radius, ri);
        const float cx = __fdiv_rn(__fdiv_rn(__fsub_rn(v[0], P.pc_x), P.vx), P.osf);
        const float cy = __fdiv_rn(__fdiv_rn(__fsub_rn(v[1], P.pc_y), P.vy), P.osf);
        // ct_int = truncation toward zero: (-1, 0) -> 0 is inside; a NaN fails both comparisons
        if (!(cx > -1.0f && cx < (float)P.W && cy > -1.0f && cy < (float)P.H)) continue;
        const int x = (int)cx, y = (int)cy;
        const size_t slot = ((size_t)task * P.B + b) * P.max_objs + k;
        cat[slot] = g - P.first[task];
        ind[slot] = (long long)y * P.W + x;
        mask[slot] = 1;
        float* a = anno_box + slot * 10;
        a[0] = __fsub_rn(cx, (float)x), a[1] = __fsub_rn(cy, (float)y), a[2] = v[2];
        a[3] = logf(v[3]), a[4] = logf(v[4]), a[5] = logf(v[5]);
        a[6] = v[6], a[7] = v[7], a[8] = sinf(v[8]), a[9] = cosf(v[8]);
        obj[slot] = make_int4(x, y, radius, g - P.first[task]);
    }
}

static __global__ __launch_bounds__(CT_THREADS) void ct_draw_kernel(const int4* __restrict__ obj, CtParams P, float* __restrict__ hm) {
    const int lane = threadIdx.x & 63, k = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int b = blockIdx.y, task = blockIdx.z;
    if (k >= P.max_objs) return;
    const int4 o = obj[((size_t)task * P.B + b) * P.max_objs + k];
    const int x = o.x, y = o.y, r = o.z, c = o.w;
    const int C = P.first[task + 1] - P.first[task];
    if (r < 0 || x < 0 || x >= P.W || y < 0 || y >= P.H || c < 0 || c >= C) return;  // empty slot (records are preset to -1)
    const int x0 = max(x - r, 0), x1 = min(x + r, P.W - 1), y0 = max(y - r, 0), y1 = min(y + r, P.H - 1);
    const int ww = x1 - x0 + 1, count = ww * (y1 - y0 + 1);
    const double sigma = (double)(2 * r + 1) / 6.0;
    const double denom = __dmul_rn(__dmul_rn(2.0, sigma), sigma);
    unsigned* plane = reinterpret_cast<unsigned*>(hm + P.hm_off[task] + ((size_t)b * C + c) * P.H * P.W);
    for (int i = lane; i < count; i += 64) {
        const int py = y0 + i / ww, px = x0 + i % ww;
        const double dx = (double)(px - x), dy = (double)(py - y);
        const float val = (float)exp(-(dx * dx + dy * dy) / denom);  // integers: the sum of squares is exact
        atomicMax(plane + (size_t)py * P.W + px, __float_as_uint(val));
    }
}

static __global__ __launch_bounds__(CT_THREADS) void ct_augment_kernel(const float* __restrict__ boxes, long n, shasta_box_augment A,
                                                                       float* __restrict__ out) {
    const long i = (long)blockIdx.x * CT_THREADS + threadIdx.x;
    if (i >= n) return;
    float v[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) v[j] = boxes[i * 9 + j];
    ct_augment(v, A);
#pragma unroll
    for (int j = 0; j < 9; ++j) out[i * 9 + j] = v[j];
}

static __global__ __launch_bounds__(CT_THREADS) void ct_filter_kernel(const float* __restrict__ boxes, long n, float xlo, float ylo, float xhi,
                                                                      float yhi, uint8_t* __restrict__ keep) {
    const long i = (long)blockIdx.x * CT_THREADS + threadIdx.x;
    if (i >= n) return;
    float v[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) v[j] = boxes[i * 9 + j];
    keep[i] = ct_box_in_range(v, xlo, ylo, xhi, yhi) ? 1 : 0;
}

// minmax_to_corner_2d in fp32: the lower corner is the range's, the upper one fl(fl(hi - lo) 1 + lo)
static void ct_rectangle(const float* r, float* xlo, float* ylo, float* xhi, float* yhi) {
    volatile float dx = r[2] - r[0], dy = r[3] - r[1];
    volatile float hx = dx + r[0], hy = dy + r[1];
    *xlo = r[0], *ylo = r[1], *xhi = hx, *yhi = hy;
}

static bool ct_grid_ok(long n) { return n >= 0 && n <= (long)CT_THREADS * 0x7fffffffL / 16; }

}  // namespace shasta

using namespace shasta;

extern "C" size_t shasta_center_targets_workspace_bytes(int B, int num_tasks, int max_objs) {
    if (!ct_sizes_ok(B, num_tasks, max_objs)) return 0;
    return CtWs(nullptr, B, num_tasks, max_objs).bytes;
}

extern "C" int shasta_center_targets_f32(const float* boxes, const int32_t* classes, const int32_t* h_offsets, int B,
                                         const shasta_center_target_cfg* cfg, const shasta_box_augment* h_augment, const float* h_bv_range,
                                         float* boxes_out, uint8_t* keep_out, float* hm, float* anno_box, int64_t* ind, uint8_t* mask,
                                         int64_t* cat, float* gt_boxes_and_cls, void* workspace, size_t workspace_bytes,
                                         shasta_stream_t stream) {
    SHASTA_REQUIRE(cfg && h_offsets && hm && anno_box && ind && mask && cat && workspace, "center targets: null pointer");
    const int T = cfg->num_tasks, max_objs = cfg->max_objs;
    if (!ct_sizes_ok(B, T, max_objs) || cfg->map_w < 1 || cfg->map_w > SHASTA_CENTER_MAX_MAP || cfg->map_h < 1 ||
        cfg->map_h > SHASTA_CENTER_MAX_MAP) {
        set_error_msg("center targets: 1..64 samples, 1..16 tasks, 1..1024 objects per task, maps up to 512 x 512");
        return SHASTA_E_UNSUPPORTED;
    }
    CtParams P = {};
    P.T = T, P.max_objs = max_objs, P.min_radius = cfg->min_radius, P.W = cfg->map_w, P.H = cfg->map_h, P.B = B;
    long long hm_elems = 0;
    for (int t = 0; t < T; ++t) {
        if (cfg->num_class[t] < 1 || cfg->num_class[t] > SHASTA_CENTER_MAX_TASK_CLASSES) {
            set_error_msg("center targets: 1..4 classes per task");
            return SHASTA_E_UNSUPPORTED;
        }
        P.first[t + 1] = P.first[t] + cfg->num_class[t];
        P.hm_off[t] = hm_elems;
        hm_elems += (long long)B * cfg->num_class[t] * P.H * P.W;
    }
    SHASTA_REQUIRE(cfg->min_radius >= 0, "center targets: a negative min_radius");
    SHASTA_REQUIRE(cfg->voxel_x > 0 && cfg->voxel_y > 0 && cfg->out_size_factor > 0, "center targets: voxel size and out_size_factor must be positive");
    SHASTA_REQUIRE(cfg->gaussian_overlap > 0 && cfg->gaussian_overlap < 1, "center targets: gaussian_overlap must lie in (0, 1)");
    SHASTA_REQUIRE(h_offsets[0] >= 0, "center targets: a negative offset");
    for (int b = 0; b < B; ++b) {
        SHASTA_REQUIRE(h_offsets[b + 1] >= h_offsets[b], "center targets: offsets must not decrease");
        if (h_offsets[b + 1] - h_offsets[b] > SHASTA_CENTER_MAX_BOXES) {
            set_error_msg("center targets: at most 4096 boxes per sample");
            return SHASTA_E_UNSUPPORTED;
        }
    }
    const long total = h_offsets[B];
    SHASTA_REQUIRE(total == 0 || (boxes && classes && boxes_out && keep_out), "center targets: null boxes, classes or their outputs");
    if ((uintptr_t)workspace % 16) {
        set_error_msg("center targets: workspace must be 16-byte aligned");
        return SHASTA_E_ALIGN;
    }
    const CtWs L(workspace, B, T, max_objs);
    if (workspace_bytes < L.bytes) {
        set_error_msg("center targets: workspace too small");
        return SHASTA_E_WORKSPACE;
    }
    const double o = cfg->gaussian_overlap;
    P.pc_x = cfg->pc_x, P.pc_y = cfg->pc_y, P.vx = cfg->voxel_x, P.vy = cfg->voxel_y, P.osf = cfg->out_size_factor;
    P.k1m = (float)(1 - o), P.k1p = (float)(1 + o), P.km2 = (float)(-2 * o), P.km1 = (float)(o - 1), P.k16 = (float)(4 * (4 * o));
    P.use_filter = h_bv_range != nullptr;
    if (h_bv_range) ct_rectangle(h_bv_range, &P.xlo, &P.ylo, &P.xhi, &P.yhi);

    hipStream_t st = as_stream(stream);
    hipError_t e;
    const size_t slots = (size_t)T * B * max_objs;
    if ((e = hipMemsetAsync(hm, 0, (size_t)hm_elems * sizeof(float), st)) != hipSuccess ||
        (e = hipMemsetAsync(anno_box, 0, slots * 10 * sizeof(float), st)) != hipSuccess ||
        (e = hipMemsetAsync(ind, 0, slots * sizeof(int64_t), st)) != hipSuccess ||
        (e = hipMemsetAsync(cat, 0, slots * sizeof(int64_t), st)) != hipSuccess ||
        (e = hipMemsetAsync(mask, 0, slots, st)) != hipSuccess ||
        (gt_boxes_and_cls && (e = hipMemsetAsync(gt_boxes_and_cls, 0, (size_t)B * max_objs * 10 * sizeof(float), st)) != hipSuccess) ||
        (e = hipMemsetAsync(L.obj, 0xff, slots * sizeof(int4), st)) != hipSuccess ||
        (e = hipMemcpyAsync(L.off, h_offsets, ((size_t)B + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st)) != hipSuccess ||
        (h_augment && (e = hipMemcpyAsync(L.aug, h_augment, (size_t)B * sizeof(shasta_box_augment), hipMemcpyHostToDevice, st)) != hipSuccess)) {
        set_error("center targets: memsets and copy of the tables", e);
        return SHASTA_E_LAUNCH;
    }
    hipLaunchKernelGGL(ct_assign_kernel, dim3((unsigned)B), dim3(CT_THREADS), 0, st, boxes, classes, L.off,
                       h_augment ? L.aug : (const shasta_box_augment*)nullptr, P, boxes_out, keep_out, anno_box,
                       reinterpret_cast<long long*>(ind), mask, reinterpret_cast<long long*>(cat), gt_boxes_and_cls, L.obj);
    int rc;
    if ((rc = check_launch("ct_assign"))) return rc;
    hipLaunchKernelGGL(ct_draw_kernel, dim3((unsigned)cdiv(max_objs, 4), (unsigned)B, (unsigned)T), dim3(CT_THREADS), 0, st, L.obj, P, hm);
    return check_launch("ct_draw");
}

extern "C" int shasta_center_box_augment_f32(const float* boxes, long n, const shasta_box_augment* h_augment, float* out,
                                             shasta_stream_t stream) {
    SHASTA_REQUIRE(h_augment, "center box augment: null table");
    SHASTA_REQUIRE(ct_grid_ok(n), "center box augment: row count out of range");
    if (n == 0) return SHASTA_OK;
    SHASTA_REQUIRE(boxes && out, "center box augment: null pointer");
    hipLaunchKernelGGL(ct_augment_kernel, dim3((unsigned)((n + CT_THREADS - 1) / CT_THREADS)), dim3(CT_THREADS), 0, as_stream(stream), boxes, n,
                       *h_augment, out);
    return check_launch("ct_augment");
}

extern "C" int shasta_center_range_filter_f32(const float* boxes, long n, const float* h_bv_range, uint8_t* keep, shasta_stream_t stream) {
    SHASTA_REQUIRE(h_bv_range, "center range filter: null range");
    SHASTA_REQUIRE(ct_grid_ok(n), "center range filter: row count out of range");
    if (n == 0) return SHASTA_OK;
    SHASTA_REQUIRE(boxes && keep, "center range filter: null pointer");
    float xlo, ylo, xhi, yhi;
    ct_rectangle(h_bv_range, &xlo, &ylo, &xhi, &yhi);
    hipLaunchKernelGGL(ct_filter_kernel, dim3((unsigned)((n + CT_THREADS - 1) / CT_THREADS)), dim3(CT_THREADS), 0, as_stream(stream), boxes, n,
                       xlo, ylo, xhi, yhi, keep);
    return check_launch("ct_filter");
}
