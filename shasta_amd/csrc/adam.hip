// Training path (SURVEY.md 8(a) row 19 / BASELINE config 5): the optimizer and the two big streams of the first aug_shape layers.
// Adam in one pass over p, g, m, v (single tensor, a table of small tensors, and a matrix whose gradient is a rank-R product formed in
// registers), and the rank-R streams of the anchor backward at small batch (dW1 = ghid^T x, dx = ghid W1): the kernels that move
// 3 GB per step.
#include <algorithm>
#include <math.h>

#include "common.hpp"

namespace shasta {

// Adam step (torch.optim.Adam semantics as used by tools/nusc_shasta/train.py:147: L2 weight decay added to the gradient,
// no amsgrad), one pass over p, g, m, v instead of the seven multi-tensor passes of the unfused optimizer:
//   g' = g + wd*p ; m += (g' - m)*(1-b1) ; v = b2*v + (1-b2)*g'*g' ; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
struct AdamArgs {
    // one_minus_beta: 1 - beta formed in DOUBLE from the caller's double beta and rounded once, like torch's scalars.  1.0f - (float)beta
    // carries beta's own rounding error relative to the thousand times smaller 1 - beta (0.999f: 1.3e-5 of every g*g added to v)
    float lr_over_bc1, beta1, beta2, one_minus_beta1, one_minus_beta2, eps, weight_decay, rsqrt_bc2;
    // non-null: everything that changes from step to step comes from DEVICE memory (dyn = {lr / bc1, 1 / sqrt(bc2), beta1, beta2, 1 - beta1, 1 - beta2},
    // written by adam_prepare_kernel from a device-side step counter and the scheduler's lr / betas) - a training step replayed from a
    // captured hipGraph cannot take them as launch arguments, which are frozen at capture time
    const float* dyn;
};
__device__ __forceinline__ AdamArgs adam_resolve(AdamArgs a) {
    if (a.dyn) {
        a.lr_over_bc1 = a.dyn[0];
        a.rsqrt_bc2 = a.dyn[1];
        a.beta1 = a.dyn[2];
        a.beta2 = a.dyn[3];
        a.one_minus_beta1 = a.dyn[4];
        a.one_minus_beta2 = a.dyn[5];
    }
    return a;
}
// one step of the device-side schedule: ++*step; hyper = {lr, beta1, beta2} (doubles, the host's own values) ->
// dyn = {lr / (1 - beta1^step), 1 / sqrt(1 - beta2^step), beta1, beta2, 1 - beta1, 1 - beta2}: what make_adam_args computes on the host
__global__ void adam_prepare_kernel(int* __restrict__ step, const double* __restrict__ hyper, float* __restrict__ dyn) {
    if (threadIdx.x || blockIdx.x) return;
    const int s = *step + 1;
    *step = s;
    const double beta1 = hyper[1], beta2 = hyper[2];
    const double bc1 = 1.0 - pow(beta1, (double)s), bc2 = 1.0 - pow(beta2, (double)s);
    dyn[0] = (float)(hyper[0] / bc1);
    dyn[1] = (float)(1.0 / sqrt(bc2));
    dyn[2] = (float)beta1;
    dyn[3] = (float)beta2;
    dyn[4] = (float)(1.0 - beta1);
    dyn[5] = (float)(1.0 - beta2);
}

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamArgs& a) {
    g = fmaf(a.weight_decay, p, g);
    m = fmaf(g - m, a.one_minus_beta1, m);
    v = fmaf(a.one_minus_beta2, g * g, a.beta2 * v);
    const float denom = fmaf(sqrtf(v), a.rsqrt_bc2, a.eps);
    p = p - a.lr_over_bc1 * (m / denom);
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, long n, AdamArgs a_in) {
    const AdamArgs a = adam_resolve(a_in);
    const long n4 = n >> 2;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
        const f32x4 gg = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g) + i);
        f32x4 mm = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = pp[k], mk = mm[k], vk = vv[k];
            adam_one(pk, gg[k], mk, vk, a);
            pp[k] = pk;
            mm[k] = mk;
            vv[k] = vk;
        }
        reinterpret_cast<f32x4*>(p)[i] = pp;
        reinterpret_cast<f32x4*>(m)[i] = mm;
        reinterpret_cast<f32x4*>(v)[i] = vv;
    }
    const long i = (n4 << 2) + (long)blockIdx.x * blockDim.x + threadIdx.x;  // tail
    if (i < n) adam_one(p[i], g[i], m[i], v[i], a);
}

// The same update for up to ADAM_MULTI tensors in one launch (the ~60 small weight / bias tensors of rows 6-16: one launch instead of
// sixty of 5 us each): the tensor table travels in the kernel arguments; blockIdx.y = tensor, a grid-stride loop over its elements.
constexpr int ADAM_MULTI = 48;
struct AdamMulti {
    float* p[ADAM_MULTI];
    const float* g[ADAM_MULTI];
    float* m[ADAM_MULTI];
    float* v[ADAM_MULTI];
    long n[ADAM_MULTI];
};

__global__ __launch_bounds__(256) void adam_multi_kernel(AdamMulti t, AdamArgs a_in) {
    const AdamArgs a = adam_resolve(a_in);
    const int k = blockIdx.y;
    float* __restrict__ p = t.p[k];
    const float* __restrict__ g = t.g[k];
    float* __restrict__ m = t.m[k];
    float* __restrict__ v = t.v[k];
    const long n = t.n[k];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) adam_one(p[i], g[i], m[i], v[i], a);
}

// Adam for a matrix whose gradient is a rank-R product, g[h][k] = sum_r G[r][h] X[r][k] (the first aug_shape layers: G = gradient of the
// hidden activations, X = the layer's inputs, R = frame-pairs of the step over all ranks): the gradient is formed in registers inside the
// Adam pass - it is never written to memory and never read back.  24 bytes per parameter (p, m, v in and out) instead of the 36 of
// "write the gradient, read it in the Adam kernel".  A thread owns COLS consecutive columns and keeps its R x COLS slice of X in
// registers; G[r][h] is uniform over the workgroup (scalar loads).
// RDX > 0: the same pass also forms Y = Gdx . W with the weights as they are BEFORE the update (Gdx: (Rdx, H) at ldgdx; the backward's
// dx = ghid . W1, which otherwise reads the matrix a second time: smallm_nn_kernel) - partial sums per row block into `part`
// ([block][r][k], summed by smallm_finish_kernel).
// (196 - 229 registers, two waves per SIMD; forced to three or four waves the pass is 5 - 10 % slower: 1.10 -> 1.18 / 1.22 ms per 1 GB matrix)
template <int RMAX, int COLS, int RDX = 0>
__global__ __launch_bounds__(256) void adam_lowrank_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                           const float* __restrict__ G, int ldg, const float* __restrict__ X, int ldx, int R,
                                                           int H, int K, int rows_per_block, AdamArgs a_in, const float* __restrict__ Gdx = nullptr,
                                                           int ldgdx = 0, int Rdx = 0, float* __restrict__ part = nullptr) {
    const AdamArgs a = adam_resolve(a_in);
    typedef float fv __attribute__((ext_vector_type(COLS)));
    const long k0 = ((long)blockIdx.x * 256 + threadIdx.x) * COLS;
    fv dacc[RDX > 0 ? RDX : 1];
#pragma unroll
    for (int r = 0; r < (RDX > 0 ? RDX : 1); ++r) dacc[r] = fv(0.0f);
    // RMAX > 16 (the factors of a step over several ranks): G[r][h] for one h and all r lies in R different cache lines - as scalar loads
    // they bound the pass (2.38 ms per 1 GB matrix at R = 64, 2.6 TB/s).  The block's (R, rows) slice of G goes through LDS instead,
    // transposed to [row][r], and is read back as broadcasts.
    constexpr bool G_LDS = RMAX > 16;
    __shared__ __attribute__((aligned(16))) float s_g[G_LDS ? 64 * RMAX : 4];
    fv xv[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) {
        xv[r] = fv(0.0f);
        if (r < R && k0 < K) xv[r] = *reinterpret_cast<const fv*>(X + (size_t)r * ldx + k0);
    }
    const int h0 = blockIdx.y * rows_per_block, h1 = min(H, h0 + rows_per_block);
    if (G_LDS) {  // (rows_per_block <= 64; every thread of the block gets here: threads past the last column leave after the barrier)
        const int rows = h1 - h0;
        for (int e = threadIdx.x; e < RMAX * rows; e += 256) {
            const int r = e / rows, hl = e - r * rows;
            s_g[hl * RMAX + r] = r < R ? G[(size_t)r * ldg + h0 + hl] : 0.0f;
        }
        __syncthreads();
    }
    if (k0 >= K) return;
    for (int h = h0; h < h1; ++h) {
        const size_t at = (size_t)h * K + k0;
        // (3 GB stream through once per step: non-temporal loads and stores, 1.06 -> 1.00 ms per 1 GB matrix = 6.1 TB/s over p, m, v in
        // and out; unrolling the row loop on top of that: nothing)
        fv pp = __builtin_nontemporal_load(reinterpret_cast<const fv*>(p + at)), mm = __builtin_nontemporal_load(reinterpret_cast<const fv*>(m + at)),
           vv = __builtin_nontemporal_load(reinterpret_cast<const fv*>(v + at));
        if (RDX > 0) {
#pragma unroll
            for (int r = 0; r < RDX; ++r) {
                const float gd = r < Rdx ? Gdx[(size_t)r * ldgdx + h] : 0.0f;
#pragma unroll
                for (int c = 0; c < COLS; ++c) dacc[r][c] = fmaf(gd, pp[c], dacc[r][c]);
            }
        }
        fv g = fv(0.0f);
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            const float gr = G_LDS ? s_g[(h - h0) * RMAX + r] : (r < R ? G[(size_t)r * ldg + h] : 0.0f);  // wave-uniform: LDS broadcast / scalar load
#pragma unroll
            for (int c = 0; c < COLS; ++c) g[c] = fmaf(gr, xv[r][c], g[c]);
        }
#pragma unroll
        for (int c = 0; c < COLS; ++c) {
            float pk = pp[c], mk = mm[c], vk = vv[c];
            adam_one(pk, g[c], mk, vk, a);
            pp[c] = pk;
            mm[c] = mk;
            vv[c] = vk;
        }
        __builtin_nontemporal_store(pp, reinterpret_cast<fv*>(p + at));
        __builtin_nontemporal_store(mm, reinterpret_cast<fv*>(m + at));
        __builtin_nontemporal_store(vv, reinterpret_cast<fv*>(v + at));
    }
    if (RDX > 0) {
        for (int r = 0; r < Rdx; ++r) *reinterpret_cast<fv*>(part + ((size_t)blockIdx.y * Rdx + r) * K + k0) = dacc[r];
    }
}

// ---- the two big streams of the anchor backward at small batch ----------------------------------------------------------
// dW1 = ghid^T x is a rank-R update of an (H, K) matrix (1 GB at N = 500) and dx = ghid W1 reads that matrix once; with R =
// (world x) batch <= 16 both are pure HBM streams with R FMAs per element, which a 64 x 64-tile GEMM with a K = R
// reduction serves at only ~2.7 TB/s.  One thread owns 4 consecutive columns (one 16-byte access per row).
template <int RMAX>
__global__ __launch_bounds__(256) void lowrank_outer_kernel(const float* __restrict__ G, int ldg, const float* __restrict__ X, int ldx,
                                                            int R, int H, int K, int rows_per_block, float* __restrict__ dW) {
    const long k4 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (k4 >= K) return;
    f32x4 xv[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) xv[r] = r < R ? *reinterpret_cast<const f32x4*>(X + (size_t)r * ldx + k4) : f32x4{0, 0, 0, 0};
    const int h0 = blockIdx.y * rows_per_block, h1 = min(H, h0 + rows_per_block);
    for (int h = h0; h < h1; ++h) {
        f32x4 o = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            const float g = r < R ? G[(size_t)r * ldg + h] : 0.0f;  // wave-uniform: scalar load
#pragma unroll
            for (int c = 0; c < 4; ++c) o[c] = fmaf(g, xv[r][c], o[c]);
        }
        __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(dW + (size_t)h * K + k4));
    }
}

// part[chunk][r][k] = sum_{h in chunk} G[r][h] * W[h][k]
template <int RMAX>
__global__ __launch_bounds__(256) void smallm_nn_kernel(const float* __restrict__ G, int ldg, const float* __restrict__ W, int R, int H,
                                                        int K, int rows_per_chunk, float* __restrict__ part) {
    const long k4 = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (k4 >= K) return;
    f32x4 acc[RMAX];
#pragma unroll
    for (int r = 0; r < RMAX; ++r) acc[r] = f32x4{0, 0, 0, 0};
    const int h0 = blockIdx.y * rows_per_chunk, h1 = min(H, h0 + rows_per_chunk);
#pragma unroll 2
    for (int h = h0; h < h1; ++h) {
        const f32x4 wv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(W + (size_t)h * K + k4));
#pragma unroll
        for (int r = 0; r < RMAX; ++r) {
            const float g = r < R ? G[(size_t)r * ldg + h] : 0.0f;
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[r][c] = fmaf(g, wv[c], acc[r][c]);
        }
    }
    for (int r = 0; r < R; ++r) *reinterpret_cast<f32x4*>(part + ((size_t)blockIdx.y * R + r) * K + k4) = acc[r];
}

__global__ __launch_bounds__(256) void smallm_finish_kernel(const float* __restrict__ part, int chunks, int R, int K, float* __restrict__ Y,
                                                            long ldy, int accumulate) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)R * K) return;
    const int r = (int)(i / K);
    const long k = i - (long)r * K;
    float s = 0.0f;
    for (int c = 0; c < chunks; ++c) s += part[((size_t)c * R + r) * K + k];
    float* y = Y + (size_t)r * ldy + k;
    *y = accumulate ? *y + s : s;
}

}  // namespace shasta

using namespace shasta;

// d_dyn (device, 6 floats, or NULL): when given, lr, betas and step are ignored - the kernels read lr / bc1, 1 / sqrt(bc2) and the betas
// from it (shasta_adam_prepare_f32 writes them from a device-side step counter and {lr, beta1, beta2} once per optimizer step)
static AdamArgs make_adam_args(double lr, double beta1, double beta2, float eps, float weight_decay, int step, const float* d_dyn) {
    const double s = step >= 1 ? (double)step : 1.0;
    const double bc1 = 1.0 - pow(beta1, s), bc2 = 1.0 - pow(beta2, s);
    AdamArgs a;
    a.lr_over_bc1 = (float)(lr / bc1);
    a.beta1 = (float)beta1;
    a.beta2 = (float)beta2;
    a.one_minus_beta1 = (float)(1.0 - beta1);
    a.one_minus_beta2 = (float)(1.0 - beta2);
    a.eps = eps;
    a.weight_decay = weight_decay;
    a.rsqrt_bc2 = (float)(1.0 / sqrt(bc2));
    a.dyn = d_dyn;
    return a;
}

extern "C" int shasta_adam_prepare_f32(int* d_step, const double* d_hyper, float* d_dyn, shasta_stream_t stream) {
    SHASTA_REQUIRE(d_step && d_hyper && d_dyn, "adam_prepare: null pointer");
    hipLaunchKernelGGL(adam_prepare_kernel, dim3(1), dim3(1), 0, as_stream(stream), d_step, d_hyper, d_dyn);
    return check_launch("adam_prepare");
}

extern "C" int shasta_adam_step_f32(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, double lr, double beta1,
                                    double beta2, float eps, float weight_decay, int step, const float* d_dyn, shasta_stream_t stream) {
    SHASTA_REQUIRE(param && grad && exp_avg && exp_avg_sq && n >= 0 && (step >= 1 || d_dyn), "adam_step: bad argument");
    SHASTA_REQUIRE((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0,
                   "adam_step: tensors must be 16-byte aligned");
    if (n == 0) return SHASTA_OK;
    const AdamArgs a = make_adam_args(lr, beta1, beta2, eps, weight_decay, step, d_dyn);
    const long blocks = std::min<long>((n / 4 + 255) / 256 + 1, 256L * 16);
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), param, grad, exp_avg, exp_avg_sq, n, a);
    return check_launch("adam_step");
}

extern "C" int shasta_adam_multi_f32(int count, float* const* param, const float* const* grad, float* const* exp_avg,
                                     float* const* exp_avg_sq, const long* n, double lr, double beta1, double beta2, float eps,
                                     float weight_decay, int step, const float* d_dyn, shasta_stream_t stream) {
    SHASTA_REQUIRE(count >= 0 && (step >= 1 || d_dyn) && (count == 0 || (param && grad && exp_avg && exp_avg_sq && n)), "adam_multi: bad argument");
    const AdamArgs a = make_adam_args(lr, beta1, beta2, eps, weight_decay, step, d_dyn);
    for (int k0 = 0; k0 < count; k0 += ADAM_MULTI) {
        AdamMulti t;
        const int c = std::min(ADAM_MULTI, count - k0);
        long nmax = 0;
        for (int k = 0; k < ADAM_MULTI; ++k) {
            const int j = k0 + std::min(k, c - 1);  // (unused slots repeat the last tensor with n = 0)
            SHASTA_REQUIRE(param[j] && grad[j] && exp_avg[j] && exp_avg_sq[j] && n[j] >= 0, "adam_multi: null tensor");
            t.p[k] = param[j]; t.g[k] = grad[j]; t.m[k] = exp_avg[j]; t.v[k] = exp_avg_sq[j];
            t.n[k] = k < c ? n[j] : 0;
            nmax = std::max(nmax, t.n[k]);
        }
        if (nmax == 0) continue;
        const unsigned bx = (unsigned)std::min<long>((nmax + 255) / 256, 64);
        hipLaunchKernelGGL(adam_multi_kernel, dim3(bx, c), dim3(256), 0, as_stream(stream), t, a);
        int rc = check_launch("adam_multi");
        if (rc) return rc;
    }
    return SHASTA_OK;
}

namespace {
// the grid of adam_lowrank_kernel at `cols` columns per thread: kblocks x chunks workgroups, chunk = rows_per_block rows of the matrix
struct AdamLowrankPlan {
    int kblocks, chunks, rows_per_block;
};
AdamLowrankPlan adam_lowrank_plan(int H, int K, int cols) {
    AdamLowrankPlan p;
    p.kblocks = cdiv(K / cols, 256);
    p.rows_per_block = std::max(1, std::min(64, cdiv(H, std::max(1, 4096 / p.kblocks))));  // >= ~4096 workgroups, <= 64 rows each
    p.chunks = cdiv(H, p.rows_per_block);
    return p;
}
}  // namespace

extern "C" size_t shasta_adam_lowrank_dx_workspace_bytes(int H, int K, int Rdx) {
    if (H <= 0 || K <= 0 || Rdx <= 0) return 0;
    const int chunks = std::max(adam_lowrank_plan(H, K, 4).chunks, adam_lowrank_plan(H, K, 2).chunks);
    return (size_t)chunks * Rdx * K * sizeof(float);  // (4 columns per thread up to rank 16, 2 above)
}

extern "C" int shasta_adam_lowrank_dx_f32(float* param, float* exp_avg, float* exp_avg_sq, int H, int K, const float* G, int ldg, const float* X,
                                          int ldx, int R, const float* Gdx, int ldgdx, int Rdx, float* Y, long ldy, int accumulate, void* workspace,
                                          size_t workspace_bytes, double lr, double beta1, double beta2, float eps, float weight_decay, int step,
                                          const float* d_dyn, shasta_stream_t stream) {
    SHASTA_REQUIRE(param && exp_avg && exp_avg_sq && G && X && Gdx && Y && workspace && H >= 1 && K >= 4 && (step >= 1 || d_dyn), "adam_lowrank_dx: bad argument");
    SHASTA_REQUIRE(R >= 1 && R <= 64 && Rdx >= 1 && Rdx <= 16, "adam_lowrank_dx: 1 <= R <= 64, 1 <= Rdx <= 16");
    SHASTA_REQUIRE(K % 4 == 0 && ldx % 4 == 0 && ldg >= H && ldx >= K && ldgdx >= H, "adam_lowrank_dx: K and ldx multiples of 4, ldg, ldgdx >= H, ldx >= K");
    SHASTA_REQUIRE((((uintptr_t)param | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)X | (uintptr_t)workspace) & 15) == 0,
                   "adam_lowrank_dx: 16-byte alignment");
    if (workspace_bytes < shasta_adam_lowrank_dx_workspace_bytes(H, K, Rdx)) {
        set_error_msg("adam_lowrank_dx: workspace too small");
        return SHASTA_E_WORKSPACE;
    }
    const AdamArgs a = make_adam_args(lr, beta1, beta2, eps, weight_decay, step, d_dyn);
    const AdamLowrankPlan pl = adam_lowrank_plan(H, K, R <= 16 ? 4 : 2);
    float* part = static_cast<float*>(workspace);
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(pl.kblocks, pl.chunks), dim3(256), 0, as_stream(stream), param, exp_avg, exp_avg_sq, G, ldg, X, ldx, R, H, K,
                           pl.rows_per_block, a, Gdx, ldgdx, Rdx, part);
    };
    if (R <= 8) Rdx <= 8 ? launch(adam_lowrank_kernel<8, 4, 8>) : launch(adam_lowrank_kernel<8, 4, 16>);
    else if (R <= 16) Rdx <= 8 ? launch(adam_lowrank_kernel<16, 4, 8>) : launch(adam_lowrank_kernel<16, 4, 16>);
    else if (R <= 32) Rdx <= 8 ? launch(adam_lowrank_kernel<32, 2, 8>) : launch(adam_lowrank_kernel<32, 2, 16>);
    else Rdx <= 8 ? launch(adam_lowrank_kernel<64, 2, 8>) : launch(adam_lowrank_kernel<64, 2, 16>);
    int rc = check_launch("adam_lowrank_dx");
    if (rc) return rc;
    hipLaunchKernelGGL(smallm_finish_kernel, dim3((unsigned)(((long)Rdx * K + 255) / 256)), dim3(256), 0, as_stream(stream), part, pl.chunks, Rdx, K,
                       Y, ldy, accumulate);
    return check_launch("adam_lowrank_dx finish");
}

extern "C" int shasta_adam_lowrank_f32(float* param, float* exp_avg, float* exp_avg_sq, int H, int K, const float* G, int ldg, const float* X,
                                       int ldx, int R, double lr, double beta1, double beta2, float eps, float weight_decay, int step,
                                       const float* d_dyn, shasta_stream_t stream) {
    SHASTA_REQUIRE(param && exp_avg && exp_avg_sq && G && X && H >= 0 && K >= 0 && (step >= 1 || d_dyn), "adam_lowrank: bad argument");
    SHASTA_REQUIRE(R >= 1 && R <= 64, "adam_lowrank: 1 <= R <= 64 (frame-pairs of a step over all ranks)");
    SHASTA_REQUIRE(K % 4 == 0 && ldx % 4 == 0 && ldg >= H && ldx >= K, "adam_lowrank: K and ldx multiples of 4, ldg >= H, ldx >= K");
    SHASTA_REQUIRE((((uintptr_t)param | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)X) & 15) == 0, "adam_lowrank: 16-byte alignment");
    if (H == 0 || K == 0) return SHASTA_OK;
    const AdamArgs a = make_adam_args(lr, beta1, beta2, eps, weight_decay, step, d_dyn);
    auto launch = [&](auto kern, int cols) {
        const AdamLowrankPlan pl = adam_lowrank_plan(H, K, cols);
        hipLaunchKernelGGL(kern, dim3(pl.kblocks, pl.chunks), dim3(256), 0, as_stream(stream), param, exp_avg, exp_avg_sq, G, ldg, X, ldx, R, H, K,
                           pl.rows_per_block, a, (const float*)nullptr, 0, 0, (float*)nullptr);
    };
    // Columns per thread.  Large matrices (the 2000 x 128000 first layers at N = 500): 4 up to rank 16, 2 above (1.10 ms per matrix at
    // R = 8; one column at R = 64: 1.31 -> 1.37 ms).  Small ones (the car configuration's 450 x 28800): fewer columns = more workgroups
    // and, above rank 32, half the registers for the X rows - 0.072 -> 0.063 ms at R = 8, 0.069 -> 0.063 at R = 32, 0.113 -> 0.092 at
    // R = 64 (two columns at R = 16: 0.056 -> 0.21, the scalar loads of G then bound it: kept at 4).  Same arithmetic per element.
    const bool small = (long)H * K <= (1L << 26);
    if (R <= 8) small ? launch(adam_lowrank_kernel<8, 2>, 2) : launch(adam_lowrank_kernel<8, 4>, 4);
    else if (R <= 16) launch(adam_lowrank_kernel<16, 4>, 4);
    else if (R <= 32) small ? launch(adam_lowrank_kernel<32, 1>, 1) : launch(adam_lowrank_kernel<32, 2>, 2);
    else small ? launch(adam_lowrank_kernel<64, 1>, 1) : launch(adam_lowrank_kernel<64, 2>, 2);
    return check_launch("adam_lowrank");
}

extern "C" int shasta_lowrank_outer_f32(const float* G, int ldg, const float* X, int ldx, int R, int H, int K, float* dW,
                                        shasta_stream_t stream) {
    SHASTA_REQUIRE(G && X && dW && R >= 1 && R <= 16 && H >= 0 && K >= 0, "lowrank_outer: bad argument (1 <= R <= 16)");
    SHASTA_REQUIRE(K % 4 == 0 && ldx % 4 == 0 && (((uintptr_t)X | (uintptr_t)dW) & 15) == 0, "lowrank_outer: K, ldx multiples of 4, 16-byte aligned");
    if (H == 0 || K == 0) return SHASTA_OK;
    const int kblocks = cdiv(K / 4, 256);
    const int rpb = std::max(1, std::min(64, cdiv(H, std::max(1, 2048 / kblocks))));  // >= ~2048 workgroups, <= 64 rows each
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(kblocks, cdiv(H, rpb)), dim3(256), 0, as_stream(stream), G, ldg, X, ldx, R, H, K, rpb, dW);
    };
    if (R <= 4) launch(lowrank_outer_kernel<4>);
    else if (R <= 8) launch(lowrank_outer_kernel<8>);
    else launch(lowrank_outer_kernel<16>);
    return check_launch("lowrank_outer");
}

namespace {
// the grid of smallm_nn_kernel: kblocks x chunks workgroups, chunk = rows_per_chunk rows of W.  The workspace is sized for ws_chunks,
// the chunk count before the rows per chunk are rounded up (>= chunks); the query also answers for H < 1 and K < 4 as for 1 and 4.
struct SmallmPlan {
    int kblocks, chunks, rows_per_chunk, ws_chunks;
};
SmallmPlan smallm_nn_plan(int H, int K) {
    H = std::max(H, 1);
    SmallmPlan p;
    p.kblocks = cdiv(std::max(K, 4) / 4, 256);
    p.ws_chunks = std::max(1, std::min(cdiv(H, 64), cdiv(2048, p.kblocks)));
    p.rows_per_chunk = cdiv(H, p.ws_chunks);
    p.chunks = cdiv(H, p.rows_per_chunk);
    return p;
}
}  // namespace

extern "C" size_t shasta_smallm_nn_workspace_bytes(int R, int H, int K) {
    return (size_t)smallm_nn_plan(H, K).ws_chunks * std::max(R, 1) * std::max(K, 4) * sizeof(float);
}

extern "C" int shasta_smallm_nn_f32(const float* G, int ldg, const float* W, int R, int H, int K, float* Y, long ldy, int accumulate,
                                    void* workspace, size_t workspace_bytes, shasta_stream_t stream) {
    SHASTA_REQUIRE(G && W && Y && workspace && R >= 1 && R <= 16 && H >= 1 && K >= 4, "smallm_nn: bad argument (1 <= R <= 16)");
    SHASTA_REQUIRE(K % 4 == 0 && (((uintptr_t)W | (uintptr_t)workspace) & 15) == 0, "smallm_nn: K multiple of 4, 16-byte aligned");
    if (workspace_bytes < shasta_smallm_nn_workspace_bytes(R, H, K)) {
        set_error_msg("smallm_nn: workspace too small");
        return SHASTA_E_WORKSPACE;
    }
    const SmallmPlan pl = smallm_nn_plan(H, K);
    float* part = static_cast<float*>(workspace);
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(pl.kblocks, pl.chunks), dim3(256), 0, as_stream(stream), G, ldg, W, R, H, K, pl.rows_per_chunk, part);
    };
    if (R <= 4) launch(smallm_nn_kernel<4>);
    else if (R <= 8) launch(smallm_nn_kernel<8>);
    else launch(smallm_nn_kernel<16>);
    int rc = check_launch("smallm_nn");
    if (rc) return rc;
    hipLaunchKernelGGL(smallm_finish_kernel, dim3((unsigned)(((long)R * K + 255) / 256)), dim3(256), 0, as_stream(stream), part, pl.chunks, R, K, Y,
                       ldy, accumulate);
    return check_launch("smallm_finish");
}
