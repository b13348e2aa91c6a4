// Training path (SURVEY.md 8(a) row 19 / BASELINE config 5): auxiliary kernels of the backward pass.
// The dense layers run on the strided matrix-core GEMM (gemm_f32.hip: Y = X W^T, dX = dY W, dW = dY^T X); this file holds
// what is not a GEMM: the factorised first layer of the pair MLPs and its transpose (the cat/expand of
// det3d/models/tracker/shasta.py:286-313 and their autograd), the hand-designed residual and its gradient (:277-283), the
// combine's gradient (:319), the loss and its gradient, the two softmax backward passes (:324-325), bias-gradient column sums and
// |x| backward.  The (B, T*D, 2F) pair tensor of the reference is not materialised; the narrow hidden activations
// of each pair are.  All reductions have a fixed order.  (The optimizer: adam.hip; the gather's scatter-add: bev_gather_bwd.hip.)
#include <algorithm>
#include <math.h>

#include "common.hpp"

namespace shasta {

// red[k][0] = sum over the 256 threads of red[k][tid], k < K, as a tree: offsets 128 ... 1, a barrier per level (the order is part of the
// results).  Every thread of the block calls it after writing its red[k][tid]; the sums may be read on return.
template <int K, int ROWS>
__device__ __forceinline__ void block_sum_256(float (&red)[ROWS][256], int tid) {
    static_assert(K <= ROWS, "block_sum_256: more sums than rows");
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off)
#pragma unroll
            for (int k = 0; k < K; ++k) red[k][tid] += red[k][tid + off];
        __syncthreads();
    }
}

// ---- factorised first layer of the pair MLPs ---------------------------------------------------------------------------
// W0 . [prev_t ; cur_d] + b0 = UP[t] + UC[d] (pair_layout.hpp): the hidden activations of every pair are
//   H[(b,t,d)][j] = relu(UP[(b,t)][j] + UC[(b,d)][j]),
// and the gradient of the pre-activation Z folds back onto the table rows by two fixed-order sums,
//   gUP[(b,t)][j] = sum_d gZ[(b,t,d)][j],   gUC[(b,d)][j] = sum_t gZ[(b,t,d)][j],
// after which dW0, db0 and the table gradients are small GEMMs over B*T rows instead of B*T*D pairs.
__global__ __launch_bounds__(256) void pair_hidden_kernel(const float* __restrict__ UP, int ldp, const float* __restrict__ UC, int ldc,
                                                          int T, int D, int E, long total, float* __restrict__ H) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;  // element (b,t,d,j)
    if (i >= total) return;
    const int j = i % E;
    const long pr = i / E;
    const int d = pr % D;
    const long bt = pr / D;
    const long b = bt / T;
    H[i] = fmaxf(UP[bt * ldp + j] + UC[(b * D + d) * ldc + j], 0.0f);
}

// block = (row r of side `which`, batch b); threads = E columns x G row groups
__global__ __launch_bounds__(256) void pair_reduce_kernel(const float* __restrict__ gZ, int T, int D, int E, int EP,
                                                          float* __restrict__ gUP, float* __restrict__ gUC) {
    __shared__ float red[256];
    const int which = blockIdx.y, b = blockIdx.z, r = blockIdx.x;
    const int j = threadIdx.x % EP, q = threadIdx.x / EP, G = 256 / EP;
    const int n = which == 0 ? D : T;
    float s = 0.0f;
    if (j < E) {
        if (which == 0)
            for (int d = q; d < n; d += G) s += gZ[(((size_t)b * T + r) * D + d) * E + j];
        else
            for (int t = q; t < n; t += G) s += gZ[(((size_t)b * T + t) * D + r) * E + j];
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (q == 0 && j < E) {
        float t = 0.0f;
        for (int k = 0; k < G; ++k) t += red[k * EP + j];
        (which == 0 ? gUP : gUC)[((size_t)b * (which == 0 ? T : D) + r) * E + j] = t;
    }
}

// ---- hand-designed residual (shasta.py:277-283), materialised, and its gradient w.r.t. the box tables -------------
// squared distance of two box rows over their first nf entries
__device__ __forceinline__ float box_dist2(const float* p, const float* q, int nf) {
    float d2 = 0.0f;
    for (int k = 0; k < nf; ++k) {
        const float df = p[k] - q[k];
        d2 += df * df;
    }
    return d2;
}
// `denom` has two (B, D) halves: the column norms ||d2[b, :, d]|| written by the forward, and behind them the column sums
// gs[b, d] = sum_t g[b,t,d] * d2[b,t,d] that the backward writes for the normalisation's gradient
__device__ __forceinline__ size_t denom_norm_at(int b, int d, int D) { return (size_t)b * D + d; }
__device__ __forceinline__ size_t denom_gs_at(int B, int b, int d, int D) { return (size_t)B * D + (size_t)b * D + d; }

__device__ __forceinline__ float hand_pair(const float* p, const float* q, int nf, float den) {
    const float dim = (fabsf(logf(p[3] + 1e-10f) - logf(q[3] + 1e-10f)) + fabsf(logf(p[4] + 1e-10f) - logf(q[4] + 1e-10f))) +
                      fabsf(logf(p[5] + 1e-10f) - logf(q[5] + 1e-10f));
    const float dc = cosf(p[6]) - cosf(q[6]), ds = sinf(p[6]) - sinf(q[6]);
    return (box_dist2(p, q, nf) / den + dim) + sqrtf(dc * dc + ds * ds);
}

// one block per (b, d): column norm, then dist[b, :, d]
__global__ __launch_bounds__(256) void hand_dist_fwd_kernel(const float* __restrict__ prev_tab, const float* __restrict__ det_tab,
                                                            int T, int D, int nf, float* __restrict__ dist, int ld,
                                                            float* __restrict__ denom) {
    __shared__ float red[1][256];
    const int d = blockIdx.x, b = blockIdx.y;
    const float* q = det_tab + ((size_t)b * D + d) * 8;
    float ssq = 0.0f;
    for (int t = threadIdx.x; t < T; t += 256) {
        const float d2 = box_dist2(prev_tab + ((size_t)b * T + t) * 8, q, nf);
        ssq += d2 * d2;
    }
    red[0][threadIdx.x] = ssq;
    block_sum_256<1>(red, threadIdx.x);
    const float den = fmaxf(sqrtf(red[0][0]), 1e-12f);
    if (threadIdx.x == 0) denom[denom_norm_at(b, d, D)] = den;
    for (int t = threadIdx.x; t < T; t += 256)
        dist[((size_t)b * T + t) * ld + d] = hand_pair(prev_tab + ((size_t)b * T + t) * 8, q, nf, den);
}

// gradient of dist w.r.t. box rows; one block per (b, side, row) where side 0 = previous table row t, 1 = detection row d.
// Only rows listed by the caller are evaluated (the anchor rows N, N+1: real boxes are inputs without gradient).
__global__ __launch_bounds__(256) void hand_dist_bwd_kernel(const float* __restrict__ gdist, int ldg,
                                                            const float* __restrict__ prev_tab, const float* __restrict__ det_tab,
                                                            const float* __restrict__ denom, int B, int T, int D, int nf, int row0,
                                                            float* __restrict__ dprev_tab, float* __restrict__ ddet_tab) {
    __shared__ float red[8][256];
    const int side = blockIdx.y, b = blockIdx.z, r = row0 + blockIdx.x;
    float acc[7] = {0, 0, 0, 0, 0, 0, 0};
    const int n = side == 0 ? D : T;
    for (int o = threadIdx.x; o < n; o += 256) {
        const int t = side == 0 ? r : o, d = side == 0 ? o : r;
        const float* p = prev_tab + ((size_t)b * T + t) * 8;
        const float* q = det_tab + ((size_t)b * D + d) * 8;
        const float den = denom[denom_norm_at(b, d, D)];
        const float g = gdist[((size_t)b * T + t) * ldg + d];
        // d2 term incl. the normalisation: r = d2/den, den = ||d2[:,d]|| -> dr/dd2[t] = 1/den - d2[t]*S/den^3 with
        // S = gs[b,d] = sum_t' g[t',d]*d2[t',d], the column sums of hand_gs_kernel
        const float d2 = box_dist2(p, q, nf);
        const float gs = denom[denom_gs_at(B, b, d, D)];
        const float gd2 = den > 1e-12f ? g / den - gs * d2 / (den * den * den) : g / den;
        const float sgn = side == 0 ? 1.0f : -1.0f;
        for (int k = 0; k < nf; ++k) acc[k] += sgn * gd2 * 2.0f * (p[k] - q[k]);
        for (int k = 3; k < 6; ++k) {
            const float lp = logf(p[k] + 1e-10f), lq = logf(q[k] + 1e-10f);
            const float s = lp > lq ? 1.0f : (lp < lq ? -1.0f : 0.0f);
            acc[k] += side == 0 ? g * s / (p[k] + 1e-10f) : -g * s / (q[k] + 1e-10f);
        }
        const float cp = cosf(p[6]), sp = sinf(p[6]), cq = cosf(q[6]), sq = sinf(q[6]);
        const float dc = cp - cq, ds = sp - sq, rot = sqrtf(dc * dc + ds * ds);
        if (side == 0) acc[6] += g * (dc * (-sp) + ds * cp) / rot;
        else acc[6] += g * (dc * sq - ds * cq) / rot;
    }
    for (int k = 0; k < 7; ++k) red[k][threadIdx.x] = acc[k];
    block_sum_256<7>(red, threadIdx.x);
    if (threadIdx.x < 7) {
        float* o = side == 0 ? dprev_tab + ((size_t)b * T + r) * 8 : ddet_tab + ((size_t)b * D + r) * 8;
        o[threadIdx.x] += red[threadIdx.x][0];
    }
}

// gs[b,d] = sum_t g[b,t,d] * d2[b,t,d]  (column sums needed by the normalisation's gradient), stored behind the norms in denom
__global__ __launch_bounds__(256) void hand_gs_kernel(const float* __restrict__ gdist, int ldg, const float* __restrict__ prev_tab,
                                                      const float* __restrict__ det_tab, int T, int D, int nf, int B,
                                                      float* __restrict__ denom) {
    __shared__ float red[1][256];
    const int d = blockIdx.x, b = blockIdx.y;
    const float* q = det_tab + ((size_t)b * D + d) * 8;
    float s = 0.0f;
    for (int t = threadIdx.x; t < T; t += 256) s += gdist[((size_t)b * T + t) * ldg + d] * box_dist2(prev_tab + ((size_t)b * T + t) * 8, q, nf);
    red[0][threadIdx.x] = s;
    block_sum_256<1>(red, threadIdx.x);
    if (threadIdx.x == 0) denom[denom_gs_at(B, b, d, D)] = red[0][0];
}

// ---- combine (shasta.py:319) ------------------------------------------------------------------------------------------
// residual = alpha*fused + beta*dist + omega*shape ; coeff (P, ldc>=3), fused (P), shape (P), dist/residual (B,T,ld)
__global__ void combine_bwd_kernel(const float* __restrict__ gres, const float* __restrict__ coeff, int ldc,
                                   const float* __restrict__ fused, int ldf, const float* __restrict__ shape, int lds_,
                                   const float* __restrict__ dist, int D, int ld, long P, float* __restrict__ gcoeff,
                                   float* __restrict__ gfused, float* __restrict__ gshape, float* __restrict__ gdist) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const int d = i % D;
    const long bt = i / D;
    const float g = gres[bt * ld + d];
    const float a = coeff[i * ldc], be = coeff[i * ldc + 1], om = coeff[i * ldc + 2];
    gcoeff[i * ldc] = g * fused[i * ldf];
    gcoeff[i * ldc + 1] = g * dist[bt * ld + d];
    gcoeff[i * ldc + 2] = g * shape[i * lds_];
    for (int c = 3; c < ldc; ++c) gcoeff[i * ldc + c] = 0.0f;
    gfused[i * ldf] = g * a;
    for (int c = 1; c < ldf; ++c) gfused[i * ldf + c] = 0.0f;
    gshape[i * lds_] = g * om;
    for (int c = 1; c < lds_; ++c) gshape[i * lds_ + c] = 0.0f;
    gdist[bt * ld + d] = g * be;
}

// ---- the training loss (tools/nusc_shasta/train.py:200-211) and its gradient ------------------------------------------------
//   loss = (sum(gt1 . -log(m1 + 1e-10)) / sum(gt1) + sum(gt2 . -log(m2 + 1e-10)) / sum(gt2)) / 2,  gt1 = gt[:, :N, :], gt2 = gt[:, :, :N]
//   (each quotient only where its sum(gt) > 0: train.py:208-209)
// one block per row (b, t) of gt: the four sums of the row in a fixed order; loss_finish_kernel adds the rows in order.
__global__ __launch_bounds__(256) void loss_rows_kernel(const float* __restrict__ m1, const float* __restrict__ m2, const float* __restrict__ gt,
                                                        int N, float* __restrict__ part) {
    __shared__ float red[4][256];
    const int T = N + 2, t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const float* g = gt + ((size_t)b * T + t) * T;
    float s1 = 0.0f, c1 = 0.0f, s2 = 0.0f, c2 = 0.0f;
    for (int d = tid; d < T; d += 256) {
        const float w = g[d];
        if (t < N) {
            s1 = fmaf(w, -logf(m1[((size_t)b * N + t) * T + d] + 1e-10f), s1);
            c1 += w;
        }
        if (d < N) {
            s2 = fmaf(w, -logf(m2[((size_t)b * T + t) * N + d] + 1e-10f), s2);
            c2 += w;
        }
    }
    red[0][tid] = s1; red[1][tid] = c1; red[2][tid] = s2; red[3][tid] = c2;
    block_sum_256<4>(red, tid);
    if (tid < 4) part[((size_t)b * T + t) * 4 + tid] = red[tid][0];
}

// sums[0..3] = (s1, c1, s2, c2) over all rows, sums[4] = the loss
__global__ __launch_bounds__(256) void loss_finish_kernel(const float* __restrict__ part, int rows, float* __restrict__ sums) {
    __shared__ float red[4][64];
    const int k = threadIdx.x & 3, q = threadIdx.x >> 2;
    float s = 0.0f;
#pragma unroll 8
    for (int r = q; r < rows; r += 64) s += part[(size_t)r * 4 + k];
    red[k][q] = s;
    __syncthreads();
    if (threadIdx.x < 4) {
        float t = 0.0f;
        for (int j = 0; j < 64; ++j) t += red[threadIdx.x][j];
        sums[threadIdx.x] = t;
    }
    __syncthreads();
    // (train.py:208-209: a direction without a single ground-truth entry contributes its plain sum - zero - not 0 / 0)
    if (threadIdx.x == 0) sums[4] = ((sums[1] > 0.0f ? sums[0] / sums[1] : sums[0]) + (sums[3] > 0.0f ? sums[2] / sums[3] : sums[2])) * 0.5f;
}

// g1 = dloss/dm1 = -gt1 / (m1 + 1e-10) * gloss / (2 sum(gt1)), g2 likewise; gloss read from device memory
__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ m1, const float* __restrict__ m2, const float* __restrict__ gt,
                                                       const float* __restrict__ sums, const float* __restrict__ gloss, int N, long n1,
                                                       float* __restrict__ g1, float* __restrict__ g2) {
    const int T = N + 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n1) return;
    const float gl = gloss[0] * 0.5f;
    {  // element i of m1 (B, N, T)
        const int d = i % T;
        const long bt = i / T;
        const long b = bt / N;
        const int t = bt - b * N;
        g1[i] = -gt[((size_t)b * T + t) * T + d] / (m1[i] + 1e-10f) * (sums[1] > 0.0f ? gl / sums[1] : gl);
    }
    {  // element i of m2 (B, T, N): the same count
        const int d = i % N;
        const long bt = i / N;
        g2[i] = -gt[(size_t)bt * T + d] / (m2[i] + 1e-10f) * (sums[3] > 0.0f ? gl / sums[3] : gl);
    }
}

// ---- softmax backward (shasta.py:324-325): gmatched = rows-part + cols-part ------------------------------------------
// rows t < N: gz = m1 * (g1 - sum_d g1*m1) over the D entries ; cols d < N: gz = m2 * (g2 - sum_t g2*m2) over the T entries
__global__ __launch_bounds__(256) void softmax_bwd_rows_kernel(const float* __restrict__ m1, const float* __restrict__ g1, int B,
                                                               int N, int T, int D, int ld, float* __restrict__ gm) {
    const int lane = threadIdx.x & 63;
    const int item = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= B * T) return;
    const int b = item / T, t = item % T;
    float* o = gm + ((size_t)b * T + t) * ld;
    if (t >= N) {
        for (int d = lane; d < D; d += 64) o[d] = 0.0f;
        return;
    }
    const float* m = m1 + ((size_t)b * N + t) * D;
    const float* g = g1 + ((size_t)b * N + t) * D;
    float s = 0.0f;
    for (int d = lane; d < D; d += 64) s += g[d] * m[d];
    s = wave_sum(s);
    for (int d = lane; d < D; d += 64) o[d] = m[d] * (g[d] - s);
}

__global__ __launch_bounds__(256) void softmax_bwd_cols_kernel(const float* __restrict__ m2, const float* __restrict__ g2, int N,
                                                               int T, int ld, float* __restrict__ gm) {
    __shared__ float red[4][64];
    const int b = blockIdx.y, dl = threadIdx.x & 63, tq = threadIdx.x >> 6;
    const int d = blockIdx.x * 64 + dl;
    const int dc = min(d, N - 1);
    const float* m = m2 + (size_t)b * T * N + dc;
    const float* g = g2 + (size_t)b * T * N + dc;
    float s = 0.0f;
    // eight rows' loads in flight, the products added in the rows' order (the same sum as a row at a time: a loop of one dependent
    // load pair per step was latency bound - 77 us at N = 500 x 8 frame pairs on 64 workgroups)
    for (int t0 = tq; t0 < T; t0 += 32) {
        float tg[8], tm[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const size_t t = (size_t)min(t0 + 4 * u, T - 1);
            tg[u] = g[t * N];
            tm[u] = m[t * N];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (t0 + 4 * u < T) s += tg[u] * tm[u];
    }
    red[tq][dl] = s;
    __syncthreads();
    s = (red[0][dl] + red[1][dl]) + (red[2][dl] + red[3][dl]);
    if (d >= N) return;
    for (int t0 = tq; t0 < T; t0 += 16) {
        float tg[4], tm[4], to[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const size_t t = (size_t)min(t0 + 4 * u, T - 1);
            tg[u] = g[t * N];
            tm[u] = m[t * N];
            to[u] = gm[((size_t)b * T + t) * ld + d];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (t0 + 4 * u < T) gm[((size_t)b * T + t0 + 4 * u) * ld + d] = to[u] + tm[u] * (tg[u] - s);
    }
}

// ---- small helpers ------------------------------------------------------------------------------------------------------
// out[n] = sum_m Y[m][n] (bias gradient): block (x: 64 columns, y: row chunk) sums its rows in a fixed order into
// part[chunk][n]; a second launch adds the chunks in order (single chunk: written directly).  Deterministic.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ Y, int ldy, int M, int N, int rows_per_chunk,
                                                     float* __restrict__ out) {
    __shared__ float red[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), q = threadIdx.x >> 6;
    const int m0 = blockIdx.y * rows_per_chunk, m1 = min(M, m0 + rows_per_chunk);
    float s0 = 0.0f, s1 = 0.0f;
    if (c < N) {
        int m = m0 + q;
        for (; m + 4 < m1; m += 8) {
            s0 += Y[(size_t)m * ldy + c];
            s1 += Y[(size_t)(m + 4) * ldy + c];
        }
        if (m < m1) s0 += Y[(size_t)m * ldy + c];
    }
    red[q][threadIdx.x & 63] = s0 + s1;
    __syncthreads();
    if (q == 0 && c < N)
        out[(size_t)blockIdx.y * N + c] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// narrow matrices (N < 64): one wave per row chunk would idle most lanes, so lanes split the rows instead: lane l of a
// 256-thread block owns column l % NP and every (256/NP)-th row of the chunk
__global__ __launch_bounds__(256) void colsum_narrow_kernel(const float* __restrict__ Y, int ldy, int M, int N, int NP,
                                                            int rows_per_chunk, float* __restrict__ out) {
    __shared__ float red[256];
    const int c = threadIdx.x % NP, q = threadIdx.x / NP, nq = 256 / NP;
    const int m0 = blockIdx.y * rows_per_chunk, m1 = min(M, m0 + rows_per_chunk);
    float s = 0.0f;
    if (c < N)
        for (int m = m0 + q; m < m1; m += nq) s += Y[(size_t)m * ldy + c];
    red[threadIdx.x] = s;
    __syncthreads();
    if (q == 0 && c < N) {
        float t = 0.0f;
        for (int k = 0; k < nq; ++k) t += red[k * NP + c];
        out[(size_t)blockIdx.y * N + c] = t;
    }
}

// one wave per column: lanes stride over the chunks, then a fixed-order wave reduction
__global__ __launch_bounds__(256) void colsum_finish_kernel(const float* __restrict__ part, int chunks, int N, float* __restrict__ out) {
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (c >= N) return;
    float s = 0.0f;
    for (int k = lane; k < chunks; k += 64) s += part[(size_t)k * N + c];
    s = wave_sum(s);
    if (lane == 0) out[c] = s;
}

// y = |x| (mode 0) ; g_out = g * sign(x) (mode 1) over `cols` columns of each row, columns [c0, c1) only (others copied / passed)
__global__ void abs_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ out, long n, int cols,
                           int c0, int c1, int mode) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int c = i % cols;
    const bool in = c >= c0 && c < c1;
    if (mode == 0) out[i] = in ? fabsf(x[i]) : x[i];
    else out[i] = in ? (x[i] > 0.0f ? g[i] : (x[i] < 0.0f ? -g[i] : 0.0f)) : g[i];
}

__global__ void scale_kernel(float* __restrict__ x, long n, float alpha) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= alpha;
}

}  // namespace shasta

using namespace shasta;

extern "C" int shasta_pair_hidden_f32(const float* UP, int ldp, const float* UC, int ldc, int B, int T, int D, int E, float* H,
                                      shasta_stream_t stream) {
    SHASTA_REQUIRE(UP && UC && H && E >= 1 && ldp >= E && ldc >= E, "pair_hidden: bad argument");
    const long total = (long)B * T * D * E;
    if (total == 0) return SHASTA_OK;
    SHASTA_REQUIRE((total + 255) / 256 < (1L << 31), "pair_hidden: too many pairs");
    hipLaunchKernelGGL(pair_hidden_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream), UP, ldp, UC, ldc, T, D, E,
                       total, H);
    return check_launch("pair_hidden");
}

extern "C" int shasta_pair_reduce_f32(const float* gZ, int B, int T, int D, int E, float* gUP, float* gUC, shasta_stream_t stream) {
    SHASTA_REQUIRE(gZ && gUP && gUC && E >= 1 && E <= 256 && T == D, "pair_reduce: bad argument (E <= 256, T == D)");
    if (B == 0 || T == 0) return SHASTA_OK;
    int EP = 1;
    while (EP < E) EP *= 2;
    hipLaunchKernelGGL(pair_reduce_kernel, dim3(T, 2, B), dim3(256), 0, as_stream(stream), gZ, T, D, E, EP, gUP, gUC);
    return check_launch("pair_reduce");
}

extern "C" int shasta_hand_dist_f32(const float* prev_tab, const float* det_tab, int B, int T, int D, int nf, float* dist, int ld,
                                    float* denom, shasta_stream_t stream) {
    SHASTA_REQUIRE(prev_tab && det_tab && dist && denom, "hand_dist: null pointer");
    if (B == 0) return SHASTA_OK;
    hipLaunchKernelGGL(hand_dist_fwd_kernel, dim3(D, B), dim3(256), 0, as_stream(stream), prev_tab, det_tab, T, D, nf, dist, ld, denom);
    return check_launch("hand_dist_fwd");
}

// denom must have room for 2*B*D floats (norms, then the column sums written here)
extern "C" int shasta_hand_dist_bwd_f32(const float* gdist, int ldg, const float* prev_tab, const float* det_tab, float* denom, int B,
                                        int T, int D, int nf, int row0, int nrows, float* dprev_tab, float* ddet_tab,
                                        shasta_stream_t stream) {
    SHASTA_REQUIRE(gdist && prev_tab && det_tab && denom && dprev_tab && ddet_tab, "hand_dist_bwd: null pointer");
    if (B == 0 || nrows == 0) return SHASTA_OK;
    hipLaunchKernelGGL(hand_gs_kernel, dim3(D, B), dim3(256), 0, as_stream(stream), gdist, ldg, prev_tab, det_tab, T, D, nf, B, denom);
    int rc = check_launch("hand_gs");
    if (rc) return rc;
    hipLaunchKernelGGL(hand_dist_bwd_kernel, dim3(nrows, 2, B), dim3(256), 0, as_stream(stream), gdist, ldg, prev_tab, det_tab, denom,
                       B, T, D, nf, row0, dprev_tab, ddet_tab);
    return check_launch("hand_dist_bwd");
}

extern "C" int shasta_combine_bwd_f32(const float* gres, const float* coeff, int ldc, const float* fused, int ldf, const float* shape,
                                      int lds_, const float* dist, int B, int T, int D, int ld, float* gcoeff, float* gfused,
                                      float* gshape, float* gdist, shasta_stream_t stream) {
    SHASTA_REQUIRE(gres && coeff && fused && shape && dist && gcoeff && gfused && gshape && gdist && ldc >= 3, "combine_bwd: bad argument");
    const long P = (long)B * T * D;
    if (P == 0) return SHASTA_OK;
    hipLaunchKernelGGL(combine_bwd_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, as_stream(stream), gres, coeff, ldc, fused,
                       ldf, shape, lds_, dist, D, ld, P, gcoeff, gfused, gshape, gdist);
    return check_launch("combine_bwd");
}

extern "C" int shasta_affinity_loss_f32(const float* m1, const float* m2, const float* gt, int B, int N, float* ws, float* sums,
                                        shasta_stream_t stream) {
    SHASTA_REQUIRE(m1 && m2 && gt && ws && sums && B > 0 && N > 0, "affinity_loss: bad argument");
    hipLaunchKernelGGL(loss_rows_kernel, dim3(N + 2, B), dim3(256), 0, as_stream(stream), m1, m2, gt, N, ws);
    int rc = check_launch("affinity_loss rows");
    if (rc) return rc;
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, as_stream(stream), ws, B * (N + 2), sums);
    return check_launch("affinity_loss");
}

extern "C" int shasta_affinity_loss_bwd_f32(const float* m1, const float* m2, const float* gt, const float* sums, const float* gloss, int B,
                                            int N, float* g1, float* g2, shasta_stream_t stream) {
    SHASTA_REQUIRE(m1 && m2 && gt && sums && gloss && g1 && g2 && B > 0 && N > 0, "affinity_loss_bwd: bad argument");
    const long n1 = (long)B * N * (N + 2);
    hipLaunchKernelGGL(loss_bwd_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, as_stream(stream), m1, m2, gt, sums, gloss, N, n1, g1,
                       g2);
    return check_launch("affinity_loss_bwd");
}

extern "C" int shasta_softmax_bwd_f32(const float* m1, const float* g1, const float* m2, const float* g2, int B, int N, float* gmatched,
                                      int ld, shasta_stream_t stream) {
    SHASTA_REQUIRE(m1 && g1 && m2 && g2 && gmatched && ld >= N + 2, "softmax_bwd: bad argument");
    if (B == 0) return SHASTA_OK;
    const int T = N + 2, D = N + 2;
    hipLaunchKernelGGL(softmax_bwd_rows_kernel, dim3(cdiv(B * T, 4)), dim3(256), 0, as_stream(stream), m1, g1, B, N, T, D, ld, gmatched);
    int rc = check_launch("softmax_bwd_rows");
    if (rc) return rc;
    hipLaunchKernelGGL(softmax_bwd_cols_kernel, dim3(cdiv(N, 64), B), dim3(256), 0, as_stream(stream), m2, g2, N, T, ld, gmatched);
    return check_launch("softmax_bwd_cols");
}

extern "C" int shasta_colsum_f32(const float* Y, int ldy, int M, int N, float* out, float* ws, size_t ws_bytes,
                                 shasta_stream_t stream) {
    SHASTA_REQUIRE(Y && out && M >= 0 && N >= 0, "colsum: bad argument");
    if (N == 0) return SHASTA_OK;
    // row chunks: enough blocks to fill the chip, at least 64 rows each, bounded by the scratch the caller gave
    const int colblocks = N >= 64 ? cdiv(N, 64) : 1;
    int chunks = std::min(std::max(1, 1024 / colblocks), std::max(1, M / 64));
    if (!ws) chunks = 1;
    else chunks = (int)std::min<size_t>((size_t)chunks, ws_bytes / (sizeof(float) * (size_t)N));
    chunks = std::max(chunks, 1);
    const int rpc = cdiv(std::max(M, 1), chunks);
    chunks = cdiv(std::max(M, 1), rpc);
    float* dst = chunks == 1 ? out : ws;
    if (N >= 64) {
        hipLaunchKernelGGL(colsum_kernel, dim3(colblocks, chunks), dim3(256), 0, as_stream(stream), Y, ldy, M, N, rpc, dst);
    } else {
        int NP = 1;
        while (NP < N) NP *= 2;
        hipLaunchKernelGGL(colsum_narrow_kernel, dim3(1, chunks), dim3(256), 0, as_stream(stream), Y, ldy, M, N, NP, rpc, dst);
    }
    int rc = check_launch("colsum");
    if (rc || chunks == 1) return rc;
    hipLaunchKernelGGL(colsum_finish_kernel, dim3(cdiv(N, 4)), dim3(256), 0, as_stream(stream), ws, chunks, N, out);
    return check_launch("colsum_finish");
}

extern "C" int shasta_abs_f32(const float* x, const float* g, float* out, long n, int cols, int c0, int c1, int backward,
                              shasta_stream_t stream) {
    SHASTA_REQUIRE(x && out && cols > 0 && (!backward || g), "abs: bad argument");
    if (n == 0) return SHASTA_OK;
    hipLaunchKernelGGL(abs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), x, g, out, n, cols, c0, c1,
                       backward ? 1 : 0);
    return check_launch("abs");
}

extern "C" int shasta_scale_f32(float* x, long n, float alpha, shasta_stream_t stream) {
    SHASTA_REQUIRE(x && n >= 0, "scale: bad argument");
    if (n == 0) return SHASTA_OK;
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, as_stream(stream), x, n, alpha);
    return check_launch("scale");
}
