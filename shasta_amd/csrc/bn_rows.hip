// The sparse backbone in train() mode: BatchNorm1d with BATCH statistics over the feature rows of one level (tools/nusc_shasta/train.py:184-193
// freezes backbone and neck but leaves them in train() mode, so every BatchNorm1d of SpMiddleResNetFHD normalises with the statistics of
// the current batch and updates its running statistics).  A layer is four calls:
//   y = sum_t W_t x + bias          shasta_spconv_layer_f32 (sparse_conv.hip, unchanged) on a RAW pack: alpha = 1, beta' = bias
//   mean, M2 of y                   bn_rows_stats_kernel + bn_rows_combine_kernel
//   stat, running statistics        bn_rows_finalize_kernel
//   out = relu?(bn(y) + residual?)  bn_rows_apply_kernel
// y is (n, C) fp32 rows, C = 16, 32, 64 or 128 (the backbone's widths).
//
// STATISTICS follow bn_stats_kernel of shared_conv_train.hip: per channel sum and sum of squares in float64 (the square of an fp32 value
// is exact in float64), one partial per workgroup, combined by ONE workgroup in a fixed tree.  No float atomics: the same bits on every
// run.  A workgroup of 256 threads = 256 / C row groups x C channels takes a contiguous slice of rows; thread (g, c) adds rows
// beg + g, beg + g + G, .. of channel c in order, the G group sums are then added in order.  The slices: at least BNR_ROWS_MIN rows each,
// BNR_SLICES at most (both ends are seams: n below one slice, n where the slice count saturates; a slice may be empty - per = ceil(n /
// slices) can leave the last workgroups without rows - and then contributes exact zeros).
#include "bn_finalize.hpp"

namespace shasta {

constexpr int BNR_SLICES = 512;    // workgroups (and partials) of the statistics pass at most
constexpr int BNR_ROWS_MIN = 64;   // rows per slice at least: below BNR_SLICES * BNR_ROWS_MIN rows the slice count follows n

static bool bnr_channels_ok(int C) { return C == 16 || C == 32 || C == 64 || C == 128; }
static int bnr_slices(long n) {
    const long s = (n + BNR_ROWS_MIN - 1) / BNR_ROWS_MIN;
    return (int)(s < 1 ? 1 : s > BNR_SLICES ? BNR_SLICES : s);
}

// part: [slice][2][C] float64 = sum y, sum y^2 of the slice's rows
template <int C>
__global__ __launch_bounds__(256) void bn_rows_stats_kernel(const float* __restrict__ y, long n, double* __restrict__ part) {
    constexpr int G = 256 / C;
    __shared__ double red[2][G][C];
    const int c = threadIdx.x % C, g = threadIdx.x / C;
    const long per = (n + gridDim.x - 1) / gridDim.x, beg = blockIdx.x * per, end = min(n, beg + per);
    double s = 0.0, ss = 0.0;
    // eight rows' loads in flight, then the adds in the rows' order (the same sums as a row at a time)
    for (long p0 = beg + g; p0 < end; p0 += 8 * G) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = y[min(p0 + G * u, end - 1) * C + c];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (p0 + G * u < end) {
                const double v = (double)t[u];
                s += v;
                ss += v * v;
            }
        }
    }
    red[0][g][c] = s;
    red[1][g][c] = ss;
    __syncthreads();
    if (g == 0) {
        double a = red[0][0][c], b = red[1][0][c];
#pragma unroll
        for (int j = 1; j < G; ++j) {
            a += red[0][j][c];
            b += red[1][j][c];
        }
        part[((size_t)blockIdx.x * 2 + 0) * C + c] = a;
        part[((size_t)blockIdx.x * 2 + 1) * C + c] = b;
    }
}

// ONE workgroup of 1024 threads = 1024 / C groups x C channels: thread (g, c) adds the slices g, g + G, .. of channel c in order, the G
// group sums are then added in order.  mean_m2[0:C] = mean, [C:2C] = sum of squared deviations from it (>= 0).
template <int C>
__global__ __launch_bounds__(1024) void bn_rows_combine_kernel(const double* __restrict__ part, int nslice, long n, float* __restrict__ mean_m2) {
    constexpr int G = 1024 / C;
    __shared__ double red[2][G][C];
    const int c = threadIdx.x % C, g = threadIdx.x / C;
    double s = 0.0, ss = 0.0;
    for (int i0 = g; i0 < nslice; i0 += 8 * G) {  // (eight slices' loads in flight: the adds keep their order)
        double t[8][2];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = min(i0 + G * u, nslice - 1);
            t[u][0] = part[((size_t)i * 2 + 0) * C + c];
            t[u][1] = part[((size_t)i * 2 + 1) * C + c];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (i0 + G * u < nslice) {
                s += t[u][0];
                ss += t[u][1];
            }
        }
    }
    red[0][g][c] = s;
    red[1][g][c] = ss;
    __syncthreads();
    if (g == 0) {
        double a = red[0][0][c], b = red[1][0][c];
        for (int j = 1; j < G; ++j) {
            a += red[0][j][c];
            b += red[1][j][c];
        }
        const double mean = a / (double)n;
        const double m2 = b - a * mean;
        mean_m2[c] = (float)mean;
        mean_m2[C + c] = (float)(m2 > 0.0 ? m2 : 0.0);
    }
}

// mean / M2 / n of the whole batch -> stat and the running statistics as nn.BatchNorm1d keeps them (bn_finalize.hpp)
__global__ __launch_bounds__(128) void bn_rows_finalize_kernel(const float* __restrict__ mean_m2, int C, double n, float eps, float momentum,
                                                               float* __restrict__ stat, float* __restrict__ running_mean,
                                                               float* __restrict__ running_var, long* __restrict__ nbt) {
    const int c = threadIdx.x;
    if (c >= C) return;
    bn_finalize_channel(mean_m2, C, c, n, eps, momentum, stat, running_mean, running_var);
    if (nbt && c == 0) nbt[0] += 1;
}

// out = relu?(((y - mean) invstd) gamma + beta + residual?), four channels per thread: a row is C / 4 consecutive threads, a workgroup
// pass 1024 / C rows.  Every element is read (y, residual) and written (out) by the same thread: out may alias y or residual.
__global__ __launch_bounds__(256) void bn_rows_apply_kernel(const float* y, long n4, int C, const float* __restrict__ stat,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            const float* residual, int relu, float* out) {
    const int c4 = (threadIdx.x % (C / 4)) * 4;
    float mean[4], inv[4], ga[4], be[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        mean[j] = stat[c4 + j];
        inv[j] = stat[C + c4 + j];
        ga[j] = gamma[c4 + j];
        be[j] = beta[c4 + j];
    }
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {  // i % (C / 4) == threadIdx.x % (C / 4)
        const f32x4 v = reinterpret_cast<const f32x4*>(y)[i];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = ((v[j] - mean[j]) * inv[j]) * ga[j] + be[j];
        if (residual) {
            const f32x4 r = reinterpret_cast<const f32x4*>(residual)[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] += r[j];
        }
        if (relu) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = relu_nan(o[j]);
        }
        reinterpret_cast<f32x4*>(out)[i] = o;
    }
}

// the packed layer of sparse_conv.hip ([tap][cin_pad][Cout] weights, alpha[Cout], beta'[Cout]) with alpha = 1, beta' = bias
__global__ void sp_pack_raw_kernel(const float* __restrict__ w, const float* __restrict__ bias, int Cin, int cin_pad, int Cout, int K, long total,
                                   float* __restrict__ out) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    for (long e = tid; e < total; e += nth) {
        const int co = (int)(e % Cout);
        const int c = (int)((e / Cout) % cin_pad);
        const int tap = (int)(e / Cout / cin_pad);
        out[e] = c < Cin ? w[((size_t)co * K + tap) * Cin + c] : 0.0f;  // (Cout, kD, kH, kW, Cin)
    }
    for (long n = tid; n < Cout; n += nth) {
        out[total + n] = 1.0f;
        out[total + Cout + n] = bias ? bias[n] : 0.0f;
    }
}

}  // namespace shasta

using namespace shasta;

extern "C" int shasta_spconv_layer_pack_raw_f32(const float* weight, const float* bias, int Cin, int Cout, int K, void* packed,
                                                size_t packed_bytes, shasta_stream_t stream) {
    SHASTA_REQUIRE(weight && packed, "spconv_layer_pack_raw: null pointer");
    const size_t need = shasta_spconv_layer_packed_bytes(Cin, Cout, K);  // 0: a layer sparse_conv.hip does not serve
    if (need == 0) {
        set_error_msg("spconv_layer_pack_raw: Cin <= 8, 16, 32, 64 or 128; Cout 16, 32, 64 or 128; 1, 3, 9 or 27 taps");
        return SHASTA_E_UNSUPPORTED;
    }
    if ((uintptr_t)packed % 16) {
        set_error_msg("spconv_layer_pack_raw: packed buffer must be 16-byte aligned");
        return SHASTA_E_ALIGN;
    }
    if (packed_bytes < need) {
        set_error_msg("spconv_layer_pack_raw: packed buffer too small");
        return SHASTA_E_WORKSPACE;
    }
    const long total = (long)(need / sizeof(float)) - 2 * Cout;  // K * cin_pad * Cout
    const int cin_pad = (int)(total / ((long)K * Cout));
    hipLaunchKernelGGL(sp_pack_raw_kernel, dim3(128), dim3(256), 0, as_stream(stream), weight, bias, Cin, cin_pad, Cout, K, total,
                       static_cast<float*>(packed));
    return check_launch("spconv_layer_pack_raw");
}

extern "C" int shasta_bn_rows_supported(int C) { return bnr_channels_ok(C) ? 1 : 0; }

extern "C" size_t shasta_bn_rows_workspace_bytes(int C) { return bnr_channels_ok(C) ? (size_t)BNR_SLICES * 2 * C * sizeof(double) : 0; }

#define BNR_REQUIRE_CHANNELS(C, what)                                          \
    do {                                                                       \
        if (!bnr_channels_ok(C)) {                                             \
            set_error_msg(what ": rows of 16, 32, 64 or 128 channels only");   \
            return SHASTA_E_UNSUPPORTED;                                       \
        }                                                                      \
    } while (0)

extern "C" int shasta_bn_rows_stats_f32(const float* y, long n, int C, float* mean_m2, void* workspace, size_t workspace_bytes,
                                        shasta_stream_t stream) {
    BNR_REQUIRE_CHANNELS(C, "bn_rows_stats");
    SHASTA_REQUIRE(y && mean_m2 && workspace && n > 0, "bn_rows_stats: null pointer or no rows");
    if ((uintptr_t)workspace % 8) {
        set_error_msg("bn_rows_stats: workspace must be 8-byte aligned");
        return SHASTA_E_ALIGN;
    }
    if (workspace_bytes < shasta_bn_rows_workspace_bytes(C)) {
        set_error_msg("bn_rows_stats: workspace too small");
        return SHASTA_E_WORKSPACE;
    }
    const int ns = bnr_slices(n);
    double* part = static_cast<double*>(workspace);
    hipStream_t st = as_stream(stream);
#define BNR_STATS(CC)                                                                                          \
    do {                                                                                                       \
        hipLaunchKernelGGL(bn_rows_stats_kernel<CC>, dim3(ns), dim3(256), 0, st, y, n, part);                  \
        hipLaunchKernelGGL(bn_rows_combine_kernel<CC>, dim3(1), dim3(1024), 0, st, part, ns, n, mean_m2);      \
    } while (0)
    if (C == 16) BNR_STATS(16);
    else if (C == 32) BNR_STATS(32);
    else if (C == 64) BNR_STATS(64);
    else BNR_STATS(128);
#undef BNR_STATS
    return check_launch("bn_rows_stats");
}

extern "C" int shasta_bn_rows_finalize_f32(const float* mean_m2, int C, double n, float eps, float momentum, float* stat, float* running_mean,
                                           float* running_var, long* num_batches_tracked, shasta_stream_t stream) {
    BNR_REQUIRE_CHANNELS(C, "bn_rows_finalize");
    SHASTA_REQUIRE(mean_m2 && stat && n >= 1.0, "bn_rows_finalize: null pointer or n < 1");
    hipLaunchKernelGGL(bn_rows_finalize_kernel, dim3(1), dim3(128), 0, as_stream(stream), mean_m2, C, n, eps, momentum, stat, running_mean,
                       running_var, num_batches_tracked);
    return check_launch("bn_rows_finalize");
}

extern "C" int shasta_bn_rows_apply_f32(const float* y, long n, int C, const float* stat, const float* gamma, const float* beta,
                                        const float* residual, int relu, float* out, shasta_stream_t stream) {
    BNR_REQUIRE_CHANNELS(C, "bn_rows_apply");
    SHASTA_REQUIRE(y && stat && gamma && beta && out && n > 0, "bn_rows_apply: null pointer or no rows");
    if (((uintptr_t)y | (uintptr_t)out | (uintptr_t)residual) % 16) {
        set_error_msg("bn_rows_apply: y, residual and out must be 16-byte aligned");
        return SHASTA_E_ALIGN;
    }
    const long n4 = n * (C / 4);
    const long blocks = (n4 + 255) / 256;
    hipLaunchKernelGGL(bn_rows_apply_kernel, dim3((unsigned)(blocks > 8192 ? 8192 : blocks)), dim3(256), 0, as_stream(stream), y, n4, C, stat,
                       gamma, beta, residual, relu, out);
    return check_launch("bn_rows_apply");
}
