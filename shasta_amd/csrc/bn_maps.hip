// The RPN neck in train() mode: BatchNorm2d with BATCH statistics over fp32 NCHW maps (tools/nusc_shasta/train.py:184-193 freezes
// backbone and neck but leaves them in train() mode, so every BatchNorm2d of the neck normalises with the statistics of the current
// batch and updates its running statistics).  A layer is four calls, as in the backbone (bn_rows.hip):
//   y = conv(x)                     shasta_neck_layer_raw_f32 (neck.hip: the eval kernels' RAW instantiation, the same packed weights)
//   mean, M2 of y                   bn_maps_stats_kernel + bn_maps_combine_kernel
//   stat, running statistics        bn_maps_finalize_kernel (bn_finalize.hpp, shared with bn_rows.hip)
//   y = relu?(bn(y)) in place       bn_maps_apply_kernel
// y is addressed like a neck layer's output: (base, B, C, plane = OH * OW, channels_total, channel_offset); channel c of image b is the
// `plane` contiguous floats at ((b * channels_total + channel_offset + c) * plane).  C is a multiple of 32 (every Cout of neck.hip).
//
// STATISTICS: per channel sum and sum of squares in float64 (the square of an fp32 value is exact in float64), one partial per
// workgroup, combined by ONE workgroup in a fixed tree.  No float atomics: the same bits on every run.  The division of the work depends
// on (B, C, plane) only: a plane is cut into bnm_plane_slices(plane) slices of at least BNM_PIX_MIN floats, BNM_SLICES at most (both ends
// are seams; the slice length is rounded up to a multiple of 4, so the last slices of a plane may be short or empty - an empty one
// contributes exact zeros); a workgroup (slice, channel, image) of 256 threads reads its slice in order, thread t the elements (VEC:
// the 16-byte quads) t, t + 256, ..; the 256 thread sums are added in a fixed binary tree.  base is 16-byte aligned, so with
// plane % 4 == 0 every plane and every slice starts on 16 bytes: the VEC form; other planes start on 4 bytes only and take the scalar
// form (the form is a function of plane alone).
#include "bn_finalize.hpp"

namespace shasta {

constexpr int BNM_PIX_MIN = 4096;   // floats per slice at least: below BNM_SLICES * BNM_PIX_MIN floats the slice count follows the plane
constexpr int BNM_SLICES = 16;      // slices (workgroups, partials) of one plane at most
constexpr int BNM_APPLY_SEG = 4096; // floats of a plane per workgroup of the apply pass

static bool bnm_channels_ok(int C) { return C > 0 && C % 32 == 0; }
static int bnm_plane_slices(long plane) {
    const long s = (plane + BNM_PIX_MIN - 1) / BNM_PIX_MIN;
    return (int)(s < 1 ? 1 : s > BNM_SLICES ? BNM_SLICES : s);
}
static long bnm_slice_len(long plane, int slices) { return ((plane + slices - 1) / slices + 3) & ~3L; }

// part: [image * slices + slice][2][C] float64 = sum y, sum y^2 of the slice
template <bool VEC>
__global__ __launch_bounds__(256) void bn_maps_stats_kernel(const float* __restrict__ y, long plane, int C, int ctot, int coff, long per,
                                                            double* __restrict__ part) {
    __shared__ double red[2][256];
    const int t = threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    const float* p = y + ((size_t)b * ctot + coff + c) * plane;
    const long beg = min(plane, (long)blockIdx.x * per), end = min(plane, beg + per);
    double s = 0.0, ss = 0.0;
    if constexpr (VEC) {  // beg and end are multiples of 4
        const f32x4* p4 = reinterpret_cast<const f32x4*>(p + beg);
        const long nq = (end - beg) >> 2;
        for (long q0 = t; q0 < nq; q0 += 4 * 256) {  // four quads' loads in flight, then the adds in the elements' order
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = p4[min(q0 + 256 * u, nq - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (q0 + 256 * u < nq) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double d = (double)v[u][j];
                        s += d;
                        ss += d * d;
                    }
                }
            }
        }
    } else {
        for (long i0 = beg + t; i0 < end; i0 += 8 * 256) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[min(i0 + 256 * u, end - 1)];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (i0 + 256 * u < end) {
                    const double d = (double)v[u];
                    s += d;
                    ss += d * d;
                }
            }
        }
    }
    red[0][t] = s;
    red[1][t] = ss;
    __syncthreads();
#pragma unroll
    for (int o = 128; o >= 1; o >>= 1) {
        if (t < o) {
            red[0][t] += red[0][t + o];
            red[1][t] += red[1][t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        const size_t sl = (size_t)b * gridDim.x + blockIdx.x;
        part[(sl * 2 + 0) * C + c] = red[0][0];
        part[(sl * 2 + 1) * C + c] = red[1][0];
    }
}

// ONE workgroup of 1024 threads = 32 groups x 32 channels, 32 channels at a time: thread (g, c) adds the partials g, g + 32, .. of its
// channel in order, the 32 group sums are then added in order.  mean_m2[0:C] = mean, [C:2C] = sum of squared deviations from it (>= 0).
__global__ __launch_bounds__(1024) void bn_maps_combine_kernel(const double* __restrict__ part, int npart, int C, double n,
                                                               float* __restrict__ mean_m2) {
    __shared__ double red[2][32][32];
    const int cl = threadIdx.x & 31, g = threadIdx.x >> 5;
    for (int c0 = 0; c0 < C; c0 += 32) {
        const int c = c0 + cl;
        double s = 0.0, ss = 0.0;
        for (int i = g; i < npart; i += 32) {
            s += part[((size_t)i * 2 + 0) * C + c];
            ss += part[((size_t)i * 2 + 1) * C + c];
        }
        red[0][g][cl] = s;
        red[1][g][cl] = ss;
        __syncthreads();
        if (g == 0) {
            double a = red[0][0][cl], q = red[1][0][cl];
            for (int j = 1; j < 32; ++j) {
                a += red[0][j][cl];
                q += red[1][j][cl];
            }
            const double mean = a / n;
            const double m2 = q - a * mean;
            mean_m2[c] = (float)mean;
            mean_m2[C + c] = (float)(m2 > 0.0 ? m2 : 0.0);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(128) void bn_maps_finalize_kernel(const float* __restrict__ mean_m2, int C, double n, float eps, float momentum,
                                                               float* __restrict__ stat, float* __restrict__ running_mean,
                                                               float* __restrict__ running_var, long* __restrict__ nbt) {
    const int c = blockIdx.x * 128 + threadIdx.x;
    if (c >= C) return;
    bn_finalize_channel(mean_m2, C, c, n, eps, momentum, stat, running_mean, running_var);
    if (nbt && c == 0) nbt[0] += 1;
}

// y = relu?(((y - mean) invstd) gamma + beta) in place: a workgroup (segment, channel, image) owns BNM_APPLY_SEG floats of one plane;
// every element is read and written by the same thread, nothing outside the slice is touched.
template <bool VEC>
__global__ __launch_bounds__(256) void bn_maps_apply_kernel(float* y, long plane, int C, int ctot, int coff, const float* __restrict__ stat,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta, int relu) {
    const int t = threadIdx.x, c = blockIdx.y, b = blockIdx.z;
    const float mean = stat[c], inv = stat[C + c], ga = gamma[c], be = beta[c];
    const long beg = (long)blockIdx.x * BNM_APPLY_SEG;
    float* p = y + ((size_t)b * ctot + coff + c) * plane + beg;
    const long left = plane - beg;
    if constexpr (VEC) {
        f32x4* p4 = reinterpret_cast<f32x4*>(p);
        const long nq = left >> 2;  // plane % 4 == 0
        f32x4 v[BNM_APPLY_SEG / 1024];
#pragma unroll
        for (int u = 0; u < BNM_APPLY_SEG / 1024; ++u) v[u] = p4[min((long)t + 256 * u, nq - 1)];
#pragma unroll
        for (int u = 0; u < BNM_APPLY_SEG / 1024; ++u) {
            if (t + 256 * u < nq) {
                f32x4 o;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    o[j] = ((v[u][j] - mean) * inv) * ga + be;
                    if (relu) o[j] = relu_nan(o[j]);
                }
                p4[t + 256 * u] = o;
            }
        }
    } else {
#pragma unroll 4
        for (int u = 0; u < BNM_APPLY_SEG / 256; ++u) {
            const long i = t + 256 * u;
            if (i < left) {
                float o = ((p[i] - mean) * inv) * ga + be;
                if (relu) o = relu_nan(o);
                p[i] = o;
            }
        }
    }
}

// the checks every call on a slice shares; 0 or the error code (message set)
static int bnm_check_slice(const char* what_channels, const char* what_arg, const char* what_grid, const char* what_align, const void* y,
                           int B, int C, long plane, int ctot, int coff) {
    if (!bnm_channels_ok(C)) {
        set_error_msg(what_channels);
        return SHASTA_E_UNSUPPORTED;
    }
    if (!(y && B > 0 && plane > 0 && coff >= 0 && ctot > 0 && (long)coff + C <= ctot)) {
        set_error_msg(what_arg);
        return SHASTA_E_ARG;
    }
    if (C > 65535 || B > 65535 || plane >= (1L << 40)) {
        set_error_msg(what_grid);
        return SHASTA_E_UNSUPPORTED;
    }
    if ((uintptr_t)y % 16) {
        set_error_msg(what_align);
        return SHASTA_E_ALIGN;
    }
    return SHASTA_OK;
}

}  // namespace shasta

using namespace shasta;

extern "C" int shasta_bn_maps_supported(int C) { return bnm_channels_ok(C) && C <= 65535 ? 1 : 0; }

extern "C" size_t shasta_bn_maps_workspace_bytes(int B, int C, long plane) {
    if (!bnm_channels_ok(C) || B < 1 || plane < 1) return 0;
    return (size_t)B * bnm_plane_slices(plane) * 2 * C * sizeof(double);
}

extern "C" int shasta_bn_maps_stats_f32(const float* y, int B, int C, long plane, int channels_total, int channel_offset, float* mean_m2,
                                        void* workspace, size_t workspace_bytes, shasta_stream_t stream) {
    const int rc = bnm_check_slice("bn_maps_stats: channel counts that are multiples of 32 only",
                                   "bn_maps_stats: null pointer, no values (B x plane = 0) or a channel slice that leaves the tensor",
                                   "bn_maps_stats: B or C exceeds the grid limit (65535)", "bn_maps_stats: y must be 16-byte aligned", y, B, C, plane,
                                   channels_total, channel_offset);
    if (rc != SHASTA_OK) return rc;
    SHASTA_REQUIRE(mean_m2 && workspace, "bn_maps_stats: null pointer");
    if ((uintptr_t)workspace % 8) {
        set_error_msg("bn_maps_stats: workspace must be 8-byte aligned");
        return SHASTA_E_ALIGN;
    }
    if (workspace_bytes < shasta_bn_maps_workspace_bytes(B, C, plane)) {
        set_error_msg("bn_maps_stats: workspace too small");
        return SHASTA_E_WORKSPACE;
    }
    const int sp = bnm_plane_slices(plane);
    const long per = bnm_slice_len(plane, sp);
    double* part = static_cast<double*>(workspace);
    hipStream_t st = as_stream(stream);
    const dim3 grid(sp, C, B);
    if (plane % 4 == 0)
        hipLaunchKernelGGL(bn_maps_stats_kernel<true>, grid, dim3(256), 0, st, y, plane, C, channels_total, channel_offset, per, part);
    else
        hipLaunchKernelGGL(bn_maps_stats_kernel<false>, grid, dim3(256), 0, st, y, plane, C, channels_total, channel_offset, per, part);
    hipLaunchKernelGGL(bn_maps_combine_kernel, dim3(1), dim3(1024), 0, st, part, B * sp, C, (double)B * (double)plane, mean_m2);
    return check_launch("bn_maps_stats");
}

extern "C" int shasta_bn_maps_finalize_f32(const float* mean_m2, int C, double n, float eps, float momentum, float* stat, float* running_mean,
                                           float* running_var, long* num_batches_tracked, shasta_stream_t stream) {
    if (!shasta_bn_maps_supported(C)) {
        set_error_msg("bn_maps_finalize: channel counts that are multiples of 32 (65535 at most) only");
        return SHASTA_E_UNSUPPORTED;
    }
    SHASTA_REQUIRE(mean_m2 && stat && n >= 1.0, "bn_maps_finalize: null pointer or n < 1");
    hipLaunchKernelGGL(bn_maps_finalize_kernel, dim3(cdiv(C, 128)), dim3(128), 0, as_stream(stream), mean_m2, C, n, eps, momentum, stat,
                       running_mean, running_var, num_batches_tracked);
    return check_launch("bn_maps_finalize");
}

extern "C" int shasta_bn_maps_apply_f32(float* y, int B, int C, long plane, int channels_total, int channel_offset, const float* stat,
                                        const float* gamma, const float* beta, int relu, shasta_stream_t stream) {
    const int rc = bnm_check_slice("bn_maps_apply: channel counts that are multiples of 32 only",
                                   "bn_maps_apply: null pointer, no values (B x plane = 0) or a channel slice that leaves the tensor",
                                   "bn_maps_apply: B or C exceeds the grid limit (65535)", "bn_maps_apply: y must be 16-byte aligned", y, B, C, plane,
                                   channels_total, channel_offset);
    if (rc != SHASTA_OK) return rc;
    SHASTA_REQUIRE(stat && gamma && beta, "bn_maps_apply: null pointer");
    const dim3 grid((unsigned)((plane + BNM_APPLY_SEG - 1) / BNM_APPLY_SEG), C, B);
    hipStream_t st = as_stream(stream);
    if (plane % 4 == 0)
        hipLaunchKernelGGL(bn_maps_apply_kernel<true>, grid, dim3(256), 0, st, y, plane, C, channels_total, channel_offset, stat, gamma, beta, relu);
    else
        hipLaunchKernelGGL(bn_maps_apply_kernel<false>, grid, dim3(256), 0, st, y, plane, C, channels_total, channel_offset, stat, gamma, beta, relu);
    return check_launch("bn_maps_apply");
}
