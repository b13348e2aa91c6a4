// K0: shared_conv of the affinity network (det3d/models/tracker/shasta.py:42-47, applied :223-228):
//   Conv2d(Cin -> 64, 3x3, padding 1, bias) -> BatchNorm2d(64) in eval mode -> ReLU -> permute to NHWC.
// Input: the neck output (B, Cin, H, W) fp32 NCHW (Cin = 512, H = W = 180 in the shipped configs); output
// (B, H, W, 64) fp32 NHWC = example['bev_feature'].  19.1 GFLOP per map: the largest dense op of a real nuScenes forward.
//
// The convolution bodies of conv3x3_f32.hpp with the pixels as the MFMA's A operand: M = pixels, N = 64 output channels, K = Cin*9;
// a lane of the epilogue owns one channel of 16 pixels.  Weights are pre-packed once as [chunk of 8 channels][k = c_local*9 + tap][n];
// BatchNorm is applied in the epilogue exactly as PyTorch's eval kernel does: y = (acc + bias) * alpha + beta',
// alpha = gamma / sqrt(var + eps), beta' = beta - mean * alpha.
// grid.z runs over the images of BOTH maps of a frame pair (current: z < B, previous: z >= B), so one launch fills the chip with
// twice as many workgroups (a 180 x 180 map in the flattened-pixel form is exactly one wave per SIMD, a pair two).
#include "conv3x3_f32.hpp"

namespace shasta {

// packed layout: [Cin/8][72][64] weights, then alpha[64], beta'[64], bias[64], then [192] = 1.0 for a RAW pack (conv + bias, no BN, no ReLU)
__global__ void shared_conv_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias,
                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                        const float* __restrict__ mean, const float* __restrict__ var, float eps, int Cin,
                                        float* __restrict__ out, int raw) {
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, nth = gridDim.x * blockDim.x;
    const int total = Cin * 9 * 64;
    for (int e = tid; e < total; e += nth) {
        const int n = e & 63, k = (e >> 6) % 72, chunk = (e >> 6) / 72;
        const int c = chunk * 8 + k / 9, tap = k % 9;
        out[e] = w[((size_t)n * Cin + c) * 9 + tap];
    }
    for (int n = tid; n < 64; n += nth) {
        const float alpha = raw ? 1.0f : bn_alpha(var[n], eps, gamma[n]);
        out[total + n] = alpha;
        out[total + 64 + n] = raw ? 0.0f : beta[n] - mean[n] * alpha;
        out[total + 128 + n] = bias[n];
        if (n == 0) out[total + 192] = raw ? 1.0f : 0.0f;
    }
}

// the map, image and output of workgroup z
struct K0Map {
    const float* x;
    float* out;
    int b;
};
__device__ __forceinline__ K0Map k0_map(const float* xa, const float* xb, float* outa, float* outb, int B) {
    const bool second = (int)blockIdx.z >= B;
    return {second ? xb : xa, second ? outb : outa, second ? (int)blockIdx.z - B : (int)blockIdx.z};
}

// D[pixel][channel]: the lane's channels (lane & 31) and 32 + (lane & 31) of pixels first + mfma32_row(r, h) < limit of the NHWC rows at o
__device__ __forceinline__ void k0_epilogue(const f32x16& acc0, const f32x16& acc1, const float* par, float* o, int first, int limit) {
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const bool raw = par[192] != 0.0f;  // uniform
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        const int chn = 32 * nb + (lane & 31);
        const float alpha = par[chn], beta2 = par[64 + chn], bias = par[128 + chn];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int px = first + mfma32_row(r, h);
            if (px < limit) {
                const float a = nb ? acc1[r] : acc0[r];
                const float v = (a + bias) * alpha + beta2;
                o[(size_t)px * 64 + chn] = raw ? v : relu_nan(v);
            }
        }
    }
}

// maps wider than 256 columns: the rectangular form, wave w owns 32 pixels of row y0 + w
__global__ __launch_bounds__(256) void shared_conv_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                          const float* __restrict__ packed, float* __restrict__ outa,
                                                          float* __restrict__ outb, int B, int Cin, int H, int W) {
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x0 = blockIdx.x * CONV_TC, y0 = blockIdx.y * CONV_TR;
    const K0Map m = k0_map(xa, xb, outa, outb, B);
    f32x16 acc0, acc1;
    conv_body<true, 1>(ConvRectTile<0>(x0, y0), m.x + (size_t)m.b * Cin * H * W, packed, Cin, H, W, Cin / 8, acc0, acc1);
    const int gy = y0 + wv;
    if (gy >= H) return;
    k0_epilogue(acc0, acc1, packed + (size_t)Cin * 9 * 64, m.out + (((size_t)m.b * H + gy) * W) * 64, x0, W);
}

// the flattened-pixel form: one load chunk ahead (two or three workgroups per CU cover the latency)
template <int IN_PT>
__global__ __launch_bounds__(256) void shared_conv_flat_kernel(const float* __restrict__ xa, const float* __restrict__ xb,
                                                               const float* __restrict__ packed, float* __restrict__ outa,
                                                               float* __restrict__ outb, int B, int Cin, int H, int W) {
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int npix = H * W;
    const K0Map m = k0_map(xa, xb, outa, outb, B);
    f32x16 acc0, acc1;
    conv_body<true, 1>(ConvFlatTile<IN_PT>(H, W), m.x + (size_t)m.b * Cin * npix, packed, Cin, H, W, Cin / 4, acc0, acc1);
    k0_epilogue(acc0, acc1, packed + (size_t)Cin * 9 * 64, m.out + (size_t)m.b * npix * 64, blockIdx.x * 128 + 32 * wv, npix);
}

}  // namespace shasta

using namespace shasta;

extern "C" size_t shasta_shared_conv_packed_bytes(int in_channels) {
    if (in_channels <= 0 || in_channels % 8) return 0;
    return ((size_t)in_channels * 9 * 64 + 256) * sizeof(float);
}

extern "C" int shasta_shared_conv_pack_f32(const float* weight, const float* bias, const float* bn_weight,
                                           const float* bn_bias, const float* bn_mean, const float* bn_var, float bn_eps,
                                           int in_channels, void* packed, size_t packed_bytes, shasta_stream_t stream) {
    SHASTA_REQUIRE(weight && bias && bn_weight && bn_bias && bn_mean && bn_var && packed, "shared_conv_pack: null pointer");
    SHASTA_REQUIRE(in_channels > 0 && in_channels % 8 == 0, "shared_conv: in_channels must be a multiple of 8");
    SHASTA_REQUIRE((uintptr_t)packed % 16 == 0, "shared_conv_pack: packed buffer must be 16-byte aligned");
    if (packed_bytes < shasta_shared_conv_packed_bytes(in_channels)) {
        set_error_msg("shared_conv_pack: packed buffer too small");
        return SHASTA_E_WORKSPACE;
    }
    hipLaunchKernelGGL(shared_conv_pack_kernel, dim3(256), dim3(256), 0, as_stream(stream), weight, bias, bn_weight, bn_bias,
                       bn_mean, bn_var, bn_eps, in_channels, static_cast<float*>(packed), 0);
    return check_launch("shared_conv_pack");
}

extern "C" int shasta_shared_conv_pack_raw_f32(const float* weight, const float* bias, int in_channels, void* packed, size_t packed_bytes,
                                               shasta_stream_t stream) {
    SHASTA_REQUIRE(weight && bias && packed, "shared_conv_pack_raw: null pointer");
    SHASTA_REQUIRE(in_channels > 0 && in_channels % 8 == 0, "shared_conv_pack_raw: in_channels must be a multiple of 8");
    SHASTA_REQUIRE((uintptr_t)packed % 16 == 0, "shared_conv_pack_raw: packed buffer must be 16-byte aligned");
    if (packed_bytes < shasta_shared_conv_packed_bytes(in_channels)) {
        set_error_msg("shared_conv_pack_raw: packed buffer too small");
        return SHASTA_E_WORKSPACE;
    }
    hipLaunchKernelGGL(shared_conv_pack_kernel, dim3(256), dim3(256), 0, as_stream(stream), weight, bias, nullptr, nullptr, nullptr, nullptr,
                       0.0f, in_channels, static_cast<float*>(packed), 1);
    return check_launch("shared_conv_pack_raw");
}

extern "C" int shasta_shared_conv_f32(const float* x, const float* x_prev, int B, int in_channels, int H, int W,
                                      const void* packed, float* out, float* out_prev, shasta_stream_t stream) {
    SHASTA_REQUIRE(x && packed && out, "shared_conv: null pointer");
    SHASTA_REQUIRE((x_prev == nullptr) == (out_prev == nullptr), "shared_conv: x_prev and out_prev go together");
    SHASTA_REQUIRE(B >= 0 && H > 0 && W > 0, "shared_conv: bad size");
    SHASTA_REQUIRE(in_channels > 0 && in_channels % 8 == 0, "shared_conv: in_channels must be a multiple of 8");
    SHASTA_REQUIRE((uintptr_t)packed % 16 == 0, "shared_conv: packed buffer must be 16-byte aligned");
    SHASTA_REQUIRE((long)in_channels * H * W < (1L << 31), "shared_conv: one image exceeds 2^31 elements");
    if (B == 0) return SHASTA_OK;
    const int nz = x_prev ? 2 * B : B;
    const float* pk = static_cast<const float*>(packed);
    const ConvFlatPlan plan = conv_flat_plan(H, W);
    if (plan.fits) {
        conv_flat_dispatch(plan.in_pt, [&](auto pt) {
            hipLaunchKernelGGL(shared_conv_flat_kernel<decltype(pt)::value>, dim3(cdiv(H * W, 128), 1, nz), dim3(256), plan.lds,
                               as_stream(stream), x, x_prev, pk, out, out_prev, B, in_channels, H, W);
        });
        return check_launch("shared_conv_flat");
    }
    hipLaunchKernelGGL(shared_conv_kernel, dim3(cdiv(W, CONV_TC), cdiv(H, CONV_TR), nz), dim3(256), 0, as_stream(stream), x, x_prev, pk,
                       out, out_prev, B, in_channels, H, W);
    return check_launch("shared_conv");
}
