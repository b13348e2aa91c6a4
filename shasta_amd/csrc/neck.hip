// The RPN neck (det3d/models/necks/rpn.py:24-163) layer by layer: conv / transposed conv (no bias) -> BatchNorm2d in eval mode -> ReLU,
// strict fp32 on v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain per output, fp32 accumulation), NCHW fp32 in and out.  Four kinds:
//   C3S1  Conv2d(3, padding 1)                 (also ZeroPad2d(1) + Conv2d(3, stride 1))     out H x W
//   C3S2  ZeroPad2d(1) + Conv2d(3, stride 2)                                                 out H/2 x W/2 (H, W even)
//   C1    ConvTranspose2d(k 1, s 1) = 1x1 convolution, weight (Cin, Cout, 1, 1)              out H x W
//   D2    ConvTranspose2d(k 2, s 2): out[co, 2y+dy, 2x+dx] = sum_ci x[ci, y, x] w[ci, co, dy, dx]   out 2H x 2W
// The output is addressed by (out, out_channels_total, out_channel_offset): the deblocks write their halves of the concatenated
// (B, 512, H, W) result in place.  No atomics: the same bits on every run.
//
// The convolution bodies of conv3x3_f32.hpp with the pixels as the MFMA's B operand: M = output channels (the A operand, from the packed
// weights), N = pixels along x, K = Cin x taps.  Lanes run along x, so every accumulator register of a half-wave stores 128 contiguous
// bytes of one output channel's row (D2: every second float of a 256-byte stretch).  A workgroup owns 64 output channels x 4 rows x
// 32 columns of the "pixel domain" (output pixels for C3S1 / C3S2 / C1, input pixels for D2, where a workgroup also owns ONE of the four
// (dy, dx) sub-pixel positions: grid.z runs over image x [sub-pixel] x 64-channel block); C3S1 on maps up to 256 columns wide (every
// shipped layer: 11 of the neck's 14 layers, 115 of its 126 GFLOP per map): 128 consecutive pixels of the flattened image - in NCHW
// a run of flattened pixels is as contiguous as a row - on a grid that fits the chip: 64 pixel groups x 4 channel blocks = 256 workgroups
// for the 256-channel layers at 90 x 90, 254 x 2 = 508 for the 128-channel layers at 180 x 180 (256 CUs; the rectangular tiling gives 276
// and 540: a second, nearly empty round of workgroups).
//
//                          CK   LDS bytes (2 buffers)   MFMAs / wave / chunk   VGPR + AGPR   waves / SIMD   (compiler's resource report;
//   C3S1 (W > 256)          8   49 920                  72                     117 + 48      3               no scratch in any kernel)
//   C3S2                    4   37 152                  36                     119 + 48      3
//   C1 / D2                32   49 152                  32                     106 + 48      3
//   C3S1 flat (W <= 256)    4   2048 IN_PT + 18 432     36                     IN_PT 8: 97 + 32 (3), 12: 120 + 32 (3), 14: 132 + 32 (3),
//     (IN_PT by map width: W = 90 -> 8, W = 180 -> 12)                         16: 145 + 32 (2), 18: 159 + 32 (2)
// Every kernel has a second, RAW instantiation for train() mode (shasta_neck_layer_raw_f32: the accumulator stored as it is, bn_maps.hip
// takes the batch statistics and normalises afterwards): the same registers and waves per SIMD, C1 / D2 112 + 48 (3), no scratch.
//
// Packed layer: [virtual 64-channel block vb][Cin rounded up to CK][tap][64] weights (a straight copy per chunk; channels >= Cout and
// >= Cin are zeros), then alpha[Cout rounded up to 64], beta'[same]: alpha = gamma / sqrt(var + eps), beta' = beta - mean * alpha,
// y = relu(acc * alpha + beta') - the formula of shared_conv.hip's epilogue.  vb = block for the convolutions, (dy*2+dx) * blocks + block for D2.
#include "conv3x3_f32.hpp"

namespace shasta {

constexpr int NK_KINDS = 4;  // SHASTA_NECK_C3S1 .. SHASTA_NECK_D2 = ConvRectTile's KIND

static int neck_ck(int kind) { return kind == 0 ? 8 : kind == 1 ? 4 : 32; }
static int neck_taps(int kind) { return kind <= 1 ? 9 : 1; }
static int neck_cin_pad(int kind, int Cin) { return cdiv(Cin, neck_ck(kind)) * neck_ck(kind); }
static int neck_blocks(int kind, int Cout) { return cdiv(Cout, 64) * (kind == 3 ? 4 : 1); }
static size_t neck_weight_floats(int kind, int Cin, int Cout) {
    return (size_t)neck_blocks(kind, Cout) * neck_cin_pad(kind, Cin) * neck_taps(kind) * 64;
}

__global__ void neck_pack_kernel(const float* __restrict__ w, const float* __restrict__ gamma, const float* __restrict__ beta,
                                 const float* __restrict__ mean, const float* __restrict__ var, float eps, int kind, int Cin, int Cout,
                                 int cin_pad, int taps, long total, float* __restrict__ out) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x, nth = (long)gridDim.x * blockDim.x;
    const int ncb = (Cout + 63) / 64;
    for (long e = tid; e < total; e += nth) {
        const int n = (int)(e & 63);
        const long k = e >> 6;
        const int tap = (int)(k % taps);
        const int c = (int)((k / taps) % cin_pad);
        const int vb = (int)(k / taps / cin_pad);
        const int q = vb / ncb, co = (vb % ncb) * 64 + n;
        float v = 0.0f;
        if (c < Cin && co < Cout) {
            if (kind <= 1) v = w[((size_t)co * Cin + c) * 9 + tap];         // Conv2d: (Cout, Cin, 3, 3)
            else if (kind == 2) v = w[(size_t)c * Cout + co];               // ConvTranspose2d: (Cin, Cout, 1, 1)
            else v = w[((size_t)c * Cout + co) * 4 + q];                    // ConvTranspose2d: (Cin, Cout, 2, 2), q = dy*2+dx
        }
        out[e] = v;
    }
    const int cout_pad = ncb * 64;
    for (long n = tid; n < cout_pad; n += nth) {
        float alpha = 0.0f, beta2 = 0.0f;
        if (n < Cout) {
            alpha = bn_alpha(var[n], eps, gamma[n]);
            beta2 = beta[n] - mean[n] * alpha;
        }
        out[total + n] = alpha;
        out[total + cout_pad + n] = beta2;
    }
}

// D[channel][pixel]: channels cb * 64 + 32 nb + mfma32_row(r, h) < Cout of the lane's pixel at o, `plane` floats from channel to channel.
// RAW (train() mode, bn_maps.hip normalises afterwards): the accumulator as it is - no affine, no ReLU, par not read.
template <bool RAW>
__device__ __forceinline__ void neck_epilogue(const f32x16& acc0, const f32x16& acc1, const float* par, int cout_pad, int cb, int Cout,
                                              float* o, size_t plane) {
    const int h = (threadIdx.x & 63) >> 5;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int chn = cb * 64 + nb * 32 + mfma32_row(r, h);
            if (chn < Cout) {
                const float a = nb ? acc1[r] : acc0[r];
                if constexpr (RAW) {
                    o[(size_t)chn * plane] = a;
                } else {
                    const float v = a * par[chn] + par[cout_pad + chn];
                    o[(size_t)chn * plane] = relu_nan(v);
                }
            }
        }
    }
}

// PH x PW: the pixel domain (H/2 x W/2 for C3S2, else H x W).  nchunk = cin_pad / CK; blocks = neck_blocks().
template <int KIND, bool RAW>
__global__ __launch_bounds__(256) void neck_layer_kernel(const float* __restrict__ x, const float* __restrict__ packed,
                                                         float* __restrict__ out, int Cin, int H, int W, int Cout, int PH, int PW,
                                                         int ctot, int coff, int blocks, int nchunk) {
    using G = ConvRectTile<KIND>;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x0 = blockIdx.x * CONV_TC, y0 = blockIdx.y * CONV_TR;
    const int b = blockIdx.z / blocks, vb = blockIdx.z - b * blocks;
    f32x16 acc0, acc1;
    conv_body<false, 1>(G(x0, y0), x + (size_t)b * Cin * H * W, packed + (size_t)vb * nchunk * G::WT, Cin, H, W, nchunk, acc0, acc1);
    const int py = y0 + wv, px = x0 + (threadIdx.x & 31);
    if (py >= PH || px >= PW) return;
    const int ncb = KIND == 3 ? blocks / 4 : blocks;
    const int q = vb / ncb, cb = vb - q * ncb;
    const int OH = KIND == 3 ? 2 * H : PH, OW = KIND == 3 ? 2 * W : PW;
    const int oy = KIND == 3 ? 2 * py + (q >> 1) : py, ox = KIND == 3 ? 2 * px + (q & 1) : px;
    const size_t oplane = (size_t)OH * OW;
    neck_epilogue<RAW>(acc0, acc1, packed + (size_t)blocks * nchunk * G::WT, ncb * 64, cb, Cout,
                       out + ((size_t)b * ctot + coff) * oplane + (size_t)oy * OW + ox, oplane);
}

// C3S1 up to 256 columns: the flattened-pixel form, two load chunks ahead (the [Cin][9][64] weights of a channel block read as [Cin/4][36][64])
template <int IN_PT, bool RAW>
__global__ __launch_bounds__(256) void neck_c3s1_flat_kernel(const float* __restrict__ x, const float* __restrict__ packed,
                                                             float* __restrict__ out, int Cin, int H, int W, int Cout, int ctot, int coff,
                                                             int blocks) {
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.z / blocks, cb = blockIdx.z - b * blocks;
    const int npix = H * W, pp = blockIdx.x * 128 + 32 * wv + (threadIdx.x & 31);
    f32x16 acc0, acc1;
    conv_body<false, 2>(ConvFlatTile<IN_PT>(H, W), x + (size_t)b * Cin * npix, packed + (size_t)cb * Cin * 9 * 64, Cin, H, W, Cin / 4, acc0, acc1);
    if (pp >= npix) return;
    neck_epilogue<RAW>(acc0, acc1, packed + (size_t)blocks * Cin * 9 * 64, blocks * 64, cb, Cout, out + ((size_t)b * ctot + coff) * npix + pp, npix);
}

static bool neck_shape_ok(int kind, int Cin, int Cout, int H, int W) {
    if (kind < 0 || kind >= NK_KINDS || Cin <= 0 || Cin % 8 || Cout <= 0 || Cout % 32 || H < 1 || W < 1) return false;
    if (kind == 1 && ((H | W) & 1)) return false;
    if ((long)neck_cin_pad(kind, Cin) * H * W >= (1L << 31)) return false;  // 32-bit offsets inside one image
    const int PH = kind == 1 ? H / 2 : H;
    if (cdiv(PH, CONV_TR) > 65535 || neck_blocks(kind, Cout) > 65535) return false;
    return true;
}

}  // namespace shasta

using namespace shasta;

extern "C" int shasta_neck_layer_supported(int kind, int Cin, int Cout, int H, int W) { return neck_shape_ok(kind, Cin, Cout, H, W) ? 1 : 0; }

extern "C" size_t shasta_neck_layer_packed_bytes(int kind, int Cin, int Cout) {
    if (!neck_shape_ok(kind, Cin, Cout, 2, 2)) return 0;
    return (neck_weight_floats(kind, Cin, Cout) + 2 * (size_t)cdiv(Cout, 64) * 64) * sizeof(float);
}

extern "C" int shasta_neck_layer_pack_f32(const float* weight, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                                          const float* bn_var, float bn_eps, int kind, int Cin, int Cout, void* packed,
                                          size_t packed_bytes, shasta_stream_t stream) {
    SHASTA_REQUIRE(weight && bn_weight && bn_bias && bn_mean && bn_var && packed, "neck_layer_pack: null pointer");
    if (!neck_shape_ok(kind, Cin, Cout, 2, 2)) {
        set_error_msg("neck_layer_pack: kind 0..3, Cin a multiple of 8, Cout a multiple of 32");
        return SHASTA_E_UNSUPPORTED;
    }
    if ((uintptr_t)packed % 16) {
        set_error_msg("neck_layer_pack: packed buffer must be 16-byte aligned");
        return SHASTA_E_ALIGN;
    }
    if (packed_bytes < shasta_neck_layer_packed_bytes(kind, Cin, Cout)) {
        set_error_msg("neck_layer_pack: packed buffer too small");
        return SHASTA_E_WORKSPACE;
    }
    const long total = (long)neck_weight_floats(kind, Cin, Cout);
    hipLaunchKernelGGL(neck_pack_kernel, dim3(256), dim3(256), 0, as_stream(stream), weight, bn_weight, bn_bias, bn_mean, bn_var, bn_eps,
                       kind, Cin, Cout, neck_cin_pad(kind, Cin), neck_taps(kind), total, static_cast<float*>(packed));
    return check_launch("neck_layer_pack");
}

// The checks and the launch plan of a layer, shared by the eval entry point and the raw one (RAW: the same packed buffer, weights only)
template <bool RAW>
static int neck_layer_run(const float* x, int B, int Cin, int H, int W, const void* packed, size_t packed_bytes, int kind, int Cout, float* out,
                          int out_channels_total, int out_channel_offset, shasta_stream_t stream) {
    SHASTA_REQUIRE(x && packed && out, "neck_layer: null pointer");
    SHASTA_REQUIRE(B >= 0, "neck_layer: bad batch size");
    if (!neck_shape_ok(kind, Cin, Cout, H, W)) {
        set_error_msg("neck_layer: unsupported layer (kind 0..3, Cin % 8 == 0, Cout % 32 == 0, H and W >= 1 and even under stride 2)");
        return SHASTA_E_UNSUPPORTED;
    }
    SHASTA_REQUIRE(out_channel_offset >= 0 && out_channels_total > 0 && (long)out_channel_offset + Cout <= out_channels_total,
                   "neck_layer: the channel slice leaves the output");
    if ((uintptr_t)packed % 16) {
        set_error_msg("neck_layer: packed buffer must be 16-byte aligned");
        return SHASTA_E_ALIGN;
    }
    if (packed_bytes < shasta_neck_layer_packed_bytes(kind, Cin, Cout)) {
        set_error_msg("neck_layer: packed buffer too small");
        return SHASTA_E_WORKSPACE;
    }
    if (B == 0) return SHASTA_OK;
    const int blocks = neck_blocks(kind, Cout);
    if ((long)B * blocks > 65535) {
        set_error_msg("neck_layer: B x channel blocks exceeds the grid limit (split the batch)");
        return SHASTA_E_UNSUPPORTED;
    }
    const int PH = kind == 1 ? H / 2 : H, PW = kind == 1 ? W / 2 : W;
    const int nchunk = neck_cin_pad(kind, Cin) / neck_ck(kind);
    const dim3 grid(cdiv(PW, CONV_TC), cdiv(PH, CONV_TR), B * blocks);
    const float* pk = static_cast<const float*>(packed);
    const ConvFlatPlan plan = conv_flat_plan(H, W);
    if (kind == 0 && plan.fits) {
        conv_flat_dispatch(plan.in_pt, [&](auto pt) {
            hipLaunchKernelGGL((neck_c3s1_flat_kernel<decltype(pt)::value, RAW>), dim3(cdiv(H * W, 128), 1, B * blocks), dim3(256), plan.lds,
                               as_stream(stream), x, pk, out, Cin, H, W, Cout, out_channels_total, out_channel_offset, blocks);
        });
        return check_launch("neck_layer_flat");
    }
#define SHASTA_NECK_LAUNCH(K) \
    hipLaunchKernelGGL((neck_layer_kernel<K, RAW>), grid, dim3(256), 0, as_stream(stream), x, pk, out, Cin, H, W, Cout, PH, PW, out_channels_total, \
                       out_channel_offset, blocks, nchunk)
    if (kind == 0) SHASTA_NECK_LAUNCH(0);
    else if (kind == 1) SHASTA_NECK_LAUNCH(1);
    else if (kind == 2) SHASTA_NECK_LAUNCH(2);
    else SHASTA_NECK_LAUNCH(3);
#undef SHASTA_NECK_LAUNCH
    return check_launch("neck_layer");
}

extern "C" int shasta_neck_layer_f32(const float* x, int B, int Cin, int H, int W, const void* packed, size_t packed_bytes, int kind,
                                     int Cout, float* out, int out_channels_total, int out_channel_offset, shasta_stream_t stream) {
    return neck_layer_run<false>(x, B, Cin, H, W, packed, packed_bytes, kind, Cout, out, out_channels_total, out_channel_offset, stream);
}

extern "C" int shasta_neck_layer_raw_f32(const float* x, int B, int Cin, int H, int W, const void* packed, size_t packed_bytes, int kind,
                                         int Cout, float* out, int out_channels_total, int out_channel_offset, shasta_stream_t stream) {
    return neck_layer_run<true>(x, B, Cin, H, W, packed, packed_bytes, kind, Cout, out, out_channels_total, out_channel_offset, stream);
}
