// The CenterPoint detection head behind the neck map: the kernels that neck.hip's layers do not already provide.
//
// The head's Conv2d(3, padding 1, bias) -> BatchNorm2d (eval) -> ReLU layers - `shared_conv` and the first convolution of every head -
// ARE neck layers (SHASTA_NECK_C3S1 of neck.hip on conv3x3_f32.hpp's body): the convolution bias b only moves the epilogue constant,
// (acc + b - mean) alpha + beta = acc alpha + (beta - (mean - b) alpha), so the host hands `mean - b` to shasta_neck_layer_pack_f32 and
// runs the first convolutions of all heads of a task as ONE layer with Cout = 64 x heads.  Nothing of that is repeated here.
//
// 1. head_final_kernel - the heads' last convolutions: 3x3, padding 1, the 64 channels [64 h, 64 h + 64) of the (B, 64 heads, H, W)
//    tensor to k <= 3 channels of the task's (B, C_task, H, W) tensor, + bias, no norm, no ReLU.  Strict fp32 on v_mfma_f32_16x16x4_f32
//    (exact fp32, a k-ordered fmaf chain per output like the 32x32x2 form): M = 16 output channels of which rows 0 .. k - 1 are real
//    (the A operand: weights from LDS, zero for rows >= 4), N = 16 pixels (the B operand), K = 4 input channels of ONE tap per
//    instruction, so a lane's pixel address is a per-lane constant plus a wave-uniform channel offset.  conv_body's 64-channel block
//    would execute 64 / k channel rows per real one; this executes 16 / k (DESIGN.md states executed against useful FLOP).
//    A workgroup = (256 consecutive pixels of the flattened image, one head, one image); a wave owns 64 of them as four independent
//    16-pixel accumulators (the 16x16x4 form needs >= 2 independent accumulators to issue back to back).  The input is read straight
//    from global memory - 9 taps re-read 64-byte runs that stay in the L1 - with clamped offsets and a select for the padding; the
//    head's 576 x 4 weights and its bias sit in LDS.  Rows 0 .. 3 of D are the four registers of lanes 0 .. 15: those lanes store.
//    Packed head (host-written, see include/shasta_hip.h): [cc = 16][tap = 9][kq = 4][i = 4] weights w[i][4 cc + kq][tap], bias[4].
//
// 2. shasta_head_decode_f32 - one task's raw maps to a compacted candidate list per image, in ascending pixel order, counts on the
//    device: count (one pixel per thread, wave ballot -> a block's count), scan (one workgroup per image over its block counts), write
//    (the flags recomputed by the same function, place = block offset + lower waves + lower lanes).  No atomics.  The ballot step and
//    the scan kernel are scan.hpp's.
#include "common.hpp"
#include "scan.hpp"

namespace shasta {

constexpr int HF_MAX_HEADS = SHASTA_HEAD_MAX_HEADS;
constexpr int HF_PIX = 256;                  // pixels per workgroup
constexpr int HF_HEAD_FLOATS = 576 * 4 + 4;  // packed floats per head

struct HeadFinalPlan {
    int width[HF_MAX_HEADS];  // output channels of head h (1 .. 3)
    int coff[HF_MAX_HEADS];   // its first channel in the task's tensor
};

__global__ __launch_bounds__(256) void head_final_kernel(const float* __restrict__ x, const float* __restrict__ packed, float* __restrict__ out,
                                                         int heads, int H, int W, int ctask, HeadFinalPlan plan) {
    __shared__ float s_w[HF_HEAD_FLOATS];
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    for (int e = tid; e < HF_HEAD_FLOATS; e += 256) s_w[e] = packed[(size_t)h * HF_HEAD_FLOATS + e];
    __syncthreads();
    const int lane = tid & 63, wv = tid >> 6, i = lane & 15, kq = lane >> 4;
    const int npix = H * W;
    const float* xin = x + ((size_t)b * heads + h) * 64 * npix + (size_t)kq * npix;  // the lane's channel of the first chunk

    unsigned off[4][9];
    bool ok[4][9];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int p = blockIdx.x * HF_PIX + wv * 64 + g * 16 + i;
        const int pc = min(p, npix - 1), py = pc / W, px = pc - py * W;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int yy = py + tap / 3 - 1, xx = px + tap % 3 - 1;
            const bool in = p < npix && yy >= 0 && yy < H && xx >= 0 && xx < W;
            ok[g][tap] = in;
            off[g][tap] = in ? (unsigned)(yy * W + xx) : 0u;
        }
    }
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = f32x4{0, 0, 0, 0};
    const float* wl = s_w + kq * 4 + (i & 3);
#pragma unroll 1
    for (int cc = 0; cc < 16; ++cc) {
        const float* xc = xin + (size_t)cc * 4 * npix;  // wave-uniform step
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const float wraw = wl[(cc * 9 + tap) * 16];
            const float a = i < 4 ? wraw : 0.0f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float v = xc[off[g][tap]];
                acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ok[g][tap] ? v : 0.0f, acc[g], 0, 0, 0);
            }
        }
    }
    if (kq != 0) return;  // rows 0 .. 3 of D: lanes 0 .. 15
    const int width = plan.width[h];
    float* o = out + ((size_t)b * ctask + plan.coff[h]) * npix;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int p = blockIdx.x * HF_PIX + wv * 64 + g * 16 + i;
        if (p >= npix) continue;
#pragma unroll
        for (int r = 0; r < 3; ++r)
            if (r < width) o[(size_t)r * npix + p] = acc[g][r] + s_w[576 * 4 + r];
    }
}

static bool head_final_ok(int heads, const int* widths, int H, int W) {
    if (heads < 1 || heads > HF_MAX_HEADS || !widths || H < 1 || W < 1) return false;
    long ctask = 0;
    for (int h = 0; h < heads; ++h) {
        if (widths[h] < 1 || widths[h] > 3) return false;
        ctask += widths[h];
    }
    if ((long)heads * 64 * H * W >= (1L << 31) || ctask * H * W >= (1L << 31)) return false;  // 32-bit offsets inside one image
    return true;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// decode

struct DecodedPixel {
    float box[9], score;
    int label;
    bool keep;
};

__device__ __forceinline__ DecodedPixel head_decode_pixel(const float* __restrict__ raw, int npix, int W, int p, const shasta_head_decode_cfg& c) {
    DecodedPixel d;
    const int iy = p / W, ix = p - iy * W;
    float best = 0.0f;
    int label = 0;
    for (int k = 0; k < c.num_class; ++k) {
        const float s = 1.0f / (1.0f + expf(-raw[(size_t)(c.hm + k) * npix + p]));
        if (k == 0 || s > best) best = s, label = k;  // the first arg-max
    }
    const float r0 = raw[(size_t)c.reg * npix + p], r1 = raw[(size_t)(c.reg + 1) * npix + p];
    const float xs = ((float)ix + r0) * c.out_size_factor * c.voxel_x + c.pc_x;  // products before the sum; no contraction (-ffp-contract=off)
    const float ys = ((float)iy + r1) * c.out_size_factor * c.voxel_y + c.pc_y;
    const float zs = raw[(size_t)c.height * npix + p];
    d.box[0] = xs, d.box[1] = ys, d.box[2] = zs;
#pragma unroll
    for (int k = 0; k < 3; ++k) d.box[3 + k] = expf(raw[(size_t)(c.dim + k) * npix + p]);
    d.box[6] = raw[(size_t)c.vel * npix + p];
    d.box[7] = raw[(size_t)(c.vel + 1) * npix + p];
    d.box[8] = atan2f(raw[(size_t)c.rot * npix + p], raw[(size_t)(c.rot + 1) * npix + p]);
    d.score = best;
    d.label = label;
    d.keep = best > c.score_threshold && xs >= c.range[0] && ys >= c.range[1] && zs >= c.range[2] && xs <= c.range[3] && ys <= c.range[4] &&
             zs <= c.range[5];
    return d;
}

__global__ __launch_bounds__(256) void head_decode_count_kernel(const float* __restrict__ raw, int C, int npix, int W, shasta_head_decode_cfg cfg,
                                                                uint32_t* __restrict__ cnt) {
    __shared__ int s_wave[4];
    const int t = threadIdx.x, b = blockIdx.y, p = blockIdx.x * 256 + t;
    bool keep = false;
    if (p < npix) keep = head_decode_pixel(raw + (size_t)b * C * npix, npix, W, p, cfg).keep;
    const int kept = block_place(keep, s_wave).count;
    if (t == 0) cnt[(size_t)b * gridDim.x + blockIdx.x] = (uint32_t)kept;
}

__global__ __launch_bounds__(256) void head_decode_write_kernel(const float* __restrict__ raw, int C, int npix, int W, shasta_head_decode_cfg cfg,
                                                                const uint32_t* __restrict__ off, int cap, float* __restrict__ box,
                                                                float* __restrict__ score, int32_t* __restrict__ label, int32_t* __restrict__ pixel) {
    __shared__ int s_wave[4];
    const int t = threadIdx.x, b = blockIdx.y, p = blockIdx.x * 256 + t;
    DecodedPixel d;
    d.keep = false;
    if (p < npix) d = head_decode_pixel(raw + (size_t)b * C * npix, npix, W, p, cfg);
    const BlockPlace bp = block_place(d.keep, s_wave);
    if (!d.keep) return;  // (after the barrier inside block_place)
    const long place = (long)off[(size_t)b * gridDim.x + blockIdx.x] + bp.place;
    if (place >= cap) return;  // counted, not written
    const size_t at = (size_t)b * cap + place;
#pragma unroll
    for (int k = 0; k < 9; ++k) box[at * 9 + k] = d.box[k];
    score[at] = d.score;
    label[at] = d.label;
    pixel[at] = p;
}

static bool head_decode_ok(int B, int C, int H, int W) {
    return B >= 0 && B <= 65535 && C >= 1 && H >= 1 && W >= 1 && (long)C * H * W < (1L << 31) && (long)H * W <= (long)INT32_MAX - 256;
}

}  // namespace shasta

using namespace shasta;

extern "C" int shasta_head_supported(int in_channels, int share_conv_channel, int heads, const int* widths, int H, int W) {
    if (in_channels <= 0 || in_channels % 8 || share_conv_channel <= 0 || share_conv_channel % 32) return 0;
    if (!head_final_ok(heads, widths, H, W)) return 0;
    return shasta_neck_layer_supported(SHASTA_NECK_C3S1, in_channels, share_conv_channel, H, W) &&
                   shasta_neck_layer_supported(SHASTA_NECK_C3S1, share_conv_channel, 64 * heads, H, W)
               ? 1
               : 0;
}

extern "C" size_t shasta_head_final_packed_bytes(int heads) {
    if (heads < 1 || heads > HF_MAX_HEADS) return 0;
    return (size_t)heads * HF_HEAD_FLOATS * sizeof(float);
}

extern "C" int shasta_head_final_f32(const float* x, int B, int heads, const int* widths, int H, int W, const void* packed, size_t packed_bytes,
                                     float* out, shasta_stream_t stream) {
    SHASTA_REQUIRE(x && packed && out && widths, "head_final: null pointer");
    SHASTA_REQUIRE(B >= 0, "head_final: bad batch size");
    if (!head_final_ok(heads, widths, H, W)) {
        set_error_msg("head_final: unsupported shape (1 .. 16 heads of 64 channels, final widths 1 .. 3, H and W >= 1, one image below 2^31 elements)");
        return SHASTA_E_UNSUPPORTED;
    }
    if (packed_bytes < shasta_head_final_packed_bytes(heads)) {
        set_error_msg("head_final: packed buffer too small");
        return SHASTA_E_WORKSPACE;
    }
    if (B == 0) return SHASTA_OK;
    if (B > 65535) {
        set_error_msg("head_final: B exceeds the grid limit (split the batch)");
        return SHASTA_E_UNSUPPORTED;
    }
    HeadFinalPlan plan = {};
    int ctask = 0;
    for (int h = 0; h < heads; ++h) plan.width[h] = widths[h], plan.coff[h] = ctask, ctask += widths[h];
    hipLaunchKernelGGL(head_final_kernel, dim3(cdiv(H * W, HF_PIX), heads, B), dim3(256), 0, as_stream(stream), x,
                       static_cast<const float*>(packed), out, heads, H, W, ctask, plan);
    return check_launch("head_final");
}

extern "C" size_t shasta_head_decode_workspace_bytes(int B, int H, int W) {
    if (!head_decode_ok(B, 1, H, W)) return 0;
    return align_up((size_t)std::max(B, 1) * cdiv(H * W, 256) * sizeof(uint32_t), 256);
}

extern "C" int shasta_head_decode_f32(const float* raw, int B, int C, int H, int W, const shasta_head_decode_cfg* cfg, int cap, float* box,
                                      float* score, int32_t* label, int32_t* pixel, int32_t* count, void* workspace, size_t workspace_bytes,
                                      shasta_stream_t stream) {
    SHASTA_REQUIRE(cfg, "head_decode: null pointer");
    if (!head_decode_ok(B, C, H, W)) {
        set_error_msg("head_decode: unsupported shape (B <= 65535, one image below 2^31 elements)");
        return SHASTA_E_UNSUPPORTED;
    }
    SHASTA_REQUIRE(cap >= 0, "head_decode: bad capacity");
    {
        const shasta_head_decode_cfg& c = *cfg;
        const bool in = c.num_class >= 1 && c.reg >= 0 && c.reg + 2 <= C && c.height >= 0 && c.height + 1 <= C && c.dim >= 0 && c.dim + 3 <= C &&
                        c.rot >= 0 && c.rot + 2 <= C && c.vel >= 0 && c.vel + 2 <= C && c.hm >= 0 && (long)c.hm + c.num_class <= C;
        SHASTA_REQUIRE(in, "head_decode: a head's channels leave the tensor");
    }
    if (B == 0) return SHASTA_OK;
    SHASTA_REQUIRE(raw && count && workspace, "head_decode: null pointer");
    SHASTA_REQUIRE(cap == 0 || (box && score && label && pixel), "head_decode: null pointer");
    if (workspace_bytes < shasta_head_decode_workspace_bytes(B, H, W)) {
        set_error_msg("head_decode: workspace too small");
        return SHASTA_E_WORKSPACE;
    }
    const int npix = H * W, nblk = cdiv(npix, 256);
    uint32_t* cnt = static_cast<uint32_t*>(workspace);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(head_decode_count_kernel, dim3(nblk, B), dim3(256), 0, st, raw, C, npix, W, *cfg, cnt);
    int rc = check_launch("head_decode_count");
    if (rc) return rc;
    hipLaunchKernelGGL(scan_sums_kernel<false>, dim3(B), dim3(256), 0, st, cnt, nblk, count);  // one workgroup per image: count[b] = its candidates
    rc = check_launch("head_decode_scan");
    if (rc) return rc;
    if (cap == 0) return SHASTA_OK;
    hipLaunchKernelGGL(head_decode_write_kernel, dim3(nblk, B), dim3(256), 0, st, raw, C, npix, W, *cfg, cnt, cap, box, score, label, pixel);
    return check_launch("head_decode_write");
}
