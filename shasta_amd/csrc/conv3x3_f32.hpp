// The f32 convolution body of K0 (shared_conv.hip) and of the neck's layers (neck.hip): implicit GEMM on v_mfma_f32_32x32x2_f32 (exact
// fp32: a k-ordered fmaf chain per output).  One side of the GEMM is 64 output channels (from the packed weights), the other 32 pixels per
// wave; PIX_A says which MFMA operand the pixels are.  A: D is [pixel][channel], a lane owns one channel (K0 stores NHWC).  B: D is
// [channel][pixel], a lane owns one pixel (the neck stores NCHW).  Products commute, so both orders give the same bits.  A wave holds two
// 32 x 32 accumulators (channels 0-31, 32-63 of the block) that share every pixel fragment.  K is walked in chunks of CK input channels:
// the input tile with its halo and the (CK x taps x 64) weight slice - a straight copy out of the packed [chunk][c * taps + tap][64]
// layout - are staged through LDS, double buffered: a chunk's global loads are issued before an earlier chunk's MFMAs and written to LDS
// after them.  The two k values of one MFMA are the same tap of channels c and c + CK/2, so every LDS address is a per-lane constant
// plus an offset that is the same for all lanes.
//
// The f32 MFMA does not overlap VALU work, so the chunk loop is kept free of it.  The halo / padding decisions are taken once per thread
// (clamped 32-bit offsets + a select per element instead of predicated loads: the address is always valid) and the loads use the scalar
// chunk base + a per-lane offset.  No condition surrounds the accumulators: two chunks per trip make the buffer roles compile-time and
// the tail is peeled (with the condition inside the loop the register allocator moved all 32 accumulators through VGPRs every chunk:
// 233 VALU instructions per 36 MFMAs).
//
// conv_body fills the two accumulators of a tile (a workgroup of 256 threads, 4 waves); a kernel keeps its own prologue (which map,
// which channel block) and its own epilogue.  Two tiles:
//
// ConvRectTile<KIND>: 4 rows x 32 columns of the pixel domain, wave w row w.  KIND 0: 3x3, stride 1 (6 x 34 input tile, chunks of 8
// channels); 1: 3x3, stride 2 behind ZeroPad2d(1) (9 x 65, chunks of 4); 2, 3: one tap (4 x 32, chunks of 32: the neck's 1x1 kinds).
//
// ConvFlatTile<IN_PT>: 3x3 stride 1 on maps up to 256 columns wide (every shipped configuration): 128 CONSECUTIVE pixels of the
// flattened (y * W + x) image, each wave 32 of them.  No row / column padding (4 x 32 tiles waste 6 % of a 180 x 180 map and 11 % of a
// 90 x 90 one) and 254 pixel groups per 180 x 180 map instead of 270.  The staged input tile covers the <= 128/W + 2 image rows the pixels
// touch plus one halo row either side, full width plus one halo column either side.  K chunks are 4 channels so that the double-buffered
// tiles (2 x (11.6 + 9.2) KB at W = 180) leave room for 3 workgroups per CU; packed [Cin/8][72][64] weights read as [Cin/4][36][64].
// IN_PT = staged input floats per thread for the map width, from conv_flat_plan (W = 90 -> 8, W = 180 -> 12).
#pragma once
#include <type_traits>
#include "common.hpp"

namespace shasta {

// alpha of the eval-mode BatchNorm epilogue y = acc * alpha + beta', as torch's kernel computes it
__device__ __forceinline__ float bn_alpha(float var, float eps, float gamma) { return (1.0f / sqrtf(var + eps)) * gamma; }

constexpr int CONV_TR = 4, CONV_TC = 32;  // the rectangular tile's rows / columns in the pixel domain

// A tile: CK, TAPS, WT (weight floats per chunk), IN_PT (staged input floats per thread), IN_CAP (floats of one LDS input buffer),
// PAST_CIN; lds(); the staged input
// is rows x cols image pixels per channel from pixel (gy0, gx0); p_base: the lane's offset in it (channel c_lo + (CK/2) h, tap 0).
template <int KIND>
struct ConvRectTile {
    static constexpr bool k3 = KIND <= 1;
    static constexpr int TAPS = k3 ? 9 : 1;
    static constexpr int S = KIND == 1 ? 2 : 1;                    // input pixels per pixel-domain step
    static constexpr int CK = KIND == 0 ? 8 : KIND == 1 ? 4 : 32;  // input channels per chunk
    static constexpr int PAD = k3 ? 1 : 0;
    static constexpr int IR = (CONV_TR - 1) * S + (k3 ? 3 : 1);    // staged input rows / columns
    static constexpr int IC = (CONV_TC - 1) * S + (k3 ? 3 : 1);
    static constexpr int IN_CAP = CK * IR * IC;                    // (even: the weight buffers behind 2 IN_CAP floats stay 16-byte aligned)
    static constexpr int IN_PT = (IN_CAP + 255) / 256;
    static constexpr int WT = CK * TAPS * 64;
    static constexpr bool PAST_CIN = !k3;      // the last chunk may run past Cin (Cin % 32 != 0): those channels are zeros, like their weights
    int rows, cols, gy0, gx0, p_base;
    static __device__ __forceinline__ float* lds() {
        __shared__ __attribute__((aligned(16))) float s[2 * IN_CAP + 2 * WT];
        return s;
    }
    __device__ __forceinline__ ConvRectTile(int x0, int y0) : rows(IR), cols(IC), gy0(y0 * S - PAD), gx0(x0 * S - PAD) {
        const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        p_base = ((lane >> 5) * (CK / 2)) * (IR * IC) + (wv * S) * IC + (lane & 31) * S;
    }
};

template <int IN_PT_>
struct ConvFlatTile {
    static constexpr int TAPS = 9, CK = 4, WT = CK * TAPS * 64;
    static constexpr int IN_PT = IN_PT_, IN_CAP = 256 * IN_PT;  // (IN_CAP >= CK * rows * cols: the host picks IN_PT)
    static constexpr bool PAST_CIN = false;
    int rows, cols, gy0, gx0, p_base;
    static __device__ __forceinline__ float* lds() {
        extern __shared__ __attribute__((aligned(16))) float s_conv[];
        return s_conv;
    }
    __device__ __forceinline__ ConvFlatTile(int H, int W) {
        const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int npix = H * W, p0 = blockIdx.x * 128;
        const int y_first = p0 / W, y_last = min(H - 1, (min(p0 + 127, npix - 1)) / W);
        rows = y_last - y_first + 3;  // incl. halo
        cols = W + 2;
        gy0 = y_first - 1;
        gx0 = -1;
        const int p = min(p0 + 32 * wv + (lane & 31), npix - 1);
        const int py = p / W, px = p - py * W;
        p_base = (2 * (lane >> 5)) * (rows * cols) + (py - y_first) * cols + px;
    }
};

struct ConvFlatPlan {
    int in_pt;   // ConvFlatTile's IN_PT: 8, 12, 14, 16 or 18 (19: does not fit)
    size_t lds;  // dynamic LDS bytes
    bool fits;   // else: the rectangular tile
};
inline ConvFlatPlan conv_flat_plan(int H, int W) {
    const int rt_max = min(H, 128 / W + 2) + 2;           // tile rows incl. halo, upper bound over the workgroups
    const int in_need = cdiv(4 * rt_max * (W + 2), 256);  // staged input floats per thread
    const int in_pt = in_need <= 8 ? 8 : in_need <= 12 ? 12 : in_need <= 14 ? 14 : in_need <= 16 ? 16 : in_need <= 18 ? 18 : 19;
    const size_t lds = ((size_t)2 * 256 * in_pt + 2 * 4 * 9 * 64) * sizeof(float);
    return {in_pt, lds, W <= 256 && in_pt <= 18 && lds <= 64 * 1024};
}
// launch(std::integral_constant<int, IN_PT>) for a plan that fits
template <class F>
inline void conv_flat_dispatch(int in_pt, F launch) {
    if (in_pt == 8) launch(std::integral_constant<int, 8>());
    else if (in_pt == 12) launch(std::integral_constant<int, 12>());
    else if (in_pt == 14) launch(std::integral_constant<int, 14>());
    else if (in_pt == 16) launch(std::integral_constant<int, 16>());
    else launch(std::integral_constant<int, 18>());
}

// xin: the image (Cin, H, W); wblk: the channel block's [nchunk][CK * TAPS][64] weights.
// AHEAD = how many chunks a chunk's global loads are issued ahead of its MFMAs, with as many register sets.  1: any nchunk >= 1.
// 2: nchunk even (the flat tile with Cin % 8 == 0).  With one wave per SIMD - the neck's 256-channel layers at 90 x 90 are 256
// workgroups on 256 CUs - nothing else covers the load latency: one chunk ahead 75 TFLOP/s there, two 100 (128 channels at 180 x 180,
// two workgroups per CU: 98 -> 104).
template <bool PIX_A, int AHEAD, class T>
__device__ __forceinline__ void conv_body(const T t, const float* xin, const float* wblk, int Cin, int H, int W, int nchunk, f32x16& acc0,
                                          f32x16& acc1) {
    constexpr int IN_PT = T::IN_PT, WT = T::WT, WT4 = WT / 4, WT_PT = (WT4 + 255) / 256;  // staged weight float4: per chunk, per thread
    float* s_in0 = T::lds();
    float* s_in1 = s_in0 + T::IN_CAP;
    float* s_w0 = s_in0 + 2 * T::IN_CAP;
    float* s_w1 = s_w0 + WT;
    const int tid = threadIdx.x, npix = H * W, plane = t.rows * t.cols;

    // staging roles (fixed per thread): element e of the tile -> (channel, row, column); offset inside one chunk, 0 where outside
    unsigned in_off[IN_PT];
    bool in_ok[IN_PT];
#pragma unroll
    for (int j = 0; j < IN_PT; ++j) {
        const int e = tid + 256 * j;
        const int c = e / plane, rem = e - c * plane;
        const int r = rem / t.cols, col = rem - r * t.cols;
        const int gy = t.gy0 + r, gx = t.gx0 + col;
        const bool ok = e < T::CK * plane && gy >= 0 && gy < H && gx >= 0 && gx < W;
        in_ok[j] = ok;
        in_off[j] = ok ? (unsigned)c * (unsigned)npix + (unsigned)(gy * W + gx) : 0u;
    }
    auto load_chunk = [&](int ch, float (&rin)[IN_PT], f32x4 (&rwt)[WT_PT]) {
#pragma unroll
        for (int j = 0; j < IN_PT; ++j) {
            if constexpr (T::PAST_CIN) {
                const unsigned o = (unsigned)ch * (unsigned)(T::CK * npix) + in_off[j];
                const bool ok = in_ok[j] && o < (unsigned)Cin * (unsigned)npix;
                const float v = xin[ok ? o : 0u];
                rin[j] = ok ? v : 0.0f;
            } else {  // Cin is a multiple of CK: the chunk lies inside the image
                const float v = (xin + (size_t)ch * T::CK * npix)[in_off[j]];  // wave-uniform base
                rin[j] = in_ok[j] ? v : 0.0f;
            }
        }
        const f32x4* wc = reinterpret_cast<const f32x4*>(wblk + (size_t)ch * WT);
#pragma unroll
        for (int j = 0; j < WT_PT; ++j) rwt[j] = wc[256 * (j + 1) <= WT4 ? tid + 256 * j : min(tid + 256 * j, WT4 - 1)];
    };
    auto store_chunk = [&](float* si, float* sw, const float (&rin)[IN_PT], const f32x4 (&rwt)[WT_PT]) {
#pragma unroll
        for (int j = 0; j < IN_PT; ++j)
            if (256 * (j + 1) <= T::IN_CAP || tid + 256 * j < T::IN_CAP) si[tid + 256 * j] = rin[j];
#pragma unroll
        for (int j = 0; j < WT_PT; ++j)
            if (256 * (j + 1) <= WT4 || tid + 256 * j < WT4) reinterpret_cast<f32x4*>(sw)[tid + 256 * j] = rwt[j];
    };

    acc0 = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    acc1 = acc0;
    // weights: s_w[(c * TAPS + tap)][32 * nb + i], c = c_lo + (CK/2) h ; pixels: s_in[c][row + ky][column + kx]
    const int w_base = ((tid & 63) >> 5) * (T::CK / 2) * T::TAPS * 64 + (tid & 31);
    auto compute = [&](const float* si, const float* sw) {
        const float* wp = sw + w_base;
        const float* pp = si + t.p_base;
#pragma unroll
        for (int kp = 0; kp < T::CK * T::TAPS / 2; ++kp) {
            const int c_lo = kp / T::TAPS, tap = kp % T::TAPS, ky = tap / 3, kx = tap % 3;
            const float pix = pp[c_lo * plane + ky * t.cols + kx], w0 = wp[kp * 64], w1 = wp[kp * 64 + 32];
            if constexpr (PIX_A) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(pix, w0, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(pix, w1, acc1, 0, 0, 0);
            } else {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, pix, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, pix, acc1, 0, 0, 0);
            }
        }
    };

    float rin_a[IN_PT];
    f32x4 rwt_a[WT_PT];
    load_chunk(0, rin_a, rwt_a);
    store_chunk(s_in0, s_w0, rin_a, rwt_a);
    __syncthreads();
    int ch = 0;
    if constexpr (AHEAD == 1) {
#pragma unroll 1
        for (; ch + 2 < nchunk; ch += 2) {  // steady state: chunk ch in buffer 0; every trip stages two more chunks
            load_chunk(ch + 1, rin_a, rwt_a);
            compute(s_in0, s_w0);
            store_chunk(s_in1, s_w1, rin_a, rwt_a);
            __syncthreads();
            load_chunk(ch + 2, rin_a, rwt_a);
            compute(s_in1, s_w1);
            store_chunk(s_in0, s_w0, rin_a, rwt_a);
            __syncthreads();
        }
        if (ch + 1 < nchunk) {  // tail: one or two chunks left, the first of them is in buffer 0
            load_chunk(ch + 1, rin_a, rwt_a);
            compute(s_in0, s_w0);
            store_chunk(s_in1, s_w1, rin_a, rwt_a);
            __syncthreads();
            compute(s_in1, s_w1);
        } else {
            compute(s_in0, s_w0);
        }
    } else {
        float rin_b[IN_PT];
        f32x4 rwt_b[WT_PT];
        load_chunk(1, rin_a, rwt_a);
#pragma unroll 1
        for (; ch + 2 < nchunk; ch += 2) {  // steady state: chunk ch in buffer 0, chunk ch + 1 in set a (in flight); set roles compile-time too
            load_chunk(ch + 2, rin_b, rwt_b);
            compute(s_in0, s_w0);
            store_chunk(s_in1, s_w1, rin_a, rwt_a);
            __syncthreads();
            load_chunk(ch + 3, rin_a, rwt_a);
            compute(s_in1, s_w1);
            store_chunk(s_in0, s_w0, rin_b, rwt_b);
            __syncthreads();
        }
        // tail: chunk nchunk - 2 in buffer 0, the last one in set a
        compute(s_in0, s_w0);
        store_chunk(s_in1, s_w1, rin_a, rwt_a);
        __syncthreads();
        compute(s_in1, s_w1);
    }
}

}  // namespace shasta
