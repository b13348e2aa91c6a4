// The RPN neck (det3d/models/necks/rpn.py:24-163) layer by layer: conv / transposed conv (no bias) -> BatchNorm2d in eval mode -> ReLU,
// strict fp32 on v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain per output, fp32 accumulation), NCHW fp32 in and out.  Four kinds:
//   C3S1  Conv2d(3, padding 1)                 (also ZeroPad2d(1) + Conv2d(3, stride 1))     out H x W
//   C3S2  ZeroPad2d(1) + Conv2d(3, stride 2)                                                 out H/2 x W/2 (H, W even)
//   C1    ConvTranspose2d(k 1, s 1) = 1x1 convolution, weight (Cin, Cout, 1, 1)              out H x W
//   D2    ConvTranspose2d(k 2, s 2): out[co, 2y+dy, 2x+dx] = sum_ci x[ci, y, x] w[ci, co, dy, dx]   out 2H x 2W
// The output is addressed by (out, out_channels_total, out_channel_offset): the deblocks write their halves of the concatenated
// (B, 512, H, W) result in place.  No atomics: the same bits on every run.
//
// Implicit GEMM, one kernel template for the four kinds: M = output channels (the MFMA's A operand, from the packed weights),
// N = pixels along x (the B operand), K = Cin x taps.  Lanes run along x, so every accumulator register of a half-wave stores 128
// contiguous bytes of one output channel's row (D2: every second float of a 256-byte stretch).
// A workgroup (256 threads, 4 waves) owns 64 output channels x 4 rows x 32 columns of the "pixel domain" (output pixels for C3S1 / C3S2 /
// C1, input pixels for D2, where a workgroup also owns ONE of the four (dy, dx) sub-pixel positions: grid.z runs over
// image x [sub-pixel] x 64-channel block).  Wave w owns row w: two 32 x 32 accumulators (channels 0-31, 32-63 of the block) that share
// every input fragment.  K is walked in chunks of CK input channels; the input tile (with halo: 6 x 34, 9 x 65 under stride 2, 4 x 32 for
// the 1x1 kinds) and the (CK x taps x 64) weight slice are staged through LDS, double buffered: the next chunk's global loads are issued
// before the current chunk's MFMAs and written to LDS after them.  The two k values of one MFMA are the same tap of channels c and
// c + CK/2, so every LDS address is a per-lane constant plus an immediate.
//
//                          CK   LDS bytes (2 buffers)   MFMAs / wave / chunk   VGPR + AGPR   waves / SIMD   (compiler's resource report;
//   C3S1 (W > 256)          8   49 920                  72                     113 + 48      3               no scratch in any kernel)
//   C3S2                    4   37 152                  36                      82 + 48      3
//   C1 / D2                32   49 152                  32                     117 + 48      3
//   C3S1 flat (W <= 256)    4   2048 IN_PT + 18 432     36                     IN_PT 8: 101 + 32 (3), 12: 126 + 32 (3), 14: 138 + 32 (2),
//     (below; IN_PT by map width: W = 90 -> 8, W = 180 -> 12)                  16: 149 + 32 (2), 18: 163 + 32 (2)
//
// Packed layer: [virtual 64-channel block vb][Cin rounded up to CK][tap][64] weights (a straight copy per chunk; channels >= Cout and
// >= Cin are zeros), then alpha[Cout rounded up to 64], beta'[same]: alpha = gamma / sqrt(var + eps), beta' = beta - mean * alpha,
// y = relu(acc * alpha + beta') - the formula of shared_conv.hip's epilogue.  vb = block for the convolutions, (dy*2+dx) * blocks + block for D2.
#include "common.hpp"

namespace shasta {

constexpr int NK_TR = 4, NK_TC = 32;  // pixel-domain tile rows / columns
constexpr int NK_KINDS = 4;           // SHASTA_NECK_C3S1 .. SHASTA_NECK_D2

template <int KIND>
struct NeckGeom {
    static constexpr bool k3 = KIND <= 1;
    static constexpr int TAPS = k3 ? 9 : 1;
    static constexpr int S = KIND == 1 ? 2 : 1;              // input pixels per pixel-domain step
    static constexpr int CK = KIND == 0 ? 8 : KIND == 1 ? 4 : 32;  // input channels per chunk
    static constexpr int PAD = k3 ? 1 : 0;
    static constexpr int IR = (NK_TR - 1) * S + (k3 ? 3 : 1);  // staged input rows / columns
    static constexpr int IC = (NK_TC - 1) * S + (k3 ? 3 : 1);
    static constexpr int IN = CK * IR * IC;
    static constexpr int WT = CK * TAPS * 64;
    static constexpr int IN_PT = (IN + 255) / 256;       // staged input floats per thread
    static constexpr int WT_PT = (WT / 4 + 255) / 256;   // staged weight float4 per thread
    static constexpr int KP = CK * TAPS / 2;             // MFMA k steps per chunk
};

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
            alpha = (1.0f / sqrtf(var[n] + eps)) * gamma[n];
            beta2 = beta[n] - mean[n] * alpha;
        }
        out[total + n] = alpha;
        out[total + cout_pad + n] = beta2;
    }
}

// PH x PW: the pixel domain (H/2 x W/2 for C3S2, else H x W).  nchunk = cin_pad / CK; blocks = neck_blocks(); limit = Cin * H * W.
template <int KIND>
__global__ __launch_bounds__(256) void neck_layer_kernel(const float* __restrict__ x, const float* __restrict__ packed,
                                                         float* __restrict__ out, int Cin, int H, int W, int Cout, int PH, int PW,
                                                         int ctot, int coff, int blocks, int nchunk) {
    using G = NeckGeom<KIND>;
    __shared__ __attribute__((aligned(16))) float s_in[2][G::IN];
    __shared__ __attribute__((aligned(16))) float s_w[2][G::WT];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int x0 = blockIdx.x * NK_TC, y0 = blockIdx.y * NK_TR;
    const int b = blockIdx.z / blocks, vb = blockIdx.z - b * blocks;
    const int npix = H * W;
    const unsigned limit = (unsigned)Cin * (unsigned)npix;
    const float* xin = x + (size_t)b * Cin * npix;
    const float* wblk = packed + (size_t)vb * nchunk * G::WT;

    // staging roles (fixed per thread): element e of the tile -> (channel, row, column); offset inside one chunk, 0 where outside
    unsigned in_off[G::IN_PT];
    bool in_ok[G::IN_PT];
#pragma unroll
    for (int j = 0; j < G::IN_PT; ++j) {
        const int e = tid + 256 * j;
        const int c = e / (G::IR * G::IC), rem = e - c * (G::IR * G::IC);
        const int r = rem / G::IC, col = rem - r * G::IC;
        const int gy = y0 * G::S - G::PAD + r, gx = x0 * G::S - G::PAD + col;
        const bool ok = e < G::IN && gy >= 0 && gy < H && gx >= 0 && gx < W;
        in_ok[j] = ok;
        in_off[j] = ok ? (unsigned)(c * npix + gy * W + gx) : 0u;
    }
    float rin[G::IN_PT];
    f32x4 rwt[G::WT_PT];
    auto load_chunk = [&](int ch) {
        const unsigned cbase = (unsigned)ch * (unsigned)(G::CK * npix);  // wave-uniform
#pragma unroll
        for (int j = 0; j < G::IN_PT; ++j) {
            if constexpr (G::k3) {  // Cin is a multiple of CK: the chunk lies inside the image
                const float v = xin[cbase + in_off[j]];
                rin[j] = in_ok[j] ? v : 0.0f;
            } else {                // the last chunk may run past Cin (Cin % 32 != 0): those channels are zeros, like their weights
                const unsigned o = cbase + in_off[j];
                const bool ok = in_ok[j] && o < limit;
                const float v = xin[ok ? o : 0u];
                rin[j] = ok ? v : 0.0f;
            }
        }
        const f32x4* wc = reinterpret_cast<const f32x4*>(wblk + (size_t)ch * G::WT);
#pragma unroll
        for (int j = 0; j < G::WT_PT; ++j) rwt[j] = wc[min(tid + 256 * j, G::WT / 4 - 1)];
    };
    auto store_chunk = [&](int buf) {
#pragma unroll
        for (int j = 0; j < G::IN_PT; ++j)
            if (G::IN % 256 == 0 || tid + 256 * j < G::IN) s_in[buf][tid + 256 * j] = rin[j];
        f32x4* wd = reinterpret_cast<f32x4*>(s_w[buf]);
#pragma unroll
        for (int j = 0; j < G::WT_PT; ++j)
            if ((G::WT / 4) % 256 == 0 || tid + 256 * j < G::WT / 4) wd[tid + 256 * j] = rwt[j];
    };

    f32x16 acc0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    f32x16 acc1 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int i = lane & 31, h = lane >> 5;
    // A (weights): s_w[(c*TAPS + tap)][32*nb + i], c = c_lo + (CK/2) h ; B (input): s_in[c][wv*S + ky][i*S + kx]
    const int a_base = (h * (G::CK / 2) * G::TAPS) * 64 + i;
    const int b_base = (h * (G::CK / 2)) * (G::IR * G::IC) + (wv * G::S) * G::IC + i * G::S;
    auto compute = [&](int buf) {
        const float* aw = s_w[buf] + a_base;
        const float* bin = s_in[buf] + b_base;
#pragma unroll
        for (int kp = 0; kp < G::KP; ++kp) {
            const int c_lo = kp / G::TAPS, tap = kp % G::TAPS, ky = tap / 3, kx = tap % 3;
            const float bv = bin[c_lo * (G::IR * G::IC) + ky * G::IC + kx];
            const float a0 = aw[kp * 64], a1 = aw[kp * 64 + 32];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc1, 0, 0, 0);
        }
    };

    load_chunk(0);
    store_chunk(0);
    __syncthreads();
    // steady state: two chunks per trip so that the buffer roles are compile-time and no condition surrounds the accumulators
    int ch = 0;
#pragma unroll 1
    for (; ch + 2 < nchunk; ch += 2) {
        load_chunk(ch + 1);
        compute(0);
        store_chunk(1);
        __syncthreads();
        load_chunk(ch + 2);
        compute(1);
        store_chunk(0);
        __syncthreads();
    }
    if (ch + 1 < nchunk) {  // tail: one or two chunks left, the first of them is in buffer 0
        load_chunk(ch + 1);
        compute(0);
        store_chunk(1);
        __syncthreads();
        compute(1);
    } else {
        compute(0);
    }

    // epilogue: D[channel row][pixel column]; column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 h
    const int py = y0 + wv, px = x0 + i;
    if (py >= PH || px >= PW) return;
    const int ncb = KIND == 3 ? blocks / 4 : blocks;
    const int q = vb / ncb, cb = vb - q * ncb;
    const float* par = packed + (size_t)blocks * nchunk * G::WT;
    const int cout_pad = ncb * 64;
    const int OH = KIND == 3 ? 2 * H : PH, OW = KIND == 3 ? 2 * W : PW;
    const int oy = KIND == 3 ? 2 * py + (q >> 1) : py, ox = KIND == 3 ? 2 * px + (q & 1) : px;
    const size_t oplane = (size_t)OH * OW;
    float* obase = out + ((size_t)b * ctot + coff) * oplane + (size_t)oy * OW + ox;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int chn = cb * 64 + nb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (chn < Cout) {
                const float a = nb ? acc1[r] : acc0[r];
                const float v = a * par[chn] + par[cout_pad + chn];
                obase[(size_t)chn * oplane] = relu_nan(v);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// C3S1 on maps up to 256 columns wide (every shipped layer: 11 of the neck's 14 layers, 115 of its 126 GFLOP per map): the
// flattened-pixel tiling of shared_conv.hip's flat kernel.  A workgroup owns 128 CONSECUTIVE pixels of the flattened (y*W + x) image
// and 64 output channels, each wave 32 of the pixels - in NCHW a run of flattened pixels is as contiguous as a row.  No row / column
// padding (4 x 32 tiles waste 11 % of a 90 x 90 map and 6 % of a 180 x 180 one) and a grid that fits the chip: 64 pixel groups x 4 channel
// blocks = 256 workgroups for the 256-channel layers at 90 x 90, 254 x 2 = 508 for the 128-channel layers at 180 x 180 (256 CUs; the
// rectangular tiling gives 276 and 540: a second, nearly empty round of workgroups).  The staged input tile covers the <= 128/W + 2 image
// rows the pixels touch plus one halo row either side, full width plus one halo column either side; K chunks are 4 channels (k pair = same tap of
// channels c and c + 2) so that the double-buffered tiles (2 x (11.6 + 9.2) KB at W = 180) leave room for 3 workgroups per CU.  The
// packed layer is the same buffer: [Cin][9][64] per channel block reads as [Cin/4][36][64].
// ------------------------------------------------------------------------------------------------------------------
constexpr int NF_CK = 4;
constexpr int NF_WT = NF_CK * 9 * 64;  // 2304 floats per chunk
constexpr int NF_IN_PT = 18;           // staged input floats per thread, upper bound (W <= 256)

// IN_PT = staged input floats per thread for this map width (ceil(4 * rows * (W + 2) / 256)).  The chunk loop is kept free of VALU work
// as in shared_conv_flat_kernel: halo decisions once (clamped offsets + a select per element), the last chunk peeled.
template <int IN_PT>
__global__ __launch_bounds__(256) void neck_c3s1_flat_kernel(const float* __restrict__ x, const float* __restrict__ packed,
                                                             float* __restrict__ out, int Cin, int H, int W, int Cout, int ctot, int coff,
                                                             int blocks) {
    extern __shared__ __attribute__((aligned(16))) float s_nf[];
    const int WT = W + 2;
    constexpr int in_cap = 256 * IN_PT;  // floats per input buffer (>= NF_CK * rows * WT: the host picks IN_PT)
    float* s_in0 = s_nf;
    float* s_in1 = s_nf + in_cap;
    float* s_w0 = s_nf + 2 * in_cap;
    float* s_w1 = s_w0 + NF_WT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.z / blocks, cb = blockIdx.z - b * blocks;
    const int npix = H * W, p0 = blockIdx.x * 128;
    const int y_first = p0 / W, y_last = min(H - 1, (min(p0 + 127, npix - 1)) / W);
    const int RT = y_last - y_first + 3;  // rows of the tile incl. halo
    const int plane = RT * WT;
    const int nchunk = Cin / NF_CK;
    const float* xin = x + (size_t)b * Cin * npix;
    const float* wblk = packed + (size_t)cb * Cin * 9 * 64;

    unsigned in_off[IN_PT];  // element offset inside one 4-channel chunk (0 where the tile is outside the image)
    bool in_ok[IN_PT];
#pragma unroll
    for (int j = 0; j < IN_PT; ++j) {
        const int e = tid + 256 * j;
        int off = -1;
        if (e < NF_CK * plane) {
            const int c = e / plane, rem = e - c * plane;
            const int r = rem / WT, col = rem - r * WT;
            const int gy = y_first - 1 + r, gx = col - 1;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) off = c * npix + gy * W + gx;
        }
        in_ok[j] = off >= 0;
        in_off[j] = (unsigned)max(off, 0);
    }
    // two register sets: a chunk's global loads are issued TWO chunks ahead of its MFMAs.  With one wave per SIMD - 256 workgroups on
    // 256 CUs for the 256-channel layers at 90 x 90 - nothing else covers the load latency: one chunk ahead 75 TFLOP/s there, two 100
    // (128 channels at 180 x 180, two workgroups per CU: 98 -> 104)
    float rin_a[IN_PT], rin_b[IN_PT];
    f32x4 rwt_a[3], rwt_b[3];
    auto load_chunk = [&](int ch, float (&rin)[IN_PT], f32x4 (&rwt)[3]) {
        const float* xc = xin + (size_t)ch * NF_CK * npix;  // wave-uniform
#pragma unroll
        for (int j = 0; j < IN_PT; ++j) {
            const float v = xc[in_off[j]];  // always a valid address
            rin[j] = in_ok[j] ? v : 0.0f;
        }
        const f32x4* wc = reinterpret_cast<const f32x4*>(wblk + (size_t)ch * NF_WT);
        rwt[0] = wc[tid];
        rwt[1] = wc[tid + 256];
        rwt[2] = wc[min(tid, 63) + 512];
    };
    auto store_chunk = [&](float* si, float* sw, const float (&rin)[IN_PT], const f32x4 (&rwt)[3]) {
#pragma unroll
        for (int j = 0; j < IN_PT; ++j) si[tid + 256 * j] = rin[j];  // the buffer holds all 256 * IN_PT slots
        reinterpret_cast<f32x4*>(sw)[tid] = rwt[0];
        reinterpret_cast<f32x4*>(sw)[tid + 256] = rwt[1];
        if (tid < 64) reinterpret_cast<f32x4*>(sw)[tid + 512] = rwt[2];
    };

    f32x16 acc0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    f32x16 acc1 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const int i = lane & 31, h = lane >> 5;
    const int pp = p0 + 32 * wv + i;
    const int p = min(pp, npix - 1);
    const int py = p / W, px = p - py * W;
    // A (weights): s_w[kp + 18h][32*nb + i] ; B (input): tile[c = c_lo + 2h][py - y_first + 1 + dy][px + 1 + dx]
    const int a_base = (18 * h) * 64 + i;
    const int b_base = (2 * h) * plane + (py - y_first + 1) * WT + px + 1;
    auto compute = [&](const float* si, const float* sw) {
        const float* aw = sw + a_base;
        const float* bin = si + b_base;
#pragma unroll
        for (int kp = 0; kp < 18; ++kp) {
            const int c_lo = kp / 9, tap = kp % 9, dy = tap / 3 - 1, dx = tap % 3 - 1;
            const float bv = bin[c_lo * plane + dy * WT + dx];
            const float a0 = aw[kp * 64], a1 = aw[kp * 64 + 32];
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc1, 0, 0, 0);
        }
    };

    load_chunk(0, rin_a, rwt_a);
    store_chunk(s_in0, s_w0, rin_a, rwt_a);
    __syncthreads();
    load_chunk(1, rin_a, rwt_a);  // (Cin is a multiple of 8: an even number of chunks, at least two)
    // steady state: buffer 0 holds chunk ch, set a chunk ch + 1 (in flight); two chunks per trip, buffer and set roles compile-time
    int ch = 0;
#pragma unroll 1
    for (; ch + 2 < nchunk; ch += 2) {
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

    if (pp >= npix) return;
    const float* par = packed + (size_t)blocks * Cin * 9 * 64;
    const int cout_pad = blocks * 64;
    float* obase = out + ((size_t)b * ctot + coff) * npix + pp;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int chn = cb * 64 + nb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (chn < Cout) {
                const float a = nb ? acc1[r] : acc0[r];
                const float v = a * par[chn] + par[cout_pad + chn];
                obase[(size_t)chn * npix] = relu_nan(v);
            }
        }
    }
}

static bool neck_shape_ok(int kind, int Cin, int Cout, int H, int W) {
    if (kind < 0 || kind >= NK_KINDS || Cin <= 0 || Cin % 8 || Cout <= 0 || Cout % 32 || H < 1 || W < 1) return false;
    if (kind == 1 && ((H | W) & 1)) return false;
    if ((long)neck_cin_pad(kind, Cin) * H * W >= (1L << 31)) return false;  // 32-bit offsets inside one image
    const int PH = kind == 1 ? H / 2 : H;
    if (cdiv(PH, NK_TR) > 65535 || neck_blocks(kind, Cout) > 65535) return false;
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

extern "C" int shasta_neck_layer_f32(const float* x, int B, int Cin, int H, int W, const void* packed, size_t packed_bytes, int kind,
                                     int Cout, float* out, int out_channels_total, int out_channel_offset, shasta_stream_t stream) {
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
    const dim3 grid(cdiv(PW, NK_TC), cdiv(PH, NK_TR), B * blocks);
    const float* pk = static_cast<const float*>(packed);
    if (kind == 0 && W <= 256) {  // the flattened-pixel form
        const int rt_max = min(H, 128 / W + 2) + 2;                  // tile rows incl. halo, upper bound over the workgroups
        const int in_need = cdiv(NF_CK * rt_max * (W + 2), 256);     // staged input floats per thread
        const int in_pt = in_need <= 8 ? 8 : in_need <= 12 ? 12 : in_need <= 14 ? 14 : in_need <= 16 ? 16 : in_need <= 18 ? 18 : 19;  // template value (19: does not fit)
        const size_t lds = ((size_t)2 * 256 * in_pt + 2 * NF_WT) * sizeof(float);
        if (in_pt <= NF_IN_PT && lds <= 64 * 1024) {
            const dim3 fgrid(cdiv(H * W, 128), 1, B * blocks);
#define SHASTA_NECK_FLAT(PT) \
    hipLaunchKernelGGL(neck_c3s1_flat_kernel<PT>, fgrid, dim3(256), lds, as_stream(stream), x, pk, out, Cin, H, W, Cout, out_channels_total, \
                       out_channel_offset, blocks)
            if (in_pt == 8) SHASTA_NECK_FLAT(8);
            else if (in_pt == 12) SHASTA_NECK_FLAT(12);
            else if (in_pt == 14) SHASTA_NECK_FLAT(14);
            else if (in_pt == 16) SHASTA_NECK_FLAT(16);
            else SHASTA_NECK_FLAT(18);
#undef SHASTA_NECK_FLAT
            return check_launch("neck_layer_flat");
        }
    }
#define SHASTA_NECK_LAUNCH(K) \
    hipLaunchKernelGGL(neck_layer_kernel<K>, grid, dim3(256), 0, as_stream(stream), x, pk, out, Cin, H, W, Cout, PH, PW, out_channels_total, \
                       out_channel_offset, blocks, nchunk)
    if (kind == 0) SHASTA_NECK_LAUNCH(0);
    else if (kind == 1) SHASTA_NECK_LAUNCH(1);
    else if (kind == 2) SHASTA_NECK_LAUNCH(2);
    else SHASTA_NECK_LAUNCH(3);
#undef SHASTA_NECK_LAUNCH
    return check_launch("neck_layer");
}
