// K4c, fp16-piece form (SHASTA_OPT_F16X2_PAIR, F = 256): the per-pair MLP tails of det3d/models/tracker/shasta.py:286-319 with
// their SECOND layers - 1792 of the 1984 multiply-adds per pair - on the f16 matrix path, everything else as in pair_mfma4_kernel.
//
// Why only the second layers: the activations h1 = relu(UP[t] + UC[d]) exist per pair, so cutting them into pieces is VALU work
// per pair; it pays where one cut value feeds 16 multiply-adds (layer 2: 64 -> 16, 32 -> 16, 32 -> 8) and not for the narrow
// layers behind it.  Arithmetic: the two-piece fp16 form of pieces.hpp (three products), three v_mfma_f32_16x16x32_f16 instead of
// sixteen f32 4x4x1 MFMA slots per 16 x 16 x 32 block; fp32 accumulation.
//
// Two forms of the pieces of h1 (PairF16Mode): PAIR_SELECT, the "f16x2" default, and PAIR_GRID ("f16grid", opt-in, further down).
//
// PAIR_SELECT does not cut per pair.  relu(u + v) = max(v, -u) + u with u = UP[t][k], v = UC[d][k]: max(v, -u) is one of two numbers
// that exist per table ROW, so their fp16 pieces are cut once - UC[d] when the detection tile is loaded, -UP[t] once per track by
// its wave - into one orderable 32-bit word per value (pieces.hpp: cut_select_word), and per pair and hidden unit ONE v_max_f32 picks
// the word of the larger value.  The "+ u" passes through the linear second layers as S[t] = bias2 + W2 UP[t], 40 floats per track
// row (pair.hip: row_select_kernel), the addend of the descale fma in phase (2).  Unlike a fixed grid every word keeps the relative
// precision of its own value (tools/pair_quant_sim.py `select`: max / rms error 1.0 - 1.2 x the f32 kernel's).
//
// Layouts.  A wave owns 64 detections x a range of tracks.  Per track:
//  (1) four sub-steps of 16 detections in the MFMA layout lane = (pair p = lane & 15, k block kb = lane >> 4).  A word is [hi | lo]
//      of ONE real k, so an instruction's 32 k are 16 real k: the lane holds words 16 c + 4 kb + jj, jj < 4, of instruction c < 8
//      (c = 0, 1 fuse_shape | 2 .. 5 res_coeff | 6, 7 fuse_det), and the weight fragments hold every weight twice ([Wh|Wh], [Wl|Wl]:
//      all four piece products).  Per sub-step: 8 ds_read_b128 of UC words, 32 v_max_f32 in place, 16 MFMAs (12 in the per-pair cut
//      this replaced); the three result blocks (4 consecutive output features of pair p per lane) go to a wave-private LDS tile
//      [64 pairs][40 features].
//  (2) lane = pair: the lane reads its 40 layer-2 pre-activations, descales (exact power of two) and adds S[t] with one fma each,
//      and runs layers 3-4, the hand-designed residual and the combine exactly as pair_mfma4_kernel does.
// Range: ONE scale 2^e per (workgroup's tracks, detection tile) - two words are only comparable under the same scale -, the one
// that puts (largest finite max |UP[t]| of the workgroup's tracks + largest max |UC[d]| of the tile) into (2^13, 2^14]; the row
// maxima come from embed_rows / row_prep (slot 13 of the hand rows).  The second-layer weights are cut once at pack time with one
// exponent per MLP (pair_f16_pack_kernel).
// Counted in the ISA: 311 vector instructions per track and wave (184 of them v_max_f32; the per-pair cut had 552, 384 of them
// conversions, mixes and packed fp32 ops), 64 + 69 MFMAs (48 + 69), 234 registers, two waves per SIMD.  Measured at 1024
// frame-pairs, N = M = 500 (profiles/pair_select_ab.txt): pair stage by events, row_select_kernel included, 8.20 - 8.26 -> 7.58 - 7.79
// ms with the tracks still dealt 1000 : 615, 7.47 - 7.82 ms dealt 1000 : 760 (launch_pair_f16).  Far less than the instruction count:
// the vector pipe is no longer the limit; per track and wave the LDS now serves ~85 b128 reads and 12 b128 writes.
#include "stages.hpp"
#include "pair_lane.hpp"
#include "pieces.hpp"

namespace shasta {

// (fma2_relu01, f16_res_lo / _hi: every result passes through the packed multiply or v_cvt_pk_f16_f32 before it reaches an MFMA -
// hazard rule of pieces.hpp)

// ---- pack: the three second layers as A operands of v_mfma_f32_16x16x32_f16 -----------------------------------------------
// fragments (1 KB each = [64 lanes][8 fp16]): 0 fuse_shape.2 (16 x 32) | 1, 2 res_coeff.2 (16 x 64, two k steps) | 3 fuse_det.2
// (8 x 32, rows 8..15 zero); lane (i = lane & 15, kb = lane >> 4) holds W[i][32 ks + 8 kb + j] * 2^e_mlp; high pieces then low pieces.
// layout (dwords): [piece 2][fragment 4][lane 64][4], then 3 int exponents (fs, rc, fd), padded to 4 (P16_FRAG_DW, pair_layout.hpp).
// Behind them, in the p16w section (free at F = 256), for PAIR_SELECT (P16_SEL_DW): [piece 2][instruction 8][lane 64][4].  An activation word is [hi | lo] of ONE real k, so
// an instruction's 32 k are 16 real k, each twice: lane (i, kb) holds W[i][16 c + 4 kb + jj] 2^e_mlp, jj < 4, in BOTH halves of dword
// jj - the fragments [Wh|Wh] and [Wl|Wl], all four piece products.  c = 0, 1 fuse_shape.2 | 2 .. 5 res_coeff.2 | 6, 7 fuse_det.2.
// And (P16_SUM_DW) float wsum = high + low piece (exact in fp32) as [k][j] per MLP: what row_select_kernel multiplies a track's
// words by.

__global__ __launch_bounds__(256) void pair_f16_pack_kernel(PairF16PackArgs a) {
    __shared__ float red[3][4];
    __shared__ int ex[3];
    const int tid = threadIdx.x;
    const float* W[3] = {a.w_fs2, a.w_rc2, a.w_fd2};
    const int cnt[3] = {16 * 32, 16 * 64, 8 * 32};
    pair2_range_exponents(W, cnt, a.out, P16_FRAG_DW, red, ex);
    const int lane = tid & 63, frag = tid >> 6;  // 4 fragments, one wave each
    const int i = lane & 15, kb = lane >> 4;
    const int mlp = frag == 0 ? 0 : frag == 3 ? 2 : 1;
    const int rows = mlp == 2 ? 8 : 16, kin = mlp == 1 ? 64 : 32, ks = frag == 2 ? 1 : 0;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = i < rows ? __builtin_ldexpf(W[mlp][i * kin + 32 * ks + 8 * kb + j], ex[mlp]) : 0.0f;
    store_weight_pieces(v, a.out, 4, frag, lane);
    // select fragments: two instructions per wave
    for (int c = 2 * frag; c < 2 * frag + 2; ++c) {
        const int m = c < 2 ? 0 : c < 6 ? 1 : 2, c0 = c < 2 ? 0 : c < 6 ? 2 : 6;
        const int mrows = m == 2 ? 8 : 16, mkin = m == 1 ? 64 : 32;
        u32x4 hi, lo;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
            const float x = i < mrows ? __builtin_ldexpf(W[m][i * mkin + 16 * (c - c0) + 4 * kb + jj], ex[m]) : 0.0f;
            _Float16 h, l;
            cut2_f16(x, h, l);
            hi[jj] = pack_f16x2(h, h);
            lo[jj] = pack_f16x2(l, l);
        }
        reinterpret_cast<u32x4*>(a.out + P16_SEL_DW)[(0 * 8 + c) * 64 + lane] = hi;
        reinterpret_cast<u32x4*>(a.out + P16_SEL_DW)[(1 * 8 + c) * 64 + lane] = lo;
    }
    float* wsum = reinterpret_cast<float*>(a.out + P16_SUM_DW);
    for (int e = tid; e < PAIR_SEL_SUM; e += 256) {
        // [k][j]: rc [64][16] | fs [32][16] | fd [32][8]
        const int m = e < 1024 ? 1 : e < 1536 ? 0 : 2, el = e < 1024 ? e : e < 1536 ? e - 1024 : e - 1536;
        const int nj = m == 2 ? 8 : 16, mkin = m == 1 ? 64 : 32, k = el / nj, j = el - k * nj;
        _Float16 h, l;
        cut2_f16(__builtin_ldexpf(W[m][j * mkin + k], ex[m]), h, l);
        wsum[e] = (float)h + (float)l;
    }
}

int pair_f16_pack(const shasta_weights* w, float* out, hipStream_t st) {
    hipLaunchKernelGGL(pair_f16_pack_kernel, dim3(1), dim3(256), 0, st, pair_f16_pack_args(w, out));
    return check_launch("pair_f16_pack");
}

// ---- the kernel (F = 256: H1 = 32, R1 = 64, fuse_det 32; H2 = 16, R2 = 16, 8) ---------------------------------------------
constexpr int PF_TS = 44;  // floats per pair in the transposition tile: 40 + 4 pad (conflict-free b128 reads at stride 44)
constexpr int GR_ROW = 136;  // GRID: fp16 per row of the detection tile: 128 + 8 pad (272 B)

// dynamic LDS of pair_f16_kernel (float offsets): the kernel carves it, the launcher sizes it.  GRID: the detection tile holds fp16
// pieces - [64][GR_ROW] high pieces, then the same of low pieces, 1 KB more than the fp32 tile - and every wave has a row of UP pieces
// behind the transposition tiles
template <int WPB, PairF16Mode MODE>
struct PairF16Lds {
    static constexpr bool GRID = MODE == PAIR_GRID, SEL = MODE == PAIR_SELECT;
    static constexpr int US = PairDims(256).ET + 4;               // floats per row of the fp32 detection tile
    static constexpr int uc = 0;                                  // [64][US], GRID: [2][64][GR_ROW / 2] words
    static constexpr int ucl = uc + 64 * (GR_ROW / 2);            // GRID: the low pieces
    // [a4_total(256)] 4x4x1 operand table (layers 3-4 and the layer-2 biases)
    static constexpr int a4 = uc + (GRID ? 2 * 64 * (GR_ROW / 2) : 64 * US);
    static constexpr int up = a4 + pad4(a4_total(256));           // [WPB][3 slots][UP_SLOT]
    static constexpr int tr = up + WPB * 3 * UP_SLOT;             // [WPB][64 pairs][PF_TS]
    static constexpr int upp = tr + WPB * 64 * PF_TS;             // GRID: [WPB][2][64] words; SEL: [WPB][128] words
    static constexpr size_t bytes = (size_t)(upp + (GRID || SEL ? WPB * 128 : 0)) * sizeof(float);
};
// PAIR_SELECT: the detection tile holds select words in the fp32 tile's layout and size, and every wave a row of its track's words
static_assert(PairF16Lds<8, PAIR_GRID>::bytes == 162032 && PairF16Lds<8, PAIR_SELECT>::bytes == 161008, "the sizes the launcher spells out");
// floats of a wave's UP slot: [ET row embeddings | 16 hand floats | PAIR_SEL_ROW floats S[t] (PAIR_SELECT)]
constexpr int UPS_SEL = 128 + 16;
static_assert(UPS_SEL + PAIR_SEL_ROW <= UP_SLOT);

// GRID (SHASTA_OPT_F16GRID_PAIR, opt-in): the pieces of h1 are not cut per pair.  UP[t] and UC[d] are cut ONCE per row into two
// fp16 pieces on a common fixed grid per MLP - high piece an integer, low piece a multiple of 2^-11, after scaling the largest
// possible |UP| + |UC| of the (workgroup's tracks, detection tile) to at most 2^11 -, so that per pair the pieces of UP + UC are
// two exact packed adds and its ReLU two packed maxima (h' = max(h, -1), l' = max(l, -h'): for h >= 1 both pieces stay, for h = 0
// the low piece is clamped at 0, for h <= -1 the two cancel): 256 packed fp16 instructions per track and wave instead of 384
// conversions / mixes / packed fp32 ops.  The price is accuracy: a fixed grid spends its 22 bits on the LARGEST sum of the tile
// (tools/pair_quant_sim.py: max / rms error of `residual` 2x / 5x the fp32 kernels', 1e-6 of its range), which is why this is
// not the default arithmetic.

template <int WPB, PairF16Mode MODE>
__global__ __launch_bounds__(64 * WPB) void pair_f16_kernel(const float* __restrict__ packed, const uint32_t* __restrict__ p16,
                                                       const float* __restrict__ UP, const float* __restrict__ UC,
                                                       const float* __restrict__ hand_prev, const float* __restrict__ hand_det,
                                                       const float* __restrict__ sel_prev, const float* __restrict__ denom, float* __restrict__ residual, int T,
                                                       int D, int ld, int nf, int TWG, int TA, int TB) {
    // TWG tracks per workgroup: TA to each of the waves 0 .. 3, TB to each of the waves 4 .. 7 (launch_pair_f16: the two waves of a
    // SIMD do not advance at the same rate)
    constexpr int F = 256;
    constexpr bool GRID = MODE == PAIR_GRID, SEL = MODE == PAIR_SELECT;
    constexpr PairDims dm(F);
    constexpr int ET = dm.ET;
    static_assert(dm.H1 == 32 && dm.R1 == 64 && ET == 128 && dm.H2 == 16 && dm.R2 == 16, "pair_f16_kernel is laid out for F = 256");
    using Lds = PairF16Lds<WPB, MODE>;
    constexpr int US = Lds::US;
    extern __shared__ __attribute__((aligned(16))) float s_dynh[];
    float* s_a4 = s_dynh + Lds::a4;
    float* s_up = s_dynh + Lds::up;
    float* s_tr = s_dynh + Lds::tr;
    // (all piece storage is written and read as 32-bit words = fp16 pairs: one access type, no type punning through memory)
    uint32_t* s_uch = reinterpret_cast<uint32_t*>(s_dynh + Lds::uc);
    uint32_t* s_ucl = reinterpret_cast<uint32_t*>(s_dynh + Lds::ucl);
    uint32_t* s_upp = reinterpret_cast<uint32_t*>(s_dynh + Lds::upp);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    // (Placing the 8 detection tiles of a frame-pair on ONE XCD - they all read that frame-pair's UP / hand tables, 265 KB, which with
    // the plain order is fetched into eight L2s - was measured: 1.5 % less energy per step, pair kernel 4.21 - 4.30 -> 4.35 ms; not kept.)
    int lbx, by, b;
    xcd_logical_block(lbx, by, b);  // the detection tiles of a frame on one XCD: its UP / UC rows come from HBM once
    const int d0 = lbx * 64;
    const int d = d0 + lane, dcl = min(d, D - 1);
    {
        a4_stage<F, 64 * WPB>(packed, s_a4, tid);
    }
    float hd[12];
    // largest |UC| of this lane's detection row (row_prep), then of the whole 64-detection tile
    float mc = load_hand_det(hand_det + ((size_t)b * D + dcl) * 16, hd);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mc = absmax_keep_nan(mc, __shfl_xor(mc, off, 64));  // a NaN / inf row maximum survives
    const float dnm = denom[(size_t)b * D + dcl], rdn = 1.0f / dnm;
    // GRID: one grid per MLP for all tracks of this workgroup and the detections of this tile.  Largest magnitudes per column range
    // (hand slots: 14 fuse_shape, 15 res_coeff, 13 = all columns, the bound used for fuse_det) of the tile's UC rows and of the
    // workgroup's UP rows; ge[r] = the exponent that puts their sum into (2^10, 2^11].
    int ge[3] = {0, 0, 0};
    bool grid_finite = true;
    if constexpr (GRID) {
        float mcr[3], mur[3] = {0.0f, 0.0f, 0.0f};
        {
            const float* h = hand_det + ((size_t)b * D + dcl) * 16;
            mcr[0] = h[14];
            mcr[1] = h[15];
            mcr[2] = h[13];
        }
        const int tw0 = by * TWG, tw1 = min(T, tw0 + TWG);
        for (int t = tw0 + tid; t < tw1; t += 64 * WPB) {
            const float* h = hand_prev + ((size_t)b * T + t) * 16;
            mur[0] = absmax_keep_nan(mur[0], h[14]);
            mur[1] = absmax_keep_nan(mur[1], h[15]);
            mur[2] = absmax_keep_nan(mur[2], h[13]);
        }
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                mcr[r] = absmax_keep_nan(mcr[r], __shfl_xor(mcr[r], off, 64));
                mur[r] = absmax_keep_nan(mur[r], __shfl_xor(mur[r], off, 64));
            }
        float* red = s_tr;  // scratch: the transposition tiles are not in use yet
        if (lane == 0) {
            red[wid * 3 + 0] = mur[0];
            red[wid * 3 + 1] = mur[1];
            red[wid * 3 + 2] = mur[2];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            float m = red[r];
            for (int w = 1; w < WPB; ++w) m = absmax_keep_nan(m, red[w * 3 + r]);
            // (+ 0.2 %: the two high pieces are rounded to integers separately, their sum must stay below 2048, where fp16 still
            // holds every integer)
            const float bound = (m + mcr[r]) * 1.002f;
            grid_finite = grid_finite && (bound < INFINITY);
            ge[r] = range_exponent_bits(__float_as_uint(bound)) - 3;
        }
        __syncthreads();  // red is read by everyone before the tiles are written
        // the tile: UC rows cut on the grids
        const f32x4* src = reinterpret_cast<const f32x4*>(UC);
        for (int e = tid; e < 64 * (ET / 4); e += 64 * WPB) {
            const int r = e / (ET / 4), c = e - r * (ET / 4);  // float4 c = columns 4 c .. 4 c + 3: one MLP range
            const f32x4 v = src[((size_t)b * D + min(d0 + r, D - 1)) * (ET / 4) + c];
            const int ex = c < 8 ? ge[0] : c < 24 ? ge[1] : ge[2];
            _Float16 hh[4], ll[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float sv = __builtin_ldexpf(v[q], ex), hi = rintf(sv);
                hh[q] = (_Float16)hi;
                ll[q] = (_Float16)(rintf((sv - hi) * 2048.0f) * (1.0f / 2048.0f));
            }
            typedef uint32_t pu2 __attribute__((ext_vector_type(2)));
            typedef _Float16 ph2t __attribute__((ext_vector_type(2)));
            *reinterpret_cast<pu2*>(s_uch + r * (GR_ROW / 2) + 2 * c) =
                pu2{__builtin_bit_cast(uint32_t, ph2t{hh[0], hh[1]}), __builtin_bit_cast(uint32_t, ph2t{hh[2], hh[3]})};
            *reinterpret_cast<pu2*>(s_ucl + r * (GR_ROW / 2) + 2 * c) =
                pu2{__builtin_bit_cast(uint32_t, ph2t{ll[0], ll[1]}), __builtin_bit_cast(uint32_t, ph2t{ll[2], ll[3]})};
        }
    }
    // PAIR_SELECT: ONE scale for all tracks of this workgroup and the detections of this tile - the exponent that puts (largest finite
    // |UP| of the workgroup's tracks + largest |UC| of the tile) into (2^13, 2^14] -, because a pair's two words must be comparable.
    // A track whose own maximum is not finite takes no part in it (it gets NaN below, its neighbours keep their scale); a non-finite
    // tile maximum makes the bound non-finite: NaN for the tile.
    int e_sel = 0;
    bool sel_finite = true;
    uint32_t* s_ucw = reinterpret_cast<uint32_t*>(s_dynh + Lds::uc);  // the tile as select words, laid out like the fp32 tile
    if constexpr (SEL) {
        float mu = 0.0f;
        const int tw0 = by * TWG, tw1 = min(T, tw0 + TWG);
        for (int t = tw0 + tid; t < tw1; t += 64 * WPB) {
            const float m = hand_prev[((size_t)b * T + t) * 16 + 13];
            if (m < INFINITY) mu = fmaxf(mu, m);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mu = fmaxf(mu, __shfl_xor(mu, off, 64));
        float* red = s_tr;  // scratch: the transposition tiles are not in use yet
        if (lane == 0) red[wid] = mu;
        __syncthreads();
        mu = red[0];
        for (int w = 1; w < WPB; ++w) mu = fmaxf(mu, red[w]);
        const float bound = mu + mc;
        sel_finite = bound < INFINITY;  // false for NaN and +inf
        e_sel = range_exponent_bits(__float_as_uint(bound));
        __syncthreads();  // red is read by everyone before the tiles are written
        const f32x4* src = reinterpret_cast<const f32x4*>(UC);
#pragma unroll 2
        for (int e = tid; e < 64 * (ET / 4); e += 64 * WPB) {
            const int r = e / (ET / 4), c = e - r * (ET / 4);
            // float4 c of the row = the four real k of MFMA instruction c >> 2, k block c & 3: stored k-block-major, the blocks in the
            // order 0, 2, 1, 3 and 64 words apart in pairs - the fp32 tile's bank layout (load_uc below), read with the same addresses
            const int cp = ((c & 1) << 6) | (((c >> 1) & 1) << 5) | ((c >> 2) << 2);
            const f32x4 v = src[((size_t)b * D + min(d0 + r, D - 1)) * (ET / 4) + c];
            *reinterpret_cast<u32x4*>(&s_ucw[r * US + cp]) =
                u32x4{cut_select_word(__builtin_ldexpf(v[0], e_sel)), cut_select_word(__builtin_ldexpf(v[1], e_sel)),
                      cut_select_word(__builtin_ldexpf(v[2], e_sel)), cut_select_word(__builtin_ldexpf(v[3], e_sel))};
        }
    }
    // second-layer weight pieces: 4 fragments x {high, low} (PAIR_SELECT: 8 instructions x {[Wh|Wh], [Wl|Wl]}), registers for the
    // whole kernel
    u32x4 wh[4], wl[4], sh[8], sl[8];
    if constexpr (SEL) {
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            sh[c] = reinterpret_cast<const u32x4*>(p16 + P16_SEL_DW)[(0 * 8 + c) * 64 + lane];
            sl[c] = reinterpret_cast<const u32x4*>(p16 + P16_SEL_DW)[(1 * 8 + c) * 64 + lane];
        }
    } else {
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            wh[f] = reinterpret_cast<const u32x4*>(p16)[(0 * 4 + f) * 64 + lane];
            wl[f] = reinterpret_cast<const u32x4*>(p16)[(1 * 4 + f) * 64 + lane];
        }
    }
    const int ew_fs = reinterpret_cast<const int*>(p16)[P16_FRAG_DW + 0], ew_rc = reinterpret_cast<const int*>(p16)[P16_FRAG_DW + 1],
              ew_fd = reinterpret_cast<const int*>(p16)[P16_FRAG_DW + 2];
    __syncthreads();
    const A4Lane a4l(s_a4, lane);
    const f32x4 zero4 = {0, 0, 0, 0};
    const int p = lane & 15, kb = lane >> 4;
    float* my_tr = s_tr + wid * (64 * PF_TS);

    const int t_beg = by * TWG + (wid < 4 ? wid * TA : 4 * TA + (wid - 4) * TB);
    const int t_end = min(min(T, (by + 1) * TWG), t_beg + (wid < 4 ? TA : TB));
    float* my_up = s_up + wid * (3 * UP_SLOT);
    const bool hp_lane = lane >= ET / 4 && lane < ET / 4 + 4;
    const bool sv_lane = SEL && lane >= UPS_SEL / 4 && lane < (UPS_SEL + PAIR_SEL_ROW) / 4;  // PAIR_SELECT: the track's S[t] behind its hand row
    const int up_lane = 4 * min(lane, ET / 4 - 1), hp_off = 4 * (lane - ET / 4), sv_off = 4 * (lane - UPS_SEL / 4);
    // (one copy per kernel: as a function in pair_lane.hpp it changed this kernel's schedule)
    auto dma_up = [&](int row, int slot) {
        const size_t r = (size_t)b * T + min(row, T - 1);
        const float* src = hp_lane ? hand_prev + r * 16 + hp_off : sv_lane ? sel_prev + r * PAIR_SEL_ROW + sv_off : UP + r * ET + up_lane;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(my_up + slot * UP_SLOT), 16, 0, 0);
    };
    if (t_beg < t_end) {
        dma_up(t_beg, 0);
        dma_up(t_beg + 1, 1);
    }
    for (int t = t_beg; t < t_end; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        dma_up(t + 2, (t - t_beg + 2) % 3);
        unsigned upo = (unsigned)(unsigned long long)(my_up + ((t - t_beg) % 3) * UP_SLOT);
        asm volatile("" : "+v"(upo));
        const lfloat* up = (const lfloat*)(unsigned long long)upo;
        float hp[16];  // (read back here: through a function of pair_lane.hpp the register allocation moved)
        {
            const f32x4 h0 = *reinterpret_cast<const lf32x4*>(up + ET), h1 = *reinterpret_cast<const lf32x4*>(up + ET + 4),
                        h2 = *reinterpret_cast<const lf32x4*>(up + ET + 8), h3 = *reinterpret_cast<const lf32x4*>(up + ET + 12);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                hp[k] = h0[k];
                hp[4 + k] = h1[k];
                hp[8 + k] = h2[k];
                hp[12 + k] = h3[k];
            }
        }
        typedef _Float16 ph2 __attribute__((ext_vector_type(2)));
        bool finite_bound;
        int e1 = 0;
        u32x4 uph[GRID ? 4 : 1], upl[GRID ? 4 : 1];  // GRID: this lane's UP pieces, 8 per k step
        float upw[SEL ? 32 : 1];  // PAIR_SELECT: this lane's words of -UP[t], 4 per MFMA instruction
        if constexpr (SEL) {
            // a track whose bound is not finite gets NaN for the whole tile, as in the other forms
            finite_bound = sel_finite && hp[13] < INFINITY;
            // the track's -UP row cut by the wave into its word row: lane L cuts columns 2 L, 2 L + 1; every lane then reads the four
            // words of its k block per instruction back (LDS broadcast within a k block)
            uint32_t* my_p = s_upp + wid * 128;
            {
                typedef __attribute__((address_space(3))) f32x2 lf32x2;
                typedef uint32_t pu2 __attribute__((ext_vector_type(2)));
                const f32x2 v = *reinterpret_cast<const lf32x2*>(up + 2 * lane);
                *reinterpret_cast<pu2*>(my_p + 2 * lane) =
                    pu2{cut_select_word(__builtin_ldexpf(-v[0], e_sel)), cut_select_word(__builtin_ldexpf(-v[1], e_sel))};
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const f32x4 w4 = __builtin_bit_cast(f32x4, *reinterpret_cast<const u32x4*>(my_p + 16 * c + 4 * kb));
                upw[4 * c] = w4[0];
                upw[4 * c + 1] = w4[1];
                upw[4 * c + 2] = w4[2];
                upw[4 * c + 3] = w4[3];
            }
        } else {
            finite_bound = grid_finite;
            // the track's UP row cut on the grids: lane L cuts columns 2 L, 2 L + 1 (L < 16: fuse_shape, < 48: res_coeff, else fuse_det)
            // into the wave's piece rows; every lane then reads its 8 values per k step back (LDS broadcast within a k block)
            uint32_t* my_p = s_upp + wid * 128;  // [high 64 words | low 64 words]
            {
                typedef __attribute__((address_space(3))) f32x2 lf32x2;
                const f32x2 v = *reinterpret_cast<const lf32x2*>(up + 2 * lane);
                const int ex = lane < 16 ? ge[0] : lane < 48 ? ge[1] : ge[2];
                const float s0 = __builtin_ldexpf(v[0], ex), s1 = __builtin_ldexpf(v[1], ex);
                const float h0 = rintf(s0), h1v = rintf(s1);
                const ph2 hh = {(_Float16)h0, (_Float16)h1v};
                const ph2 ll = {(_Float16)(rintf((s0 - h0) * 2048.0f) * (1.0f / 2048.0f)), (_Float16)(rintf((s1 - h1v) * 2048.0f) * (1.0f / 2048.0f))};
                my_p[lane] = __builtin_bit_cast(uint32_t, hh);
                my_p[64 + lane] = __builtin_bit_cast(uint32_t, ll);
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                uph[s] = *reinterpret_cast<const u32x4*>(my_p + 16 * s + 4 * kb);
                upl[s] = *reinterpret_cast<const u32x4*>(my_p + 64 + 16 * s + 4 * kb);
            }
        }
        // Software pipeline over the four sub-steps: the UC reads of sub-step s+1 are issued before the arithmetic of sub-step s,
        // and the pieces of sub-step s+1 are cut before the MFMAs of sub-step s are issued (they run under the cut of s+1).
        auto load_uc = [&](int sub, f32x4 (&u)[8]) {
            if constexpr (GRID) {
                // u[0..3] = the high pieces of the four k steps (8 fp16 each), u[4..7] = the low pieces
                const uint32_t* hr = s_uch + (16 * sub + p) * (GR_ROW / 2) + 4 * kb;
                const uint32_t* lr = s_ucl + (16 * sub + p) * (GR_ROW / 2) + 4 * kb;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    u[s] = __builtin_bit_cast(f32x4, *reinterpret_cast<const u32x4*>(hr + 16 * s));
                    u[4 + s] = __builtin_bit_cast(f32x4, *reinterpret_cast<const u32x4*>(lr + 16 * s));
                }
                return;
            }
            // (PAIR_SELECT reads its tile in load_w below)
        };
        auto cut = [&](const f32x4 (&u)[8], u32x4 (&xh)[4], u32x4 (&xl)[4]) {
            if constexpr (GRID) {
                // pieces of relu(UP + UC): exact packed adds, then h' = max(h, -1), l' = max(l, -h'); on whole 8-halves vectors (the
                // compiler lowers them to v_pk_add_f16 / v_pk_max_f16 with the negation as an operand modifier; written dword by dword
                // through bit casts of vector elements hipcc 7.2 computed element 0 only and replicated it)
                const _Float16 m1 = (_Float16)-1.0f;
                const f16x8 neg1 = {m1, m1, m1, m1, m1, m1, m1, m1};
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const f16x8 h = __builtin_bit_cast(f16x8, u[s]) + __builtin_bit_cast(f16x8, uph[s]);
                    const f16x8 l = __builtin_bit_cast(f16x8, u[4 + s]) + __builtin_bit_cast(f16x8, upl[s]);
                    const f16x8 h2 = __builtin_elementwise_max(h, neg1);
                    const f16x8 l2 = __builtin_elementwise_max(l, -h2);
                    xh[s] = __builtin_bit_cast(u32x4, h2);
                    xl[s] = __builtin_bit_cast(u32x4, l2);
                }
                return;
            }
        };
        auto mma = [&](const u32x4 (&xh)[4], const u32x4 (&xl)[4], f32x4& a_fs, f32x4& a_rc, f32x4& a_fd) {
            a_fs = a_rc = a_fd = zero4;
            a_fs = mfma_16x16x32_f16(wl[0], xh[0], a_fs);
            a_rc = mfma_16x16x32_f16(wl[1], xh[1], a_rc);
            a_fd = mfma_16x16x32_f16(wl[3], xh[3], a_fd);
            a_fs = mfma_16x16x32_f16(wh[0], xl[0], a_fs);
            a_rc = mfma_16x16x32_f16(wh[1], xl[1], a_rc);
            a_fd = mfma_16x16x32_f16(wh[3], xl[3], a_fd);
            a_rc = mfma_16x16x32_f16(wl[2], xh[2], a_rc);
            a_fs = mfma_16x16x32_f16(wh[0], xh[0], a_fs);
            a_fd = mfma_16x16x32_f16(wh[3], xh[3], a_fd);
            a_rc = mfma_16x16x32_f16(wh[2], xl[2], a_rc);
            a_rc = mfma_16x16x32_f16(wh[1], xh[1], a_rc);
            a_rc = mfma_16x16x32_f16(wh[2], xh[2], a_rc);
        };
        // (storing a sub-step's results behind the NEXT sub-step's MFMAs instead of right behind their own - where each store waits
        // 5 - 7 idle states for its accumulator - measured slower: 4.20 -> 4.30 ms; the compiler fills those states elsewhere)
        auto store = [&](int sub, const f32x4& a_fs, const f32x4& a_rc, const f32x4& a_fd) {
            // lane (p, kb) holds output features 4 kb .. 4 kb + 3 of pair 16 sub + p: [rc 16 | fs 16 | fd 8]
            float* row = my_tr + (16 * sub + p) * PF_TS + 4 * kb;
            *reinterpret_cast<f32x4*>(row) = a_rc;
            *reinterpret_cast<f32x4*>(row + 16) = a_fs;
            if (kb < 2) *reinterpret_cast<f32x4*>(row + 32) = a_fd;
        };
        // PAIR_SELECT, per sub-step: the lane's 32 UC words (8 instructions x 4 real k), 32 v_max_f32 against the track's words IN
        // PLACE - the word of the larger of UC[d][k] and -UP[t][k], cut_select_word's ordering contract -, 16 MFMAs.  The maxima are
        // inline asm: from fmaxf the compiler cannot know that no word is a signalling NaN and canonicalises both operands first
        // (three instructions per maximum).  Each statement ends with the two wait states a VALU result needs before an MFMA reads it
        // (pieces.hpp, hazard rule).
        auto load_w = [&](int sub, float (&x)[32]) {
            const uint32_t* ucr = s_ucw + (16 * sub + p) * US + ((kb & 1) << 6) + ((kb >> 1) << 5);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const f32x4 w4 = __builtin_bit_cast(f32x4, *reinterpret_cast<const u32x4*>(ucr + 4 * c));
                x[4 * c] = w4[0];
                x[4 * c + 1] = w4[1];
                x[4 * c + 2] = w4[2];
                x[4 * c + 3] = w4[3];
            }
        };
        auto pick = [&](float (&x)[32]) {
#pragma unroll
            for (int q = 0; q < 32; q += 8)
                asm("v_max_f32 %0, %0, %8\n\tv_max_f32 %1, %1, %9\n\tv_max_f32 %2, %2, %10\n\tv_max_f32 %3, %3, %11\n\t"
                    "v_max_f32 %4, %4, %12\n\tv_max_f32 %5, %5, %13\n\tv_max_f32 %6, %6, %14\n\tv_max_f32 %7, %7, %15\n\ts_nop 1"
                    : "+v"(x[q]), "+v"(x[q + 1]), "+v"(x[q + 2]), "+v"(x[q + 3]), "+v"(x[q + 4]), "+v"(x[q + 5]), "+v"(x[q + 6]), "+v"(x[q + 7])
                    : "v"(upw[SEL ? q : 0]), "v"(upw[SEL ? q + 1 : 0]), "v"(upw[SEL ? q + 2 : 0]), "v"(upw[SEL ? q + 3 : 0]),
                      "v"(upw[SEL ? q + 4 : 0]), "v"(upw[SEL ? q + 5 : 0]), "v"(upw[SEL ? q + 6 : 0]), "v"(upw[SEL ? q + 7 : 0]));
        };
        // per accumulator small to large: the [Wl|Wl] instructions, then the [Wh|Wh] ones (fs: c = 0, 1; rc: 2 .. 5; fd: 6, 7)
        auto mma_sel = [&](const float (&x)[32], f32x4& a_fs, f32x4& a_rc, f32x4& a_fd) {
            u32x4 xv[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) xv[c] = __builtin_bit_cast(u32x4, f32x4{x[4 * c], x[4 * c + 1], x[4 * c + 2], x[4 * c + 3]});
            a_fs = a_rc = a_fd = zero4;
            a_fs = mfma_16x16x32_f16(sl[0], xv[0], a_fs);
            a_rc = mfma_16x16x32_f16(sl[2], xv[2], a_rc);
            a_fd = mfma_16x16x32_f16(sl[6], xv[6], a_fd);
            a_fs = mfma_16x16x32_f16(sl[1], xv[1], a_fs);
            a_rc = mfma_16x16x32_f16(sl[3], xv[3], a_rc);
            a_fd = mfma_16x16x32_f16(sl[7], xv[7], a_fd);
            a_rc = mfma_16x16x32_f16(sl[4], xv[4], a_rc);
            a_fs = mfma_16x16x32_f16(sh[0], xv[0], a_fs);
            a_rc = mfma_16x16x32_f16(sl[5], xv[5], a_rc);
            a_fd = mfma_16x16x32_f16(sh[6], xv[6], a_fd);
            a_rc = mfma_16x16x32_f16(sh[2], xv[2], a_rc);
            a_fs = mfma_16x16x32_f16(sh[1], xv[1], a_fs);
            a_rc = mfma_16x16x32_f16(sh[3], xv[3], a_rc);
            a_fd = mfma_16x16x32_f16(sh[7], xv[7], a_fd);
            a_rc = mfma_16x16x32_f16(sh[4], xv[4], a_rc);
            a_rc = mfma_16x16x32_f16(sh[5], xv[5], a_rc);
        };
        if constexpr (SEL) {
            // one buffer per sub-step in flight: the words of sub-step s + 2 are read into the buffer whose MFMAs have been issued
            float xa[32], xb[32];
            f32x4 fsA, rcA, fdA, fsB, rcB, fdB;
            load_w(0, xa);
            load_w(1, xb);
            pick(xa);
            mma_sel(xa, fsA, rcA, fdA);
            load_w(2, xa);
            store(0, fsA, rcA, fdA);
            pick(xb);
            mma_sel(xb, fsB, rcB, fdB);
            load_w(3, xb);
            store(1, fsB, rcB, fdB);
            pick(xa);
            mma_sel(xa, fsA, rcA, fdA);
            store(2, fsA, rcA, fdA);
            pick(xb);
            mma_sel(xb, fsB, rcB, fdB);
            store(3, fsB, rcB, fdB);
        } else {
            f32x4 ua[8], ub[8];
            u32x4 xha[4], xla[4], xhb[4], xlb[4];
            f32x4 fsA, rcA, fdA, fsB, rcB, fdB;
            load_uc(0, ua);
            load_uc(1, ub);
            cut(ua, xha, xla);
            load_uc(2, ua);
            cut(ub, xhb, xlb);
            mma(xha, xla, fsA, rcA, fdA);
            store(0, fsA, rcA, fdA);
            load_uc(3, ub);
            cut(ua, xha, xla);
            mma(xhb, xlb, fsB, rcB, fdB);
            store(1, fsB, rcB, fdB);
            cut(ub, xhb, xlb);
            mma(xha, xla, fsA, rcA, fdA);
            store(2, fsA, rcA, fdA);
            mma(xhb, xlb, fsB, rcB, fdB);
            store(3, fsB, rcB, fdB);
        }
        // ---- lane = pair from here on: descale + bias, layers 3-4, hand residual, combine (as pair_mfma4_kernel) ----
        const lfloat *arow, *abias;
        a4l.per_track(arow, abias);
        // exact descaling: one exponent per track (default form) or one per MLP and workgroup (GRID)
        if constexpr (SEL) e1 = e_sel;
        const float i_rc = __builtin_ldexpf(1.0f, -((GRID ? ge[1] : e1) + ew_rc)), i_fs = __builtin_ldexpf(1.0f, -((GRID ? ge[0] : e1) + ew_fs)),
                    i_fd = __builtin_ldexpf(1.0f, -((GRID ? ge[2] : e1) + ew_fd));
        f32x4 a_rc2[4], a_fs2[4], a_fd2[2];
        {
            const float* mine = my_tr + lane * PF_TS;
            // the layer-2 biases sit behind the 4x4x1 operands of their layers in the LDS table ([ob][i], A4<..>::BIAS)
            const float* b_rc = s_a4 + A4<F, L_RC2>::OFF + A4<F, L_RC2>::BIAS;
            const float* b_fs = s_a4 + A4<F, L_FS2>::OFF + A4<F, L_FS2>::BIAS;
            const float* b_fd = s_a4 + A4<F, L_FD2>::OFF + A4<F, L_FD2>::BIAS;
            // PAIR_SELECT: the addend is the track's S[t] = bias + W2 UP[t] (the "+ u" of relu(u + v) = max(v, -u) + u through the linear
            // layer; row_prep's select role), fetched with the track's row, in the tile's order [rc 16 | fs 16 | fd 8]
            const lfloat* sv = up + UPS_SEL;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 c_rc = SEL ? *reinterpret_cast<const lf32x4*>(sv + 4 * g) : *reinterpret_cast<const f32x4*>(b_rc + 4 * g);
                const f32x4 c_fs = SEL ? *reinterpret_cast<const lf32x4*>(sv + 16 + 4 * g) : *reinterpret_cast<const f32x4*>(b_fs + 4 * g);
                a_rc2[g] = a4_descale_relu(*reinterpret_cast<const f32x4*>(mine + 4 * g), i_rc, c_rc);
                a_fs2[g] = a4_descale_relu(*reinterpret_cast<const f32x4*>(mine + 16 + 4 * g), i_fs, c_fs);
            }
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                const f32x4 c_fd = SEL ? *reinterpret_cast<const lf32x4*>(sv + 32 + 4 * g) : *reinterpret_cast<const f32x4*>(b_fd + 4 * g);
                a_fd2[g] = a4_descale_relu(*reinterpret_cast<const f32x4*>(mine + 32 + 4 * g), i_fd, c_fd);
            }
        }
        // All forty ReLUs of the layer-2 outputs are done before the first MFMA of layers 3-4 (the empty asm pins them there): a VALU
        // result read by the MFMA right behind it costs two wait states, and the compiler had put one v_max + s_nop 1 in front of
        // every 4x4x1.  With the third layers interleaved below: 53 -> 36 s_nop per track, pair kernel 4.73 - 4.95 -> 4.56 - 4.62 ms.
        asm volatile("" : "+v"(a_rc2[0]), "+v"(a_rc2[1]), "+v"(a_rc2[2]), "+v"(a_rc2[3]), "+v"(a_fs2[0]), "+v"(a_fs2[1]), "+v"(a_fs2[2]),
                     "+v"(a_fs2[3]), "+v"(a_fd2[0]), "+v"(a_fd2[1]));
        f32x4 a_rc3[A4<F, L_RC3>::NOB], a_fs3[A4<F, L_FS3>::NOB], a_fs4[A4<F, L_FS4>::NOB], a_fd3[A4<F, L_FD3>::NOB];
        {
            // the three third layers side by side: every accumulator is touched once per round, so no 4x4x1 waits for the one before it
            // (one copy per fp16 kernel: a function shared by the two changed both schedules)
            using RC = A4<F, L_RC3>;
            using FS = A4<F, L_FS3>;
            using FD = A4<F, L_FD3>;
            static_assert(RC::NOB == 1 && FS::NOB == 2 && FD::NOB == 1 && RC::KG == 4 && FS::KG == 4 && FD::KG == 2, "F = 256");
            a4_init<RC>(abias, a_rc3);
            a4_init<FS>(abias, a_fs3);
            a4_init<FD>(abias, a_fd3);
#pragma unroll
            for (int kg = 0; kg < 4; ++kg) {
                const f32x4 w_rc = *reinterpret_cast<const lf32x4*>(arow + RC::OFF + kg * 16);
                const f32x4 w_f0 = *reinterpret_cast<const lf32x4*>(arow + FS::OFF + kg * 16);
                const f32x4 w_f1 = *reinterpret_cast<const lf32x4*>(arow + FS::OFF + (FS::KG + kg) * 16);
                f32x4 w_fd = zero4;
                if (kg < 2) w_fd = *reinterpret_cast<const lf32x4*>(arow + FD::OFF + kg * 16);
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    a_rc3[0] = MFMA4(w_rc[kk], a_rc2[kg][kk], a_rc3[0]);
                    a_fs3[0] = MFMA4(w_f0[kk], a_fs2[kg][kk], a_fs3[0]);
                    a_fs3[1] = MFMA4(w_f1[kk], a_fs2[kg][kk], a_fs3[1]);
                    if (kg < 2) a_fd3[0] = MFMA4(w_fd[kk], a_fd2[kg][kk], a_fd3[0]);
                }
            }
        }
        a4_layer<A4<F, L_FS4>, A4_RELU_FMAX>(arow, abias, a_fs3, a_fs4);

        // ---- hand-designed residual (shasta.py:277-283) ----
        const float dist = hand_dist(hp, hd, dnm, rdn);
        const float res = pair_combine(a_rc3[0], a_fd3[0][0], dist, a_fs4[0][0]);
        if (d < D) residual[((size_t)b * T + t) * ld + d] = finite_bound ? res : __builtin_nanf("");
    }
}

int launch_pair_f16(const float* packed, const float* p16, const float* UP, const float* UC, const float* hand_prev,
                    const float* hand_det, const float* sel_prev, const float* denom, float* residual, int B, int T, int D, int ld,
                    int nf, PairF16Mode mode, hipStream_t st) {
    constexpr int wpb = 8;
    // tracks per workgroup: the T tracks dealt evenly to the ny workgroups of a detection tile, ny the smallest power of two that leaves
    // 512 workgroups (two rounds of the CU array).  A workgroup's prologue - the detection tile and the operand table into LDS behind a
    // barrier - is paid once per workgroup: 5.42 / 5.23 / 5.11 / 5.05 ms for 8 / 16 / 32 / 64 tracks per wave at 512 frame-pairs.
    // Tracks per WAVE: the LDS allows one workgroup per CU, so its waves w and w + 4 share a SIMD for the whole kernel, and the SIMD
    // issues from the older wave first: stamped per wave (a clock-stamp build, removed after commit 96899a8), waves 0 .. 3 ran their tracks at the pace of a wave
    // that has the SIMD to itself (6 870 cycles per track) while waves 4 .. 7 advanced 0.625 tracks per track of theirs, then finished
    // alone - the slow way, one wave per SIMD - for the last quarter of the workgroup's time, with the CU's LDS held.  Dealing the
    // tracks 78 : 48 instead of 63 : 63 lets both finish together (within 7 us of 234): pair stage 4.41 -> 4.16 ms at 512 frame-pairs;
    // 55 : 100 and 68 : 100 measured 1 - 2 % behind 61.5 : 100.  PAIR_SELECT halved the vector instructions, the late wave finds more
    // free issue slots: 1000 : 760 now (pair stage 7.47 - 7.82 ms against 8.06 - 8.12 at 1000 : 615 and 7.71 - 8.03 at 1000 : 900, one
    // box, two rounds; profiles/pair_select_ab.txt).  (s_setprio by phase - the wave in its lane-per-pair phase first, or
    // last - with even or uneven tracks: at best equal, 7.71 against 7.65 ms at 1024 frame-pairs; not kept.)
    int ny = 1;
    while ((long)B * cdiv(D, 64) * ny < 512 && cdiv(T, wpb * ny * 2) >= 2) ny *= 2;
    const int twg = cdiv(cdiv(T, ny), wpb) * wpb;  // a multiple of the waves
    int ta = twg / wpb, tb = ta;
    if (wpb == 8) {
        const int per_simd = twg / 4;
        ta = (per_simd * 1000 + (1000 + 760) / 2) / (1000 + 760);  // to nearest; 760 tracks of a late wave per 1000 of an early one
        tb = per_simd - ta;
    }
    dim3 grd(cdiv(D, 64), cdiv(T, twg), B);
#define SHASTA_LAUNCH_PAIR_F16(MODE)                                                                                                     \
    do {                                                                                                                                  \
        constexpr size_t lds = PairF16Lds<wpb, MODE>::bytes;                                                                              \
        (void)hipFuncSetAttribute((const void*)pair_f16_kernel<wpb, MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);         \
        hipLaunchKernelGGL((pair_f16_kernel<wpb, MODE>), grd, dim3(64 * wpb), lds, st, packed, reinterpret_cast<const uint32_t*>(p16), UP, \
                           UC, hand_prev, hand_det, sel_prev, denom, residual, T, D, ld, nf, twg, ta, tb);                                \
    } while (0)
    switch (mode) {
        case PAIR_SELECT: SHASTA_LAUNCH_PAIR_F16(PAIR_SELECT); break;
        case PAIR_GRID: SHASTA_LAUNCH_PAIR_F16(PAIR_GRID); break;
    }
#undef SHASTA_LAUNCH_PAIR_F16
    return check_launch("pair_f16");
}

}  // namespace shasta
