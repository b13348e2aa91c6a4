// Split-operand arithmetic: fp32 products formed on the bf16 / fp16 matrix paths from exact pieces of the fp32 operands.
// The piece formats and the order of the piece products below decide the bits that the parity tests pin; every kernel that
// uses them takes them from here.
//
// bf16 pieces (gemm_pieces, aff_pieces, embed_rows, anchor_split NP = 3).  Every fp32 operand is cut - exactly, by truncation -
// into three bf16 pieces
//   a = a_hi + a_mid + a_lo      (8 + 8 + 8 significand bits; a_lo is exact because the remainder has at most 8 bits left)
// and  w * x  is accumulated (in the fp32 accumulator of v_mfma_f32_32x32x16_bf16) as the six piece products of weight
// 2^0 .. 2^-16:  w_lo x_hi + w_hi x_lo + w_mid x_mid + w_mid x_hi + w_hi x_mid + w_hi x_hi.
// Each bf16 x bf16 product is exact in fp32; the three dropped products are below 2^-24 |w x|, i.e. below the rounding error
// of the fp32 FMA they replace (tests/test_hip_parity.py compares the kernels with the float64 oracle: same error level).
// Six bf16 MFMAs of K = 16 replace 8 f32 MFMAs of K = 2: 2.7 x fewer matrix cycles per fp32 product.
//
// fp16 pieces (the "f16x2" default: anchor_split NP = 2, pair_f16*, aff_f16, shared_conv_f16 / _train).  a * 2^e = h + l + err with
// h = fp16(a 2^e) and l = fp16(a 2^e - h), both rounded to nearest: |err| <= 2^-24 |a 2^e|, half an ulp of the fp32 value itself.
// 2^e is an exact power of two - per row, per matrix or per block, chosen by each kernel - that puts the largest magnitude into
// (2^13, 2^14] (range_exponent_bits, common.hpp); the results are scaled back exactly.  w * x is then the THREE products
// w_l x_h + w_h x_l + w_h x_h (each exact in the fp32 accumulator of the f16 MFMA; the dropped w_l x_l is at most 2^-22 |w x|), half
// the matrix work of the six bf16 piece products.
//
// Order: the products of one accumulator are issued small to large (kProductsBf16 / kProductsF16), so that the small terms reach the
// accumulator first and are not rounded away against the large ones.  Kernels that interleave the products of several accumulators
// (pair_f16, pair_f16w, aff_f16 layer 1, shared_conv_f16 / _train) keep that order per accumulator in their hand-written schedules.
#pragma once
#include "common.hpp"

namespace shasta {

// ---- bf16 pieces ---------------------------------------------------------------------------------------------------------------

// a = h + m + l exactly, each with at most 8 significand bits (bf16-representable by truncation)
__device__ __forceinline__ void cut3_bf16(float a, float& h, float& m, float& l) {
    h = __uint_as_float(__float_as_uint(a) & 0xffff0000u);
    const float r = a - h;
    m = __uint_as_float(__float_as_uint(r) & 0xffff0000u);
    l = r - m;
}
// {bf16(even), bf16(odd)} of two floats whose low 16 bits are not needed
__device__ __forceinline__ uint32_t pack_bf16x2(float even, float odd) {
    return __builtin_amdgcn_perm(__float_as_uint(odd), __float_as_uint(even), 0x07060302u);
}
// 8 consecutive k of one operand fragment -> its three piece fragments (out[0] = high)
__device__ __forceinline__ void cut3_bf16x8(const float (&v)[8], u32x4 (&out)[3]) {
    float h[8], m[8], l[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) cut3_bf16(v[j], h[j], m[j], l[j]);
    out[0] = u32x4{pack_bf16x2(h[0], h[1]), pack_bf16x2(h[2], h[3]), pack_bf16x2(h[4], h[5]), pack_bf16x2(h[6], h[7])};
    out[1] = u32x4{pack_bf16x2(m[0], m[1]), pack_bf16x2(m[2], m[3]), pack_bf16x2(m[4], m[5]), pack_bf16x2(m[6], m[7])};
    out[2] = u32x4{pack_bf16x2(l[0], l[1]), pack_bf16x2(l[2], l[3]), pack_bf16x2(l[4], l[5]), pack_bf16x2(l[6], l[7])};
}

// ---- fp16 pieces ---------------------------------------------------------------------------------------------------------------

// a = h + l + err, both rounded to nearest (a already range-scaled)
__device__ __forceinline__ void cut2_f16(float a, _Float16& h, _Float16& l) {
    h = (_Float16)a;
    l = (_Float16)(a - (float)h);
}
// two fp16 values -> one packed pair
__device__ __forceinline__ uint32_t pack_f16x2(_Float16 even, _Float16 odd) {
    const f16x2 v = {even, odd};
    return __builtin_bit_cast(uint32_t, v);
}
// two fp32 values -> one packed fp16 pair, round to nearest even (v_cvt_pk_f16_f32)
__device__ __forceinline__ uint32_t cvt_f16x2(float a, float b) {
    const f16x2 v = {(_Float16)a, (_Float16)b};
    return __builtin_bit_cast(uint32_t, v);
}
// 8 consecutive k of one operand fragment, v(0) .. v(7), scaled by 2^e -> its high and low piece fragments
template <class V>
__device__ __forceinline__ void cut2_f16x8(V v, int e, u32x4& hi, u32x4& lo) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        _Float16 h0, l0, h1, l1;
        cut2_f16(__builtin_ldexpf(v(2 * j), e), h0, l0);
        cut2_f16(__builtin_ldexpf(v(2 * j + 1), e), h1, l1);
        hi[j] = pack_f16x2(h0, h1);
        lo[j] = pack_f16x2(l0, l1);
    }
}

// ---- select words (pair_f16.hip, PAIR_SELECT; row_prep's per-row vector) -------------------------------------------------------------
// relu(u + v) = max(v, -u) + u: the pieces of max(v, -u) are the pieces of ONE of two numbers that exist per table row, so they
// are cut once per row and PICKED per pair.  A value (already range-scaled: |scaled| <= 2^14) becomes one 32-bit word
//     [ hi : fp16 | lo : fp16 ]     hi = scaled truncated (toward zero) to fp16, lo = fp16(scaled - hi) rounded to nearest,
// magnitudes below 2^-14 (where hi would be an fp16 denormal) flushed to the word 0.  |hi + lo - scaled| <= 2^-22 |scaled| while
// lo is a normal fp16, and at most 2^-25 where it is a denormal one.
// ORDERING CONTRACT: read as fp32 bit patterns the words are monotone in the value,  x <= y  =>  word(x) <= word(y)  as fp32, and
// equal values give equal words, so v_max_f32 of two words is the word of the larger value.  Why: fp32 orders by sign, then by
// magnitude bits; the upper half of the word is hi (truncation is monotone, and positive fp16 bit patterns order like their values);
// among values with equal hi the remainder has the sign of hi (truncation toward zero) and is monotone, rounding is monotone, and
// the lower half holds it as [sign | magnitude bits] - for a negative hi the set sign bit of lo is a constant of the magnitude
// comparison (a remainder of exactly 0 gives lo = +0, below every -0 or negative lo in magnitude: still monotone).
// NEVER A DENORMAL, INF OR NaN as fp32: the fp32 exponent field of a word is the 5 exponent bits of hi and its 3 leading mantissa
// bits.  hi is a normal fp16 (exponent field >= 1, by the flush), so the fp32 field is >= 8; the range scaling keeps |scaled| <= 2^14
// (fp16 exponent field <= 29), so the fp32 field is <= 239 < 255.  No mode of v_max_f32 flushes or quiets such an operand.
// The same function runs in the kernels and in tests/test_pair_select.py's host program.
__host__ __device__ inline uint32_t cut_select_word(float scaled) {
    const uint32_t b = __builtin_bit_cast(uint32_t, scaled);
    if ((b & 0x7fffffffu) < 0x38800000u) return 0u;  // |scaled| < 2^-14 (and -0): +0
    const float hi = __builtin_bit_cast(float, b & 0xffffe000u);  // 11 significant bits kept: exact in fp16
    const _Float16 h = (_Float16)hi, l = (_Float16)(scaled - hi);  // the remainder is exact in fp32
    return (uint32_t)__builtin_bit_cast(uint16_t, h) << 16 | __builtin_bit_cast(uint16_t, l);
}
// the value a select word stands for, hi + lo (exact in fp32: the two pieces span at most the 24 bits of the value they were cut from)
__host__ __device__ inline float select_word_value(uint32_t w) {
    return (float)__builtin_bit_cast(_Float16, (uint16_t)(w >> 16)) + (float)__builtin_bit_cast(_Float16, (uint16_t)(w & 0xffffu));
}

// HAZARD RULE for the asm helpers below: the compiler inserts the wait states a VALU result needs before an MFMA or a
// half-register reader consumes it only for its OWN instructions, not around inline asm.  Every result of these helpers must
// therefore pass through a compiler-generated VALU instruction (e.g. a packed multiply, v_cvt_pk_f16_f32) before it reaches an
// MFMA operand; feeding one straight into an MFMA needs an explicit "s_nop 1" (the clamp-fma tried in pair_mfma4).

// x - h (exact in fp32) with h = the low / high half of a packed fp16 pair read as an fp16 operand (v_fma_mix_f32)
__device__ __forceinline__ float f16_res_lo(float x, uint32_t hpk) {
    float r;
    asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(r) : "v"(x), "v"(hpk));
    return r;
}
__device__ __forceinline__ float f16_res_hi(float x, uint32_t hpk) {
    float r;
    asm("v_fma_mix_f32 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(r) : "v"(x), "v"(hpk));
    return r;
}
// {clamp01(a0 * c + b0), clamp01(a1 * c + b1)}: with a, b pre-scaled so that every sum is at most 1, the clamp IS the ReLU
__device__ __forceinline__ f32x2 fma2_relu01(f32x2 a, f32x2 c, f32x2 b) {
    f32x2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 clamp" : "=v"(r) : "v"(a), "v"(c), "v"(b));
    return r;
}

// ---- MFMAs on piece fragments (16 bytes per lane, 8 pieces) --------------------------------------------------------------------

__device__ __forceinline__ f32x16 mfma_32x32x16_bf16(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 mfma_32x32x16_f16(u32x4 a, u32x4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ f32x4 mfma_16x16x32_f16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}

// ---- product order -------------------------------------------------------------------------------------------------------------

// One piece product: piece index of the first (A) and the second (B) MFMA operand, 0 = high piece.  The first operand holds the
// weights in every kernel but gemm_pieces (activations first there); the products are symmetric, so the order serves both.
struct PieceProduct {
    int a, b;
};
// small to large: three terms of weight 2^-16, two of 2^-8, one of 2^0 (w_lo x_hi, w_hi x_lo, w_mid x_mid, w_mid x_hi, w_hi x_mid, w_hi x_hi)
constexpr PieceProduct kProductsBf16[6] = {{2, 0}, {0, 2}, {1, 1}, {1, 0}, {0, 1}, {0, 0}};
// small to large: w_l x_h, w_h x_l, w_h x_h
constexpr PieceProduct kProductsF16[3] = {{1, 0}, {0, 1}, {0, 0}};

}  // namespace shasta
