// The lane-per-pair phase of the three pair kernels (pair.hip: pair_mfma4_kernel, pair_f16.hip, pair_f16w.hip), device only: the
// 4x4x1 operand table in LDS and the layers that read it, the hand rows, the hand-designed residual, and the range exponents of the
// fp16 pack kernels.  The kernels differ in how the second layers are formed; what is here is the same in all of them.  (The
// layouts are in pair_layout.hpp, which host code includes too.)
#pragma once
#include "common.hpp"
#include "pair_layout.hpp"
#include "pieces.hpp"

namespace shasta {

typedef __attribute__((address_space(3))) float lfloat;
typedef __attribute__((address_space(3))) f32x4 lf32x4;

// floats per UP row slot of a wave in LDS (a row = ET + 16 hand floats; one 1 KB LDS-DMA per row)
constexpr int UP_SLOT = 256;

#define MFMA4(a, b, c) __builtin_amdgcn_mfma_f32_4x4x1f32((a), (b), (c), 0, 0, 0)

// layer L of width F in the 4x4x1 operand table (pair_layout.hpp: a4_offset)
template <int F, int L>
struct A4 {
    static constexpr LayerDesc D = layer_desc(F, L);
    static constexpr int NOB = a4_nob(F, L), KG = a4_kg(F, L), OFF = a4_offset(F, L), KIN = D.kin, BIAS = NOB * KG * 16;
};

// the table from the packed buffer into LDS (NT threads; a barrier before its first use).  (tid by reference, as a lambda captures it:
// passed by value, the compiler addressed the copy differently in pair_mfma4_kernel and pair_f16_kernel and their allocation moved.)
template <int F, int NT>
__device__ __forceinline__ void a4_stage(const float* __restrict__ packed, float* s_a4, const int& tid) {
    const PackedLayout P(0, 0, F);
    const f32x4* asrc = reinterpret_cast<const f32x4*>(packed + P.a4);
#pragma unroll 2
    for (int e = tid; e < a4_total(F) / 4; e += NT) reinterpret_cast<f32x4*>(s_a4)[e] = asrc[e];
}

// LDS byte addresses of the table as a lane sees it: arow = its row i = lane & 3 inside every [i][kk] group, abias = its element of
// every bias quad
struct A4Lane {
    unsigned arow_base, abias_base;
    __device__ __forceinline__ A4Lane(const float* s_a4, int lane)
        : arow_base((unsigned)(unsigned long long)(s_a4 + (lane & 3) * 4)), abias_base((unsigned)(unsigned long long)(s_a4 + (lane & 3))) {}
    // the A table is loop invariant: an opaque copy of its address per track keeps the 128 ds_read_b128 inside the
    // loop instead of 512 hoisted registers
    __device__ __forceinline__ void per_track(const lfloat*& arow, const lfloat*& abias) const {
        unsigned ao = arow_base, bo = abias_base;
        asm volatile("" : "+v"(ao), "+v"(bo));
        arow = (const lfloat*)(unsigned long long)ao;
        abias = (const lfloat*)(unsigned long long)bo;
    }
};

// bias: acc[ob] = bias[4*ob + i] * 1
template <class AL>
__device__ __forceinline__ void a4_init(const lfloat* abias, f32x4* acc) {
    const f32x4 zero4 = {0, 0, 0, 0};
#pragma unroll
    for (int ob = 0; ob < AL::NOB; ++ob) acc[ob] = MFMA4(abias[AL::OFF + AL::BIAS + ob * 4], 1.0f, zero4);
}

// ReLU of a later layer's inputs.  A4_RELU_NAN: as torch computes it (relu_nan, common.hpp).  A4_RELU_FMAX: fmaxf, in the fp16
// kernels (see a4_descale_relu)
enum A4Relu { A4_RELU_FMAX, A4_RELU_NAN };

// acc = bias + W . relu(in): the k-th input is register k & 3 of the previous layer's block k >> 2
template <class AL, A4Relu RELU>
__device__ __forceinline__ void a4_layer(const lfloat* arow, const lfloat* abias, const f32x4* in, f32x4* acc) {
    a4_init<AL>(abias, acc);
#pragma unroll
    for (int kg = 0; kg < AL::KG; ++kg) {
        f32x4 a4[AL::NOB];
#pragma unroll
        for (int ob = 0; ob < AL::NOB; ++ob) a4[ob] = *reinterpret_cast<const lf32x4*>(arow + AL::OFF + (ob * AL::KG + kg) * 16);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            if (4 * kg + kk < AL::KIN) {
                const float h = RELU == A4_RELU_NAN ? relu_nan(in[kg][kk]) : fmaxf(in[kg][kk], 0.0f);
#pragma unroll
                for (int ob = 0; ob < AL::NOB; ++ob) acc[ob] = MFMA4(a4[ob][kk], h, acc[ob]);
            }
        }
    }
}

// A quad of layer-2 results of the fp16 kernels: exact descaling (sc a power of two) + bias as packed fmas (two values per 5-cycle slot
// instead of one per 6), ReLU right behind them
__device__ __forceinline__ f32x4 a4_descale_relu(const f32x4& v, float sc, const f32x4& bb) {
    const f32x2 s2 = {sc, sc};
    const f32x2 lo = __builtin_elementwise_fma(f32x2{v[0], v[1]}, s2, f32x2{bb[0], bb[1]});
    const f32x2 hi = __builtin_elementwise_fma(f32x2{v[2], v[3]}, s2, f32x2{bb[2], bb[3]});
    // (fmaxf, not the NaN-propagating relu_nan of pair_mfma4_kernel: non-finite inputs never get here - the kernels' finite_bound -
    // and v_maximum3_f32 in pair_f16_kernel's track loop measured 1 - 3 % of the kernel: 4.39 - 4.43 -> 4.45 - 4.56 ms)
    return f32x4{fmaxf(lo[0], 0.0f), fmaxf(lo[1], 0.0f), fmaxf(hi[0], 0.0f), fmaxf(hi[1], 0.0f)};
}

// The hand row of a detection (16 floats at `row`) as hand_dist takes it: hd = slots 0 - 6 and 8 - 12.  Returns slot 13, the largest
// |UC| of the row (row_prep / embed_rows), which the fp16 kernels scale by.
__device__ __forceinline__ float load_hand_det(const float* row, float (&hd)[12]) {
    const f32x4* h = reinterpret_cast<const f32x4*>(row);
    const f32x4 a = h[0], c = h[1], e = h[2], g = h[3];
    hd[0] = a[0]; hd[1] = a[1]; hd[2] = a[2]; hd[3] = a[3]; hd[4] = c[0]; hd[5] = c[1]; hd[6] = c[2];
    hd[7] = e[0]; hd[8] = e[1]; hd[9] = e[2]; hd[10] = e[3]; hd[11] = g[0];
    return g[1];
}

// The hand-designed residual of one pair (det3d/models/tracker/shasta.py:277-283) from the hand rows of its track (hp, 16 floats)
// and of its detection (hd: slots 0 - 6 and 8 - 12 of that row), the column norm dnm = max(||.||, 1e-12) of the detection and
// rdn = 1.0f / dnm (IEEE, once per lane).  row_prep writes zeros into the box slots >= num_feats of both rows, so the sum of squares
// runs over all seven slots in the reference's order (x + 0.0 is exact) without a per-slot select.  The division by the
// loop-invariant dnm is a multiplication by rdn with one residual correction (q = d2 rdn; q += fma(-q, dnm, d2) rdn: the correctly
// rounded quotient whenever rdn is the correctly rounded reciprocal - Markstein - in 3 instructions instead of the 11 of the generic
// IEEE sequence); the square root is the hardware's (1 ulp; its operand comes from this library's own cosf / sinf of the yaws).
__device__ __forceinline__ float hand_dist(const float (&hp)[16], const float (&hd)[12], float dnm, float rdn) {
    typedef float hpf2 __attribute__((ext_vector_type(2)));
    hpf2 d01 = hpf2{hp[0], hp[1]} - hpf2{hd[0], hd[1]}, d23 = hpf2{hp[2], hp[3]} - hpf2{hd[2], hd[3]},
         d45 = hpf2{hp[4], hp[5]} - hpf2{hd[4], hd[5]};
    const float d6 = hp[6] - hd[6];
    d01 *= d01;
    d23 *= d23;
    d45 *= d45;
    const float d2 = (((((d01[0] + d01[1]) + d23[0]) + d23[1]) + d45[0]) + d45[1]) + d6 * d6;
    const float q = d2 * rdn;
    const float r = __builtin_fmaf(__builtin_fmaf(-q, dnm, d2), rdn, q);
    const float dim = (__builtin_fabsf(hp[8] - hd[7]) + __builtin_fabsf(hp[9] - hd[8])) + __builtin_fabsf(hp[10] - hd[9]);
    hpf2 cs = hpf2{hp[11], hp[12]} - hpf2{hd[10], hd[11]};
    cs *= cs;
    return (r + dim) + __builtin_amdgcn_sqrtf(cs[0] + cs[1]);
}

// combine (shasta.py:316-319): rc = the three coefficients of res_coeff, fused / dist / shape = the outputs they weigh
__device__ __forceinline__ float pair_combine(const f32x4& rc, float fused, float dist, float shape) {
    return (rc[0] * fused + rc[1] * dist) + rc[2] * shape;
}

// ---- pack kernels of the fp16 pair kernels (pair_f16.hip, pair_f16w.hip) -------------------------------------------------------------
struct PairF16PackArgs {
    const float* w_fs2;  // fuse_shape.2.weight (H2, H1)
    const float* w_rc2;  // res_coeff.2.weight (R2, R1)
    const float* w_fd2;  // fuse_det.2.weight (8, 32)
    uint32_t* out;       // the p16 / p16w section of the packed buffer
};

inline PairF16PackArgs pair_f16_pack_args(const shasta_weights* w, float* out) {
    return {w->fuse_shape[1].weight, w->res_coeff[1].weight, w->fuse_det[1].weight, reinterpret_cast<uint32_t*>(out)};
}

// a lane's eight scaled weights of fragment `frag` (of nfrag) cut into fp16 high and low pieces, stored at [piece][fragment][lane]
__device__ __forceinline__ void store_weight_pieces(const float (&v)[8], uint32_t* out, int nfrag, int frag, int lane) {
    u32x4 hi, lo;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const _Float16 h0 = (_Float16)v[2 * j], h1 = (_Float16)v[2 * j + 1];
        const f16x2 hh = {h0, h1};
        hi[j] = __builtin_bit_cast(uint32_t, hh);
        lo[j] = cvt_f16x2(v[2 * j] - (float)h0, v[2 * j + 1] - (float)h1);
    }
    reinterpret_cast<u32x4*>(out)[(0 * nfrag + frag) * 64 + lane] = hi;
    reinterpret_cast<u32x4*>(out)[(1 * nfrag + frag) * 64 + lane] = lo;
}

// 256 threads: the range exponent of each of the three second-layer matrices W[m] (cnt[m] floats; maxima by fmaxf), one per MLP.  On
// return every thread sees them in ex (LDS, like red); they are also stored as ints at out[at + m], and out[at + 3] = 0.
__device__ __forceinline__ void pair2_range_exponents(const float* const (&W)[3], const int (&cnt)[3], uint32_t* out, int at,
                                                      float (&red)[3][4], int (&ex)[3]) {
    const int tid = threadIdx.x;
    for (int m = 0; m < 3; ++m) {
        float mx = 0.0f;
        for (int i = tid; i < cnt[m]; i += 256) mx = fmaxf(mx, fabsf(W[m][i]));
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        if ((tid & 63) == 0) red[m][tid >> 6] = mx;
    }
    __syncthreads();
    if (tid < 3) {
        const float mx = fmaxf(fmaxf(red[tid][0], red[tid][1]), fmaxf(red[tid][2], red[tid][3]));
        ex[tid] = range_exponent_bits(__float_as_uint(mx));
        reinterpret_cast<int*>(out)[at + tid] = ex[tid];
    }
    if (tid == 3) out[at + 3] = 0;
    __syncthreads();
}

}  // namespace shasta
