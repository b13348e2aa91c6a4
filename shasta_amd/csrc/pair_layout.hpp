// Layout of the packed pair-MLP weights, shared by the pack kernel and the pair kernel.
//
// The three pair MLPs of the reference (det3d/models/tracker/shasta.py:59-67 fuse_shape, :78-84 fuse_det,
// :86-92 res_coeff) are applied to every (track t, detection d) pair on an input that is a CONCATENATION of a
// per-track part and a per-detection part.  Their first Linear is therefore separable:
//     W1 . [prev_t ; cur_d] + b1  =  (W1[:, prev cols] . prev_t)  +  (W1[:, cur cols] . cur_d + b1)
// The two halves ("row embeddings" UP[t], UC[d], ET floats per table row) are produced once per table row by the
// generic GEMM; the pair kernel only adds them, applies ReLU and runs the remaining small layers on the matrix
// cores.  The (B, T*D, 2F) pair tensor of the reference (516 MB at N=500) is never materialised.
//
// Later layers run with one LANE per pair on v_mfma_f32_4x4x1_16B_f32 (pair.hip): the four result registers of a lane are
// four output features of its own pair, so a layer's accumulators are, unmoved, the next layer's inputs.
// Layouts only, for host and device code; the device helpers of the lane-per-pair phase are in pair_lane.hpp.
#pragma once
#if defined(__HIPCC__)
#include "common.hpp"
#endif

namespace shasta {

#if defined(__HIPCC__)
#define SH_HD __host__ __device__
#else
#define SH_HD
#endif

struct PairDims {
    int F, H1, H2, H3, R1, R2, ET;
    SH_HD constexpr PairDims(int f)
        : F(f), H1(f / 8), H2(f / 16), H3(f / 32), R1(32 + f / 8), R2(8 + f / 32), ET(f / 8 + 32 + f / 8 + 32) {}
};

// layer ids in packed order
enum { L_FS2 = 0, L_FS3, L_FS4, L_RC2, L_RC3, L_FD2, L_FD3, L_COUNT };

struct LayerDesc {
    int hout;  // output features
    int kin;   // input features
};

SH_HD constexpr LayerDesc layer_desc(int F, int l) {
    const PairDims d(F);
    return l == L_FS2   ? LayerDesc{d.H2, d.H1}
           : l == L_FS3 ? LayerDesc{d.H3, d.H2}
           : l == L_FS4 ? LayerDesc{1, d.H3}
           : l == L_RC2 ? LayerDesc{d.R2, d.R1}
           : l == L_RC3 ? LayerDesc{3, d.R2}
           : l == L_FD2 ? LayerDesc{8, 32}
                        : LayerDesc{1, 8};
}

// 4x4x1 formulation (pair_mfma4_kernel): layer l as A operands of v_mfma_f32_4x4x1_16B_f32.  Per output block ob (4
// features) and k-group kg (4 inputs): 16 floats [i][kk] = W[4*ob + i][4*kg + kk] (zero padded); after all blocks, the
// bias as [ob][i].  Lane l reads the float4 of row i = l & 3.
SH_HD constexpr int a4_nob(int F, int l) { return (layer_desc(F, l).hout + 3) / 4; }
SH_HD constexpr int a4_kg(int F, int l) { return (layer_desc(F, l).kin + 3) / 4; }
SH_HD constexpr int a4_size(int F, int l) { return a4_nob(F, l) * a4_kg(F, l) * 16 + a4_nob(F, l) * 4; }
SH_HD constexpr int a4_offset(int F, int l) {
    int o = 0;
    for (int i = 0; i < l; ++i) o += a4_size(F, i);
    return o;
}
SH_HD constexpr int a4_total(int F) { return a4_offset(F, L_COUNT); }

// aff layers as bf16 piece fragments (aff_pieces.hip): k steps (16 wide) and feature blocks (32 wide) of the six layers for a
// table of D = N + 2 columns; one fragment = [64 lanes][16 B] = 256 dwords, three pieces per (feature block, k step)
SH_HD constexpr int ap_ksteps(int layer, int D) {
    return layer == 0 ? (D + 15) / 16 : layer == 1 ? 8 : layer == 2 ? 4 : layer == 3 ? 2 : layer == 4 ? 4 : 8;
}
SH_HD constexpr int ap_fblocks(int layer, int D) {
    return layer == 0 ? 4 : layer == 1 ? 2 : layer == 2 ? 1 : layer == 3 ? 2 : layer == 4 ? 4 : (D + 31) / 32;
}
SH_HD constexpr int ap_kin(int layer, int D) { return layer == 0 ? D : layer == 1 ? 128 : layer == 2 ? 64 : layer == 3 ? 32 : layer == 4 ? 64 : 128; }
SH_HD constexpr int ap_out(int layer, int D) { return layer == 0 ? 128 : layer == 1 ? 64 : layer == 2 ? 32 : layer == 3 ? 64 : layer == 4 ? 128 : D; }
SH_HD constexpr size_t ap_layer_offset(int layer, int D) {  // in fragments
    size_t o = 0;
    for (int l = 0; l < layer; ++l) o += (size_t)ap_fblocks(l, D) * ap_ksteps(l, D) * 3;
    return o;
}

// the same layers as fp16 piece fragments (aff_f16.hip): two pieces per (feature block, k step), every output row scaled by a
// power of two; behind the fragments one float per output feature and layer (padded to whole feature blocks): the factor 2^-e that
// undoes the scale.  Offsets in floats from the start of the section.
SH_HD constexpr size_t ap16_frag_offset(int layer, int D) {  // in fragments of 256 floats
    size_t o = 0;
    for (int l = 0; l < layer; ++l) o += (size_t)ap_fblocks(l, D) * ap_ksteps(l, D) * 2;
    return o;
}
SH_HD constexpr size_t ap16_scale_offset(int layer, int D) {
    size_t o = (ap16_frag_offset(6, D) + 2) * 256;  // two spare fragments: the phantom k step behind an odd layer-1 width reads them
    for (int l = 0; l < layer; ++l) o += (size_t)ap_fblocks(l, D) * 32;
    return o;
}
SH_HD constexpr size_t ap16_total(int D) { return ap16_scale_offset(6, D); }

// p16 section of the packed buffer (pair_f16.hip, F = 256), in dwords, and what follows it.  The p16w section behind it holds
// pair_f16w.hip's fragments at F = 320 and is free at F = 256, where it holds the select form's operands instead:
//   [0, P16_FRAG_DW)            the second layers as fp16 piece fragments [piece 2][fragment 4][lane 64][4]   (PAIR_GRID)
//   [P16_FRAG_DW, + 4)          3 int exponents (fs, rc, fd), padded to 4; the p16 section ends here
//   [P16_SEL_DW, + 2 * 8 KB)    the same weights for select words [piece 2][instruction 8][lane 64][4]: every weight twice, under
//                               the hi and the lo half of its activation word                               (PAIR_SELECT)
//   [P16_SUM_DW, + 1792)        float wsum = (high + low piece) of the scaled weights as [k][j]: res_coeff.2 [64][16] | fuse_shape.2
//                               [32][16] | fuse_det.2 [32][8]: what row_select_kernel multiplies a track's words by
constexpr int P16_FRAG_DW = 2 * 4 * 64 * 4;
constexpr int P16_DW = P16_FRAG_DW + 4;
constexpr int P16W_DW = 2 * 16 * 64 * 4 + 4;
constexpr int P16_SEL_DW = P16_DW;
constexpr int P16_SUM_DW = P16_SEL_DW + 2 * 8 * 64 * 4;
constexpr int PAIR_SEL_SUM = 16 * 64 + 16 * 32 + 8 * 32;
constexpr int PAIR_SEL_ROW = 40;  // floats per row of PairWs::sel_prev
static_assert(P16_SUM_DW + PAIR_SEL_SUM <= P16_DW + P16W_DW, "the select operands fit the p16w section");

// n rounded up to a multiple of 4: the padded width Dp of a table of T = N + 2 columns (16-byte aligned rows)
SH_HD constexpr int pad4(int n) { return (n + 3) / 4 * 4; }

// Packed buffer sections (float offsets).  Dp = padded aff width (multiple of 4).
struct PackedLayout {
    int F, nf, N, D, Dp, E12, ET;
    size_t a4, wemb_prev, wemb_cur, bemb_cur, wbox_prev, wbox_cur, bbox_cur, aff0, affp, p16, p16w, embp, aff16, total;
    SH_HD PackedLayout(int max_obj, int num_feats, int f) {
        const PairDims d(f);
        F = f;
        nf = num_feats;
        N = max_obj;
        D = max_obj + 2;
        Dp = pad4(D);
        E12 = d.H1 + d.R1;
        ET = d.ET;
        size_t o = 0;
        a4 = o;         o += (size_t)((a4_total(f) + 3) / 4 * 4);  // 4x4x1 MFMA A operands of layers 2-4
        wemb_prev = o;  o += (size_t)E12 * f;          // [E12][F]   fuse_shape.0 / res_coeff.0, prev feature cols
        wemb_cur = o;   o += (size_t)E12 * f;          // [E12][F]   ... cur feature cols
        bemb_cur = o;   o += (size_t)((E12 + 3) / 4 * 4);  // [E12]  fuse_shape.0.bias | res_coeff.0.bias
        wbox_prev = o;  o += (size_t)(d.R1 + 32) * 8;  // [R1+32][8] res_coeff.0 / fuse_det.0 prev box cols (nf used)
        wbox_cur = o;   o += (size_t)(d.R1 + 32) * 8;  // [R1+32][8] ... cur box cols
        bbox_cur = o;   o += (size_t)32;               // [32]       fuse_det.0.bias
        aff0 = o;       o += (size_t)128 * Dp;         // aff.0.weight zero padded to (128, Dp)
        affp = o;       o += ap_layer_offset(6, D) * 256;  // the six aff layers as bf16 piece fragments (aff_pieces.hip)
        p16 = o;        o += (size_t)P16_DW;  // second layers of the pair MLPs as fp16 piece fragments + 3 exponents (pair_f16.hip; see P16_*)
        p16w = o;       o += (size_t)P16W_DW;  // the same as 32x32x16 fragments (pair_f16w.hip: up to 16 fragments x 2 pieces x 1 KB); F = 256: PAIR_SELECT's
        // wemb_prev / wemb_cur as bf16 piece fragments [side][feature block][k step][piece][64 lanes] x 16 B (embed_rows.hip)
        embp = o;       o += (size_t)2 * ((E12 + 31) / 32) * (f / 16) * 3 * 256;
        aff16 = o;      o += ap16_total(D);  // the six aff layers as fp16 piece fragments + their descale factors (aff_f16.hip)
        total = o;
    }
};

}  // namespace shasta
