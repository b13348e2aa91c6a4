// Everything of the affinity forward that crosses a file boundary: the host functions one .hip file defines and another calls (each
// declared once, here; the defining file includes this header too, so a changed signature fails to compile instead of to link) and the
// layouts of the stage workspaces (one struct each, used by the size query and by the launcher that carves the workspace).
#pragma once
#include "common.hpp"
#include "pair_layout.hpp"

namespace shasta {

// ---- bev_gather.hip ------------------------------------------------------------------------------------------------------------------
// scratch lines the gather posts the magnitudes of `items` batch items into: [items][slots][128 B]
size_t bev_absmax_slot_bytes(int items);
// ... reduced to one maximum (float bit pattern) per item
int launch_absmax_finalize(const unsigned* slots, unsigned* out, int items, hipStream_t st);
// bev2 / boxes2 / out2 / absmax2: null, or the pair's other frame (same shapes and strides), gathered by the same launch
int launch_bev_gather(const float* bev, int B, int H, int W, int C, const float* boxes, int N, int box_stride, int box_batch_stride,
                      int num_point, float pc_x0, float pc_y0, float vs_x, float vs_y, float out_stride, float* out, int out_row_stride,
                      int out_batch_stride, unsigned* absmax, hipStream_t st, const float* bev2 = nullptr, const float* boxes2 = nullptr,
                      float* out2 = nullptr, unsigned* absmax2 = nullptr);

// ---- gemm_f32.hip --------------------------------------------------------------------------------------------------------------------
// C0 = A0 W0^T (+bias0), C1 = A1 W1^T (+bias1), same shapes and leading dimensions; falls back to two launches when the
// vector-load preconditions do not hold
int launch_gemm_nt_dual(const float* A0, const float* W0, const float* bias0, float* C0, const float* A1, const float* W1,
                        const float* bias1, float* C1, int lda, int ldw, int ldc, int M, int N, int K, int act, hipStream_t st);
// four products C[i] = act(A[i] W[i]^T + bias[i]) of one shape in one launch; act: 0 none, 1 ReLU, 2 |.|
int launch_gemm_nt_quad(const float* const A[4], const float* const W[4], const float* const bias[4], float* const C[4], int lda,
                        int ldw, int ldc, int M, int N, int K, int act, hipStream_t st);
// true when launch_gemm_nt_quad will take the direct form for these operands
bool gemm_nt_quad_direct_ok(const float* const A[4], const float* const W[4], int lda, int ldw, int K);

// ---- anchor_mfma.hip -----------------------------------------------------------------------------------------------------------------
// returns 0 when launched, 1 when the shape is not served by this kernel
int launch_anchor_l1_mfma(const float* const W[4], const float* feat, const float* prev_feat, float* part, int H, int K, int B,
                          int x_batch_stride, int* ks_out, hipStream_t st);

// ---- anchor_split.hip ----------------------------------------------------------------------------------------------------------------
// maxima of the batch rows of both feature tables (frame 0: feat, frame 1: prev_feat): xmax[2][B]
int launch_x_maxima(const float* feat, const float* prev_feat, int K, int B, int x_batch_stride, unsigned* xmax, hipStream_t st);
// maxima of the 4 x H weight rows of the aug_shape first layers (pack time): wmax[4][H]
// sumabs (optional): [4][H] floats + 16 floats of summary behind them (the stats section of the companion buffer, common.hpp)
int launch_w_maxima(const float* const W[4], int H, int K, unsigned* wmax, float* sumabs, hipStream_t st);
// the first-layer weights cut once into the fp16 piece image the weight stream reads (SHASTA_OPT_PRECUT_WEIGHT_STREAM); 0: no such form
size_t precut_image_bytes(int H, int K);
int launch_precut_weights(const float* const W[4], const unsigned* wmax, void* img, int H, int K, hipStream_t st);
// bytes of the piece image of the activations (0 for batches the f32 kernels serve): sized for the larger of the two forms
size_t anchor_split_workspace_bytes(int B, int K);
// true when anchor_l1_split_kernel serves this shape (otherwise the f32 kernels of anchor_mfma.hip / anchor.hip do)
bool anchor_split_serves(int B, int K, int x_batch_stride);
// cut the activations of both frames into the bf16 fragment image `xs`
void launch_split_x(const float* feat, const float* prev_feat, void* xs, int K, int B, int x_batch_stride, int np, const unsigned* xmax,
                    bool precut, hipStream_t st);
// np = pieces per operand: 3 = bf16 (six products), 2 = fp16 (three products, SHASTA_OPT_F16X2_WEIGHT_STREAM)
void launch_anchor_l1_split(const float* const W[4], const void* xs, float* part, int H, int K, int B, int* ks_out, int np,
                            const unsigned* wmax, const void* wimg, hipStream_t st);

// ---- anchor.hip ----------------------------------------------------------------------------------------------------------------------
// ws: AnchorShapeWs.  wmax: the row maxima of the first-layer weights (companion buffer) or null; xmax_ready: the producer of the
// tables has left the activation row maxima in the workspace already
int anchor_shape(const shasta_weights* w, int B, float* feat, float* prev_feat, void* ws, size_t ws_bytes, hipStream_t st,
                 hipEvent_t ev0, hipEvent_t ev1, const unsigned* wmax, bool xmax_ready);
// does anchor_shape take the two-piece fp16 weight stream for this call (and therefore need the activation row maxima)?
bool anchor_shape_uses_xmax(const shasta_weights* w, int B);
// hid_ws: AnchorBoxesWs
int anchor_boxes(const shasta_weights* w, int B, float* det_boxes, const float* prev_det_boxes, int box_stride, float* det_tab,
                 float* prev_tab, float* hid_ws, hipStream_t st, float* anchors_out);
// Both anchor stages of a small batch in fewer launches.  ws: AnchorShapeWs followed by AnchorBoxesWs.
bool anchor_stage_fused_serves(const shasta_weights* w, int B);
int anchor_stage_fused(const shasta_weights* w, int B, float* feat, float* prev_feat, float* det_boxes, const float* prev_det_boxes,
                       int box_stride, float* det_tab, float* prev_tab, void* ws, size_t ws_bytes, hipStream_t st, hipEvent_t ev0,
                       hipEvent_t ev1, const unsigned* wmax, bool xmax_ready, float* anchors_out);

// ---- pair_f16.hip, pair_f16w.hip -----------------------------------------------------------------------------------------------------
// second layers of the three pair MLPs as fp16 piece fragments: the p16 (F = 256) / p16w (F = 320) section of the packed buffer
int pair_f16_pack(const shasta_weights* w, float* out, hipStream_t st);
// how pair_f16_kernel forms the pieces of h1 = relu(UP[t] + UC[d]): PAIR_SELECT picks pre-cut words per pair (the "f16x2" default; needs
// sel_prev, PairWs), PAIR_GRID adds pre-cut pieces on a fixed grid ("f16grid").  (Cutting every pair's fp32 sum is the form pair_f16w.hip
// has at F = 320.)
enum PairF16Mode { PAIR_GRID, PAIR_SELECT };
int launch_pair_f16(const float* packed, const float* p16, const float* UP, const float* UC, const float* hand_prev,
                    const float* hand_det, const float* sel_prev, const float* denom, float* residual, int B, int T, int D, int ld,
                    int nf, PairF16Mode mode, hipStream_t st);
bool pair_f16w_serves(int F);
int pair_f16w_pack(const shasta_weights* w, float* out, hipStream_t st);
// SHASTA_E_UNSUPPORTED when the device does not grant the kernel's LDS
int launch_pair_f16w(const float* packed, const float* p16, const float* UP, const float* UC, const float* hand_prev,
                     const float* hand_det, const float* denom, float* residual, int B, int T, int D, int ld, int F, hipStream_t st);

// ---- embed_rows.hip ------------------------------------------------------------------------------------------------------------------
// `packed` = the packed weight buffer (PackedLayout); writes its embp section from its wemb_* sections
int embed_pack(const shasta_weights* w, float* packed, hipStream_t st);
bool embed_rows_serves(int F);
// row embeddings UP / UC of M table rows with the box columns added, and the hand rows
int launch_embed_rows(const shasta_weights* w, const float* packed, const float* prev_feat, const float* feat, const float* prev_tab,
                      const float* det_tab, float* UP, float* UC, float* hand_prev, float* hand_det, int M, hipStream_t st);

// ---- pair.hip ------------------------------------------------------------------------------------------------------------------------
// ws: PairWs
int pair_residual(const shasta_weights* w, const float* packed, int B, const float* feat, const float* prev_feat, const float* det_tab,
                  const float* prev_tab, float* residual, int ld, void* ws, size_t ws_bytes, hipStream_t st, hipEvent_t ev0,
                  hipEvent_t ev1);
// every section of the packed buffer (PackedLayout)
int pack_weights(const shasta_weights* w, float* packed, hipStream_t st);

// ---- aff_pieces.hip, aff_f16.hip -----------------------------------------------------------------------------------------------------
// the six aff layers as bf16 / fp16 piece fragments: the affp / aff16 section of the packed buffer
int aff_pieces_pack(const shasta_weights* w, float* out, hipStream_t st);
int aff_f16_pack(const shasta_weights* w, float* out, hipStream_t st);
// the piece kernels serve tables of up to 512 columns
bool aff_pieces_serves(int D);
// the six layers and the row softmax; `matched` (M x ldm) receives the logits for the column softmax
int launch_aff_pieces(const shasta_weights* w, const float* packed_pieces, const float* residual, int ld, float* matched, int ldm,
                      float* m1, int M, hipStream_t st);
// the six layers and both softmaxes in one launch.  `matched` (B T x ldm, optional) receives the logits; ws: AffWs
int launch_aff_frame(const shasta_weights* w, const float* packed_pieces, const float* residual, int ld, float* matched, int ldm, float* m1,
                     float* m2, int B, void* ws, hipStream_t st);
// the same on fp16 pieces; packed16 = the aff16 section of the packed buffer
int launch_aff_frame16(const shasta_weights* w, const float* packed16, const float* residual, int ld, float* matched, int ldm, float* m1,
                       float* m2, int B, void* ws, hipStream_t st);

// ---- aff.hip -------------------------------------------------------------------------------------------------------------------------
// Status word of the most recent aff launch on workspace `ws` (AffWs): 0, or bit 0 = a row group's wait for its siblings timed out.
// Synchronises on the stream.  `ld`: the residual's leading dimension of that launch.
int aff_status(const shasta_weights* w, int B, int ld, const void* ws, int* status, hipStream_t st);
// ws: AffWs
int aff_softmax(const shasta_weights* w, const float* packed, int B, const float* residual, int ld, float* m1, float* m2,
                float* matched_out, void* ws, size_t ws_bytes, hipStream_t st);

// ---- stage workspaces ----------------------------------------------------------------------------------------------------------------
// One struct per workspace: the constructor bumps an offset through 256-byte aligned sections and records where each starts.

// the section at `o` (returned), `o` moved behind it
inline size_t ws_take(size_t& o, size_t bytes) {
    const size_t at = o;
    o += align_up(bytes, 256);
    return at;
}

// anchor_shape: H = N F / 64 hidden units per MLP
struct AnchorShapeWs {
    size_t part, hidden, xs, xmax, wmax, slots, total;
    AnchorShapeWs(int B, int N, int F) {
        const size_t H = (size_t)N * F / 64;
        size_t o = 0;
        part = ws_take(o, (size_t)64 * B * 4 * H * sizeof(float));  // split-K partials, worst-case KS = 64
        hidden = ws_take(o, (size_t)B * 4 * H * sizeof(float));     // relu(W1 x + b1): (B, 4H), MLP-major inside a row (the training path copies it)
        xs = ws_take(o, anchor_split_workspace_bytes(B, N * F));    // piece image of the activations (anchor_split.hip)
        xmax = ws_take(o, (size_t)2 * B * sizeof(unsigned));        // activation row maxima [2 frames: feat, prev_feat][B]
        wmax = ws_take(o, (size_t)4 * H * sizeof(unsigned));        // weight row maxima when the caller brings no companion buffer
        slots = o;                                                  // scratch lines of the gather (bev_gather.hip): [2 B][slots][128 B]
        total = o + bev_absmax_slot_bytes(2 * B);
    }
};

// anchor_boxes: HD = 7N / 32 hidden units per MLP
struct AnchorBoxesWs {
    size_t hid, x7, total;
    AnchorBoxesWs(int B, int N) {
        const int HD = 7 * N / 32;
        size_t o = 0;
        hid = ws_take(o, (size_t)B * 4 * (HD > 1 ? HD : 1) * sizeof(float));       // (B, 4, HD)
        x7 = ws_take(o, (size_t)2 * B * pad4(7 * N) * sizeof(float));      // packed box rows (2, B, ceil4(7N)) for the GEMM form
        total = o;
    }
};

// pair_residual: T = N + 2 table rows per frame
struct PairWs {
    size_t up, uc, hand_prev, hand_det, sel_prev, denom, total;
    PairWs(int B, int N, int F) {
        const size_t rows = (size_t)B * (N + 2);
        size_t o = 0;
        up = ws_take(o, rows * PairDims(F).ET * sizeof(float));  // row embeddings of the tracks ...
        uc = ws_take(o, rows * PairDims(F).ET * sizeof(float));  // ... and of the detections
        hand_prev = ws_take(o, rows * 16 * sizeof(float));       // hand tables
        hand_det = ws_take(o, rows * 16 * sizeof(float));
        // per track row: S[t] = bias2 + W2 UP[t] of the three second layers, [rc 16 | fs 16 | fd 8] (row_prep's select role, F = 256)
        sel_prev = ws_take(o, rows * PAIR_SEL_ROW * sizeof(float));
        denom = ws_take(o, rows * sizeof(float));                // column norms
        total = o;
    }
};

// aff_softmax: matched (B, T, Dp) between the row MLP and the column softmax (two-kernel forms), then the control words
// [status, ticket, arrive[B]] (one memset per launch) and the column partials of the one-pass form
struct AffWs {
    size_t matched, ctrl, part, total;
    AffWs(int B, int N) {
        const int T = N + 2;
        size_t o = 0;
        matched = ws_take(o, (size_t)B * T * pad4(T) * sizeof(float));
        ctrl = ws_take(o, (size_t)(B + 2) * sizeof(unsigned));
        part = ws_take(o, (size_t)B * cdiv(T, 64) * 1024 * sizeof(float));  // the 64-row shape needs the most partials
        total = o;
    }
};

}  // namespace shasta
