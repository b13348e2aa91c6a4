// Where a gather point of a box falls on the BEV map: the one copy of the coordinate rule, shared by the forward (bev_gather.hip) and
// its transpose (bev_gather_bwd.hip).  Restates Shasta.get_box_center (det3d/models/tracker/shasta.py:121-161), center_to_corner_box2d
// (det3d/core/bbox/box_torch_ops.py:184-203), the metric -> pixel map of BEVFeatureExtractor.forward
// (det3d/models/second_stage/bird_eye_view.py:18-41) and the corners and weights of bilinear_interpolate_torch
// (det3d/core/utils/center_utils.py:92-121).
#pragma once
#include "common.hpp"

namespace shasta {

// Arithmetic notes (parity): every product/sum below is a separately rounded fp32 op
// (__fmul_rn/__fadd_rn/__fsub_rn, never contracted) because the reference evaluates them as
// separate ATen ops; the metric->pixel map keeps the reference's two successive divisions
// (bird_eye_view.py:19-20) -- a fused reciprocal changes floor() for ~1e-6 of coordinates.
struct GatherPoint {
    int x0, x1, y0, y1;  // the corner columns / rows, clamped to the map
    float w[4];          // weights of (y0 x0, y1 x0, y0 x1, y1 x1): the order of the forward's terms
};
// point `pt` of the box row `box` (x, y, z, w, l, h, yaw; only x, y are read at num_point == 1) on an H x W map
__device__ __forceinline__ GatherPoint bev_gather_point(const float* box, int num_point, int pt, float pc_x0, float pc_y0, float vs_x,
                                                        float vs_y, float out_stride_px, int H, int W) {
    const float cx = box[0], cy = box[1];
    float px = cx, py = cy;
    // point type: num_point==5 -> [centre, front, back, left, right]; 4 -> no centre; 1 -> centre
    const int edge = (num_point == 5) ? pt - 1 : (num_point == 4 ? pt : -1);
    if (edge >= 0) {
        const float w = box[3], l = box[4], yaw = box[6];
        const float s = sinf(yaw), c = cosf(yaw);
        // unit corners (clockwise from the minimum point): (-.5,-.5) (-.5,.5) (.5,.5) (.5,-.5)
        // edge mid-points: front=(c0+c1)/2, back=(c2+c3)/2, left=(c0+c3)/2, right=(c1+c2)/2
        const int ia = (edge == 0) ? 0 : (edge == 1) ? 2 : (edge == 2) ? 0 : 1;
        const int ib = (edge == 0) ? 1 : (edge == 1) ? 3 : (edge == 2) ? 3 : 2;
        float qx[2], qy[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int ci = k ? ib : ia;
            const float ux = (ci < 2) ? -0.5f : 0.5f;
            const float uy = (ci == 1 || ci == 2) ? 0.5f : -0.5f;
            const float dx = __fmul_rn(w, ux), dy = __fmul_rn(l, uy);
            // rotation_2d: x' = x*cos + y*sin ; y' = -x*sin + y*cos   (box_torch_ops.py:145-158)
            const float rx = __fadd_rn(__fmul_rn(dx, c), __fmul_rn(dy, s));
            const float ry = __fadd_rn(__fmul_rn(-dx, s), __fmul_rn(dy, c));
            qx[k] = __fadd_rn(rx, cx);
            qy[k] = __fadd_rn(ry, cy);
        }
        px = __fdiv_rn(__fadd_rn(qx[0], qx[1]), 2.0f);
        py = __fdiv_rn(__fadd_rn(qy[0], qy[1]), 2.0f);
    }
    const float x = __fdiv_rn(__fdiv_rn(__fsub_rn(px, pc_x0), vs_x), out_stride_px);
    const float y = __fdiv_rn(__fdiv_rn(__fsub_rn(py, pc_y0), vs_y), out_stride_px);
    // floor -> int with clamping done in float first so that wild coordinates (inf/NaN/1e30)
    // cannot overflow the conversion; the reference clamps the int64 indices.
    const float fx = floorf(x), fy = floorf(y);
    auto clampi = [](float f, int hi) -> int {
        if (!(f > -2.0f)) return 0 - 1;  // also NaN -> behaves like far-left (weights become NaN anyway)
        if (f > (float)(hi + 1)) return hi + 1;
        return (int)f;
    };
    int x0 = clampi(fx, W), y0 = clampi(fy, H);
    int x1 = x0 + 1, y1 = y0 + 1;
    x0 = min(max(x0, 0), W - 1);
    x1 = min(max(x1, 0), W - 1);
    y0 = min(max(y0, 0), H - 1);
    y1 = min(max(y1, 0), H - 1);
    const float fx0 = (float)x0, fx1 = (float)x1, fy0 = (float)y0, fy1 = (float)y1;
    GatherPoint g;
    g.x0 = x0; g.x1 = x1; g.y0 = y0; g.y1 = y1;
    g.w[0] = __fmul_rn(__fsub_rn(fx1, x), __fsub_rn(fy1, y));
    g.w[1] = __fmul_rn(__fsub_rn(fx1, x), __fsub_rn(y, fy0));
    g.w[2] = __fmul_rn(__fsub_rn(x, fx0), __fsub_rn(fy1, y));
    g.w[3] = __fmul_rn(__fsub_rn(x, fx0), __fsub_rn(y, fy0));
    return g;
}

}  // namespace shasta
