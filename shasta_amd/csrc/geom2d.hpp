// Planar geometry shared by the rotated-IoU matrix (iou3d.hip) and the rotated NMS (nms.hip): float64 throughout.
// clip_area: Sutherland-Hodgman clip of a quadrilateral by a convex quadrilateral.  Each half-plane keeps the vertices inside and adds
// one crossing per change of side, of which a convex polygon has at most two: at most one vertex more per clip edge, 8 in all (the
// scratch polygons hold 10).  A vertex ON a clip line counts as inside and its crossing (t = 0) repeats it; the repeated vertex and
// either tie rule (>= or >) leave the area unchanged.
// Callers pass corners in the frame of the pair's first box: the shoelace sum cancels products of the coordinates' size, so in world
// coordinates C the area error grows like eps C^2 (4e-10 m^2 at 2000 m, 4e-6 at 1e5 m); in the local frame it is eps L^2 of the
// boxes' size L whatever C is.
// PINNED against exact geometry (60-digit decimal evaluation from the box parameters, tests/exact_geometry.py) at the degenerate
// poses - identical boxes, quarter / half turns, rotations of 1e-15 ... 1e-6 rad, slides along an own axis, edge and corner contact,
// containment with shared edge lines, slivers, zero-length boxes, ties in the hull's sort - at world offsets 0 ... 1e5 m, in both
// argument orders (tests/test_geometry_exact.py).  Bar: tolA = 16 eps (C + L) L on the area, carried through the IoU / GIoU formulas.
// Largest error / bar on an MI355X: shasta_iou3d_distance_f64 0.016 (IoU) and 0.018 (GIoU); shasta_boxes_bev_f32 0.48 of the overlap
// bar (2^-23 exact + tolA: the float32 rounding of the result itself is 0.5), 0.06 of 2e-6 (BEV IoU), 0.02 of 5e-6 (3-D IoU); rotated
// NMS keeps exactly what greedy NMS on the exact IoU matrix keeps.
#pragma once

namespace shasta {

struct P2 {
    double x, y;
};

__device__ __forceinline__ double shoelace(const P2* p, int n) {
    if (n < 3) return 0.0;
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
        const P2 a = p[i], b = p[(i + 1) % n];
        s += a.x * b.y - a.y * b.x;
    }
    return s * 0.5;
}

__device__ inline double clip_area(const P2* subj, const P2* clip) {
    P2 buf0[10], buf1[10];
    P2* in = buf0;
    P2* out = buf1;
    int n = 4;
    for (int i = 0; i < 4; ++i) in[i] = subj[i];
    const double sgn = shoelace(clip, 4) >= 0 ? 1.0 : -1.0;
    for (int e = 0; e < 4 && n > 0; ++e) {
        const P2 a = clip[e], b = clip[(e + 1) & 3];
        const double ex = b.x - a.x, ey = b.y - a.y;
        int m = 0;
        for (int j = 0; j < n; ++j) {
            const P2 p = in[j], q = in[(j + 1) % n];
            const double sp = sgn * (ex * (p.y - a.y) - ey * (p.x - a.x));
            const double sq = sgn * (ex * (q.y - a.y) - ey * (q.x - a.x));
            if (sp >= 0) out[m++] = p;
            if ((sp >= 0) != (sq >= 0)) {
                const double t = sp / (sp - sq);
                out[m++] = {p.x + t * (q.x - p.x), p.y + t * (q.y - p.y)};
            }
        }
        P2* tmp = in;
        in = out;
        out = tmp;
        n = m;
    }
    return fabs(shoelace(in, n));
}

}  // namespace shasta
