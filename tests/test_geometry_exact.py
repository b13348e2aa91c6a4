"""Rotated IoU / GIoU / BEV matrices / rotated NMS against EXACT geometry at degenerate poses (next row f-2).

`tests/exact_geometry.py` evaluates every quantity from the box parameters in 60-digit decimal arithmetic; it shares nothing with
`csrc/geom2d.hpp` or `oracle/iou_oracle.py`, which restate one another.  The poses are the ones where clipping code goes wrong
(identical boxes, quarter and half turns, rotations of 1e-15 ... 1e-6 rad, slides along an own axis, edge and corner contact,
containment with shared edge lines, slivers, zero-length boxes, ties in the hull's sort), each at world offsets of 0, 50, 2000 and
1e5 m and in both argument orders.

Bars.  tolA = 16 eps (C + L) L is the float64 format's floor for an area held in world coordinates (C the largest centre coordinate,
L the longest side).  The distance kernel returns only 1 - IoU / 1 - GIoU, so tolA is carried through the formula to first order at
the exact values (`exact_geometry.iou_distance_bar`).  The float32 matrices: overlap 2^-23 exact + tolA, BEV IoU 2e-6, 3-D IoU 5e-6
(the bars of tests/test_nms.py).  The CPU test on `oracle/iou_oracle.py` at tolA / 4 shows that the inputs are fair: the same
algorithm in numpy float64 meets a quarter of the bar.

Largest error / bar measured on an MI355X (every family, every offset, both orders):
  shasta_iou3d_distance_f64   IoU 0.016, GIoU 0.018 (both at offset 0; 0.004 at 50 m, 2e-4 at 2000 m, below 1e-4 at 1e5 m: the bar grows
                              with the offset, the kernel's error does not); offset 0 against 2000 m: 0.009 / 0.010 of the summed bars
  shasta_boxes_bev_f32        overlap 0.48 (the float32 rounding of the result alone is 0.5), BEV IoU 0.06, 3-D IoU 0.02
With the corners held in the world frame, as they were before these tests, a float64 restatement of the clip reaches 50 x tolA at
2000 m and 1.8e3 x at 1e5 m, and the float32 overlap matrix 50 x and 2e3 x its bar: both kernels now work in the frame of the pair's
first box.
"""
import functools
import math
from decimal import Decimal as D

import numpy as np
import pytest
from scipy.spatial import QhullError

from oracle import iou_oracle as IO
from tests import exact_geometry as X


# ---- the exact reference's own known answers (CPU) ---------------------------------------------------------------------------

def _mot(x=0, y=0, z=0, o=0, l=2, w=1, h=1):
    return np.array([x, y, z, o, l, w, h], float)


@X.exact
def test_exact_reference_known_answers():
    tiny = D(10) ** -50
    sqrt2 = D(2).sqrt()
    s1, s2 = _mot(l=2, w=2), _mot(l=2, w=2, o=math.pi / 4)
    # two concentric squares of side 2, one turned by o: 8 / (1 + sin o + cos o); at pi/4 the octagon 8 (sqrt 2 - 1), a minimum, so the
    # 1e-17 rad by which the double misses pi/4 moves it by 1e-33
    assert abs(X.mot_terms(s1, s2).inter - 8 * (sqrt2 - 1)) < D("1e-30")
    for o in (1e-9, 0.3, 0.7, math.pi / 4, 1.2, math.nextafter(math.pi / 2, 0)):
        sn, cs = X.sincos(o)
        closed = 8 / (1 + sn + cs)
        assert abs(X.mot_terms(s1, _mot(l=2, w=2, o=o)).inter - closed) < tiny and abs(X.mot_terms(_mot(l=2, w=2, o=o), s1).inter - closed) < tiny
        assert abs(X.intersection_area_by_vertices(X.corners_mot(s1), X.corners_mot(_mot(l=2, w=2, o=o))) - closed) < D("1e-38")
    a = _mot()
    t = X.mot_terms(a, a)
    assert t.inter == 2 and t.hull == 2 and t.oh == 1 and t.uh == 1
    assert abs(X.iou3d(t) - 2 / (2 + X.dec(1e-5))) < tiny and X.giou3d(t) == 1
    t = X.mot_terms(a, _mot(x=1.0))                                        # half overlap along the length
    assert t.inter == 1 and t.hull == 3 and abs(X.giou3d(t) - D(1) / 3) < tiny
    t = X.mot_terms(a, _mot(x=5.0))                                        # disjoint; hull of two separated boxes 7 x 1
    assert t.inter == 0 and t.hull == 7 and X.iou3d(t) == 0 and abs(X.giou3d(t) - (0 - D(3) / 7)) < tiny
    t = X.mot_terms(a, _mot(x=5.0, y=1.0))                                 # hull of two boxes apart in both axes: hexagon 7 x 2 - 2 (5 x 1 / 2)
    assert t.hull == 9
    big, small = _mot(l=4, w=4), _mot(x=0.5, y=-0.3, o=0.7, l=1, w=0.5)   # containment, both orders
    assert abs(X.mot_terms(big, small).inter - D("0.5")) < tiny and abs(X.mot_terms(small, big).inter - D("0.5")) < tiny
    assert abs(X.mot_terms(big, small).hull - 16) < tiny
    t = X.mot_terms(a, _mot(z=0.5))                                        # half overlap in height
    assert t.oh == D("0.5") and t.uh == D("1.5") and abs(X.iou3d(t) - 1 / (3 + X.dec(1e-5))) < tiny
    assert X.mot_terms(a, _mot(z=3.0)).oh == 0
    assert X.giou3d(X.mot_terms(_mot(l=0), _mot(l=0))) is None             # two boxes of zero area: 0 / 0
    # the two conventions describe the same rectangle
    row = np.array([[1.5, -2.25, 0.3, 0.7, 3.0, 1.25, 1.5]])
    cm, cb = X.corners_mot(row[0]), X.corners_bev(X.to_bev(row, np.float64)[0])
    assert all(min(abs(p[0] - q[0]) + abs(p[1] - q[1]) for q in cb) < tiny for p in cm)
    # det3d formulas: identical -> 1; half height overlap of identical footprints -> (V / 2) / (1.5 V); the cross 2 x 2 of 4 x 2 boxes
    b = np.array([1, 2, 0, 2, 4, 2, 0.3], np.float32)
    up = b.copy()
    up[2] += 1
    assert abs(X.bev_iou(b, b) - 1) < tiny and abs(X.det3d_iou3d(b, b) - 1) < tiny and abs(X.det3d_iou3d(b, up) - D(1) / 3) < tiny
    c0 = np.array([0, 0, 0, 4, 2, 1, 0.0], np.float32)
    assert X.bev_overlap(c0, np.array([2, 0, 0, 4, 2, 1, 0.0], np.float32)) == 4
    assert X.bev_overlap(c0, np.array([10, 0, 0, 4, 2, 1, 0.3], np.float32)) == 0
    assert X.greedy_nms([[0, .6, 0], [.6, 0, .6], [0, .6, 0]], 0.5) == [0, 2]
    try:
        import mpmath
    except ImportError:
        return
    mpmath.mp.dps = 80
    for ang in (0.0, 1e-15, 0.7, math.pi / 4, math.pi / 2, math.pi, -math.pi, math.nextafter(math.pi, 0), -2.5, 3.0, 7.5):
        sn, cs = X.sincos(ang)
        assert abs(mpmath.mpf(str(sn)) - mpmath.sin(mpmath.mpf(ang))) < mpmath.mpf(10) ** -60
        assert abs(mpmath.mpf(str(cs)) - mpmath.cos(mpmath.mpf(ang))) < mpmath.mpf(10) ** -60
    assert abs(mpmath.mpf(str(X._PI)) - mpmath.pi) < mpmath.mpf(10) ** -70


@functools.lru_cache(maxsize=None)
def _pairs(offset_index, swapped=False):
    A, B, fam = X.all_pose_pairs()
    A, B = X.at_offset(A, X.OFFSETS[offset_index]), X.at_offset(B, X.OFFSETS[offset_index])
    return (B, A, fam) if swapped else (A, B, fam)


@functools.lru_cache(maxsize=None)
def _terms(offset_index, swapped=False):
    A, B, _ = _pairs(offset_index, swapped)
    return [X.mot_terms(A[i], B[i]) for i in range(len(A))]


def _tol(a, b):
    return X.tol_area(a[:2], b[:2], a[4:6], b[4:6])


def test_pose_families_are_what_they_say():
    assert len(X.FAMILIES) == 12 and all(ox != oy for ox, oy in X.OFFSETS[1:])
    A, B, fam = _pairs(0)
    t = _terms(0)
    for k, f in enumerate(X.FAMILIES):
        idx = np.flatnonzero(fam == k)
        assert len(idx) >= 40, f
        sides = np.concatenate([A[idx, 4:6], B[idx, 4:6]]).ravel()
        assert sides.max() <= 5.0
        if f not in ("sliver", "zero_length", "concentric", "half_inside"):
            assert sides.min() >= 0.5, f
        aligned = [i for i in idx if A[i, 3] == 0.0 and B[i, 3] == 0.0]
        assert len(aligned) >= 10 or f in ("turn", "tiny_rotation", "random"), f
        area_a, area_b = A[idx, 4] * A[idx, 5], B[idx, 4] * B[idx, 5]
        ov = np.array([float(t[i].inter) for i in idx])
        if f == "identical":
            assert np.array_equal(A[idx], B[idx]) and all(t[i].inter == X.dec(A[i, 4]) * X.dec(A[i, 5]) for i in aligned)
        elif f in ("edge_contact", "corner_contact"):
            assert all(t[i].inter == 0 for i in aligned) and ov.max() < 1e-14      # contact only: the turned rows touch to rounding
        elif f == "half_inside":
            assert all(t[i].inter == X.dec(B[i, 4]) * X.dec(B[i, 5]) for i in aligned) and np.abs(ov - area_b).max() < 1e-14
        elif f == "concentric":
            assert np.abs(ov - area_b).max() < 1e-14 and (area_b < area_a + 1e-12).all()
        elif f == "zero_length":
            assert (ov == 0).all() and (area_b == 0).all() and (area_a == 0).sum() >= 5
        elif f == "sliver":
            assert (B[idx, 5] == 1e-9).all() and 0 < ov.max() < 1e-8
        elif f == "axis_ties":
            assert len(aligned) >= 30
    # the float32 centres of the axis-aligned rows are the same numbers at every offset: the ties survive the cast
    for oi in range(4):
        P, Q, _ = _pairs(oi)
        for R in (P, Q):
            keep = R[:, 3] == 0.0
            assert np.array_equal(X.to_bev(R)[keep, :2].astype(np.float64), R[keep, :2])


@X.exact
def test_two_exact_routes_to_the_overlap_agree():
    """Half-plane clipping against the hull of (contained corners + edge crossings): two algorithms, one area, on every pose."""
    worst = D(0)
    for oi in (0, 2):
        A, B, _ = _pairs(oi)
        for i in range(len(A)):
            ca, cb = X.corners_mot(A[i]), X.corners_mot(B[i])
            worst = max(worst, abs(X.intersection_area(ca, cb) - X.intersection_area_by_vertices(ca, cb)),
                        abs(X.intersection_area(cb, ca) - X.intersection_area_by_vertices(ca, cb)))
    assert worst < D("1e-38"), worst


def test_oracle_within_a_quarter_of_the_area_bar_of_exact():
    """`oracle/iou_oracle.py` (numpy float64, the kernel's algorithm) against the exact areas: clip and hull within tolA / 4 on every
    family at every offset in both orders.  The hull check leaves out two slivers or two zero-length boxes on one line, and only those
    (hull below 1e-6 m^2): their eight corners are collinear to 1e-9 and Qhull, which the oracle calls like the reference does, refuses
    them as flat."""
    worst_clip, worst_hull = {}, {}
    for oi in range(4):
        for swapped in (False, True):
            A, B, fam = _pairs(oi, swapped)
            terms = _terms(oi, swapped)
            for i in range(len(A)):
                bar = _tol(A[i], B[i]) / 4
                f = (X.FAMILIES[fam[i]], oi)
                worst_clip[f] = max(worst_clip.get(f, 0.0), abs(float(X.dec(IO.intersection_area(A[i], B[i])) - terms[i].inter)) / bar)
                try:
                    hull = IO.hull_area(A[i], B[i])
                except QhullError:
                    assert terms[i].hull < 1e-6, f
                    continue
                worst_hull[f] = max(worst_hull.get(f, 0.0), abs(float(X.dec(hull) - terms[i].hull)) / bar)
    print("oracle / (tolA/4): clip %.3f hull %.3f" % (max(worst_clip.values()), max(worst_hull.values())))
    bad = {k: v for d in (worst_clip, worst_hull) for k, v in d.items() if not v <= 1.0}
    assert not bad, bad


# ---- rotated NMS sets built from the families ---------------------------------------------------------------------------------

NMS_SETS = ((64, 1, 1), (65, 3, 3), (300, 2, 3))   # (boxes, index into OFFSETS, seed of the pose pairs: chosen so that no exact IoU is near a threshold)
NMS_THRESHOLDS = (0.05, 0.3, 0.7)


def _round_robin():
    """Pair indices with the families interleaved, so that any prefix holds every family."""
    fam = _pairs(0)[2]
    rank = np.zeros(len(fam), int)
    for k in range(len(X.FAMILIES)):
        rank[fam == k] = np.arange((fam == k).sum())
    return np.lexsort((fam, rank))


@functools.lru_cache(maxsize=None)
def _nms_set(n, offset_index, seed):
    """n float32 boxes: family members and their partners, pair k moved to its own cell of a 4 m grid (boxes are up to 5 m long, so
    neighbouring cells overlap now and then), a seeded score order.  Returns (boxes, scores, exact IoU matrix in score order)."""
    A, B, _ = X.all_pose_pairs(seed=seed)
    order = _round_robin()[:(n + 1) // 2]
    g = int(math.ceil(math.sqrt(len(order))))
    rows = []
    for k, i in enumerate(order):
        for r in (A[i], B[i]):
            r = r.copy()
            r[0] += 4.0 * (k % g)
            r[1] += 4.0 * (k // g)
            rows.append(r)
    boxes = X.to_bev(X.at_offset(np.array(rows[:n]), X.OFFSETS[offset_index]))
    scores = np.random.default_rng(n).permutation(n).astype(np.float32)
    srt = boxes[np.argsort(-scores, kind="stable")]
    corners = [X.corners_bev(b) for b in srt]
    iou = [[D(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            iou[i][j] = iou[j][i] = X.bev_iou(srt[i], srt[j], X.intersection_area(corners[i], corners[j]))
    return boxes, scores, iou


@pytest.mark.parametrize("n,offset_index,seed", NMS_SETS)
def test_nms_sets_keep_clear_of_the_thresholds(n, offset_index, seed):
    """No exact IoU within 1e-6 of a threshold, so a keep list that differs from the exact one is a wrong overlap, not a rounding;
    and every threshold splits the set (some boxes go, some stay)."""
    _, _, iou = _nms_set(n, offset_index, seed)
    vals = np.array([float(iou[i][j]) for i in range(n) for j in range(i + 1, n)])
    for th in NMS_THRESHOLDS:
        assert np.abs(vals - float(np.float32(th))).min() > 1e-6, (th, np.abs(vals - th).min())
        keep = X.greedy_nms(iou, X.dec(np.float32(th)))
        assert n // 4 < len(keep) < n
    assert (vals == 1.0).any() and (vals == 0.0).any()


# ---- the kernels (GPU) --------------------------------------------------------------------------------------------------------

def _distance_check(got, A, B, fam, terms, giou):
    """(worst error / bar, rows over the bar) of the distances got[i] of the pairs (A[i], B[i])."""
    worst, bad = 0.0, []
    for i, t in enumerate(terms):
        assert math.isfinite(got[i]) or (giou and t.vola == 0 and t.volb == 0), (i, got[i])
        want = X.giou3d(t) if giou else X.iou3d(t)
        if want is None:          # two boxes of zero area: the reference's GIoU is 0 / 0; the kernel only has to return
            continue
        if not giou and t.inter == 0 and (t.vola == 0 or t.volb == 0):
            assert got[i] == 1.0, (X.FAMILIES[fam[i]], i, got[i])   # a box of zero length overlaps nothing, exactly
        bar = X.iou_distance_bar(t, _tol(A[i], B[i]), giou)
        ratio = abs(float(X.dec(got[i]) - (1 - want))) / bar
        worst = max(worst, ratio)
        if not ratio <= 1.0:
            bad.append((X.FAMILIES[fam[i]], i, ratio))
    return worst, bad


@pytest.mark.gpu
@pytest.mark.parametrize("offset_index", range(4))
@pytest.mark.parametrize("asso", ["iou", "giou"])
def test_hip_iou3d_distance_vs_exact(asso, offset_index):
    from shasta_amd import association as assoc
    n_left_out = 0
    for swapped in (False, True):
        A, B, fam = _pairs(offset_index, swapped)
        terms = _terms(offset_index, swapped)
        got = assoc.compute_iou_distance(list(A), list(B), asso).diagonal()
        worst, bad = _distance_check(got, A, B, fam, terms, asso == "giou")
        print("iou3d %s offset %g swapped %d: worst error / bar %.4f" % (asso, X.OFFSETS[offset_index][0], swapped, worst))
        assert not bad, bad[:10]
        n_left_out += sum(t.vola == 0 and t.volb == 0 for t in terms)
    assert n_left_out <= 0.1 * 2 * len(terms)


@pytest.mark.gpu
@pytest.mark.parametrize("asso", ["iou", "giou"])
def test_hip_iou3d_translation_invariance(asso):
    """The same pairs at the origin and 2000 m out: the distances differ by no more than the sum of their two bars."""
    from shasta_amd import association as assoc
    giou = asso == "giou"
    A0, B0, fam = _pairs(0)
    A2, B2, _ = _pairs(2)
    d0 = assoc.compute_iou_distance(list(A0), list(B0), asso).diagonal()
    d2 = assoc.compute_iou_distance(list(A2), list(B2), asso).diagonal()
    worst = 0.0
    for i, (t0, t2) in enumerate(zip(_terms(0), _terms(2))):
        if giou and X.giou3d(t0) is None:
            continue
        bar = X.iou_distance_bar(t0, _tol(A0[i], B0[i]), giou) + X.iou_distance_bar(t2, _tol(A2[i], B2[i]), giou)
        worst = max(worst, abs(d0[i] - d2[i]) / bar)
        assert abs(d0[i] - d2[i]) <= bar, (X.FAMILIES[fam[i]], i, d0[i], d2[i], bar)
    print("iou3d %s offset 0 vs 2000: worst difference / summed bars %.4f" % (asso, worst))


@pytest.mark.gpu
def test_hip_iou3d_c_abi_row_stride_and_poisoned_padding():
    """box_stride = 9 with NaN in the two padding columns: the same bits as the packed call, and the whole matrix within the bars."""
    import torch

    from shasta_amd import hip
    lib = hip.load()
    dev = torch.device("cuda:0")
    A, B, fam = _pairs(2)
    rr = _round_robin()
    D9, T9 = np.full((13, 9), np.nan), np.full((11, 9), np.nan)
    D9[:, :7], T9[:, :7] = A[rr[:13]], B[rr[:11]]
    for giou in (0, 1):
        outs = []
        for d, t, stride in ((D9, T9, 9), (D9[:, :7], T9[:, :7], 7)):
            td, tt = torch.from_numpy(np.ascontiguousarray(d)).to(dev), torch.from_numpy(np.ascontiguousarray(t)).to(dev)
            out = torch.full((13, 11), float("nan"), dtype=torch.float64, device=dev)
            hip.check(lib.shasta_iou3d_distance_f64(hip.ptr(td), 13, hip.ptr(tt), 11, stride, giou, hip.ptr(out), hip.stream_ptr()), "iou3d")
            outs.append(out.cpu().numpy())
        assert np.array_equal(outs[0], outs[1]) and np.isfinite(outs[0]).all()
        rows = [(i, j) for i in range(13) for j in range(11)]
        PA, PB = np.array([D9[i, :7] for i, _ in rows]), np.array([T9[j, :7] for _, j in rows])
        terms = [X.mot_terms(a, b) for a, b in zip(PA, PB)]
        worst, bad = _distance_check(outs[0].ravel(), PA, PB, fam[rr[[i for i, _ in rows]]], terms, bool(giou))
        assert not bad, bad[:10]


def _kernel_rows(rows):
    """float32 rows as the three matrix entry points see them, and the det3d-convention rows whose `to_pcdet` image they are (so that
    one exact overlap serves overlap, BEV IoU and the wrapper's 3-D IoU)."""
    import torch

    from shasta_amd import nms
    bev = X.to_bev(rows)
    det3d = bev[:, [0, 1, 2, 4, 3, 5, 6]].copy()
    det3d[:, 6] = -bev[:, 6] - np.float32(math.pi / 2)
    return nms.to_pcdet(torch.from_numpy(det3d).clone()).numpy().copy(), det3d


BEV_SIZES = ((1, 1), (3, 64), (4, 65), (5, 127), (130, 129))   # across the 64-column and 4-row block seams


@pytest.mark.gpu
@pytest.mark.parametrize("na,nb,offset_index", [(na, nb, oi) for (na, nb) in BEV_SIZES[:4] for oi in range(4)] + [(130, 129, -1)])
def test_hip_bev_matrices_vs_exact(na, nb, offset_index):
    """boxes_overlap_bev / boxes_iou_bev / boxes_iou3d_gpu: EVERY entry against the exact value, family pairs on the diagonal and
    their cross pairs off it, in both argument orders.  The largest size mixes the four offsets (pair i at offset (i // 12) % 4)."""
    import torch

    from shasta_amd import nms
    dev = torch.device("cuda:0")
    rr = _round_robin()
    n = max(na, nb)
    if offset_index >= 0:
        A, B, _ = _pairs(offset_index)
        PA, PB = A[rr[:n]], B[rr[:n]]
    else:
        PA = np.array([_pairs((k // 12) % 4)[0][i] for k, i in enumerate(rr[:n])])
        PB = np.array([_pairs((k // 12) % 4)[1][i] for k, i in enumerate(rr[:n])])
    worst = [0.0, 0.0, 0.0]
    bad = []
    for P, Q in ((PA, PB), (PB, PA)):
        ka, da = _kernel_rows(P[:na])
        kb, db = _kernel_rows(Q[:nb])
        ta, tb = torch.from_numpy(ka).to(dev), torch.from_numpy(kb).to(dev)
        ov = nms.boxes_overlap_bev(ta, tb).cpu().numpy()
        iou = nms.boxes_iou_bev(ta, tb).cpu().numpy()
        iou3 = nms.boxes_iou3d_gpu(torch.from_numpy(da).to(dev), torch.from_numpy(db).to(dev)).cpu().numpy()
        assert ov.shape == iou.shape == iou3.shape == (na, nb) and ov.dtype == np.float32
        ca, cb = [X.corners_bev(r) for r in ka], [X.corners_bev(r) for r in kb]
        for i in range(na):
            for j in range(nb):
                exact = X.intersection_area(ca[i], cb[j])
                tolA = X.tol_area(ka[i, :2], kb[j, :2], ka[i, 3:5], kb[j, 3:5])
                r = (abs(float(X.dec(ov[i, j]) - exact)) / (2.0 ** -23 * float(exact) + tolA),
                     abs(float(X.dec(iou[i, j]) - X.bev_iou(ka[i], kb[j], exact))) / 2e-6,
                     abs(float(X.dec(iou3[i, j]) - X.det3d_iou3d(ka[i], kb[j], exact))) / 5e-6)
                worst = [max(w, v) for w, v in zip(worst, r)]
                if not max(r) <= 1.0:
                    bad.append((i, j, r))
    print("bev %dx%d offset %s: worst error / bar overlap %.4f iou %.4f iou3d %.4f" % (na, nb, offset_index, *worst))
    assert not bad, bad[:10]


@pytest.mark.gpu
@pytest.mark.parametrize("n,offset_index,seed", NMS_SETS)
def test_hip_rotated_nms_keeps_what_exact_geometry_keeps(n, offset_index, seed):
    import torch

    from shasta_amd import nms
    dev = torch.device("cuda:0")
    boxes, scores, iou = _nms_set(n, offset_index, seed)
    order = np.argsort(-scores, kind="stable")
    vals = np.array([float(iou[i][j]) for i in range(n) for j in range(i + 1, n)])
    for th in NMS_THRESHOLDS:
        assert np.abs(vals - float(np.float32(th))).min() > 1e-6
        sel, _ = nms.nms_gpu(torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), th)
        want = order[X.greedy_nms(iou, X.dec(np.float32(th)))]
        assert np.array_equal(sel.cpu().numpy(), want), (n, th)
