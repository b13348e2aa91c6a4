"""Exact planar geometry for the rotated-box kernels (TEST INFRASTRUCTURE; a plain module that tests import).

An evaluation of what `csrc/iou3d.hip` and `csrc/nms.hip` compute that shares no code and no arithmetic with them or with
`oracle/iou_oracle.py`: every quantity is derived from the box parameters, taken exactly as the float64 / float32 values given,
in `decimal` arithmetic of PREC = 60 digits (cos and sin by their Taylor series after an exact quarter-turn reduction).  At that
precision a sign decision taken on a tie cannot move an area by more than 1e-50, so the tie rules of the clip and of the hull
do not matter here - which is exactly what makes it a reference for the kernels' tie rules.  Standard library only.

  corners_mot / corners_bev      corners of [x, y, z, o, l, w, h] (mot_3d, iou3d.hip) / [x, y, z, dx, dy, dz, heading] (det3d, nms.hip)
  intersection_area              two convex polygons, half-plane clipping on Python lists (no fixed scratch size)
  intersection_area_by_vertices  the same area by a second route: hull of (corners inside the other polygon + edge crossings)
  hull_area                      convex hull of a point set (monotone chain), its area
  iou3d / giou3d / bev_overlap / bev_iou / det3d_iou3d      the formulas in the kernels' header comments, on exact areas
  tol_area / iou_distance_bar    the bars of tests/test_geometry_exact.py
  pose_pairs / OFFSETS / FAMILIES  the degenerate-pose generator all those tests share
"""
import collections
import decimal
import functools
import math
from decimal import Decimal as D
from fractions import Fraction

import numpy as np

PREC = 60
_CTX = decimal.Context(prec=PREC, rounding=decimal.ROUND_HALF_EVEN, Emin=-10**6, Emax=10**6)
_WIDE = decimal.Context(prec=PREC + 15, rounding=decimal.ROUND_HALF_EVEN, Emin=-10**6, Emax=10**6)
EPS = 2.0 ** -52


def exact(fn):
    """Run `fn` under the 60-digit context whatever the caller's decimal context is (a test that does decimal arithmetic of its own
    on the results wears it too: the default context would round to 28 digits)."""
    @functools.wraps(fn)
    def run(*args, **kw):
        with decimal.localcontext(_CTX):
            return fn(*args, **kw)
    return run


def dec(v):
    """The exact value of a float (numpy float32 / float64 scalars included): binary floats are decimal fractions."""
    return v if isinstance(v, D) else D(float(v))


def _pi_wide():
    """pi to PREC + 15 digits: Machin's formula 16 atan(1/5) - 4 atan(1/239) in exact rationals, rounded once."""
    def atan_inv(q, terms):
        return sum(Fraction((-1) ** k, (2 * k + 1) * q ** (2 * k + 1)) for k in range(terms))
    f = 16 * atan_inv(5, 60) - 4 * atan_inv(239, 20)   # truncation below 5^-121 < 1e-84
    with decimal.localcontext(_WIDE):
        return D(f.numerator) / D(f.denominator)


_PI = _pi_wide()


@functools.lru_cache(maxsize=None)
def sincos(angle):
    """(sin, cos) of the float `angle`, correct to about PREC + 10 digits: angle = k * pi/2 + r with |r| <= pi/4, Taylor series in r."""
    with decimal.localcontext(_WIDE):
        x = dec(angle)
        half_pi = _PI / 2
        k = int((x / half_pi).to_integral_value(rounding=decimal.ROUND_HALF_EVEN))
        r = x - k * half_pi
        r2 = r * r
        tiny = D(10) ** -(PREC + 14)
        s, term, n = r, r, 1
        while abs(term) > tiny:
            term = -term * r2 / ((n + 1) * (n + 2))
            s += term
            n += 2
        c, term, n = D(1), D(1), 0
        while abs(term) > tiny:
            term = -term * r2 / ((n + 1) * (n + 2))
            c += term
            n += 2
        return ((s, c), (c, -s), (-s, -c), (-c, s))[k % 4]


@exact
def corners_mot(b):
    """[x, y, z, o, l, w, h] -> the four corners in the order of mot_3d's box2corners2d."""
    x, y, l, w = dec(b[0]), dec(b[1]), dec(b[4]), dec(b[5])
    sn, cs = sincos(float(b[3]))
    return [(x + cs * l / 2 + sn * w / 2, y + sn * l / 2 - cs * w / 2), (x + cs * l / 2 - sn * w / 2, y + sn * l / 2 + cs * w / 2),
            (x - cs * l / 2 - sn * w / 2, y - sn * l / 2 + cs * w / 2), (x - cs * l / 2 + sn * w / 2, y - sn * l / 2 - cs * w / 2)]


@exact
def corners_bev(b):
    """[x, y, z, dx, dy, dz, heading] -> the four corners of the footprint, counter-clockwise."""
    x, y, hx, hy = dec(b[0]), dec(b[1]), dec(b[3]) / 2, dec(b[4]) / 2
    sn, cs = sincos(float(b[6]))
    return [(x + ux * cs - uy * sn, y + ux * sn + uy * cs) for ux, uy in ((-hx, -hy), (hx, -hy), (hx, hy), (-hx, hy))]


def _twice_signed_area(p):
    return sum(p[i][0] * p[(i + 1) % len(p)][1] - p[i][1] * p[(i + 1) % len(p)][0] for i in range(len(p)))


def _disjoint_boxes(P, Q):
    """True when the axis-aligned bounding boxes are strictly apart (then so are the polygons): an exact shortcut."""
    for k in (0, 1):
        if max(p[k] for p in P) < min(q[k] for q in Q) or max(q[k] for q in Q) < min(p[k] for p in P):
            return True
    return False


@exact
def intersection_area(P, Q):
    """Area of the intersection of two convex polygons (vertex lists, either orientation; degenerate ones have none)."""
    if _disjoint_boxes(P, Q):
        return D(0)
    sp, sq = _twice_signed_area(P), _twice_signed_area(Q)
    if sp == 0 or sq == 0:
        return D(0)
    if sq < 0:
        Q = Q[::-1]
    poly = list(P)
    for i in range(len(Q)):
        a, b = Q[i], Q[(i + 1) % len(Q)]
        ex, ey = b[0] - a[0], b[1] - a[1]
        side = [ex * (p[1] - a[1]) - ey * (p[0] - a[0]) for p in poly]
        nxt = []
        for j, p in enumerate(poly):
            k = (j + 1) % len(poly)
            if side[j] >= 0:
                nxt.append(p)
            if (side[j] >= 0) != (side[k] >= 0):
                t = side[j] / (side[j] - side[k])
                nxt.append((p[0] + t * (poly[k][0] - p[0]), p[1] + t * (poly[k][1] - p[1])))
        poly = nxt
        if len(poly) < 3:
            return D(0)
    return abs(_twice_signed_area(poly)) / 2


@exact
def hull_area(points):
    """Area of the convex hull of a point set (Andrew's monotone chain; collinear points are dropped, which leaves the area)."""
    pts = sorted(set(points))
    if len(pts) < 3:
        return D(0)

    def chain(seq):
        h = []
        for p in seq:
            while len(h) >= 2 and (h[-1][0] - h[-2][0]) * (p[1] - h[-2][1]) - (h[-1][1] - h[-2][1]) * (p[0] - h[-2][0]) <= 0:
                h.pop()
            h.append(p)
        return h

    lower, upper = chain(pts), chain(pts[::-1])
    return abs(_twice_signed_area(lower[:-1] + upper[:-1])) / 2


@exact
def intersection_area_by_vertices(P, Q):
    """The same area by another route: the intersection of two convex polygons is the convex hull of the corners of each that lie
    in the other plus the crossings of their edges.  `slack` only widens 'inside' by 1e-45 of the size, so that a corner on an edge
    is not lost to the last digit; it moves the area by less than 1e-40."""
    sp, sq = _twice_signed_area(P), _twice_signed_area(Q)
    if sp == 0 or sq == 0:
        return D(0)
    P = P if sp > 0 else P[::-1]
    Q = Q if sq > 0 else Q[::-1]
    size = max(abs(c) for p in P + Q for c in p) + 1
    slack = size * size * D(10) ** -45

    def inside(p, poly):
        return all((poly[(i + 1) % 4][0] - poly[i][0]) * (p[1] - poly[i][1]) - (poly[(i + 1) % 4][1] - poly[i][1]) * (p[0] - poly[i][0]) >= -slack
                   for i in range(4))

    pts = [p for p in P if inside(p, Q)] + [q for q in Q if inside(q, P)]
    for i in range(len(P)):
        a, b = P[i], P[(i + 1) % len(P)]
        for j in range(len(Q)):
            c, d = Q[j], Q[(j + 1) % len(Q)]
            den = (b[0] - a[0]) * (d[1] - c[1]) - (b[1] - a[1]) * (d[0] - c[0])
            if abs(den) <= slack:   # parallel edges: their common part, if any, ends in corners already collected
                continue
            t = ((c[0] - a[0]) * (d[1] - c[1]) - (c[1] - a[1]) * (d[0] - c[0])) / den
            u = ((c[0] - a[0]) * (b[1] - a[1]) - (c[1] - a[1]) * (b[0] - a[0])) / den
            if 0 <= t <= 1 and 0 <= u <= 1:
                pts.append((a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1])))
    return hull_area(pts)


# ---- the kernels' formulas on exact areas -----------------------------------------------------------------------------------

MotTerms = collections.namedtuple("MotTerms", "inter hull oh uh vola volb")


@exact
def mot_terms(a, b):
    """Everything iou3d / giou3d of mot_3d/utils/geometry.py are made of, for boxes [x, y, z, o, l, w, h]."""
    ca, cb = corners_mot(a), corners_mot(b)
    za, zb, ha, hb = dec(a[2]), dec(b[2]), dec(a[6]), dec(b[6])
    d1, d2 = (za + ha / 2) - (zb - hb / 2), (zb + hb / 2) - (za - ha / 2)
    flat = dec(a[4]) * dec(a[5]) == 0 or dec(b[4]) * dec(b[5]) == 0   # a box of zero length or width overlaps nothing
    return MotTerms(D(0) if flat else intersection_area(ca, cb), hull_area(ca + cb), max(D(0), min(d1, d2)), max(d1, d2),
                    dec(a[5]) * dec(a[4]) * ha, dec(b[5]) * dec(b[4]) * hb)


@exact
def iou3d(t):
    """iou3d.hip mode 0: overlap volume / (vol_a + vol_b - overlap + 1e-5), 1e-5 being the double the kernel adds."""
    ov = t.inter * t.oh
    return ov / ((t.vola + t.volb - ov) + dec(1e-5))


@exact
def giou3d(t):
    """iou3d.hip mode 1: I / U - (C - U) / C; None where two boxes of zero area make it 0 / 0."""
    I = t.inter * t.oh
    U = t.vola + t.volb - I
    C = t.hull * t.uh
    if U == 0 or C == 0:
        return None
    return I / U - (C - U) / C


@exact
def bev_overlap(a, b):
    """Overlap area of the footprints of two [x, y, z, dx, dy, dz, heading] rows."""
    if dec(a[3]) * dec(a[4]) == 0 or dec(b[3]) * dec(b[4]) == 0:
        return D(0)
    return intersection_area(corners_bev(a), corners_bev(b))


@exact
def bev_iou(a, b, ov=None):
    """nms.hip: overlap / max(area_a + area_b - overlap, 1e-8)."""
    ov = bev_overlap(a, b) if ov is None else ov
    return ov / max(dec(a[3]) * dec(a[4]) + dec(b[3]) * dec(b[4]) - ov, dec(1e-8))


@exact
def det3d_iou3d(a, b, ov=None):
    """boxes_bev_kernel mode 2 on rows already in the kernel's convention: overlap * height overlap / max(vol_a + vol_b - that, 1e-6)."""
    ov = bev_overlap(a, b) if ov is None else ov
    amax, amin, bmax, bmin = dec(a[2]) + dec(a[5]) / 2, dec(a[2]) - dec(a[5]) / 2, dec(b[2]) + dec(b[5]) / 2, dec(b[2]) - dec(b[5]) / 2
    o3 = ov * max(min(amax, bmax) - max(amin, bmin), D(0))
    return o3 / max(dec(a[3]) * dec(a[4]) * dec(a[5]) + dec(b[3]) * dec(b[4]) * dec(b[5]) - o3, dec(1e-6))


def greedy_nms(iou, thresh):
    """Greedy suppression in the given order on a full IoU matrix (list of rows or array): the kept indices."""
    n = len(iou)
    removed = [False] * n
    keep = []
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        for j in range(i + 1, n):
            if iou[i][j] > thresh:
                removed[j] = True
    return keep


# ---- bars -------------------------------------------------------------------------------------------------------------------

def tol_area(xy_a, xy_b, sides_a, sides_b):
    """tolA = 16 eps (C + L) L: the float64 format's own floor for an area whose corners are held in the world frame, C the largest
    |x| or |y| of the two centres and L the longest side, with a margin of 16 over the unit."""
    C = max(abs(float(v)) for v in (*xy_a, *xy_b))
    L = max(float(v) for v in (*sides_a, *sides_b))
    return 16 * EPS * (C + L) * L


@exact
def iou_distance_bar(t, tolA, giou):
    """tolA carried to first order through 1 - iou3d / 1 - giou3d at the exact values (tolA * oh on the overlap volume, tolA * uh on
    the hull volume), plus 16 eps for the arithmetic of the formula itself, times two."""
    tolA = dec(tolA)
    I, U0 = t.inter * t.oh, t.vola + t.volb
    if not giou:
        den = (U0 - I) + dec(1e-5)
        bar = (U0 + dec(1e-5)) / (den * den) * tolA * t.oh
    else:
        U, C = U0 - I, t.hull * t.uh
        bar = abs(U0 / (U * U) - 1 / C) * tolA * t.oh + U / (C * C) * tolA * t.uh
    return float(2 * (bar + 16 * dec(EPS)))


# ---- pose families ----------------------------------------------------------------------------------------------------------
# Rows are [x, y, z, heading, length, width, height] = the mot_3d layout; `to_bev` reorders them for nms.hip.  Centres lie on a grid
# of 1/64 m and sides on one of 1/16 m, so that the axis-aligned half of every family is an exact tie in float64 AND in float32,
# also after one of the OFFSETS (integers, different in x and y) is added; the rotated half is as degenerate as floats allow.

OFFSETS = ((0.0, 0.0), (50.0, -30.0), (2000.0, -1250.0), (1e5, -70000.0))
FAMILIES = ("identical", "turn", "tiny_rotation", "slide", "edge_contact", "corner_contact", "half_inside", "concentric", "sliver",
            "zero_length", "axis_ties", "random")
PAIRS_PER_FAMILY = 40
RANDOM_PAIRS = 60


def _grid(v, step):
    return np.round(np.asarray(v, np.float64) / step) * step


def _shifted(a, along, across):
    """Row `a` with its centre moved by (along, across) in its own frame."""
    b = a.copy()
    c, s = math.cos(a[3]), math.sin(a[3])
    b[0] += along * c - across * s
    b[1] += along * s + across * c
    return b


def pose_pairs(family, n=None, seed=0):
    """(A, B): two (n, 7) float64 arrays of rows [x, y, z, heading, length, width, height] around the origin, pair i = (A[i], B[i])."""
    n = (RANDOM_PAIRS if family == "random" else PAIRS_PER_FAMILY) if n is None else n
    rng = np.random.default_rng([FAMILIES.index(family), seed])
    A = np.zeros((n, 7))
    A[:, 0:2] = _grid(rng.uniform(-3, 3, (n, 2)), 1 / 64)
    A[:, 2] = _grid(rng.normal(0, 0.5, n), 1 / 64)
    A[:, 3] = np.where(np.arange(n) % 2 == 0, 0.0, rng.uniform(-math.pi, math.pi, n))   # even rows axis-aligned, odd rows turned
    A[:, 4:6] = _grid(rng.uniform(0.5, 5, (n, 2)), 1 / 16)
    A[:, 6] = _grid(rng.uniform(0.5, 2, n), 1 / 16)
    B = A.copy()
    for i in range(n):
        a, v = A[i], i // 2   # v: the variant counter, independent of the aligned / turned alternation
        l, w = a[4], a[5]
        if family == "identical":
            continue
        if family == "turn":
            if v % 4 == 3:   # the same box described just inside +pi and just inside -pi
                A[i, 3] = math.nextafter(math.pi, 0) * (1 if i % 2 else -1)
                B[i] = A[i]
                B[i, 3] = -A[i, 3]
            else:
                B[i, 3] = a[3] + (math.pi / 2, math.pi, -math.pi)[v % 4]
        elif family == "tiny_rotation":
            B[i, 3] = a[3] + (1e-15, 1e-12, 1e-9, 1e-6)[v % 4]
        elif family == "slide":
            s = rng.uniform(0, 1.2)
            B[i] = _shifted(a, _grid(s * l, 1 / 64), 0) if v % 2 == 0 else _shifted(a, 0, _grid(s * w, 1 / 64))
        elif family == "edge_contact":
            B[i] = _shifted(a, l, 0) if v % 2 == 0 else _shifted(a, 0, -w)
        elif family == "corner_contact":
            B[i] = _shifted(a, (l, -l)[v % 2], (w, -w)[(v // 2) % 2])
        elif family == "half_inside":
            B[i] = _shifted(a, (l / 4, -l / 4)[v % 2], (w / 4, -w / 4)[(v // 2) % 2])
            B[i, 4:6] = l / 2, w / 2
        elif family == "concentric":
            if v % 2 == 0:
                B[i, 4:6] = _grid(rng.uniform(0.2, 0.9) * a[4:6], 1 / 16) + 1 / 16
                B[i, 4:6] = np.minimum(B[i, 4:6], a[4:6])
            else:   # any heading, small enough to stay inside: diagonal <= the shorter side
                d = min(l, w) * rng.uniform(0.3, 1.0)
                phi = rng.uniform(0.2, 1.3)
                B[i, 3] = rng.uniform(-math.pi, math.pi)
                B[i, 4:6] = d * math.cos(phi), d * math.sin(phi)
        elif family == "sliver":
            B[i, 5] = 1e-9
            if v % 3 == 0:      # through the centre at any angle
                B[i, 3] = a[3] + rng.uniform(-math.pi, math.pi)
            elif v % 3 == 1:    # two identical slivers
                A[i, 5] = 1e-9
            else:               # lying on the edge line: half of its width inside
                B[i] = _shifted(B[i], 0, w / 2)
        elif family == "zero_length":
            B[i, 4] = 0.0
            if v % 4 == 0:      # inside, any heading
                B[i, 3] = a[3] + rng.uniform(-math.pi, math.pi)
                B[i, 5] = min(l, w) / 4
            elif v % 4 == 1:    # lying on the end edge
                B[i] = _shifted(B[i], l / 2, 0)
            elif v % 4 == 2:    # both of zero length (zero area twice: GIoU is 0 / 0 there)
                A[i, 4] = 0.0
            else:               # crossing the end edge at a right angle
                B[i] = _shifted(B[i], l / 2, 0)
                B[i, 3] = a[3] + math.pi / 2
        elif family == "axis_ties":
            A[i, 3] = B[i, 3] = 0.0
            dy, dx = _grid(rng.uniform(-1.2, 1.2) * w, 1 / 64), _grid(rng.uniform(-1.2, 1.2) * l, 1 / 64)
            if v % 4 == 0:      # equal x of all corners, apart in y
                B[i, 1] += dy
            elif v % 4 == 1:    # equal y
                B[i, 0] += dx
            elif v % 4 == 2:    # one shared x only (the left edge), shorter box
                B[i, 4] = _grid(l * rng.uniform(0.3, 0.9), 1 / 16) + 1 / 16
                B[i, 0] = a[0] - l / 2 + B[i, 4] / 2
                B[i, 1] += dy
            else:               # the same footprint described a quarter turn on, apart in y
                B[i, 3] = math.pi / 2
                B[i, 4:6] = w, l
                B[i, 1] += dy
        elif family == "random":
            B[i, 0:2] = _grid(rng.uniform(-3, 3, 2), 1 / 64)
            B[i, 3] = rng.uniform(-math.pi, math.pi)
            A[i, 3] = rng.uniform(-math.pi, math.pi)
            B[i, 4:6] = _grid(rng.uniform(0.5, 5, 2), 1 / 16)
        else:
            raise ValueError(family)
        # heights differ too (never in the identical family); the height overlap stays at least a quarter of a metre
        B[i, 2] = A[i, 2] + _grid(rng.uniform(-0.25, 0.25), 1 / 64)
        B[i, 6] = _grid(rng.uniform(0.5, 2), 1 / 16)
    return A, B


def all_pose_pairs(seed=0):
    """Every family stacked: (A, B, family index per pair)."""
    As, Bs, fam = [], [], []
    for k, f in enumerate(FAMILIES):
        a, b = pose_pairs(f, seed=seed)
        As.append(a)
        Bs.append(b)
        fam += [k] * len(a)
    return np.vstack(As), np.vstack(Bs), np.array(fam)


def at_offset(rows, offset):
    out = np.array(rows, np.float64, copy=True)
    out[:, 0] += offset[0]
    out[:, 1] += offset[1]
    return out


def to_bev(rows, dtype=np.float32):
    """[x, y, z, heading, length, width, height] -> [x, y, z, dx, dy, dz, heading] rows as nms.hip takes them."""
    return np.ascontiguousarray(np.asarray(rows)[:, [0, 1, 2, 4, 5, 6, 3]].astype(dtype))
