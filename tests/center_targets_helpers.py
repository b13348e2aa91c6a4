"""numpy / float64 restatement of the reference's box augmentation, range filter and AssignLabel (nuScenes branch), and the fixed input
sets of tests/test_center_targets.py and tests/test_center_loss.py.

The reference's own functions pull in numba and cannot be imported; this follows them step by step in numpy >= 2 arithmetic: np.float32
scalars and arrays next to Python floats stay fp32, float64 arrays promote.  `gaussian_radius` therefore runs in fp32 throughout (its
arguments are fp32 scalars), the gaussian itself in float64 (np.ogrid of Python floats), and `np.maximum(..., out=fp32 view)` rounds it.
tests/test_center_targets.py::test_restatement_pins pins a few hand-computed values."""
import math

import numpy as np

F = np.float32
TASKS = [1, 2, 2]  # classes per task; the 1-based classes over all tasks are 1 | 2, 3 | 4, 5
MAX_OBJS = 8
GEOM_A = dict(pc_range=[-7.2, -6.0, -5.0, 7.2, 6.0, 3.0], voxel_size=[0.075, 0.075, 0.2], out_size_factor=8, gaussian_overlap=0.1,
              max_objs=MAX_OBJS, min_radius=2)   # 24 x 20 map
GEOM_B = dict(pc_range=[-3.0, 1.5, -5.0, 6.6, 9.5, 3.0], voxel_size=[0.1, 0.1, 0.2], out_size_factor=4, gaussian_overlap=0.1,
              max_objs=MAX_OBJS, min_radius=2)   # 24 x 20 map, shifted
MAP_W, MAP_H = 24, 20


# ---- restatement ------------------------------------------------------------------------------------------------------------------
def augment_ref(boxes, entry):
    """sampler/preprocess.py: random_flip_both, global_rotation, global_scaling_v2, global_translate_ on (n, 9) fp32 boxes for one drawn
    `sweeps.augment_entry`; the rotation in the operation order the kernels use for points (x c + y s, x (-s) + y c, fp32, no fma)."""
    b = np.array(boxes, dtype=F, copy=True)
    if entry is None:
        return b
    if entry["flip_x"]:
        b[:, 1] = -b[:, 1]
        b[:, -1] = -b[:, -1] + np.pi
        b[:, 7] = -b[:, 7]
    if entry["flip_y"]:
        b[:, 0] = -b[:, 0]
        b[:, -1] = -b[:, -1] + 2 * np.pi
        b[:, 6] = -b[:, 6]
    c, s = F(entry["c"]), F(entry["s"])
    for i, j in ((0, 1), (6, 7)):
        x, y = b[:, i].copy(), b[:, j].copy()
        b[:, i] = x * c + y * s
        b[:, j] = x * (-s) + y * c
    b[:, -1] += float(entry["angle"])
    b[:, :-1] *= float(entry["scale"])
    if entry["translate"] is not None:
        b[:, :3] += np.asarray(entry["translate"], dtype=np.float64).reshape(1, 3)
    return b


def rotate64(boxes, entry):
    """float64 value of the rotation step alone (flips before it are exact): x, y, vx, vy and the bound's |a||c| + |b||s| per column."""
    c, s = float(F(entry["c"])), float(F(entry["s"]))
    b = np.asarray(boxes, dtype=np.float64)
    out, mag = {}, {}
    for i, j in ((0, 1), (6, 7)):
        out[i], out[j] = b[:, i] * c + b[:, j] * s, b[:, i] * (-s) + b[:, j] * c
        mag[i] = mag[j] = None
        mag[i], mag[j] = np.abs(b[:, i] * c) + np.abs(b[:, j] * s), np.abs(b[:, i] * s) + np.abs(b[:, j] * c)
    return out, mag


def corners_ref(boxes):
    """center_to_corner_box2d(xy, wl, rot) in fp32 -> (n, 4, 2)."""
    b = np.asarray(boxes, dtype=F)
    norm = np.array([[-0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]], dtype=F)
    rel = b[:, None, 3:5] * norm[None]
    sn, cs = np.sin(b[:, 8]), np.cos(b[:, 8])
    out = np.empty_like(rel)
    out[:, :, 0] = rel[:, :, 0] * cs[:, None] + rel[:, :, 1] * sn[:, None]
    out[:, :, 1] = rel[:, :, 0] * (-sn)[:, None] + rel[:, :, 1] * cs[:, None]
    return out + b[:, None, 0:2]


def rectangle_ref(bv_range):
    r = np.asarray(bv_range, dtype=F)
    lo, dims = r[:2], r[2:] - r[:2]
    norm = np.array([[0, 0], [0, 1], [1, 1], [1, 0]], dtype=F)
    return dims[None] * norm + lo[None]  # (4, 2), clockwise from the minimum


def filter_ref(boxes, bv_range):
    """filter_gt_box_outside_range: any corner inside; inside iff every directed edge's cross product is < 0 (fp32 products, a float64
    accumulator, as the jitted loop types them)."""
    poly = rectangle_ref(bv_range)
    vec = poly - poly[[3, 0, 1, 2]]
    cor = corners_ref(boxes)
    keep = np.zeros(len(cor), dtype=bool)
    for i in range(len(cor)):
        for p in cor[i]:
            ok = True
            for k in range(4):
                cross = float(vec[k, 1] * (poly[k, 0] - p[0]))
                cross -= float(vec[k, 0] * (poly[k, 1] - p[1]))
                if cross >= 0:
                    ok = False
                    break
            keep[i] = keep[i] or ok
    return keep


def limit_period_ref(val, offset=0.5, period=np.pi * 2):
    return val - np.floor(val / period + offset) * period


def gaussian_radius_ref(det_size, min_overlap):
    """The CenterNet radius (three quadratics, the smallest root) in the arithmetic of its arguments: fp32 scalars stay fp32."""
    height, width = det_size
    b1 = height + width
    c1 = width * height * (1 - min_overlap) / (1 + min_overlap)
    r1 = (b1 + np.sqrt(b1 ** 2 - 4 * 1 * c1)) / 2
    b2 = 2 * (height + width)
    c2 = (1 - min_overlap) * width * height
    r2 = (b2 + np.sqrt(b2 ** 2 - 4 * 4 * c2)) / 2
    a3 = 4 * min_overlap
    b3 = -2 * min_overlap * (height + width)
    c3 = (min_overlap - 1) * width * height
    r3 = (b3 + np.sqrt(b3 ** 2 - 4 * a3 * c3)) / 2
    return min(r1, r2, r3)


def gaussian_ref(radius):
    d = 2 * radius + 1
    sigma = d / 6
    m = (d - 1.0) / 2.0
    y, x = np.ogrid[-m:m + 1, -m:m + 1]
    h = np.exp(-(x * x + y * y) / (2 * sigma * sigma))
    h[h < np.finfo(h.dtype).eps * h.max()] = 0
    return h


def draw_ref(hm, center, radius):
    g = gaussian_ref(radius)
    x, y = int(center[0]), int(center[1])
    H, W = hm.shape
    left, right, top, bottom = min(x, radius), min(W - x, radius + 1), min(y, radius), min(H - y, radius + 1)
    dst = hm[y - top:y + bottom, x - left:x + right]
    src = g[radius - top:radius + bottom, radius - left:radius + right]
    if min(src.shape) > 0 and min(dst.shape) > 0:
        np.maximum(dst, src, out=dst)


def geometry(cfg):
    pc, vs = np.array(cfg["pc_range"], dtype=F), np.array(cfg["voxel_size"], dtype=F)
    grid = np.round((pc[3:] - pc[:3]) / vs).astype(np.int64)
    return pc, vs, grid[:2] // cfg["out_size_factor"]


def assign_ref(boxes, classes, cfg, tasks=TASKS, with_gtbc=True):
    """AssignLabel.__call__ for one sample: boxes (n, 9) fp32, classes (n,) 1-based over all tasks -> dict of per-task lists."""
    pc, vs, fms = geometry(cfg)
    osf, max_objs = cfg["out_size_factor"], cfg["max_objs"]
    boxes, classes = np.asarray(boxes, dtype=F).reshape(-1, 9), np.asarray(classes, dtype=np.int32).reshape(-1)
    out = dict(hm=[], anno_box=[], ind=[], mask=[], cat=[], radius=[], ct=[])
    flag, all_boxes, all_cls = 0, [], []
    for nc in tasks:
        sel = np.concatenate([np.where(classes == flag + c + 1)[0] for c in range(nc)])
        tb, tc = boxes[sel].copy(), classes[sel] - flag
        tb[:, -1] = limit_period_ref(tb[:, -1], offset=0.5, period=np.pi * 2)
        hm = np.zeros((nc, fms[1], fms[0]), dtype=F)
        anno, ind = np.zeros((max_objs, 10), dtype=F), np.zeros(max_objs, dtype=np.int64)
        mask, cat = np.zeros(max_objs, dtype=np.uint8), np.zeros(max_objs, dtype=np.int64)
        for k in range(min(len(tb), max_objs)):
            cls_id = tc[k] - 1
            w, l = tb[k][3] / vs[0] / osf, tb[k][4] / vs[1] / osf
            if w > 0 and l > 0:
                rf = gaussian_radius_ref((l, w), min_overlap=cfg["gaussian_overlap"])
                radius = max(cfg["min_radius"], int(rf))
                ct = np.array([(tb[k][0] - pc[0]) / vs[0] / osf, (tb[k][1] - pc[1]) / vs[1] / osf], dtype=F)
                out["radius"].append(float(rf))
                out["ct"].append(ct.astype(np.float64))
                ci = ct.astype(np.int32)
                if not (0 <= ci[0] < fms[0] and 0 <= ci[1] < fms[1]):
                    continue
                draw_ref(hm[cls_id], ct, radius)
                cat[k], ind[k], mask[k] = cls_id, ci[1] * fms[0] + ci[0], 1
                anno[k] = np.concatenate((ct - (ci[0], ci[1]), tb[k][2], np.log(tb[k][3:6]), np.array(tb[k][6]), np.array(tb[k][7]),
                                          np.sin(tb[k][8]), np.cos(tb[k][8])), axis=None)
        for key, v in (("hm", hm), ("anno_box", anno), ("ind", ind), ("mask", mask), ("cat", cat)):
            out[key].append(v)
        all_boxes.append(tb)
        all_cls.append(tc + flag)
        flag += nc
    if with_gtbc:
        bc = np.concatenate((np.concatenate(all_boxes), np.concatenate(all_cls).reshape(-1, 1).astype(F)), axis=1)
        assert len(bc) <= max_objs
        g = np.zeros((max_objs, 10), dtype=F)
        g[:len(bc)] = bc[:, [0, 1, 2, 3, 4, 5, 8, 6, 7, 9]]
        out["gt_boxes_and_cls"] = g
    out["limited"] = all_boxes
    return out


# ---- margins ----------------------------------------------------------------------------------------------------------------------
def assert_margins(boxes, classes, cfg, margin=1e-3):
    """float64: every ct component and every radius keeps `margin` to the next integer.  No input is dropped: a violation fails."""
    pc, vs = np.array(cfg["pc_range"], dtype=np.float64), np.array(cfg["voxel_size"], dtype=np.float64)
    b = np.asarray(boxes, dtype=np.float64)
    osf = cfg["out_size_factor"]
    for row, c in zip(b, classes):
        if not 1 <= c <= sum(TASKS):
            continue
        w, l = row[3] / vs[0] / osf, row[4] / vs[1] / osf
        if not (w > 0 and l > 0):
            continue
        r = float(gaussian_radius_ref((l, w), cfg["gaussian_overlap"]))
        assert abs(r - round(r)) >= margin, ("radius", row, r)
        for v in ((row[0] - pc[0]) / vs[0] / osf, (row[1] - pc[1]) / vs[1] / osf):
            assert abs(v - round(v)) >= margin, ("centre", row, v)


def assert_corner_margins(boxes, bv_range, margin=1e-3):
    """float64: every BEV corner keeps `margin` metres to the rectangle's outline."""
    b = np.asarray(boxes, dtype=np.float64)
    x0, y0, x1, y1 = [float(v) for v in bv_range]
    for row in b:
        sn, cs = math.sin(row[8]), math.cos(row[8])
        for hx, hy in ((-0.5, -0.5), (-0.5, 0.5), (0.5, 0.5), (0.5, -0.5)):
            a, c = row[3] * hx, row[4] * hy
            px, py = a * cs + c * sn + row[0], -a * sn + c * cs + row[1]
            dx, dy = min(abs(px - x0), abs(px - x1)), min(abs(py - y0), abs(py - y1))
            inside_x, inside_y = x0 - margin < px < x1 + margin, y0 - margin < py < y1 + margin
            near = (dx < margin and inside_y) or (dy < margin and inside_x)
            assert not near, ("corner", row, px, py)


# ---- input sets -------------------------------------------------------------------------------------------------------------------
def _box(x, y, w, l, rot, z=-1.0, h=1.5, vx=0.3, vy=-0.2):
    return [x, y, z, w, l, h, vx, vy, rot]


def cell(cfg, cx, cy):
    """metres of the map position (cx, cy) in cells (float64; the tests' positions sit well inside their cells)."""
    s = cfg["voxel_size"][0] * cfg["out_size_factor"]
    return cfg["pc_range"][0] + cx * s, cfg["pc_range"][1] + cy * s


def special_sample(cfg):
    """13 boxes, classes interleaved, task 0 (class 1) EMPTY.  Covers: a hole (centre outside the map), w = 0, two boxes in one pixel and
    class, overlapping gaussians of the same and of different classes, clipping at the four borders and at a corner, a radius below
    min_radius, a radius >= 9, headings outside [-pi, pi]."""
    P = lambda cx, cy: cell(cfg, cx, cy)  # noqa: E731
    rows = [
        (3, _box(*P(10.3, 9.6), 1.9, 4.4, 0.4)),          # a car-sized box mid map
        (5, _box(*P(0.4, 7.3), 2.0, 4.6, 4.0)),           # left border, heading > pi
        (2, _box(*P(10.6, 9.3), 2.1, 4.9, -5.5)),         # same pixel as the next class-2 box; heading < -pi
        (4, _box(*P(23.6, 12.7), 2.2, 5.1, 7.0)),         # right border, heading > 2 pi
        (3, _box(*P(11.7, 10.4), 0.55, 0.62, 0.1)),       # radius below min_radius, overlaps the first box (same class)
        (2, _box(*P(10.2, 9.7), 1.8, 4.1, 1.2)),          # the pixel (10, 9) again, class 2
        (5, _box(*P(30.5, 5.5), 2.0, 4.5, 0.0)),          # centre outside the map: a hole in task 2
        (4, _box(*P(12.4, 0.3), 2.4, 6.3, -0.7)),         # top border
        (3, _box(*P(5.5, 5.5), 0.0, 4.0, 0.3)),           # w = 0
        (5, _box(*P(13.6, 19.7), 2.6, 6.9, 2.9)),         # bottom border
        (2, _box(*P(23.3, 19.4), 2.3, 5.7, -2.2)),        # bottom-right corner
        (4, _box(*P(14.5, 11.5), 15.2, 13.1, 0.9)),       # radius >= 9; overlaps boxes of other classes and tasks
        (2, _box(*P(12.2, 10.8), 2.9, 7.4, -1.0)),        # overlaps the class-2 boxes (same class) and class 3 (different class)
    ]
    return np.array([r[1] for r in rows], dtype=F), np.array([r[0] for r in rows], dtype=np.int32)


def truncation_sample(cfg):
    """14 boxes: 11 in task 1 (classes 2 and 3 interleaved: the partition puts the class-2 boxes first, slots 8 .. 10 are cut), 2 in task
    0, 1 in task 2, and one box of a class outside the tasks."""
    rng = np.random.RandomState(20260)
    cls = [3, 2, 1, 3, 3, 2, 5, 2, 3, 2, 1, 3, 2, 3, 7]
    rows = []
    for i, c in enumerate(cls):
        cx, cy = 2.0 + (i * 7 % 20) + 0.2 + 0.6 * rng.rand(), 2.0 + (i * 5 % 16) + 0.2 + 0.6 * rng.rand()
        rows.append(_box(*cell(cfg, cx, cy), 1.6 + 0.1 * i, 3.9 + 0.13 * i, rng.uniform(-3, 3), vx=rng.randn(), vy=rng.randn()))
    return np.array(rows, dtype=F), np.array(cls, dtype=np.int32)


def exact_sample(cfg):
    """Deliberately exact inputs for the entries WITHOUT rotation: a centre exactly on a cell boundary in both axes (the map's middle),
    one exactly on the map's lower corner, and one a cell edge short of the upper border."""
    pc = cfg["pc_range"]
    rows = [(2, _box(*cell(cfg, 12.0, 10.0), 1.9, 4.4, 0.0)), (4, _box(pc[0], pc[1], 2.0, 4.0, 0.5)), (5, _box(pc[3], pc[4], 2.0, 4.0, 0.5)),
            (1, _box(*cell(cfg, 3.0, 17.0), 0.7, 0.8, 1.0))]
    return np.array([r[1] for r in rows], dtype=F), np.array([r[0] for r in rows], dtype=np.int32)


def filter_set(bv_range, seed=7, n=48):
    """Seeded boxes around the rectangle: inside, outside, straddling, far rotated ones whose corner reaches in."""
    rng = np.random.RandomState(seed)
    x0, y0, x1, y1 = bv_range
    rows = []
    for _ in range(n):
        x, y = rng.uniform(x0 - 4, x1 + 4), rng.uniform(y0 - 4, y1 + 4)
        rows.append(_box(x, y, rng.uniform(0.5, 5), rng.uniform(0.5, 8), rng.uniform(-7, 7)))
    return np.array(rows, dtype=F)


def filter_exact_set(bv_range):
    """rot = 0 (sin 0, cos 1: the corners are exact sums): boxes whose corners lie exactly on the rectangle's edges - outside - and their
    neighbours one fp32 step inside."""
    r = np.asarray(bv_range, dtype=F)
    x1, y1, x0, y0 = r[2], r[3], r[0], r[1]
    rows = [_box(x1 + F(1.0), 0.0, 2.0, 1.0, 0.0),                                  # left corners exactly on x = x1: dropped
            _box(np.nextafter(x1 + F(1.0), F(0)), 0.0, 2.0, 1.0, 0.0),              # one step inside: kept
            _box(0.0, y0 - F(0.5), 1.0, 1.0, 0.0),                                  # upper corners exactly on y = y0: dropped
            _box(0.0, np.nextafter(y0 - F(0.5), F(0)), 1.0, 1.0, 0.0),              # kept
            _box(x0 - F(1.0), y1 + F(1.0), 2.0, 2.0, 0.0),                          # one corner exactly on the rectangle's corner: dropped
            _box(x0, y0, 0.0, 0.0, 0.0),                                            # a point on the corner: dropped
            _box(0.0, 0.0, 0.0, 0.0, 0.0)]                                          # a point inside: kept
    return np.array(rows, dtype=F)


ENTRIES_NO_ROTATION = [
    dict(flip_x=True, flip_y=False, angle=0.0, scale=1.03, translate=None),
    dict(flip_x=False, flip_y=True, angle=0.0, scale=0.96, translate=[0.21, -0.13, 0.05]),
    dict(flip_x=True, flip_y=True, angle=0.0, scale=1.0, translate=[-0.4, 0.3, -0.02]),
]
ENTRIES_ROTATION = [
    dict(flip_x=False, flip_y=False, angle=0.31, scale=1.0, translate=None),
    dict(flip_x=True, flip_y=False, angle=-0.52, scale=1.04, translate=[0.1, 0.2, -0.03]),
    dict(flip_x=False, flip_y=True, angle=0.7853, scale=0.96, translate=None),
]


def ulps(got, want64):
    """|got - want| in units of the fp32 ulp of the float64 value."""
    want64 = np.asarray(want64, dtype=np.float64)
    ulp = np.spacing(np.abs(want64).astype(F)).astype(np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - want64) / ulp
