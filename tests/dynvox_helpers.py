"""Dynamic voxelisation restated on the CPU in numpy, in this project's own words: what csrc/dynvox.hip must equal bit for bit.

Keep a point iff lo <= p <= hi on x, y, z (float32 compares); coordinate = trunc((p - lo) / vs) in float32 with a true division;
voxels = the unique (z, y, x) coordinates of a cloud in lexicographic order; a voxel's row = the float32 sum of its kept points
added one by one in ascending point index (np.add.at is unbuffered and in order), divided in float32 by the count."""
import numpy as np

SHIPPED_RANGE = [-54.0, -54.0, -5.0, 54.0, 54.0, 3.0]
SHIPPED_VOXEL = [0.075, 0.075, 0.2]


def grid_shape(pc_range, voxel_size):
    """(gx, gy, gz) int32: round-half-even of the float32 quotient, as the reader computes its `shape`."""
    r, v = np.asarray(pc_range, np.float32), np.asarray(voxel_size, np.float32)
    return np.round((r[3:] - r[:3]) / v).astype(np.int32)


def voxelize_cloud(points, pc_range, voxel_size):
    """points (P, ndim) float32 -> (voxels (V, ndim) float32, coors (V, 3) int64 rows (z, y, x), counts (V,) int32)."""
    pts = np.ascontiguousarray(points, np.float32)
    r, v = np.asarray(pc_range, np.float32), np.asarray(voxel_size, np.float32)
    with np.errstate(invalid="ignore"):
        keep = np.ones(len(pts), bool)
        for j in range(3):
            keep &= (pts[:, j] >= r[j]) & (pts[:, j] <= r[3 + j])
    kept = pts[keep]
    ndim = pts.shape[1]
    if len(kept) == 0:
        return np.zeros((0, ndim), np.float32), np.zeros((0, 3), np.int64), np.zeros(0, np.int32)
    q = (kept[:, [2, 1, 0]] - r[[2, 1, 0]]) / v[[2, 1, 0]]
    assert q.dtype == np.float32
    coords = q.astype(np.int64)  # truncation; the kept values are >= 0
    uniq, inverse = np.unique(coords, axis=0, return_inverse=True)
    inverse = inverse.reshape(-1)
    sums = np.zeros((len(uniq), ndim), np.float32)
    np.add.at(sums, inverse, kept)
    counts = np.bincount(inverse, minlength=len(uniq))
    voxels = sums / counts.astype(np.float32)[:, None]
    assert voxels.dtype == np.float32
    return voxels, uniq, counts.astype(np.int32)


def voxelize_batch(clouds, pc_range, voxel_size):
    """list of (P_i, ndim) -> (voxels (V, ndim) float32, coors (V, 4) int64 rows (cloud, z, y, x), counts (V,) int32,
    prefix (n + 1,) int32: voxels before each cloud, last = V)."""
    vs, cs, ns, prefix = [], [], [], [0]
    for b, c in enumerate(clouds):
        v, co, n = voxelize_cloud(c, pc_range, voxel_size)
        vs.append(v)
        cs.append(np.concatenate([np.full((len(co), 1), b, np.int64), co], 1))
        ns.append(n)
        prefix.append(prefix[-1] + len(v))
    return np.concatenate(vs), np.concatenate(cs), np.concatenate(ns), np.asarray(prefix, np.int32)


def radial_cloud(P, seed, ndim=5):
    """The synthetic cloud of tools/time_voxelize.py: radius ~ |N(0, 18 m)| (dense near the sensor, a few points beyond the range),
    uniform azimuth, z ~ N(-1.5, 0.6), an intensity channel."""
    rng = np.random.default_rng(seed)
    pts = np.zeros((P, ndim), np.float32)
    r = np.abs(rng.normal(0, 18, size=P)).astype(np.float32)
    th = rng.uniform(0, 2 * np.pi, size=P).astype(np.float32)
    pts[:, 0], pts[:, 1] = r * np.cos(th), r * np.sin(th)
    pts[:, 2] = rng.normal(-1.5, 0.6, size=P)
    pts[:, 3] = rng.uniform(0, 255, size=P)
    return pts
