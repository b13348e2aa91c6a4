"""numpy restatement of the multi-sweep cloud assembly (shasta_amd/sweeps.py, csrc/sweeps.hip), in this project's words, and the float64
evaluation the rotated cases are measured against.  No reference code: tests/golden/sweeps_golden.npz holds what the reference gave.

Roundings, each established by running the reference's functions on fp32 points with numpy 2.2 (tests/golden/make_sweeps_golden.py
asserts them: this restatement reproduces the reference's output bit for bit there):
  * close filter : `np.abs(x) < 1.0` on fp32 against a Python float compares exactly (fp32 -> float64 is exact): strict, NaN stays.
  * transform    : `M.dot(vstack(xyz, ones))` is a float64 product of the fp32 coordinates, assigned into the fp32 array: one rounding
                   to fp32.  The summation order is the BLAS's; here ((m0 x + m1 y) + m2 z) + m3, each operation rounded, as the kernel.
  * time column  : `time_lag * np.ones(..)` is float64, `.astype(float32)`: (float)time_lag.
  * flips        : `points[:, 1] = -points[:, 1]`: a sign-bit flip (of a NaN too).
  * rotation     : `points[:, :3] @ rot_mat_T` with the fp32 matrix [[c, -s, 0], [s, c, 0], [0, 0, 1]], c = fp32(cos), s = fp32(sin): an
                   fp32 matrix product through the BLAS, bits not fixed.  Here x' = fl(fl(x c) + fl(y s)), y' = fl(fl(x (-s)) + fl(y c)),
                   z' = z: the kernel's order.  For finite non-zero coordinates and c = 1, s = 0 every order gives x, y, z back.
  * scale        : `points[:, :3] *= noise_scale` with a Python float: numpy treats it as a weak scalar, the multiply is fp32 by
                   fp32(noise_scale).
  * translate    : `points[:, :3] += noise_translate` with a float64 (1, 3) array: a float64 add, rounded to fp32 on assignment."""
import numpy as np

U = 2.0 ** -24  # unit roundoff of fp32


def segment(rows, cloud, transform=None, drop=False, time_lag=0.0):
    """One segment in the form `shasta_amd.sweeps.segment_table` takes."""
    return (int(rows), int(cloud), None if transform is None else np.asarray(transform, np.float64), bool(drop), float(time_lag))


def assemble(raw, segments, n_clouds, keep=4, radius=1.0, augment=None):
    """raw: (total_rows, raw_ndim) fp32, segments as `segment` builds them, augment: None or per cloud a dict with flip_x, flip_y, c, s,
    scale, translate (shasta_amd.sweeps.augment_entry) or None.  -> (out (kept, keep + 1) fp32, prefix (n_clouds + 1,) int32)."""
    raw = np.ascontiguousarray(raw, np.float32)
    parts, counts, at = [], np.zeros(n_clouds, np.int64), 0
    for rows, cloud, transform, drop, lag in segments:
        p = raw[at:at + rows].copy()
        at += rows
        if drop:
            close = (np.abs(p[:, 0].astype(np.float64)) < radius) & (np.abs(p[:, 1].astype(np.float64)) < radius)
            p = p[~close]
        o = np.empty((len(p), keep + 1), np.float32)
        o.view(np.uint32)[:, :keep] = p.view(np.uint32)[:, :keep]
        if transform is not None:
            m = np.asarray(transform, np.float64)
            x, y, z = (p[:, j].astype(np.float64) for j in range(3))
            with np.errstate(all="ignore"):
                for i in range(min(3, keep)):
                    o[:, i] = (((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3]).astype(np.float32)
        o[:, keep] = np.float32(lag)
        a = augment[cloud] if augment is not None else None
        if a is not None or augment is not None:
            o = apply_augment(o, a or dict(flip_x=False, flip_y=False, c=1.0, s=0.0, scale=1.0, translate=None))
        parts.append(o)
        counts[cloud] += len(o)
    out = np.concatenate(parts, axis=0) if parts else np.zeros((0, keep + 1), np.float32)
    return out, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def apply_augment(points, a):
    """The four steps on the first three columns of fp32 `points`, in the kernel's arithmetic.  Returns a new array."""
    o = np.array(points, np.float32, copy=True)
    bits = o.view(np.uint32)
    if a["flip_x"]:
        bits[:, 1] ^= np.uint32(0x80000000)
    if a["flip_y"]:
        bits[:, 0] ^= np.uint32(0x80000000)
    c, s = np.float32(a["c"]), np.float32(a["s"])
    with np.errstate(all="ignore"):
        x, y = o[:, 0].copy(), o[:, 1].copy()
        o[:, 0] = x * c + y * s
        o[:, 1] = x * (-s) + y * c
        scale = np.float64(a["scale"])
        for j in range(3):
            v = (o[:, j].astype(np.float64) * scale).astype(np.float32)
            if a["translate"] is not None:
                v = (v.astype(np.float64) + np.float64(a["translate"][j])).astype(np.float32)
            o[:, j] = v
    return o


def augment_f64(points, a):
    """Float64 evaluation of the chain from the assembled fp32 cloud and the fp32-rounded c, s, scale: what the rotated cases are
    measured against, and the bar per coordinate: 4u (|x c| + |y s|) |scale| + 3u |result| (a three-term fp32 dot product followed by two
    roundings, a margin of one unit on each term).  -> (xyz (N, 3) float64, bar (N, 3) float64; the bar of z is 0: z is bit-equal
    through the rotation and is compared after the float64 scale and translation rounded as the chain rounds them)."""
    p = np.asarray(points, np.float32).astype(np.float64)
    x = -p[:, 0] if a["flip_y"] else p[:, 0]
    y = -p[:, 1] if a["flip_x"] else p[:, 1]
    c, s, scale = float(np.float32(a["c"])), float(np.float32(a["s"])), float(a["scale"])
    t = a["translate"] if a["translate"] is not None else [0.0, 0.0, 0.0]
    rx, ry = x * c + y * s, x * (-s) + y * c
    res = np.stack([rx * scale + t[0], ry * scale + t[1], p[:, 2] * scale + t[2]], axis=1)
    mag = np.stack([np.abs(x * c) + np.abs(y * s), np.abs(x * s) + np.abs(y * c)], axis=1) * abs(scale)
    bar = np.zeros_like(res)
    bar[:, :2] = 4 * U * mag + 3 * U * np.abs(res[:, :2])
    return res, bar


def z_through_chain(points, a):
    """z of the augmented cloud, which no BLAS touches: fp32 multiply by the scale, float64 add of the translation rounded to fp32."""
    z = (np.asarray(points, np.float32)[:, 2].astype(np.float64) * np.float64(a["scale"])).astype(np.float32)
    if a["translate"] is not None:
        z = (z.astype(np.float64) + np.float64(a["translate"][2])).astype(np.float32)
    return z


def write_bin(path, rows):
    np.ascontiguousarray(rows, np.float32).tofile(str(path))


def frame_info(tmp, name, key_rows, sweep_rows, transforms, time_lags):
    """Writes the key frame and its sweeps as (n, 5) float32 .bin files under `tmp` and returns the frame's info dict."""
    key = "%s/%s_key.bin" % (tmp, name)
    write_bin(key, key_rows)
    sweeps = []
    for i, rows in enumerate(sweep_rows):
        p = "%s/%s_sweep%d.bin" % (tmp, name, i)
        write_bin(p, rows)
        sweeps.append(dict(lidar_path=p, transform_matrix=None if transforms[i] is None else np.asarray(transforms[i], np.float64),
                           time_lag=float(time_lags[i])))
    return dict(lidar_path=key, sweeps=sweeps)


def uint(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
