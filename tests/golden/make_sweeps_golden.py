"""Generates tests/golden/sweeps_golden.npz: small synthetic sweep files and what the REFERENCE's `LoadPointCloudFromFile`
(det3d/datasets/pipelines/loading.py:111-148), `Preprocess` (preprocess.py:28-158) and the four augmentation functions
(det3d/core/sampler/preprocess.py: random_flip_both, global_rotation, global_scaling_v2, global_translate_) make of them under fixed
seeds, for shasta_amd/sweeps.py.  Build container only (imports the reference in place, nothing copied):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sweeps_golden.py

Absent third-party packages are stubbed by make_frames_golden.py's finder (pyquaternion among them).

Transforms and points are chosen so that the float64 sum m0 x + m1 y + m2 z + m3 rounds to the same fp32 in EVERY summation order,
with and without fused multiply-add: the value in extended precision (np.longdouble, 64-bit significand) must be farther from both
neighbouring fp32 rounding ties than 8 float64 units of the sum of the terms' magnitudes - an evaluation in any order errs by at most
4.  A seed with a value closer than that is skipped.  This makes bit equality a fair demand of any fixed device order.

The maker also asserts, with the numpy of this machine: the restatement tests/sweeps_helpers.py equals the reference bit for bit
(assembly, flips, scale, translate, rotation by 0); the reference's rotated output lies inside the bar of sweeps_helpers.augment_f64."""
import importlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
import make_frames_golden as F  # noqa: E402
import sweeps_helpers as H  # noqa: E402

NSWEEPS = 4
FRAME_ROWS = [[300, 517, 256, 1], [0, 130, 700, 257]]  # key frame first; rows per file
AUG_CASES = [  # name, seed, global_rot_noise, global_scale_noise, global_translate_std
    ("a0", 3, [0.0, 0.0], [0.95, 1.05], 0.5),
    ("a1", 4, [0.0, 0.0], [0.9, 1.1], 0),
    ("a2", 5, [0.0, 0.0], [0.95, 1.05], [0.2, 0.0, 0.0]),
    ("a3", 8, [0.0, 0.0], [0.5, 2.0], 0.1),
    ("r0", 11, np.pi / 4, [0.95, 1.05], 0.5),
    ("r1", 12, [-3.0, 3.0], [0.9, 1.1], 0),
]
PIPE = dict(seed=21, global_rot_noise=[0.0, 0.0], global_scale_noise=[0.9, 1.1], global_translate_std=0.5)


class Cfg(dict):
    __getattr__ = dict.__getitem__


def rigid(rng):
    """A 4 x 4 float64 sensor-to-key-frame transform: yaw, a small tilt, a translation of metres."""
    from scipy.spatial.transform import Rotation
    m = np.eye(4)
    m[:3, :3] = Rotation.from_euler("zyx", [rng.uniform(-3.1, 3.1), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05)]).as_matrix()
    m[:3, 3] = rng.uniform(-3, 3, 3)
    return m


def rows(rng, n):
    """(n, 5) fp32: half of the points near the sensor (many inside the 1 m square), half far; intensity; ring index."""
    near = rng.uniform(-3, 3, (n, 2))
    far = rng.uniform(-50, 50, (n, 2))
    xy = np.where(rng.uniform(size=(n, 1)) < 0.5, near, far)
    return np.concatenate([xy, rng.uniform(-3, 2, (n, 1)), rng.integers(0, 256, (n, 1)), rng.integers(0, 32, (n, 1))], axis=1).astype(np.float32)


def order_free(m, p):
    """True when ((m0 x + m1 y) + m2 z) + m3 rounds to the same fp32 in every order, fused or not (see the module docstring)."""
    L = np.longdouble
    x, y, z = (p[:, j].astype(L) for j in range(3))
    for i in range(3):
        t = [L(m[i, 0]) * x, L(m[i, 1]) * y, L(m[i, 2]) * z, np.full(len(p), L(m[i, 3]))]
        e = t[0] + t[1] + t[2] + t[3]
        margin = 8 * 2.0 ** -53 * (abs(t[0]) + abs(t[1]) + abs(t[2]) + abs(t[3]))
        f = e.astype(np.float32)
        for side in (np.float32(np.inf), np.float32(-np.inf)):
            tie = (f.astype(L) + np.nextafter(f, side).astype(L)) / 2
            if not np.all(abs(e - tie) > margin):
                return False
    return True


def build_inputs():
    for seed in range(2024, 2100):
        rng = np.random.default_rng(seed)
        frames = [[rows(rng, n) for n in counts] for counts in FRAME_ROWS]
        transforms = [[rigid(rng) for _ in range(NSWEEPS - 1)] for _ in FRAME_ROWS]
        transforms[1][1] = None  # a sweep without a transform between two with one
        lags = [[float(rng.uniform(0.04, 0.5)) for _ in range(NSWEEPS - 1)] for _ in FRAME_ROWS]
        if all(m is None or order_free(m, f[1 + i]) for f, ms in zip(frames, transforms) for i, m in enumerate(ms)):
            return seed, frames, transforms, lags
    raise RuntimeError("no seed without a value near a rounding tie")


def replay_draws(seed, rot, scale, std):
    """The parameters the reference's four functions draw under `seed` (None: from the stream's current state), redrawn with the same
    numpy calls in the same order."""
    if seed is not None:
        np.random.seed(seed)
    fx = bool(np.random.choice([False, True], replace=False, p=[0.5, 0.5]))
    fy = bool(np.random.choice([False, True], replace=False, p=[0.5, 0.5]))
    r = rot if isinstance(rot, list) else [-rot, rot]
    angle = np.random.uniform(r[0], r[1])
    sc = np.random.uniform(scale[0], scale[1])
    sd = std if isinstance(std, (list, tuple)) else [std, std, std]
    t = None
    if not all(e == 0 for e in sd):
        t = [float(np.random.normal(0, sd[0], 1)[0]), float(np.random.normal(0, sd[1], 1)[0]), float(np.random.normal(0, sd[0], 1)[0])]
    return dict(flip_x=fx, flip_y=fy, angle=float(angle), c=float(np.float32(np.cos(angle))), s=float(np.float32(np.sin(angle))),
                scale=float(np.float32(sc)), scale64=float(sc), translate=t)


def main():
    F.import_reference_dataset()
    loading = importlib.import_module("det3d.datasets.pipelines.loading")
    pipe_prep = importlib.import_module("det3d.datasets.pipelines.preprocess")
    prep = importlib.import_module("det3d.core.sampler.preprocess")
    seed, frames, transforms, lags = build_inputs()
    out = dict(input_seed=np.array([seed]), nsweeps=np.array([NSWEEPS]), n_frames=np.array([len(frames)]))
    combined = []
    with tempfile.TemporaryDirectory() as tmp:
        infos = [H.frame_info(tmp, "f%d" % k, f[0], f[1:], transforms[k], lags[k]) for k, f in enumerate(frames)]
        for k, (f, info) in enumerate(zip(frames, infos)):
            for i, r in enumerate(f):
                out["f%d_raw%d" % (k, i)] = r
            out["f%d_has_transform" % k] = np.array([m is not None for m in transforms[k]])
            out["f%d_transforms" % k] = np.stack([np.eye(4) if m is None else m for m in transforms[k]])
            out["f%d_lags" % k] = np.array(lags[k])
            load_seed = 100 + k
            np.random.seed(load_seed)
            order = np.random.choice(NSWEEPS - 1, NSWEEPS - 1, replace=False)
            np.random.seed(load_seed)
            res = dict(lidar=dict(nsweeps=NSWEEPS), virtual=False)
            loading.LoadPointCloudFromFile(dataset="NuScenesDataset")(res, info)
            ref = res["lidar"]["combined"]
            assert ref.dtype == np.float32 and ref.shape[1] == 5
            out["f%d_load_seed" % k], out["f%d_order" % k], out["f%d_combined" % k] = np.array([load_seed]), order, ref
            combined.append(ref)
            segs = [H.segment(len(f[0]), 0)] + [H.segment(len(f[1 + i]), 0, transforms[k][i], True, lags[k][i]) for i in order]
            mine, prefix = H.assemble(np.concatenate([f[0]] + [f[1 + i] for i in order]), segs, 1)
            assert np.array_equal(H.uint(mine), H.uint(ref)) and prefix[1] == len(ref), "restatement != reference (assembly, frame %d)" % k
            print("frame %d: %d rows in, %d out, order %s" % (k, sum(len(r) for r in f), len(ref), order))

        # the four augmentation functions on frame 0's cloud
        names, worst = [], 0.0
        for name, s, rot, scale, std in AUG_CASES:
            a = replay_draws(s, rot, scale, std)
            np.random.seed(s)
            pts, boxes = combined[0].copy(), np.zeros((0, 9), np.float32)
            boxes, pts = prep.random_flip_both(boxes, pts)
            boxes, pts = prep.global_rotation(boxes, pts, rotation=rot)
            boxes, pts = prep.global_scaling_v2(boxes, pts, *scale)
            boxes, pts = prep.global_translate_(boxes, pts, noise_translate_std=std)
            assert pts.dtype == np.float32
            mine = H.apply_augment(combined[0], a)
            if a["angle"] == 0.0:
                assert np.array_equal(H.uint(mine), H.uint(pts)), "restatement != reference (augmentation %s)" % name
            else:
                want, bar = H.augment_f64(combined[0], a)
                for got, who in ((pts, "reference"), (mine, "restatement")):
                    ratio = np.abs(got[:, :2].astype(np.float64) - want[:, :2]) / bar[:, :2]
                    assert ratio.max() <= 1.0, "%s outside the bar (%s): %g" % (who, name, ratio.max())
                    worst = max(worst, ratio.max())
                    assert np.array_equal(H.uint(got[:, 2]), H.uint(H.z_through_chain(combined[0], a))), "z not bit-equal (%s, %s)" % (who, name)
                    assert np.array_equal(H.uint(got[:, 3:]), H.uint(combined[0][:, 3:]))
            names.append(name)
            out["aug_%s_points" % name] = pts
            out["aug_%s_flags" % name] = np.array([a["flip_x"], a["flip_y"], a["translate"] is not None])
            out["aug_%s_params" % name] = np.array([a["angle"], a["scale64"]] + (a["translate"] or [0.0, 0.0, 0.0]))
            out["aug_%s_seed" % name] = np.array([s])
            out["aug_%s_cfg" % name] = np.array([float(v) for v in (rot if isinstance(rot, list) else [-rot, rot])] + [float(v) for v in scale]
                                                + [float(v) for v in (std if isinstance(std, list) else [std, std, std])])
            print("augmentation %s: flips %s %s angle %.4f scale %.4f translate %s" % (name, a["flip_x"], a["flip_y"], a["angle"], a["scale"],
                                                                                     a["translate"]))
        out["aug_names"] = np.array(names)
        print("rotated cases: largest error / bar = %.3f (reference and restatement)" % worst)
        flags = np.stack([out["aug_%s_flags" % n] for n in names])
        assert flags[:, 0].any() and not flags[:, 0].all() and flags[:, 1].any() and not flags[:, 1].all(), "flips not both ways: other seeds"

        # the whole reference pipeline in train mode on frame 1: loader, Preprocess with shuffle, one seed
        cfg = Cfg(shuffle_points=True, mode="train", global_rot_noise=PIPE["global_rot_noise"], global_scale_noise=PIPE["global_scale_noise"],
                  global_translate_std=PIPE["global_translate_std"], class_names=["car"], db_sampler=None)
        np.random.seed(PIPE["seed"])
        res = dict(lidar=dict(nsweeps=NSWEEPS, annotations=dict(boxes=np.array([[1, 2, 0, 4, 2, 1.5, 0.1, 0.2, 0.3]], np.float32), names=["car"])),
                   virtual=False)
        res, _ = loading.LoadPointCloudFromFile(dataset="NuScenesDataset")(res, infos[1])
        res, _ = pipe_prep.Preprocess(cfg=cfg)(res, infos[1])
        out["pipe_points"] = res["lidar"]["points"]
        out["pipe_cfg"] = np.array([PIPE["seed"]] + PIPE["global_rot_noise"] + PIPE["global_scale_noise"] + [PIPE["global_translate_std"]])
        # the same from the restatement and plain numpy draws
        np.random.seed(PIPE["seed"])
        order = np.random.choice(NSWEEPS - 1, NSWEEPS - 1, replace=False)
        f = frames[1]
        segs = [H.segment(len(f[0]), 0)] + [H.segment(len(f[1 + i]), 0, transforms[1][i], True, lags[1][i]) for i in order]
        cloud, _ = H.assemble(np.concatenate([f[0]] + [f[1 + i] for i in order]), segs, 1)
        a = replay_draws(None, PIPE["global_rot_noise"], PIPE["global_scale_noise"], PIPE["global_translate_std"])
        cloud = H.apply_augment(cloud, a)
        index = np.arange(len(cloud))
        np.random.shuffle(index)
        assert np.array_equal(H.uint(cloud[index]), H.uint(out["pipe_points"])), "restatement != reference (pipeline with shuffle)"
        out["pipe_order"], out["pipe_index"] = order, index
        out["pipe_flags"] = np.array([a["flip_x"], a["flip_y"], a["translate"] is not None])
        out["pipe_params"] = np.array([a["angle"], a["scale64"]] + (a["translate"] or [0.0, 0.0, 0.0]))
    path = os.path.join(HERE, "sweeps_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
