"""Seeded synthetic scenes for the ground-truth label construction (shasta_amd/gt_labels.py): objects of three classes that move,
are born and die, detections of 75 % of them with 0.7 m noise and 10 % wrong types, clutter, `vehicle.*`-style ground-truth type
strings against short detection names.  Shared by tests/golden/make_gt_labels_golden.py, tests/test_gt_labels.py and
tools/time_gt_labels.py; numpy only."""
import numpy as np

DET_NAMES = ["car", "truck", "bus"]
GT_NAMES = ["vehicle.car", "vehicle.truck", "vehicle.bus.rigid"]
# the seam scene: (detections, ground-truth boxes) per frame - both sides of a wavefront on either axis, empty sides as current and
# as previous frame
SEAM_COUNTS = [(0, 0), (0, 5), (5, 0), (1, 1), (63, 64), (64, 65), (65, 64), (130, 90), (90, 130)]


def synth_scene(seed, n_frames=12, n_obj=40, quant=True, counts=None, not_emitted=(), skip_frac=0.0, clutter=(0, 25), half=40.0):
    """A scene as the list of frame dicts gt_labels.scene_labels takes.  quant: coordinates on a 0.5 m grid and scores on a 0.1 grid,
    so that equal distances, equal scores and distances equal to a threshold of 2.0 occur.  counts: exact (detections, ground-truth
    boxes) per frame (objects 0 .. G-1 are alive).  not_emitted: frame indices with emit=False; skip_frac: further ones at random."""
    rng = np.random.default_rng(seed)
    if counts is not None:
        n_frames, n_obj = len(counts), max(max(g for _, g in counts), 1)
    pos, vel = rng.uniform(-half, half, (n_obj, 2)), rng.normal(0, 1.0, (n_obj, 2))
    cls = rng.integers(0, 3, n_obj)
    birth = rng.integers(-3, n_frames - 2, n_obj)
    death = birth + rng.integers(2, n_frames + 3, n_obj)
    grid = (lambda p: np.round(p * 2) / 2) if quant else (lambda p: p)
    frames = []
    for t in range(n_frames):
        alive = [i for i in range(n_obj) if birth[i] <= t < death[i]] if counts is None else list(range(counts[t][1]))
        n_det = None if counts is None else counts[t][0]
        gt_xy, gt_types, gt_ids, det = [], [], [], []
        for i in alive:
            p = grid(pos[i] + vel[i] * t)
            gt_xy.append(p)
            gt_types.append(GT_NAMES[cls[i]])
            gt_ids.append("inst%03d" % i)
            if rng.uniform() < 0.75 and (n_det is None or len(det) < n_det):
                q = grid(p + rng.normal(0, 0.7, 2))
                score = float(np.round(rng.uniform(0.05, 1), 1 if quant else 3))
                det.append((q, score, DET_NAMES[cls[i]] if rng.uniform() < 0.9 else DET_NAMES[rng.integers(0, 3)]))
        n_clutter = int(rng.integers(clutter[0], clutter[1])) if n_det is None else n_det - len(det)
        for _ in range(n_clutter):
            q = grid(rng.uniform(-half, half, 2))
            det.append((q, float(np.round(rng.uniform(0.05, 0.6), 1 if quant else 3)), DET_NAMES[rng.integers(0, 3)]))
        det = [det[i] for i in rng.permutation(len(det))]
        emit = t not in not_emitted and not (skip_frac > 0 and rng.uniform() < skip_frac)
        frames.append(dict(det_xy=np.array([d[0] for d in det], dtype=np.float64).reshape(-1, 2),
                           det_score=np.array([d[1] for d in det], dtype=np.float64), det_types=[d[2] for d in det],
                           gt_xy=np.array(gt_xy, dtype=np.float64).reshape(-1, 2), gt_types=gt_types, gt_ids=gt_ids, emit=bool(emit),
                           has_prev=t > 0))
    return frames


def golden_scenes():
    """The scenes of tests/golden/gt_labels_golden.json.gz, by name."""
    scenes = {"quant%d" % s: synth_scene(s) for s in range(4)}
    scenes.update({"free%d" % s: synth_scene(10 + s, quant=False) for s in range(2)})
    scenes["seam"] = synth_scene(20, counts=SEAM_COUNTS)
    scenes["skipped"] = synth_scene(30, not_emitted=(5, 6))
    scenes["crowded"] = synth_scene(40, half=8.0)  # 40 objects on 16 m x 16 m of the 0.5 m grid: equal minimal distances are common
    return scenes
