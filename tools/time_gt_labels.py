"""Times the label construction of a synthetic split: one gt_labels.split_labels(device=True) call (csrc/gt_labels.hip, one launch
for every frame of every scene) beside the host path (numpy, frame by frame) on the same box.  20 scenes x 40 frames from
tests/gt_label_scenes.py at about 300 detections and 80 ground-truth boxes per frame; 5 alternating rounds after a warm-up, median
and range, plus the device events around the ABI call alone.  The results are compared before anything is timed.

    python tools/time_gt_labels.py [--scenes 20] [--frames 40] [--rounds 5] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from shasta_amd import gt_labels, hip  # noqa: E402
from tests.gt_label_scenes import synth_scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", type=int, default=20)
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise hip.ShastaHipError("time_gt_labels needs a GPU: a time taken elsewhere says nothing")
    scenes = [synth_scene(7000 + s, n_frames=a.frames, n_obj=200, quant=False, clutter=(225, 260), half=60.0) for s in range(a.scenes)]
    n_frames = sum(len(s) for s in scenes)
    dets = sum(len(f["det_score"]) for s in scenes for f in s) / n_frames
    gts = sum(len(f["gt_ids"]) for s in scenes for f in s) / n_frames
    dev = gt_labels.split_labels(scenes, 2.0, device=True)  # warm-up: loads the code object
    host = gt_labels.split_labels(scenes, 2.0, device=False)
    for d, h in zip(dev, host):
        for (dm, dn), (hm, hn) in zip(d, h):
            assert (dm is None) == (hm is None) and (dm is None or np.array_equal(dm, hm)) and np.array_equal(dn, hn)
    # the kernels alone: events around the ABI call on prepared device buffers
    p = gt_labels._prepare(scenes)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_dev, t_host, t_kern = [], [], []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gt_labels.split_labels(scenes, 2.0, device=True)  # ends in the copy back: synchronous
        t_dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        gt_labels.split_labels(scenes, 2.0, device=False)
        t_host.append(time.perf_counter() - t0)
        ev[0].record()
        gt_labels._labels_device(p, 2.0)
        ev[1].record()
        torch.cuda.synchronize()
        t_kern.append(ev[0].elapsed_time(ev[1]) * 1e-3)

    def stat(v):
        return dict(median_ms=1e3 * statistics.median(v), min_ms=1e3 * min(v), max_ms=1e3 * max(v))
    res = dict(scenes=a.scenes, frames=n_frames, dets_per_frame=round(dets, 1), gt_per_frame=round(gts, 1), rounds=a.rounds,
               device_call=stat(t_dev), host_call=stat(t_host), device_uploads_kernels_copy_back=stat(t_kern),
               gpu=torch.cuda.get_device_name(0))
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
