"""Time the CenterPoint training targets and head losses at the shipped shape - 180 x 180 maps, the six nuScenes tasks, max_objs = 500,
B = 4, about 60 boxes per sample:
  * `targets.assign_targets` (csrc/center_targets.hip, one call for the batch) beside the numpy restatement of the reference's AssignLabel
    on the host (tests/center_targets_helpers.py, one sample after the other, as a loader worker runs it);
  * `head_loss.CenterLoss` forward + backward (csrc/center_loss.hip) beside the torch composite of the same formulas with autograd on the
    device, in the same process.
Device figures: one HIP event pair per run after a warm-up, the median of --runs runs (at least 20); the host figure is wall-clock.  Recorded,
not gated.  Writes profiles/center_targets_timing.txt and prints it.

    python tools/time_targets.py [--runs 20] [--warmup 5] [--out profiles/center_targets_timing.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from shasta_amd import head_loss, targets  # noqa: E402
from tests import center_targets_helpers as H  # noqa: E402

TASKS = [1, 2, 2, 1, 2, 2]
CFG = dict(pc_range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], voxel_size=[0.075, 0.075, 0.2], out_size_factor=8, gaussian_overlap=0.1, max_objs=500,
           min_radius=2)
WEIGHT, CODE_WEIGHTS = 0.25, [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0]
HEADS = ("hm", "reg", "height", "dim", "vel", "rot")
WIDTH = dict(hm=None, reg=2, height=1, dim=3, vel=2, rot=2)


def median_ms(fn, runs, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def sample(rng, n):
    cls = rng.randint(1, sum(TASKS) + 1, n).astype(np.int32)
    size = np.array([[1.9, 4.6, 1.7], [2.5, 6.9, 2.8], [2.8, 6.4, 3.2], [2.9, 11.0, 3.5], [2.9, 12.3, 3.9], [2.5, 0.5, 1.0], [0.8, 2.1, 1.5],
                     [0.6, 1.7, 1.3], [0.7, 0.7, 1.8], [0.4, 0.4, 1.1]], dtype=np.float32)[cls - 1]
    rows = np.concatenate([rng.uniform(-50, 50, (n, 2)), rng.uniform(-2, 0, (n, 1)), size * rng.uniform(0.9, 1.1, (n, 3)), rng.randn(n, 2),
                           rng.uniform(-3.14, 3.14, (n, 1))], 1).astype(np.float32)
    return rows, cls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "center_targets_timing.txt"))
    a = ap.parse_args()
    a.runs = max(a.runs, 20)
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(0)
    B = 4
    samples = [sample(rng, n) for n in (57, 64, 49, 71)]
    boxes = [torch.from_numpy(b).to(dev) for b, _ in samples]
    classes = [c for _, c in samples]
    prop = torch.cuda.get_device_properties(0)
    box = "%s (%s, %d CUs), torch %s, HIP %s, numpy %s" % (prop.name, getattr(prop, "gcnArchName", "?"), prop.multi_processor_count,
                                                         torch.__version__, torch.version.hip, np.__version__)
    lines = ["CenterPoint targets and head losses at B = %d, 180 x 180 maps, six nuScenes tasks, max_objs = 500, %s boxes per sample; %s; device "
             "figures: median (min .. max) of %d runs after %d warm-up runs, one HIP event pair per run"
             % (B, "/".join(str(len(c)) for c in classes), box, a.runs, a.warmup)]
    ex = targets.assign_targets(boxes, classes, TASKS, CFG)
    t = median_ms(lambda: targets.assign_targets(boxes, classes, TASKS, CFG), a.runs, a.warmup)
    lines.append("assign_targets, kernels (center_targets.hip), whole batch        %8.3f ms (%.3f .. %.3f)" % t)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        for b, c in samples:
            H.assign_ref(b, c, CFG, tasks=TASKS)
        host.append((time.perf_counter() - t0) * 1e3)
    lines.append("AssignLabel restated in numpy on the host, the %d samples in turn  %8.3f ms (best of 3 wall-clock runs, one core)" % (B, min(host)))
    g = torch.Generator().manual_seed(1)
    preds = [{n: (torch.randn(B, TASKS[t] if n == "hm" else WIDTH[n], 180, 180, generator=g) * (2.0 if n == "hm" else 1.0) - (2.19 if n == "hm" else 0.0))
              .to(dev).requires_grad_(True) for n in HEADS} for t in range(len(TASKS))]

    def step(composite):
        for pd in preds:
            for v in pd.values():
                v.grad = None
        outs = head_loss.center_loss(preds, ex, WEIGHT, CODE_WEIGHTS, force_composite=composite)
        sum(o["loss"] for o in outs).backward()
        return outs

    k, c = step(False), step(True)
    lines.append("total loss: kernels %.6f, torch composite %.6f" % (float(sum(o["loss"].detach() for o in k)), float(sum(o["loss"].detach() for o in c))))
    t = median_ms(lambda: step(False), a.runs, a.warmup)
    lines.append("CenterLoss forward + backward, kernels (center_loss.hip)          %8.3f ms (%.3f .. %.3f)" % t)
    t = median_ms(lambda: step(True), a.runs, a.warmup)
    lines.append("the same losses as a torch composite with autograd, on the device %8.3f ms (%.3f .. %.3f)" % t)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
