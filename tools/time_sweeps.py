"""Time the multi-sweep cloud assembly (shasta_sweeps_assemble_f32, csrc/sweeps.hip): 8 clouds x 10 segments x 34 720 rows of 5 floats,
the key frame plus nine sweeps of a nuScenes frame, synthetic radial rows (a few per cent inside the 1 m square).  In the same process,
after a warm-up of each, with the device synchronised around every timed call:
  chain  : shasta_amd.sweeps.assemble_rows on rows already on the device - output and workspace allocation and the copy of the
           segment table included, nothing read back
  h2d    : the copy of the raw rows from a pinned buffer to the device, which a call of assemble_clouds makes before the chain
  files  : shasta_amd.sweeps.assemble_clouds from .bin files in a temporary directory (page cache warm): file reads into the pinned
           buffer, h2d, chain, the host read of the prefix
  numpy  : the numpy restatement tests/sweeps_helpers.assemble of LoadPointCloudFromFile on the same rows in memory, on this host, cloud
           by cloud as a DataLoader worker would run it (no file reads)
The byte floor beside them is computed from the shapes: the raw rows read once by the write pass and two of their five columns by the
count pass (which the cache lines turn into the whole rows: counted as a full read), the kept rows written - at the measured copy rate
of the chip.  No pass / fail time.  One JSON line.

    python tools/time_sweeps.py [--rounds 7] [--clouds 8] [--segments 10] [--rows 34720]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from shasta_amd import sweeps  # noqa: E402
from tests import sweeps_helpers as H  # noqa: E402

HBM_RATE = 6.29e12  # B/s, measured float4 copy (tools/time_backbone.py)


def rows(rng, n):
    p = np.zeros((n, 5), np.float32)
    r = np.abs(rng.normal(0, 18, size=n)).astype(np.float32)
    th = rng.uniform(0, 2 * np.pi, size=n).astype(np.float32)
    p[:, 0], p[:, 1] = r * np.cos(th), r * np.sin(th)
    p[:, 2] = rng.normal(-1.5, 0.6, size=n)
    p[:, 3] = rng.uniform(0, 255, size=n)
    p[:, 4] = rng.integers(0, 32, size=n)
    return p


def rigid(rng):
    a = rng.uniform(-0.2, 0.2)
    m = np.eye(4)
    m[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    m[:3, 3] = rng.uniform(-5, 5, 3)
    return m


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--clouds", type=int, default=8)
    ap.add_argument("--segments", type=int, default=10)
    ap.add_argument("--rows", type=int, default=34720)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    n, S, P = a.clouds, a.segments, a.rows
    frames = [[rows(rng, P) for _ in range(S)] for _ in range(n)]
    transforms = [[rigid(rng) for _ in range(S - 1)] for _ in range(n)]
    lags = [[0.05 * (i + 1) for i in range(S - 1)] for _ in range(n)]
    segs = []
    for c in range(n):
        segs.append(H.segment(P, c))
        segs += [H.segment(P, c, transforms[c][i], True, lags[c][i]) for i in range(S - 1)]
    raw = np.concatenate([r for f in frames for r in f])
    pinned = torch.from_numpy(raw).pin_memory()
    d_raw = pinned.to(dev)
    out, prefix = sweeps.assemble_rows(d_raw, segs, n)
    kept = prefix.cpu().tolist()
    # the chain agrees with the restatement, bit for bit, before anything is timed (first cloud)
    want, _ = H.assemble(raw[:S * P], segs[:S], 1)
    assert kept[1] == len(want) and np.array_equal(H.uint(out[:kept[1]].cpu().numpy()), H.uint(want))

    def numpy_clouds():
        for c in range(n):
            H.assemble(raw[c * S * P:(c + 1) * S * P], [(r, 0, t, d, lag) for r, _, t, d, lag in segs[c * S:(c + 1) * S]], 1)

    with tempfile.TemporaryDirectory() as tmp:
        infos = [H.frame_info(tmp, "f%d" % c, f[0], f[1:], transforms[c], lags[c]) for c, f in enumerate(frames)]
        routes = {
            "chain": lambda: sweeps.assemble_rows(d_raw, segs, n),
            "h2d": lambda: d_raw.copy_(pinned, non_blocking=True),
            "files": lambda: sweeps.assemble_clouds(infos, S, dev),
            "numpy": numpy_clouds,
        }
        times = {k: [] for k in routes}
        for fn in routes.values():  # warm-up
            fn()
        for _ in range(a.rounds):
            for k, fn in routes.items():
                times[k].append(timed(fn))
    floor = 2 * raw.nbytes + kept[-1] * 5 * 4
    res = {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4),
                   median_ms_per_cloud=round(statistics.median(v) / n, 4)) for k, v in times.items()}
    print(json.dumps(dict(tool="time_sweeps", clouds=n, segments_per_cloud=S, rows_per_segment=P, rows_in=len(raw), rows_out=kept[-1],
                          rounds=a.rounds, **res, raw_mbytes_per_cloud=round(raw.nbytes / n / 1e6, 2),
                          out_mbytes_per_cloud=round(kept[-1] * 20 / n / 1e6, 2), floor_mbytes=round(floor / 1e6, 1),
                          floor_ms=round(floor / HBM_RATE * 1e3, 4), floor_ms_per_cloud=round(floor / HBM_RATE * 1e3 / n, 4),
                          host_cpus=os.cpu_count(), device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
