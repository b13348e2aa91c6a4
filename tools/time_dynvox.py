"""Time the dynamic voxeliser (shasta_dynvox_mean_f32, csrc/dynvox.hip) at the shipped range and voxel size on the synthetic radial
clouds of tools/time_voxelize.py: P = 1e5 and 3e5 points, one cloud and 16 clouds.  In the same process, in turns after a warm-up of
each, with the device synchronised around every timed call:
  dynvox : shasta_amd.dynamic_voxel_encoder.dynamic_voxelize(sync=False) - output allocation included, nothing read back
  hard   : (a) shasta_voxelize_mean_batch_f32 on the same clouds (points_to_voxel_batch_device, 10 points x 160 000 voxels per cloud,
           output allocation included, nothing read back) - another operation (capped slots, first-touch order), the project's other voxeliser
  torch  : (b) the reference's recipe written with torch device operations, cloud by cloud: keep mask, coordinates, unique(dim=0) with
           the inverse, index_add_ and a division (unique synchronises; its float sum is atomic, not bit-reproducible)
The byte floor printed beside them is computed from the shapes: the points read twice, three per-point index lists written and read,
the bitmap of all clouds' cells cleared, scanned (read, prefix written), read by the emit pass and looked up per point, the outputs
written - at the measured copy rate of the chip.  One JSON line per case.

    python tools/time_dynvox.py [--rounds 5] [--cases 100000x1 300000x1 100000x16 300000x16]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from shasta_amd.dynamic_voxel_encoder import dynamic_voxelize  # noqa: E402
from shasta_amd.voxel_generator import points_to_voxel_batch_device  # noqa: E402

VS = np.array([0.075, 0.075, 0.2], np.float32)
RG = np.array([-54, -54, -5, 54, 54, 3], np.float32)
SHAPE = (1440, 1440, 40)
HBM_RATE = 6.29e12  # B/s, measured float4 copy (tools/time_backbone.py)


def cloud(rng, P):
    pts = np.zeros((P, 5), np.float32)
    r = np.abs(rng.normal(0, 18, size=P)).astype(np.float32)
    th = rng.uniform(0, 2 * np.pi, size=P).astype(np.float32)
    pts[:, 0], pts[:, 1] = r * np.cos(th), r * np.sin(th)
    pts[:, 2] = rng.normal(-1.5, 0.6, size=P)
    pts[:, 3] = rng.uniform(0, 255, size=P)
    return pts


def torch_recipe(points, offsets, rg, vs):
    out = []
    for b in range(len(offsets) - 1):
        p = points[offsets[b]:offsets[b + 1]]
        keep = ((p[:, :3] >= rg[:3]) & (p[:, :3] <= rg[3:])).all(1)
        p = p[keep]
        coords = ((p[:, [2, 1, 0]] - rg[[2, 1, 0]]) / vs[[2, 1, 0]]).to(torch.int64)
        uniq, inv = coords.unique(return_inverse=True, dim=0)
        sums = torch.zeros(len(uniq), p.shape[1], device=p.device).index_add_(0, inv, p)
        cnt = torch.zeros(len(uniq), device=p.device).index_add_(0, inv, torch.ones(len(p), device=p.device))
        out.append((sums / cnt[:, None], uniq))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", nargs="+", default=["100000x1", "300000x1", "100000x16", "300000x16"])
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    rg, vs = torch.from_numpy(RG).to(dev), torch.from_numpy(VS).to(dev)
    for case in a.cases:
        P, n = (int(x) for x in case.split("x"))
        allp = torch.from_numpy(np.concatenate([cloud(rng, P) for _ in range(n)])).to(dev)
        offs = [P * i for i in range(n + 1)]
        routes = {
            "dynvox": lambda: dynamic_voxelize((allp, offs), RG, VS, SHAPE, sync=False),
            "hard": lambda: points_to_voxel_batch_device((allp, offs), VS, RG, 10, 160000, with_mean=True),
            "torch": lambda: torch_recipe(allp, offs, rg, vs),
        }
        # the three agree on what they share before anything is timed: voxel counts, and dynvox == torch rows up to the float sum's order
        prefix = dynamic_voxelize((allp, offs), RG, VS, SHAPE, sync=False)[3].cpu().tolist()
        ref = torch_recipe(allp, offs, rg, vs)
        assert [len(u) for _, u in ref] == [prefix[i + 1] - prefix[i] for i in range(n)]
        V = prefix[-1]
        times = {k: [] for k in routes}
        for k, fn in routes.items():  # warm-up
            fn()
        for _ in range(a.rounds):
            for k, fn in routes.items():
                times[k].append(timed(fn))
        cells = n * (SHAPE[2] + 1) * (SHAPE[1] + 1) * (SHAPE[0] + 1)
        bitmap = (cells + 31) // 32 * 4
        floor = 2 * n * P * 5 * 4 + 3 * 2 * n * P * 4 + 4 * bitmap + n * P * 4 + V * (5 * 4 + 16 + 4)
        res = {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) for k, v in times.items()}
        print(json.dumps(dict(tool="time_dynvox", points_per_cloud=P, clouds=n, voxels=V, rounds=a.rounds, **res,
                              floor_mbytes=round(floor / 1e6, 1), bitmap_mbytes=round(bitmap / 1e6, 1),
                              floor_ms=round(floor / HBM_RATE * 1e3, 4), device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
