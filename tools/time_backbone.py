"""Time the sparse backbone (SpMiddleResNetFHD.forward, csrc/sparse_conv.hip) at the shipped grid: synthetic clouds of the shipped
density -> VoxelGenerator.generate_batch_device (0.075 m x 0.075 m x 0.2 m voxels, 1440 x 1440 x 40) -> the voxeliser's per-voxel mean
(what the reader computes) -> backbone.  HIP events around every C call after a warm-up, summed per level into index build (bitmap,
scan, coordinates, neighbour tables), convolutions and the densify; next to them the rows per level, the share of taps present, and a
floor from the counted present taps: their FLOP at the f32 matrix peak and the bytes gathered, read and written at the measured HBM rate.
One JSON line per batch size.  With --train the same input goes through the train()-mode forward (batch_statistics=True, every
BatchNorm1d on batch statistics, csrc/bn_rows.hip): the convolutions then write raw sums, and the statistics, finalize and apply calls of a
level are listed next to them.

    python tools/time_backbone.py [--batches 1 2] [--iters 5] [--points 300000] [--train]

With --sync-ranks N the train()-mode forward runs on N GPUs, one fresh process each with its own clouds, the module converted with
sync_bn.convert_syncbn_model (batch statistics of all ranks over RCCL: one small all-gather and csrc/bn_sync.hip per layer); per rank
the synced forward beside the un-synced one of the same weights.  Fewer GPUs than ranks: "not measured".

    python tools/time_backbone.py --sync-ranks 4 [--batches 1 2] [--iters 5] [--points 300000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from shasta_amd import backbone, hip  # noqa: E402
from shasta_amd.voxel_generator import VoxelGenerator  # noqa: E402
from tools import sync_ranks  # noqa: E402

F32_MATRIX_PEAK = 155e12  # FLOP/s, v_mfma_f32_*_f32 measured
HBM_RATE = 6.29e12        # B/s, measured float4 copy
INDEX_CALLS = ("shasta_spconv_index_rows", "shasta_spconv_out_coords", "shasta_spconv_neighbors")
# column of a level's timing row per call: index, conv, and the three batch-statistics calls of the train()-mode forward
COLUMNS = dict({n: 0 for n in INDEX_CALLS}, shasta_spconv_layer_f32=1, shasta_bn_rows_stats_f32=2, shasta_bn_rows_finalize_f32=3,
               shasta_bn_rows_apply_f32=4)


def cloud(rng, P):
    """A lidar-like cloud: range ~ |N(0, 18 m)|, uniform azimuth, heights around the ground (tools/time_voxelize.py's)."""
    pts = np.zeros((P, 5), np.float32)
    r = np.abs(rng.normal(0, 18, size=P)).astype(np.float32)
    th = rng.uniform(0, 2 * np.pi, size=P).astype(np.float32)
    pts[:, 0], pts[:, 1] = r * np.cos(th), r * np.sin(th)
    pts[:, 2] = rng.normal(-1.5, 0.6, size=P)
    pts[:, 3] = rng.uniform(0, 255, size=P)
    return torch.from_numpy(pts)


class TimingLib:
    """The loaded library with an event pair around every spconv and bn_rows call."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith(("shasta_spconv_", "shasta_bn_rows_")) or name.endswith(("_bytes", "_supported")):
            return fn

        def timed(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            self.calls.append((name, e0, e1))
            return rc
        return timed


def per_level(calls):
    """Calls in forward order -> [index, conv, stats, finalize, apply] ms per level (a level starts at its out_coords call), densify ms."""
    levels, dense = [[0.0] * 5], 0.0
    for name, e0, e1 in calls:
        ms = e0.elapsed_time(e1)
        if name == "shasta_spconv_out_coords":
            levels.append([0.0] * 5)
        if name in COLUMNS:
            levels[-1][COLUMNS[name]] += ms
        elif name == "shasta_spconv_dense_f32":
            dense += ms
    return levels, dense


def sync_child(a):
    """One rank of --sync-ranks: the un-synced train() forward, then the same weights converted and synced over the ranks."""
    import copy
    from shasta_amd.sync_bn import convert_syncbn_model
    dev = sync_ranks.child(a)
    torch.manual_seed(0)
    plain = backbone.SpMiddleResNetFHD(num_input_features=5, ds_factor=8, batch_statistics=True).train().to(dev)
    synced = convert_syncbn_model(copy.deepcopy(plain)).train()
    vg = VoxelGenerator([0.075, 0.075, 0.2], [-54, -54, -5, 54, 54, 3], 10, max_voxels=160000)
    shape = vg.grid_size.tolist()
    rng = np.random.default_rng(a.sync_rank)  # (every rank its own clouds)
    res = dict(tool="time_backbone", mode="train, synced", ranks=a.sync_ranks, rank=a.sync_rank, points_per_cloud=a.points,
               device=torch.cuda.get_device_name(dev), batches=[])
    with torch.no_grad():
        for B in a.batches:
            clouds = [cloud(rng, a.points).to(dev) for _ in range(B)]
            _, coors, _, mean, nv = vg.generate_batch_device(clouds)
            nv = nv.cpu().tolist()
            feats = torch.cat([mean[b, :nv[b]] for b in range(B)]).contiguous()
            coords = torch.cat([torch.cat([torch.full((nv[b], 1), b, dtype=torch.int32, device=dev), coors[b, :nv[b]]], 1) for b in range(B)])
            t_plain = sync_ranks.timed_ms(lambda: plain(feats, coords, B, shape), a.iters)
            t_sync = sync_ranks.timed_ms(lambda: synced(feats, coords, B, shape), a.iters)
            res["batches"].append(dict(B_per_rank=B, voxels=sum(nv), forward_ms=round(t_plain, 3), forward_synced_ms=round(t_sync, 3)))
    print(json.dumps(res), flush=True)
    torch.distributed.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--train", action="store_true", help="time the train()-mode forward (batch-statistics BatchNorm1d)")
    sync_ranks.add_arguments(ap)
    a = ap.parse_args()
    if a.sync_rank is not None:
        return sync_child(a)
    if a.sync_ranks:
        sys.exit(sync_ranks.parent("time_backbone", a))
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = backbone.SpMiddleResNetFHD(num_input_features=5, ds_factor=8, batch_statistics=a.train).train(a.train).to(dev)
    vg = VoxelGenerator([0.075, 0.075, 0.2], [-54, -54, -5, 54, 54, 3], 10, max_voxels=160000)
    shape = vg.grid_size.tolist()
    rng = np.random.default_rng(0)
    real_load = hip.load
    for B in a.batches:
        clouds = [cloud(rng, a.points).to(dev) for _ in range(B)]
        _, coors, _, mean, nv = vg.generate_batch_device(clouds)
        nv = nv.cpu().tolist()
        feats = torch.cat([mean[b, :nv[b]] for b in range(B)]).contiguous()
        coords = torch.cat([torch.cat([torch.full((nv[b], 1), b, dtype=torch.int32, device=dev), coors[b, :nv[b]]], 1) for b in range(B)])
        with torch.no_grad():
            # one untimed pass that also counts rows and present taps per convolution
            stats = []
            real_layer = m._layer

            def counting_layer(x, n_in, nbr, conv, residual=None, relu=True):
                stats.append(dict(cin=conv.in_channels, cout=conv.out_channels, n_in=n_in, n_out=int(nbr.shape[0]), K=int(nbr.shape[1]),
                                  present=int((nbr >= 0).sum()), residual=residual is not None))
                return real_layer(x, n_in, nbr, conv, residual, relu)

            m._layer = counting_layer
            ret, _ = m(feats, coords, B, shape)
            m._layer = real_layer
            for _ in range(2):
                m(feats, coords, B, shape)
            torch.cuda.synchronize()
            tl = TimingLib(real_load())
            hip.load = lambda: tl
            try:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    m(feats, coords, B, shape)
                e1.record()
                torch.cuda.synchronize()
            finally:
                hip.load = real_load
        total = e0.elapsed_time(e1) / a.iters
        n_calls = len(tl.calls) // a.iters
        acc = None
        for it in range(a.iters):
            lv, dn = per_level(tl.calls[it * n_calls:(it + 1) * n_calls])
            flat = [v for row in lv for v in row] + [dn]
            acc = flat if acc is None else [x + y for x, y in zip(acc, flat)]
        acc = [v / a.iters for v in acc]
        # the convolutions of a level: conv1 has 5 (conv_input + two blocks), conv2..4 have 5 (strided + two blocks), the last level 1
        names, per = ("conv1", "conv2", "conv3", "conv4", "extra_conv"), (5, 5, 5, 5, 1)
        out_levels, k = [], 0
        for i, (name, cnt) in enumerate(zip(names, per)):
            ss = stats[k:k + cnt]
            k += cnt
            flop = sum(2 * s["present"] * s["cin"] * s["cout"] for s in ss)
            byts = sum(4 * (s["present"] * s["cin"] + s["n_out"] * s["K"] + s["n_out"] * s["cout"] * (2 if s["residual"] else 1)
                            + s["K"] * s["cin"] * s["cout"]) for s in ss)
            taps = sum(s["present"] for s in ss) / max(1, sum(s["n_out"] * s["K"] for s in ss))
            row = dict(level=name, rows=ss[-1]["n_out"], taps_present=round(taps, 3), index_ms=round(acc[5 * i], 4),
                       conv_ms=round(acc[5 * i + 1], 4), gflop=round(flop / 1e9, 3), mbytes=round(byts / 1e6, 2),
                       floor_flop_ms=round(flop / F32_MATRIX_PEAK * 1e3, 4), floor_bytes_ms=round(byts / HBM_RATE * 1e3, 4))
            if a.train:
                # the three passes over a layer's (rows, Cout) scratch: read; -; read + residual read + write
                bn_bytes = sum(4 * s["n_out"] * s["cout"] * (3 + (1 if s["residual"] else 0)) for s in ss)
                row.update(stats_ms=round(acc[5 * i + 2], 4), finalize_ms=round(acc[5 * i + 3], 4), apply_ms=round(acc[5 * i + 4], 4),
                           bn_mbytes=round(bn_bytes / 1e6, 2), bn_floor_bytes_ms=round(bn_bytes / HBM_RATE * 1e3, 4))
            out_levels.append(row)
        print(json.dumps(dict(tool="time_backbone", mode="train" if a.train else "eval", B=B, points_per_cloud=a.points, voxels=sum(nv), grid=[shape[2] + 1, shape[1], shape[0]],
                              forward_ms=round(total, 3), device_ms=round(sum(acc), 3), dense_ms=round(acc[-1], 4),
                              result=list(ret.shape), levels=out_levels, device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
