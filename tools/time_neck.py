"""Time the RPN neck at the shipped shape (configs/nusc: 256 -> 128 / 256 -> 512 channels, layer_nums [5, 5], 180 x 180 maps) on the
hand-written kernels (RPN.forward, csrc/neck.hip) and, with the same weights in the same run, through the module's own nn layers
(RPN.forward_layers: MIOpen).  HIP events after a warm-up; one JSON line.

    python tools/time_neck.py [--batches 1 2 8] [--iters 10] [--hw 180]

With --train (default batches 1 and 8) the train()-mode forward of the training step - the neck frozen, every BatchNorm2d on batch
statistics - is timed three ways with the same weights in the same run: on the kernels (batch_statistics=True: raw convolution,
csrc/bn_maps.hip), on the kernels in eval() mode, and through forward_layers in train() mode (MIOpen); next to them an event pair around
every C call of the train()-mode forward, summed per pass, and the counted traffic of the passes a layer has more than in eval() mode
(the statistics read y, the apply reads and writes it) at the measured HBM rate.

    python tools/time_neck.py --train [--batches 1 8] [--iters 10] [--hw 180]

With --sync-ranks N the train()-mode forward runs on N GPUs, one fresh process each, the module converted with
sync_bn.convert_syncbn_model (batch statistics of all ranks over RCCL: one small all-gather and csrc/bn_sync.hip per layer); per rank
the synced forward beside the un-synced one of the same weights.  Fewer GPUs than ranks: "not measured".

    python tools/time_neck.py --sync-ranks 4 [--batches 1 8] [--iters 10] [--hw 180]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.getcwd())
import shasta_amd  # noqa: E402
from shasta_amd import hip, neck  # noqa: E402
from tools import sync_ranks  # noqa: E402

SHIPPED = dict(layer_nums=[5, 5], ds_layer_strides=[1, 2], ds_num_filters=[128, 256], us_layer_strides=[1, 2], us_num_filters=[256, 256],
               num_input_features=256)
KIND = {neck.C3S1: "C3S1", neck.C3S2: "C3S2", neck.C1: "C1", neck.D2: "D2"}
HBM_RATE = 6.29e12  # B/s, measured float4 copy
PASSES = dict(shasta_neck_layer_raw_f32="conv_raw_ms", shasta_neck_layer_f32="conv_eval_ms", shasta_bn_maps_stats_f32="stats_ms",
              shasta_bn_maps_finalize_f32="finalize_ms", shasta_bn_maps_apply_f32="apply_ms")


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def layer_flops(kind, conv, h, w):
    """FLOP of one layer on one (h, w) input map (2 per multiply-add)."""
    taps, pix = (9, h * w) if kind == neck.C3S1 else (9, h * w // 4) if kind == neck.C3S2 else (1, h * w) if kind == neck.C1 else (4, h * w)
    return 2 * conv.in_channels * conv.out_channels * taps * pix


class TimingLib:
    """The loaded library with an event pair around every call of a forward's passes."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in PASSES:
            return fn

        def timed_call(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            self.calls.append((name, e0, e1))
            return rc
        return timed_call


def per_pass(m, x, iters):
    """ms per forward spent in each pass (HIP events around every call; the events themselves keep the launches apart)."""
    real_load = hip.load
    tl = TimingLib(real_load())
    hip.load = lambda: tl
    try:
        for _ in range(iters):
            m(x)
        torch.cuda.synchronize()
    finally:
        hip.load = real_load
    out = {v: 0.0 for v in PASSES.values()}
    for name, e0, e1 in tl.calls:
        out[PASSES[name]] += e0.elapsed_time(e1) / iters
    return {k: round(v, 4) for k, v in out.items() if v > 0}


def train_main(a):
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = shasta_amd.builder.build_neck(dict(type="RPN", batch_statistics=True, **SHIPPED)).to(dev)
    shapes = m._shapes(a.hw, a.hw)
    flop = sum(layer_flops(k, conv, s[0], s[1]) for (k, conv, _, _), s in zip(m._plan, shapes))
    y_bytes = sum(4 * conv.out_channels * s[2] * s[3] for (_, conv, _, _), s in zip(m._plan, shapes))  # every layer's output, one image
    res = dict(tool="time_neck", mode="train", hw=a.hw, gflop_per_map=round(flop / 1e9, 2), device=torch.cuda.get_device_name(0), batches=[])
    with torch.no_grad():
        for B in a.batches or [1, 8]:
            x = torch.randn(B, 256, a.hw, a.hw, device=dev) + 0.2
            m.train()
            t_train = timed(lambda: m(x), a.iters)
            passes = per_pass(m, x, a.iters)
            t_nn = timed(lambda: m.forward_layers(x), a.iters)
            m.eval()
            t_eval = timed(lambda: m(x), a.iters)
            extra = 3 * B * y_bytes  # per layer: the statistics read y; the apply reads and writes it
            res["batches"].append(dict(B=B, hip_train_ms=round(t_train, 3), hip_eval_ms=round(t_eval, 3), miopen_train_ms=round(t_nn, 3),
                                       passes=passes, extra_mbytes=round(extra / 1e6, 1), extra_floor_bytes_ms=round(extra / HBM_RATE * 1e3, 4)))
    print(json.dumps(res))


def sync_child(a):
    """One rank of --sync-ranks: the un-synced train() forward, then the same weights converted and synced over the ranks."""
    import copy
    from shasta_amd.sync_bn import convert_syncbn_model
    dev = sync_ranks.child(a)
    torch.manual_seed(0)
    plain = shasta_amd.builder.build_neck(dict(type="RPN", batch_statistics=True, **SHIPPED)).train().to(dev)
    synced = convert_syncbn_model(copy.deepcopy(plain)).train()
    res = dict(tool="time_neck", mode="train, synced", ranks=a.sync_ranks, rank=a.sync_rank, hw=a.hw, device=torch.cuda.get_device_name(dev),
               batches=[])
    with torch.no_grad():
        for B in a.batches or [1, 8]:
            x = torch.randn(B, 256, a.hw, a.hw, device=dev) + 0.2
            t_plain = sync_ranks.timed_ms(lambda: plain(x), a.iters)
            t_sync = sync_ranks.timed_ms(lambda: synced(x), a.iters)
            res["batches"].append(dict(B_per_rank=B, hip_train_ms=round(t_plain, 3), hip_train_synced_ms=round(t_sync, 3)))
    print(json.dumps(res), flush=True)
    torch.distributed.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=None)
    ap.add_argument("--train", action="store_true", help="time the train()-mode forward (batch-statistics BatchNorm2d) beside eval and MIOpen")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--hw", type=int, default=180)
    ap.add_argument("--no-layers", action="store_true", help="skip the per-layer timing")
    sync_ranks.add_arguments(ap)
    a = ap.parse_args()
    if a.sync_rank is not None:
        return sync_child(a)
    if a.sync_ranks:
        sys.exit(sync_ranks.parent("time_neck", a))
    if a.train:
        return train_main(a)
    a.batches = a.batches or [1, 2, 8]
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    m = shasta_amd.builder.build_neck(dict(type="RPN", **SHIPPED)).eval().to(dev)
    shapes = m._shapes(a.hw, a.hw)
    flop = sum(layer_flops(k, conv, s[0], s[1]) for (k, conv, _, _), s in zip(m._plan, shapes))
    res = dict(tool="time_neck", hw=a.hw, gflop_per_map=round(flop / 1e9, 2), device=torch.cuda.get_device_name(0), batches=[])
    with torch.no_grad():
        for B in a.batches:
            x = torch.relu(torch.randn(B, 256, a.hw, a.hw, device=dev))
            t_hip = timed(lambda: m(x), a.iters)
            t_nn = timed(lambda: m.forward_layers(x), a.iters)
            res["batches"].append(dict(B=B, hip_ms=round(t_hip, 3), hip_tflops=round(B * flop / t_hip / 1e9, 1), miopen_ms=round(t_nn, 3),
                                       miopen_tflops=round(B * flop / t_nn / 1e9, 1)))
        if not a.no_layers:  # every layer of the chain on its own, B = 1 (the same launches RPN.forward makes)
            lib, s = hip.load(), hip.stream_ptr()
            x = torch.relu(torch.randn(1, 256, a.hw, a.hw, device=dev))
            m(x)
            layers = []
            for (kind, conv, _, _), pk, sh in zip(m._plan, m._packed, shapes):
                xin = torch.relu(torch.randn(1, conv.in_channels, sh[0], sh[1], device=dev))
                out = torch.empty(1, conv.out_channels, sh[2], sh[3], device=dev)
                ms = timed(lambda: hip.check(lib.shasta_neck_layer_f32(hip.ptr(xin), 1, conv.in_channels, sh[0], sh[1], hip.ptr(pk), pk.numel(), kind,
                                                                       conv.out_channels, hip.ptr(out), conv.out_channels, 0, s), "neck_layer"), a.iters)
                f = layer_flops(kind, conv, sh[0], sh[1])
                layers.append(dict(kind=KIND[kind], cin=conv.in_channels, cout=conv.out_channels, hw=sh[0], gflop=round(f / 1e9, 2), ms=round(ms, 4),
                                   tflops=round(f / ms / 1e9, 1)))
            res["layers_b1"] = layers
    print(json.dumps(res))


if __name__ == "__main__":
    main()
