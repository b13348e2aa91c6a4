"""Time `shasta_bn_sync_finalize_f32` (csrc/bn_sync.hip: the merge of R ranks' (mean, M2, count) records and the finalize) beside the
plain finalize calls it stands in for, `shasta_bn_rows_finalize_f32` (C <= 128) / `shasta_bn_maps_finalize_f32`.  One thread per channel,
a few hundred bytes read: the call is launch-bound, so many launches go between one pair of events and the figure is the time per launch
in a back-to-back stream of them.  One JSON line per (C, R).

    python tools/time_bn_sync.py [--channels 128 256] [--ranks 1 4 8] [--launches 2000] [--repeats 5]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from shasta_amd import hip  # noqa: E402


def per_launch_us(call, launches, repeats):
    """Median and spread over `repeats` windows of `launches` back-to-back calls, in microseconds per call."""
    for _ in range(200):
        call()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3 / launches)
    return round(float(np.median(out)), 3), round(min(out), 3), round(max(out), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--ranks", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = hip.load()
    s = hip.stream_ptr()
    g = torch.Generator().manual_seed(0)
    for C in a.channels:
        mm = torch.cat([torch.randn(C, generator=g), 5.0 + torch.rand(C, generator=g)]).to(dev)
        stat = torch.empty(2 * C, device=dev)
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        nbt = torch.zeros(1, dtype=torch.int64, device=dev)
        nbt_p = ctypes.c_void_p(nbt.data_ptr())
        plain = lib.shasta_bn_rows_finalize_f32 if lib.shasta_bn_rows_supported(C) else lib.shasta_bn_maps_finalize_f32
        args = (hip.ptr(mm), C, 1000.0, 1e-3, 0.01, hip.ptr(stat), hip.ptr(rm), hip.ptr(rv), nbt_p, s)
        base = per_launch_us(lambda: hip.check(plain(*args), "finalize"), a.launches, a.repeats)
        rb = lib.shasta_bn_sync_record_bytes(C)
        for R in a.ranks:
            rec = torch.zeros(R, rb, dtype=torch.uint8, device=dev)
            rec[:, :8 * C] = mm.view(torch.uint8)
            rec[:, 8 * C:].view(torch.int64).fill_(1000)
            sargs = (hip.ptr(rec), R, C, 1e-3, 0.01, hip.ptr(stat), None, None, hip.ptr(rm), hip.ptr(rv), nbt_p, s)
            sync = per_launch_us(lambda: hip.check(lib.shasta_bn_sync_finalize_f32(*sargs), "sync finalize"), a.launches, a.repeats)
            print(json.dumps(dict(tool="time_bn_sync", C=C, R=R, launches=a.launches, repeats=a.repeats,
                                  plain_finalize_us=dict(median=base[0], min=base[1], max=base[2]),
                                  sync_finalize_us=dict(median=sync[0], min=sync[1], max=sync[2]),
                                  device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
