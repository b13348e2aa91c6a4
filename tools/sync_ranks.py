"""`--sync-ranks N` of tools/time_backbone.py and tools/time_neck.py: the parent side (N fresh child processes of the same tool, one GPU
each, every run under its own time limit, nothing more started after a failure) and the child side (the RCCL process group)."""
import argparse
import datetime
import json
import os
import socket
import subprocess
import sys

import torch


def add_arguments(ap):
    ap.add_argument("--sync-ranks", type=int, default=0, help="time the train()-mode forward with batch statistics synchronised over N "
                    "ranks (sync_bn.convert_syncbn_model, RCCL): N fresh child processes, one GPU each")
    ap.add_argument("--sync-rank", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--sync-port", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--sync-timeout", type=int, default=600, help="seconds each child may take")


def parent(tool, a):
    """Start the children and wait for them; returns the exit status.  On a box with fewer GPUs than ranks nothing is started: two
    processes sharing one GPU do not give a time anybody should quote."""
    n = a.sync_ranks
    have = torch.cuda.device_count()
    if have < n:
        print(json.dumps(dict(tool=tool, sync_ranks=n, result="not measured: needs %d GPUs, this box has %d" % (n, have))))
        return 0
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    argv = [v for v in sys.argv[1:]]
    procs = [subprocess.Popen([sys.executable, sys.argv[0]] + argv + ["--sync-rank", str(r), "--sync-port", str(port)]) for r in range(n)]
    status = 0
    for p in procs:
        try:
            rc = p.wait(timeout=a.sync_timeout if status == 0 else 30)
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0 and status == 0:
            status = rc
            for q in procs:  # nothing goes on after a failure
                if q.poll() is None:
                    q.terminate()
    for p in procs:
        if p.poll() is None:
            p.kill()
    return status


def child(a):
    """This rank's device, with the process group initialised on it."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(a.sync_port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(a.sync_rank)
    dev = torch.device("cuda", a.sync_rank)
    dist.init_process_group("nccl", rank=a.sync_rank, world_size=a.sync_ranks, device_id=dev, timeout=datetime.timedelta(seconds=120))
    return dev


def timed_ms(fn, iters, warmup=3):
    """Mean ms per call between two events after a warm-up (every rank makes the same number of calls: the forward holds collectives)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters
