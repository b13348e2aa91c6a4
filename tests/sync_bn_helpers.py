"""Shared by tests/test_sync_bn_merge.py (CPU), tests/test_sync_bn_kernels.py and tests/test_sync_bn_modules.py (GPU): the float64
restatement of csrc/bn_sync.hip (the sequential merge of per-rank (mean, M2, n) records and the finalize), the byte layout of the records,
a helper that cuts a tensor into ragged per-rank parts, and the launcher of the two-process tests."""
import math
import os
import socket
import traceback

import numpy as np

EPS = float(np.float32(1e-3))


# ---- the arithmetic, in float64 -----------------------------------------------------------------------------------------
def part_stats64(values):
    """(mean, M2, n) per channel of one part: `values` is (n, C) rows or (B, C, plane) maps, any dtype; float64 statistics."""
    v = np.asarray(values, np.float64)
    if v.ndim == 3:
        v = v.transpose(1, 0, 2).reshape(v.shape[1], -1).T
    n, C = v.shape
    if n == 0:
        return np.zeros(C), np.zeros(C), 0
    # the mean as an exactly rounded sum (math.fsum): with |mean| = 1e4 x std, float64 summation error in a part's mean would enter the
    # merged M2 through d = mean_r - mean at the 1e-12 level the merge is compared at
    mean = np.array([math.fsum(col) for col in v.T]) / n
    return mean, ((v - mean) ** 2).sum(0), n


def merge64(records):
    """The sequential merge of csrc/bn_sync.hip in float64: records = [(mean (C,), M2 (C,), n)] in rank order, Chan's update one record
    at a time, records of count 0 skipped, the first non-empty record taken as it is.  Returns (mean, M2, N)."""
    N, mean, m2 = 0, None, None
    for mean_r, m2_r, n_r in records:
        n_r = int(n_r)
        if n_r == 0:
            continue
        mean_r, m2_r = np.asarray(mean_r, np.float64), np.asarray(m2_r, np.float64)
        if N == 0:
            N, mean, m2 = n_r, mean_r.copy(), m2_r.copy()
            continue
        d = mean_r - mean
        Nn = N + n_r
        mean = mean + d * float(n_r) / float(Nn)
        m2 = m2 + (m2_r + d * d * float(N) * float(n_r) / float(Nn))
        N = Nn
    return mean, m2, N


def finalize64(mean, m2, N, momentum, running_mean, running_var, eps=EPS):
    """What the finalize makes of the merged statistics rounded once to fp32: (stat mean, inverse std, running mean, running var) in
    float64 - biased variance for the normalisation, unbiased for the running statistics."""
    mean = np.asarray(mean, np.float32).astype(np.float64)
    m2 = np.asarray(m2, np.float32).astype(np.float64)
    inv = 1.0 / np.sqrt(m2 / N + eps)
    rm = (1 - momentum) * np.asarray(running_mean, np.float64) + momentum * mean
    rv = (1 - momentum) * np.asarray(running_var, np.float64) + momentum * m2 / (N - 1 if N > 1 else 1)
    return mean, inv, rm, rv


# ---- records ------------------------------------------------------------------------------------------------------------
def record_bytes(C):
    return 8 * C + 8


def pack_records(records, C):
    """The gathered buffer: per record fp32 mean[C], fp32 M2[C], int64 count; uint8 array of R (8 C + 8) bytes."""
    out = np.zeros((len(records), record_bytes(C)), np.uint8)
    for r, (mean, m2, n) in enumerate(records):
        out[r, :4 * C] = np.asarray(mean, np.float32).view(np.uint8)
        out[r, 4 * C:8 * C] = np.asarray(m2, np.float32).view(np.uint8)
        out[r, 8 * C:] = np.asarray([n], np.int64).view(np.uint8)
    return out.reshape(-1)


def unpack_records(buf, C):
    """[(mean fp32, M2 fp32, n)] of a gathered buffer (what the kernel reads)."""
    rows = np.asarray(buf, np.uint8).reshape(-1, record_bytes(C))
    return [(row[:4 * C].view(np.float32).copy(), row[4 * C:8 * C].view(np.float32).copy(), int(row[8 * C:].view(np.int64)[0])) for row in rows]


# ---- ragged parts -------------------------------------------------------------------------------------------------------
def ragged_split(values, sizes):
    """Cut (n, C) rows into parts of sizes[r] rows, or (B, C, plane) maps - taken as B * plane values per channel, image after image -
    into parts (1, C, sizes[r]).  sum(sizes) must be the number of rows / values per channel; a size may be 0."""
    v = np.asarray(values)
    flat = v if v.ndim == 2 else v.transpose(1, 0, 2).reshape(v.shape[1], -1).T  # (values, C)
    assert sum(sizes) == flat.shape[0], (sizes, flat.shape)
    parts, at = [], 0
    for k in sizes:
        p = flat[at:at + k]
        parts.append(np.ascontiguousarray(p if v.ndim == 2 else p.T[None]))
        at += k
    return parts


# ---- two-process tests --------------------------------------------------------------------------------------------------
def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, backend, body, args, q):
    """One rank: process group (ranks share GPU 0 over gloo, or one GPU each over nccl), the body, the result or the traceback."""
    try:
        import datetime
        import torch
        import torch.distributed as dist
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        gpu = rank if backend == "nccl" else 0
        torch.cuda.set_device(gpu)
        dev = torch.device("cuda", gpu)
        kw = dict(device_id=dev) if backend == "nccl" else {}
        dist.init_process_group(backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60), **kw)
        try:
            out = body(rank, world, dev, *args)
            torch.cuda.synchronize()
        finally:
            dist.destroy_process_group()
        q.put((rank, True, out))
    except BaseException:  # noqa: BLE001 - the parent shows the traceback and stops the other ranks
        q.put((rank, False, traceback.format_exc()))


def run_workers(body, world, backend="gloo", args=(), timeout=300):
    """`body(rank, world, device, *args)` in `world` fresh processes (spawn); returns {rank: result}.  A failing rank's traceback is
    raised here; on any failure (or no answer within `timeout` seconds) every child is terminated and nothing more is started."""
    import queue

    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, backend, body, args, q)) for r in range(world)]
    for p in procs:
        p.start()
    res, failure = {}, None
    try:
        for _ in procs:
            try:
                rank, ok, out = q.get(timeout=timeout)
            except queue.Empty:
                failure = "no answer from the ranks %s within %d s" % (sorted(set(range(world)) - set(res)), timeout)
                break
            if not ok:
                failure = "rank %d failed:\n%s" % (rank, out)
                break
            res[rank] = out
    finally:
        for p in procs:
            if failure is not None and p.is_alive():
                p.terminate()
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert failure is None, failure
    return res
