"""Multi-sweep cloud assembly (shasta_amd/sweeps.py, csrc/sweeps.hip) against the reference's loader and augmentation
(tests/golden/sweeps_golden.npz, made by tests/golden/make_sweeps_golden.py) and the numpy restatement tests/sweeps_helpers.py.

Rotated augmentation, measured on an MI355X: error / bar of the kernel is 0.504 (case r0) and 0.326 (r1) - it computes what the
restatement computes, bit for bit -, of the reference's BLAS product 0.504 at most; bar = 4u (|x c| + |y s|) |scale| + 3u |result|."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import sweeps_helpers as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweeps_golden.npz")
SENTINEL = 0x5EADBEEF


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


def _frame(G, k):
    n = int(G["nsweeps"][0])
    raws = [G["f%d_raw%d" % (k, i)] for i in range(n)]
    transforms = [m if has else None for m, has in zip(G["f%d_transforms" % k], G["f%d_has_transform" % k])]
    return raws, transforms, [float(v) for v in G["f%d_lags" % k]]


def _frame_segments(G, k, order, cloud=0):
    raws, transforms, lags = _frame(G, k)
    segs = [H.segment(len(raws[0]), cloud)] + [H.segment(len(raws[1 + i]), cloud, transforms[i], True, lags[i]) for i in order]
    return np.concatenate([raws[0]] + [raws[1 + i] for i in order]), segs


def _aug(G, name):
    from shasta_amd import sweeps
    fx, fy, tr = (bool(v) for v in G["aug_%s_flags" % name])
    p = G["aug_%s_params" % name]
    return sweeps.augment_entry(fx, fy, p[0], p[1], p[2:5] if tr else None)


# ------------------------------------------------------------------ CPU


def test_restatement_equals_the_reference_golden():
    """Assembly of both frames, flips, scale, translate and a rotation by 0: bit for bit."""
    G = golden()
    for k in range(int(G["n_frames"][0])):
        raw, segs = _frame_segments(G, k, G["f%d_order" % k])
        out, prefix = H.assemble(raw, segs, 1)
        assert np.array_equal(H.uint(out), H.uint(G["f%d_combined" % k])) and prefix.tolist() == [0, len(G["f%d_combined" % k])]
    names = [str(n) for n in G["aug_names"]]
    flat = [n for n in names if G["aug_%s_params" % n][0] == 0.0]
    assert len(flat) >= 3
    for n in flat:
        assert np.array_equal(H.uint(H.apply_augment(G["f0_combined"], _aug(G, n))), H.uint(G["aug_%s_points" % n])), n


def test_rotated_golden_reference_and_restatement_inside_the_bar():
    G = golden()
    rotated = [str(n) for n in G["aug_names"] if G["aug_%s_params" % str(n)][0] != 0.0]
    assert len(rotated) >= 2
    for n in rotated:
        a = _aug(G, n)
        want, bar = H.augment_f64(G["f0_combined"], a)
        for who, got in (("reference", G["aug_%s_points" % n]), ("restatement", H.apply_augment(G["f0_combined"], a))):
            ratio = (np.abs(got[:, :2].astype(np.float64) - want[:, :2]) / bar[:, :2]).max()
            print("%s %s: largest error / bar = %.3f" % (n, who, ratio))
            assert ratio <= 1.0
            assert np.array_equal(H.uint(got[:, 2]), H.uint(H.z_through_chain(G["f0_combined"], a)))
            assert np.array_equal(H.uint(got[:, 3:]), H.uint(G["f0_combined"][:, 3:]))


def test_golden_holds_the_cases_it_is_for():
    from shasta_amd import sweeps
    G, R = golden(), sweeps.ROWS_PER_BLOCK
    sizes = [len(G["f%d_raw%d" % (k, i)]) for k in range(2) for i in range(4)]
    assert 0 in sizes and 1 in sizes and R in sizes and R + 1 in sizes and max(sizes) > 2 * R
    assert len(G["f1_raw0"]) == 0  # an empty key frame
    for k in range(2):
        raws, transforms, _ = _frame(G, k)
        assert sum(len(r) for r in raws) > len(G["f%d_combined" % k]) > len(raws[0])  # some rows dropped, some sweep rows kept
        assert sorted(G["f%d_order" % k].tolist()) == [0, 1, 2] and G["f%d_order" % k].tolist() != [0, 1, 2]
    key = G["f0_raw0"]
    close = (np.abs(key[:, 0]) < 1) & (np.abs(key[:, 1]) < 1)
    assert close.any() and np.array_equal(H.uint(G["f0_combined"][:len(key), :4]), H.uint(key[:, :4]))  # the key frame is never filtered
    assert not G["f1_has_transform"].all() and G["f1_has_transform"].any() and G["f0_has_transform"].all()
    flags = np.stack([G["aug_%s_flags" % str(n)] for n in G["aug_names"]])
    assert all(flags[:, j].any() and not flags[:, j].all() for j in range(3))  # either flip and the translation: drawn and not drawn
    assert G["f0_combined"].dtype == np.float32 and G["pipe_points"].dtype == np.float32 and os.path.getsize(GOLDEN) < 1 << 20


def test_registry_and_constructor_surface():
    import shasta_amd
    from shasta_amd import sweeps
    assert shasta_amd.PIPELINES.name == "pipeline"
    assert shasta_amd.PIPELINES.get("LoadPointCloudFromFile") is sweeps.LoadPointCloudFromFile
    assert shasta_amd.PIPELINES.get("Preprocess") is sweeps.Preprocess
    step = shasta_amd.build_from_cfg(dict(type="LoadPointCloudFromFile", dataset="NuScenesDataset"), shasta_amd.PIPELINES)
    assert step.type == "NuScenesDataset" and step.random_select is False and step.npoints == 16834 and step.path_map is None
    assert sweeps.LoadPointCloudFromFile().type == "NuScenesDataset"
    with pytest.raises(NotImplementedError):
        sweeps.LoadPointCloudFromFile(dataset="WaymoDataset")(dict(lidar=dict(nsweeps=1)), dict())
    with pytest.raises(NotImplementedError):
        step(dict(lidar=dict(nsweeps=1), virtual=True), dict(lidar_path="x", sweeps=[]))
    with pytest.raises(AssertionError, match="nsweeps 3 should equal to list length 1."):
        sweeps.assemble_clouds([dict(lidar_path="x", sweeps=[dict()])], 3, "cuda")
    train = dict(mode="train", shuffle_points=True, global_rot_noise=[-0.3925, 0.3925], global_scale_noise=[0.95, 1.05], db_sampler=None,
                 class_names=["car"])
    p = sweeps.Preprocess(cfg=train)
    assert p.global_translate_std == 0 and p.min_points_in_gt == -1 and p.no_augmentation is False and p.db_sampler is None
    assert sweeps.Preprocess(cfg=dict(mode="val", shuffle_points=False)).mode == "val"
    with pytest.raises(NotImplementedError):
        sweeps.Preprocess(cfg=dict(train, db_sampler=dict(type="GT-AUG")))
    with pytest.raises(NotImplementedError):
        sweeps.Preprocess(cfg=dict(train, min_points_in_gt=5))
    feeder = sweeps.SweepClouds(dict(), 10)
    assert callable(feeder) and callable(feeder.batch) and feeder.nsweeps == 10


def test_cpu_use_raises():
    from shasta_amd import hip, sweeps
    with pytest.raises(hip.ShastaHipError):
        sweeps.assemble_clouds([dict(lidar_path="x", sweeps=[])], 1, "cpu")
    with pytest.raises(hip.ShastaHipError):
        sweeps.assemble_rows(torch.zeros(3, 5), [H.segment(3, 0)], 1)
    with pytest.raises(hip.ShastaHipError):
        sweeps.Preprocess(cfg=dict(mode="val", shuffle_points=False))(dict(type="NuScenesDataset", lidar=dict(combined=torch.zeros(3, 5))), None)


def test_draws_follow_the_reference_order_under_one_seed():
    """Sweep order, augmentation parameters and shuffle permutation from one seed, as the reference's loader and Preprocess drew them."""
    from shasta_amd import sweeps
    G = golden()
    seed, r0, r1, s0, s1, std = G["pipe_cfg"]
    np.random.seed(int(seed))
    order = np.random.choice(3, 3, replace=False)
    assert order.tolist() == G["pipe_order"].tolist()
    a = sweeps.draw_augment([r0, r1], [s0, s1], std)
    assert [a["flip_x"], a["flip_y"], a["translate"] is not None] == G["pipe_flags"].tolist()
    assert a["angle"] == G["pipe_params"][0] and a["scale"] == float(np.float32(G["pipe_params"][1])) and a["translate"] == G["pipe_params"][2:5].tolist()
    raw, segs = _frame_segments(G, 1, order)
    cloud = H.apply_augment(H.assemble(raw, segs, 1)[0], a)
    index = np.arange(len(cloud))
    np.random.shuffle(index)
    assert index.tolist() == G["pipe_index"].tolist()
    assert np.array_equal(H.uint(cloud[index]), H.uint(G["pipe_points"]))
    for n in (str(n) for n in G["aug_names"]):  # the four functions alone, every case's own seed
        np.random.seed(int(G["aug_%s_seed" % n][0]))
        cfg = G["aug_%s_cfg" % n]
        std = cfg[4:7].tolist() if len(set(cfg[4:7].tolist())) > 1 else float(cfg[4])
        assert sweeps.draw_augment(cfg[0:2].tolist(), cfg[2:4].tolist(), std) == _aug(G, n), n


def _call(lib, raw, total, raw_ndim, table, nseg, n, keep, out, cap, prefix, ws, wsb, radius=1.0, aug=None):
    return lib.shasta_sweeps_assemble_f32(raw, total, raw_ndim, table, nseg, n, keep, radius, aug, out, cap, prefix, ws, wsb, None)


def _refusals(lib, raw, out, prefix, ws, wsb):
    """(status, what) of every refusal, for 3 segments of 4 rows in 2 clouds; the pointers are never dereferenced."""
    from shasta_amd import sweeps
    ok = sweeps.segment_table([H.segment(4, 0), H.segment(4, 0, np.eye(4), True, 0.1), H.segment(4, 1)])
    back = sweeps.segment_table([H.segment(4, 1), H.segment(4, 0), H.segment(4, 1)])
    high = sweeps.segment_table([H.segment(4, 0), H.segment(4, 1), H.segment(4, 2)])
    short = sweeps.segment_table([H.segment(4, 0), H.segment(3, 0), H.segment(4, 1)])
    many = sweeps.segment_table([H.segment(0, 0)] * 1025)
    return [
        (_call(lib, raw, 12, 5, None, 3, 2, 4, out, 12, prefix, ws, wsb), -1, "null segments"),
        (_call(lib, raw, 12, 5, ok, 3, 2, 4, out, 12, None, ws, wsb), -1, "null prefix"),
        (_call(lib, raw, 12, 5, ok, 3, 2, 4, out, 12, prefix, None, wsb), -1, "null workspace"),
        (_call(lib, None, 12, 5, ok, 3, 2, 4, out, 12, prefix, ws, wsb), -1, "null rows"),
        (_call(lib, raw, 12, 5, ok, 3, 2, 4, None, 12, prefix, ws, wsb), -1, "null out"),
        (_call(lib, raw, 12, 5, ok, 3, 33, 4, out, 12, prefix, ws, wsb), -1, "33 clouds"),
        (_call(lib, raw, 12, 5, ok, 3, 0, 4, out, 12, prefix, ws, wsb), -1, "no cloud"),
        (_call(lib, raw, 0, 5, many, 1025, 2, 4, out, 12, prefix, ws, wsb), -1, "1025 segments"),
        (_call(lib, raw, 12, 5, ok, 0, 2, 4, out, 12, prefix, ws, wsb), -1, "no segment"),
        (_call(lib, raw, 12, 5, back, 3, 2, 4, out, 12, prefix, ws, wsb), -1, "cloud indices decrease"),
        (_call(lib, raw, 12, 5, high, 3, 2, 4, out, 12, prefix, ws, wsb), -1, "cloud index beyond num_clouds"),
        (_call(lib, raw, 12, 5, ok, 3, 2, 0, out, 12, prefix, ws, wsb), -1, "keep 0"),
        (_call(lib, raw, 12, 5, ok, 3, 2, 6, out, 12, prefix, ws, wsb), -1, "keep beyond raw_ndim"),
        (_call(lib, raw, 12, 5, ok, 3, 2, 4, out, 11, prefix, ws, wsb), -1, "capacity below total_rows"),
        (_call(lib, raw, 12, 5, short, 3, 2, 4, out, 12, prefix, ws, wsb), -1, "rows do not sum to total_rows"),
        (_call(lib, raw, 12, 2, ok, 3, 2, 2, out, 12, prefix, ws, wsb), -5, "raw_ndim 2"),
        (_call(lib, raw, 12, 9, ok, 3, 2, 4, out, 12, prefix, ws, wsb), -5, "raw_ndim 9"),
        (_call(lib, raw, 12, 5, ok, 3, 2, 4, out, 12, prefix, ws, wsb - 1), -2, "short workspace"),
        (_call(lib, raw, 12, 5, ok, 3, 2, 4, out, 12, prefix, C.c_void_p(ws.value + 4), wsb), -4, "workspace not aligned"),
    ]


def test_size_queries_and_refusals_need_no_gpu():
    from shasta_amd import hip
    lib = hip.load()
    q = lib.shasta_sweeps_workspace_bytes
    assert q(0, 10) == 0 and q(1025, 10) == 0 and q(1, -1) == 0 and q(1, 1 << 31) == 0
    assert 0 < q(1, 0) <= q(10, 347200) < q(10, 3472000) and q(10, 347200) < q(1024, 347200) and q(10, 347200) < 1 << 20
    host = (C.c_char * 4096)()  # stands in for every device pointer: a refusal comes before anything is touched
    p = C.c_void_p(C.addressof(host) + (-C.addressof(host)) % 16)
    wsb = q(3, 12)
    for got, want, what in _refusals(lib, p, p, p, p, wsb):
        assert got == want, what
        assert lib.shasta_last_error()
    assert bytes(host) == bytes(4096)


# ------------------------------------------------------------------ GPU


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda", 0)


def _rows(rng, n, kind):
    """(n, 5) fp32 rows: 'close' inside the 1 m square, 'far' outside it, 'mix' both."""
    xy = rng.uniform(-0.99, 0.99, (n, 2)) if kind == "close" else rng.uniform(1.5, 50, (n, 2)) * rng.choice([-1.0, 1.0], (n, 2))
    if kind == "mix":
        xy = np.where(rng.uniform(size=(n, 1)) < 0.4, rng.uniform(-0.99, 0.99, (n, 2)), xy)
    return np.concatenate([xy, rng.uniform(-3, 2, (n, 1)), rng.integers(0, 256, (n, 1)), rng.integers(0, 32, (n, 1))], axis=1).astype(np.float32)


def _bits(u):
    return np.array([u], np.uint32).view(np.float32)[0]


@functools.lru_cache(maxsize=None)
def _seams():
    """Three clouds at the compaction's seams, R = rows per block of the count pass.  Per cloud: key rows, [(rows, transform, lag)]."""
    from shasta_amd import sweeps
    R, rng = sweeps.ROWS_PER_BLOCK, np.random.default_rng(7)
    T = [np.array([[np.cos(a), -np.sin(a), 0.01, tx], [np.sin(a), np.cos(a), -0.02, ty], [-0.01, 0.02, 1.0, tz], [0, 0, 0, 1]], np.float64)
         for a, tx, ty, tz in ((0.3, 1.5, -0.25, 0.1), (-2.0, -0.7, 3.1, -0.05), (1.1, 0.01, 0.02, 0.4), (3.0, 2.0, 2.0, 0.0))]
    nan, close = np.float32(np.nan), [0.5, -0.25]
    edge = _rows(rng, R + 1, "mix")
    edge[[0, R - 1, R], :2] = close  # first and last row of a block and the first of the next are dropped
    big = _rows(rng, 2 * R + 3, "far")
    big[[0, R - 1], :2] = close                      # first and last row of block 0
    big[2 * R - 3:2 * R + 3, :2] = close             # a dropped run across the seam of blocks 1 and 2
    big[2 * R + 2, :2] = [30.0, -30.0]               # (the very last row stays)
    big[5, :2], big[6, :2], big[7, :2] = [1.0, 0.5], [-1.0, -0.5], [0.5, -1.0]   # |x| or |y| exactly the radius: stays
    big[8, :2], big[9, :2] = [-0.0, 0.5], [-0.0, 40.0]                        # -0.0: close and dropped; far and transformed
    big[10, :3], big[11, :3], big[12, :3] = [nan, 0.5, 1.0], [0.5, nan, 1.0], [20.0, 0.5, nan]  # a NaN in x, in y (both stay), in z
    plain = _rows(rng, R, "far")  # no transform, nothing dropped, between two transformed segments
    plain[3, :3] = [-0.0, 2.0, -0.0]
    plain[4, :3] = [_bits(0x7FC12345), 0.5, 1.0]    # NaN payloads survive the copy
    plain[5, :3] = [0.5, _bits(0xFFC00001), 1.0]
    plain[6, :3] = [7.0, 8.0, _bits(0x7F800001)]
    plain[7, :2] = [1.0, -1.0]
    odd = _rows(rng, 5, "far")
    odd[0, :3], odd[1, :3], odd[2, :2] = [-0.0, -0.0, -0.0], [_bits(0xFFFFFFFF), 0.1, 0.2], close
    cloud0 = (_rows(rng, R + 1, "close"),  # a key frame full of close points that all stay
              [(_rows(rng, 0, "far"), T[0], 0.05), (_rows(rng, 1, "close"), T[1], 0.1), (_rows(rng, R - 1, "mix"), T[2], 0.15),
               (plain, None, 0.2), (edge, T[3], 0.25), (big, T[0], 0.3)])
    cloud1 = (_rows(rng, 70, "mix"), [])   # key frame only
    cloud2 = (_rows(rng, 0, "far"),        # an empty key frame
              [(_rows(rng, R, "close"), T[1], 0.05),  # every row dropped
               (odd, None, 0.1), (_rows(rng, 40, "mix"), T[2], 0.45), (_rows(rng, R + 1, "far"), T[3], 0.5)])  # none dropped
    return [cloud0, cloud1, cloud2]


def _flatten(clouds, orders=None):
    raws, segs = [], []
    for c, (key, sweeps_) in enumerate(clouds):
        raws.append(key)
        segs.append(H.segment(len(key), c))
        for i in (range(len(sweeps_)) if orders is None else orders[c]):
            rows, transform, lag = sweeps_[i]
            raws.append(rows)
            segs.append(H.segment(len(rows), c, transform, True, lag))
    return np.concatenate(raws), segs


def _run_abi(raw, segs, n, keep=4, augment=None, extra=7):
    """One call through the C ABI into a sentinel-filled output.  -> (out as uint32 (capacity, keep + 1), prefix)."""
    from shasta_amd import hip, sweeps
    lib, dev = hip.load(), _dev()
    total = len(raw)
    d_raw = torch.from_numpy(np.ascontiguousarray(raw)).to(dev)
    out = torch.full((total + extra, keep + 1), SENTINEL, dtype=torch.int32, device=dev)
    prefix = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    wsb = lib.shasta_sweeps_workspace_bytes(len(segs), total)
    ws = torch.empty(wsb // 4, dtype=torch.int32, device=dev)
    hip.check(lib.shasta_sweeps_assemble_f32(hip.ptr(d_raw), total, raw.shape[1], sweeps.segment_table(segs), len(segs), n, keep, 1.0,
                                             sweeps.augment_table(augment, n), hip.ptr(out), total + extra, hip.ptr(prefix), hip.ptr(ws), wsb,
                                             hip.stream_ptr()), "shasta_sweeps_assemble_f32")
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32), prefix.cpu().numpy()


def _check(got, prefix, want, want_prefix):
    assert prefix.tolist() == want_prefix.tolist()
    k = int(want_prefix[-1])
    assert len(want) == k
    bad = np.argwhere(got[:k] != H.uint(want))
    assert len(bad) == 0, "first differing (row, column): %s of %d" % (bad[:5].tolist(), len(bad))
    assert (got[k:] == SENTINEL).all(), "rows at and beyond prefix[n] were written"


@pytest.mark.gpu
def test_seams_through_the_c_abi_bit_for_bit():
    clouds = _seams()
    raw, segs = _flatten(clouds)
    want, want_prefix = H.assemble(raw, segs, 3)
    sizes = [s[0] for s in segs]
    R = 256
    assert {0, 1, R - 1, R, R + 1, 2 * R + 3} <= set(sizes)
    assert want_prefix[1] - want_prefix[0] > R + 1 and want_prefix[2] - want_prefix[1] == 70 and want_prefix[3] > want_prefix[2]
    got, prefix = _run_abi(raw, segs, 3)
    _check(got, prefix, want, want_prefix)
    again, prefix2 = _run_abi(raw, segs, 3)
    assert np.array_equal(got, again) and np.array_equal(prefix, prefix2)  # the same bits on every run
    # one cloud more than segments reach (a cloud without a segment), and a narrower cut of the columns
    want4, prefix4 = H.assemble(raw, segs, 4)
    _check(*_run_abi(raw, segs, 4), want4, prefix4)
    want3, prefix3 = H.assemble(raw, segs, 3, keep=3)
    _check(*_run_abi(raw, segs, 3, keep=3), want3, prefix3)


@pytest.mark.gpu
def test_second_trip_of_the_block_count_scan_bit_for_bit():
    """Cloud 0 is 257 blocks: the scan of the block counts makes a second trip of its carry loop.  Its sweep holds blocks 255 and 256 - it
    straddles the two trips - with dropped rows at both ends of block 255 and in the one row of block 256; cloud 1 is block 257, so
    prefix[1] is read at a block of the second trip and prefix[2] is the carry after it."""
    R, rng = 256, np.random.default_rng(11)
    close = [0.5, -0.25]
    key = _rows(rng, 255 * R, "mix")     # blocks 0 .. 254; the key frame is never filtered
    sweep = _rows(rng, R + 1, "far")     # blocks 255 and 256
    sweep[[0, R - 1, R], :2] = close
    T = np.array([[0.8, -0.6, 0.0, 1.5], [0.6, 0.8, 0.0, -0.25], [0.0, 0.0, 1.0, 0.1], [0, 0, 0, 1]], np.float64)
    raw, segs = _flatten([(key, [(sweep, T, 0.05)]), (_rows(rng, 70, "mix"), [])])
    want, want_prefix = H.assemble(raw, segs, 2)
    assert [s[0] for s in segs] == [255 * R, R + 1, 70]
    assert want_prefix.tolist() == [0, 255 * R + R - 2, 255 * R + R - 2 + 70]
    got, prefix = _run_abi(raw, segs, 2)
    _check(got, prefix, want, want_prefix)
    again, prefix2 = _run_abi(raw, segs, 2)
    assert np.array_equal(got, again) and np.array_equal(prefix, prefix2)


@pytest.mark.gpu
def test_empty_inputs_through_the_c_abi():
    raw = np.zeros((0, 5), np.float32)
    got, prefix = _run_abi(raw, [H.segment(0, 0), H.segment(0, 1, np.eye(4), True, 0.1)], 2)
    assert prefix.tolist() == [0, 0, 0] and (got == SENTINEL).all()


@pytest.mark.gpu
def test_seams_through_assemble_clouds(tmp_path):
    from shasta_amd import sweeps
    clouds = [(key, list(sw) + [(np.zeros((0, 5), np.float32), None, 0.0)] * (6 - len(sw))) for key, sw in _seams()]
    infos = [H.frame_info(tmp_path, "c%d" % c, key, [s[0] for s in sw], [s[1] for s in sw], [s[2] for s in sw])
             for c, (key, sw) in enumerate(clouds)]
    np.random.seed(5)
    orders = [np.random.choice(6, 6, replace=False) for _ in clouds]
    raw, segs = _flatten(clouds, orders)
    want, want_prefix = H.assemble(raw, segs, 3)
    np.random.seed(5)
    points, offsets = sweeps.assemble_clouds(infos, 7, _dev())
    assert offsets == want_prefix.tolist() and points.shape == (len(want), 5) and points.is_cuda
    assert np.array_equal(H.uint(points.cpu().numpy()), H.uint(want))
    np.random.seed(5)
    again, _ = sweeps.assemble_clouds(infos, 7, _dev(), path_map=lambda p: p.replace("nowhere", "elsewhere"))
    assert torch.equal(points.view(torch.int32), again.view(torch.int32))


@pytest.mark.gpu
def test_reference_golden_through_the_loader(tmp_path):
    """`combined` of the reference's LoadPointCloudFromFile, bit for bit, under the same seed; `points` and `times` are views of it."""
    import shasta_amd
    G = golden()
    step = shasta_amd.build_from_cfg(dict(type="LoadPointCloudFromFile", dataset="NuScenesDataset"), shasta_amd.PIPELINES)
    for k in range(2):
        raws, transforms, lags = _frame(G, k)
        info = H.frame_info(tmp_path, "f%d" % k, raws[0], raws[1:], transforms, lags)
        np.random.seed(int(G["f%d_load_seed" % k][0]))
        res, _ = step(dict(lidar=dict(nsweeps=4), virtual=False), info)
        lidar = res["lidar"]
        assert res["type"] == "NuScenesDataset" and lidar["combined"].is_cuda
        assert np.array_equal(H.uint(lidar["combined"].cpu().numpy()), H.uint(G["f%d_combined" % k]))
        assert lidar["points"].shape[1] == 4 and lidar["times"].shape[1] == 1
        assert lidar["points"].data_ptr() == lidar["combined"].data_ptr() and lidar["times"].data_ptr() == lidar["combined"][:, 4:].data_ptr()


@pytest.mark.gpu
def test_augmentation_against_the_golden():
    """Without rotation (angle 0): the reference's bits.  With rotation: inside the bar against float64, z bit-equal."""
    G = golden()
    cloud = G["f0_combined"]
    seg5 = [H.segment(len(cloud), 0)]
    worst = 0.0
    for n in (str(n) for n in G["aug_names"]):
        a = _aug(G, n)
        got, prefix = _run_abi(cloud, seg5, 1, keep=5, augment=[a])  # (the cloud's own five columns, a sixth of time lag 0 behind them)
        assert prefix.tolist() == [0, len(cloud)] and (got[len(cloud):] == SENTINEL).all()
        got = got[:len(cloud), :5]
        ref = G["aug_%s_points" % n]
        assert np.array_equal(got, H.uint(H.apply_augment(cloud, a))), n  # the kernel computes what the restatement computes
        if a["angle"] == 0.0:
            assert np.array_equal(got, H.uint(ref)), n
            continue
        want, bar = H.augment_f64(cloud, a)
        ratio = (np.abs(got.view(np.float32)[:, :2].astype(np.float64) - want[:, :2]) / bar[:, :2]).max()
        print("%s kernel: largest error / bar = %.3f" % (n, ratio))
        worst = max(worst, ratio)
        assert ratio <= 1.0, n
        assert np.array_equal(got[:, 2], H.uint(H.z_through_chain(cloud, a))) and np.array_equal(got[:, 2:], H.uint(ref)[:, 2:]), n
    assert worst > 0.0


@pytest.mark.gpu
def test_augmentation_in_the_assembly_pass_and_the_pipeline(tmp_path):
    """The augmentation block in the same write pass as the assembly (assemble_clouds(augment=...)), and the reference's whole train-mode
    pipeline - loader, Preprocess with shuffle - under one seed, bit for bit."""
    import shasta_amd
    from shasta_amd import sweeps
    G = golden()
    infos = []
    for k in range(2):
        raws, transforms, lags = _frame(G, k)
        infos.append(H.frame_info(tmp_path, "f%d" % k, raws[0], raws[1:], transforms, lags))
    a0, a2 = _aug(G, "a0"), _aug(G, "a2")
    np.random.seed(100)
    order0 = np.random.choice(3, 3, replace=False)
    order1 = np.random.choice(3, 3, replace=False)
    np.random.seed(100)
    points, off = sweeps.assemble_clouds(infos, 4, _dev(), augment=[a0, None])
    assert order0.tolist() == G["f0_order"].tolist()
    assert np.array_equal(H.uint(points[:off[1]].cpu().numpy()), H.uint(G["aug_a0_points"]))
    raw1, segs1 = _frame_segments(G, 1, order1)
    plain1 = H.assemble(raw1, segs1, 1, augment=[None])[0]
    assert np.array_equal(H.uint(points[off[1]:].cpu().numpy()), H.uint(plain1))
    np.random.seed(100)
    points2, _ = sweeps.assemble_clouds(infos, 4, _dev(), augment=[a2, a0])
    assert np.array_equal(H.uint(points2[:off[1]].cpu().numpy()), H.uint(G["aug_a2_points"]))
    assert np.array_equal(H.uint(points2[off[1]:].cpu().numpy()), H.uint(H.apply_augment(plain1, a0)))
    seed, r0, r1, s0, s1, std = G["pipe_cfg"]
    load = shasta_amd.build_from_cfg(dict(type="LoadPointCloudFromFile", dataset="NuScenesDataset"), shasta_amd.PIPELINES)
    prep = shasta_amd.build_from_cfg(dict(type="Preprocess", cfg=dict(mode="train", shuffle_points=True, global_rot_noise=[r0, r1],
                                                                     global_scale_noise=[s0, s1], global_translate_std=std, db_sampler=None,
                                                                     class_names=["car"])), shasta_amd.PIPELINES)
    np.random.seed(int(seed))
    res, info = load(dict(lidar=dict(nsweeps=4), virtual=False), infos[1])
    res, info = prep(res, info)
    assert res["mode"] == "train" and np.array_equal(H.uint(res["lidar"]["points"].cpu().numpy()), H.uint(G["pipe_points"]))
    val = sweeps.Preprocess(cfg=dict(mode="val", shuffle_points=False))
    res, _ = val(res, info)
    assert res["lidar"]["points"] is res["lidar"]["combined"]


@pytest.mark.gpu
def test_cloudmaps_with_sweepclouds_equals_a_callable_of_the_restatement(tmp_path):
    import shasta_amd
    from shasta_amd import sweeps
    from shasta_amd.backbone import SpMiddleResNetFHD
    from tests import backbone_helpers as BH
    from tests.neck_helpers import SHIPPED, randomize_bn
    G, dev = golden(), _dev()
    torch.manual_seed(61)
    bev = shasta_amd.build_bev(dict(type="BEVMap", reader=dict(type="DynamicVoxelEncoder", pc_range=[-54, -54, -5, 54, 54, 3],
                                                                voxel_size=[0.5625, 0.5625, 0.2]),
                                    backbone=dict(type=SpMiddleResNetFHD, num_input_features=5, ds_factor=8), neck=dict(type="RPN", **SHIPPED))).eval()
    BH.randomize(bev.backbone, torch.Generator().manual_seed(62))
    randomize_bn(bev.neck, torch.Generator().manual_seed(63))
    bev = bev.to(dev)
    infos, tokens = {}, ["t0", "t1", "t2"]
    for t, k in zip(tokens, (0, 1, 0)):
        raws, transforms, lags = _frame(G, k)
        infos[t] = H.frame_info(tmp_path, t, raws[0], raws[1:], transforms, lags)
    np.random.seed(9)
    orders = [np.random.choice(3, 3, replace=False) for _ in tokens]
    restated = {t: H.assemble(*_frame_segments(G, k, o), 1)[0] for t, k, o in zip(tokens, (0, 1, 0), orders)}
    want = shasta_amd.CloudMaps(bev, lambda t: restated[t], max_clouds=2).neck_batch(tokens, dev)
    np.random.seed(9)
    got = shasta_amd.CloudMaps(bev, sweeps.SweepClouds(infos, 4), max_clouds=2).neck_batch(tokens, dev)
    assert got.shape[0] == 3 and float(got.abs().max()) > 0 and torch.equal(got, want)
    np.random.seed(9)
    one = sweeps.SweepClouds(infos, 4)("t0")
    assert np.array_equal(H.uint(one.cpu().numpy()), H.uint(restated["t0"]))


@pytest.mark.gpu
def test_every_refusal_returns_its_status_and_leaves_out_untouched():
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    raw = torch.rand(12, 5, device=dev) + 2.0
    out = torch.full((12, 5), SENTINEL, dtype=torch.int32, device=dev)
    prefix = torch.full((3,), -1, dtype=torch.int32, device=dev)
    wsb = lib.shasta_sweeps_workspace_bytes(3, 12)
    ws = torch.empty(wsb // 4 + 8, dtype=torch.int32, device=dev)
    for got, want, what in _refusals(lib, hip.ptr(raw), hip.ptr(out), hip.ptr(prefix), hip.ptr(ws), wsb):
        assert got == want, what
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((prefix == -1).all())
