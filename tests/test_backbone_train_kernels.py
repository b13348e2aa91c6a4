"""GPU: the sparse backbone in train() mode - the kernels of csrc/bn_rows.hip through the C ABI, and `SpMiddleResNetFHD` built with
`batch_statistics=True`, against float64 and the batch-statistics dense restatement of tests/backbone_train_helpers.py.

Seams of the kernels: the statistics pass gives a workgroup a slice of at least 64 rows and runs 512 slices at most (n below one slice,
n between, n beyond 512 x 64 where the slices grow; a slice may be empty), a workgroup is 256 / C row groups with eight rows in flight;
the apply pass handles 1024 / C rows per workgroup pass and 8192 workgroups at most (beyond: its grid-stride loop)."""
import contextlib
import copy
import functools

import numpy as np
import pytest
import torch

from tests import backbone_helpers as BH
from tests import backbone_train_helpers as BT
from tests import test_backbone_kernels as TK
from tests.backbone_helpers import GEOMETRIES

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
EPS = float(np.float32(1e-3))
WIDTHS = (16, 32, 64, 128)
SLICES, ROWS_MIN = 512, 64  # csrc/bn_rows.hip: BNR_SLICES, BNR_ROWS_MIN
LEVELS = ("conv1", "conv2", "conv3", "conv4")


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda", 0)


def _stats(lib, hip, y, C):
    """mean_m2 of the rows y through the C ABI, into a sentinel-tailed buffer."""
    dev = y.device
    ws = torch.empty(lib.shasta_bn_rows_workspace_bytes(C), dtype=torch.uint8, device=dev)
    mm = torch.full((2 * C + 4,), SENTINEL, device=dev)
    rc = lib.shasta_bn_rows_stats_f32(hip.ptr(y), y.shape[0], C, hip.ptr(mm), hip.ptr(ws), ws.numel(), hip.stream_ptr())
    assert rc == 0, lib.shasta_last_error()
    mm = mm.cpu()
    assert bool((mm[2 * C:] == SENTINEL).all())
    return mm[:2 * C]


# ---- 1. statistics ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", WIDTHS)
def test_stats_vs_float64(C):
    """Bars from the float64 accumulation: the mean is one fp32 rounding of a float64 quotient (2^-24; 2^-22 leaves room for the sum's
    own error against the channel's rms), M2 = sum y^2 - (sum y) mean carries the sums' error n 2^-53 sum y^2 at most, twice."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    big = SLICES * ROWS_MIN + 77
    assert big > SLICES * 32
    for n in (1, 2, 63, 129, 4097, big):
        g = torch.Generator().manual_seed(1000 * C + n % 997)
        y = torch.randn(n, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
        y[:, 3] = 1e3 + 0.1 * torch.randn(n, generator=g)  # mean 1e3, standard deviation 0.1: sum y^2 - (sum y) mean cancels 8 digits
        y64 = y.double()
        mean = y64.mean(0)
        m2 = ((y64 - mean) ** 2).sum(0)
        sq = (y64 ** 2).sum(0)
        yd = y.to(dev)
        got = _stats(lib, hip, yd, C).double()
        e_mean, e_m2 = (got[:C] - mean).abs(), (got[C:] - m2).abs()
        bar_mean = 2.0 ** -22 * torch.maximum(mean.abs(), (sq / n).sqrt())
        bar_m2 = 2.0 ** -22 * m2 + n * 2.0 ** -52 * sq
        print("C %d n %d: mean err / bar %.3f, M2 err / bar %.3f (cancelling channel: M2 %.4g, err %.3e, bar %.3e)"
              % (C, n, float((e_mean / bar_mean).max()), float((e_m2 / bar_m2).max()), float(m2[3]), float(e_m2[3]), float(bar_m2[3])))
        assert bool((e_mean <= bar_mean).all()) and bool((e_m2 <= bar_m2).all()), n
        assert bool((got[C:] >= 0).all())
        assert torch.equal(_stats(lib, hip, yd, C).double(), got)  # the same bits on a second run


# ---- 2. finalize --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", WIDTHS)
def test_finalize_vs_float64(C):
    from shasta_amd import hip
    import ctypes
    lib, dev = hip.load(), _dev()
    g = torch.Generator().manual_seed(C)
    n, mom = 37, 0.1
    mm = torch.cat([0.5 + torch.rand(C, generator=g), 5.0 + 50.0 * torch.rand(C, generator=g)])  # mean > 0, M2 > 0
    rm0, rv0 = 0.2 + torch.rand(C, generator=g), 0.5 + torch.rand(C, generator=g)                  # running mean > 0: no cancellation
    mmd = mm.to(dev)
    stat = torch.full((2 * C + 4,), SENTINEL, device=dev)
    rm, rv = rm0.to(dev), rv0.to(dev)
    nbt = torch.tensor(5, dtype=torch.int64, device=dev)
    rc = lib.shasta_bn_rows_finalize_f32(hip.ptr(mmd), C, float(n), EPS, mom, hip.ptr(stat), hip.ptr(rm), hip.ptr(rv),
                                         ctypes.c_void_p(nbt.data_ptr()), hip.stream_ptr())
    assert rc == 0, lib.shasta_last_error()
    stat_c = stat.cpu()
    assert bool((stat_c[2 * C:] == SENTINEL).all()) and torch.equal(stat_c[:C], mm[:C])
    mean64, m264 = mm[:C].double(), mm[C:].double()
    np.testing.assert_allclose(stat_c[C:2 * C].double().numpy(), (1.0 / torch.sqrt(m264 / n + EPS)).numpy(), rtol=2.0 ** -22, atol=0)
    np.testing.assert_allclose(rm.cpu().double().numpy(), ((1 - mom) * rm0.double() + mom * mean64).numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(rv.cpu().double().numpy(), ((1 - mom) * rv0.double() + mom * m264 / (n - 1)).numpy(), rtol=1e-6, atol=0)
    assert int(nbt) == 6
    # NULL running pointers: nothing but stat is written
    stat2 = torch.full((2 * C + 4,), SENTINEL, device=dev)
    rm1, rv1 = rm.clone(), rv.clone()
    rc = lib.shasta_bn_rows_finalize_f32(hip.ptr(mmd), C, float(n), EPS, mom, hip.ptr(stat2), None, None, None, hip.stream_ptr())
    assert rc == 0, lib.shasta_last_error()
    assert torch.equal(stat2, stat) and torch.equal(rm, rm1) and torch.equal(rv, rv1) and int(nbt) == 6 and torch.equal(mmd.cpu(), mm)


# ---- 3. apply -----------------------------------------------------------------------------------------------------
def _apply_case(lib, hip, dev, C, n, g):
    y = torch.randn(n, C, generator=g) * 2.0 + 0.5
    y[n // 2, C // 2] = float("nan")  # a NaN stays a NaN through the ReLU
    res = torch.randn(n, C, generator=g)
    stat = torch.cat([0.5 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)])
    gamma, beta = 0.5 + torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)
    t = (y.double() - stat[:C].double()) * stat[C:].double() * gamma.double()
    sd, gd, bd = stat.to(dev), gamma.to(dev), beta.to(dev)
    pad = torch.full((3, C), SENTINEL)

    def check(relu, with_res, alias):
        ref = t + beta.double() + (res.double() if with_res else 0.0)
        if relu:
            ref = torch.relu(ref)
        bar = 8 * 2.0 ** -24 * (t.abs() + beta.double().abs() + (res.double().abs() if with_res else 0.0))
        yb, rb = torch.cat([y, pad]).to(dev), (torch.cat([res, pad]).to(dev) if with_res else None)
        out = {"none": torch.full((n + 3, C), SENTINEL, device=dev), "y": yb, "residual": rb}[alias]
        rc = lib.shasta_bn_rows_apply_f32(hip.ptr(yb), n, C, hip.ptr(sd), hip.ptr(gd), hip.ptr(bd), hip.ptr(rb), relu, hip.ptr(out),
                                          hip.stream_ptr())
        assert rc == 0, lib.shasta_last_error()
        o = out.cpu()
        assert bool((o[n:] == SENTINEL).all()), "rows >= n were written"
        got = o[:n].double()
        nan = torch.isnan(ref)
        assert int(nan.sum()) == 1 and bool(torch.isnan(got[nan]).all()) and not bool(torch.isnan(got[~nan]).any())
        err = (got - ref).abs()[~nan]
        ratio = float((err / bar[~nan].clamp_min(1e-300)).max())
        assert bool((err <= bar[~nan]).all()), (C, n, relu, with_res, alias, ratio)
        if relu:
            assert bool((got[~nan] >= 0).all())
        if n * C >= 1024:  # enough values for both signs: the ReLU clips a share of them, and only the ReLU does
            assert float((got[~nan] == 0).double().mean()) > 0.05 if relu else float(got[~nan].min()) < -0.1
        return ratio

    worst = 0.0
    for relu in (0, 1):
        for with_res in (False, True):
            worst = max(worst, check(relu, with_res, "none"))
    worst = max(worst, check(1, True, "y"), check(1, True, "residual"), check(0, False, "y"))
    return worst


@pytest.mark.parametrize("C", WIDTHS)
def test_apply_vs_float64(C):
    """relu x residual, out aliasing y and residual, n that is no multiple of the 1024 / C rows of a workgroup pass, sentinel rows after n;
    against float64 of the same formula from the same fp32 stat.  Bar: three roundings on the product chain and one per addition - 8 ulp of
    the magnitudes added is generous and still far below a wrong operand."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    g = torch.Generator().manual_seed(7 * C)
    rows = 1024 // C
    for n in (1, rows - 1, 3 * rows + 5):
        print("C %d n %d: worst err / bar %.3f" % (C, n, _apply_case(lib, hip, dev, C, n, g)))


def test_apply_beyond_one_grid():
    """More row quads than 8192 workgroups of 256 threads hold: the grid-stride loop."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    C = 128
    n = 8192 * 256 * 4 // C + 37
    print("C %d n %d: worst err / bar %.3f" % (C, n, _apply_case(lib, hip, dev, C, n, torch.Generator().manual_seed(5))))


# ---- 4. raw pack --------------------------------------------------------------------------------------------------
RAW_CASES = [  # cin, cout, geometry, bias, B, grid, input rows: one per served channel-pair class, K = 27 and K = 3
    (5, 16, "subm", False, 2, (6, 10, 12), 300), (16, 16, "subm", True, 2, (6, 10, 12), 129), (32, 32, "subm", True, 1, (6, 10, 12), 129),
    (64, 64, "subm", True, 2, (5, 8, 9), 200), (128, 128, "subm", True, 1, (5, 8, 9), 257), (16, 32, "k3s2p1", False, 2, (9, 12, 13), 200),
    (32, 64, "k3s2p1", False, 1, (11, 12, 12), 150), (64, 128, "k3s2p011", False, 2, (11, 8, 9), 150),
    (128, 128, "k311s211p0", False, 2, (5, 9, 8), 300),
]


@pytest.mark.parametrize("cin,cout,gname,with_bias,B,grid,n", RAW_CASES, ids=["%d-%d-%s" % (c[0], c[1], c[2]) for c in RAW_CASES])
def test_raw_pack_layer_vs_float64(cin, cout, gname, with_bias, B, grid, n):
    """shasta_spconv_layer_f32 on a raw pack, no residual, no ReLU = sum_t W_t x + bias.  Bar: test_layer_vs_float64's."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    geom, subm = GEOMETRIES[gname], gname == "subm"
    K = int(np.prod(geom[0]))
    g = torch.Generator().manual_seed(100 * cin + cout + n + 1)
    coords = BH.random_voxels(np.random.RandomState(cin + n + 1), B, grid, n)
    x = torch.randn(n, cin, generator=g)
    w, bias, _ = TK._layer_tensors(cin, cout, geom[0], with_bias, g)
    xd, mask = BH.to_dense(x.double(), coords, B, grid)
    yd, mo = BH.dense_conv(xd, mask, w.double(), None if bias is None else bias.double(), geom, subm)
    outs = coords if subm else BH.mask_coords(mo)
    ref = BH.rows_of(yd, outs)

    cd = torch.from_numpy(coords).to(dev)
    ws = TK._index_rows(lib, hip, cd, B, grid)
    od = cd if subm else TK._out_coords(lib, hip, cd, B, grid, geom, n * TK._reach(geom))[0]
    assert np.array_equal(od.cpu().numpy(), outs)
    nbr = TK._neighbors(lib, hip, od, ws, n, B, grid, geom)
    nbytes = lib.shasta_spconv_layer_packed_bytes(cin, cout, K)
    packed = torch.full((nbytes + 16,), 0x5A, dtype=torch.uint8, device=dev)
    wd, bd = w.to(dev).contiguous(), None if bias is None else bias.to(dev)
    hip.check(lib.shasta_spconv_layer_pack_raw_f32(hip.ptr(wd), hip.ptr(bd), cin, cout, K, hip.ptr(packed), nbytes, hip.stream_ptr()),
              "shasta_spconv_layer_pack_raw_f32")
    assert bool((packed[nbytes:] == 0x5A).all())  # the eval pack's byte count, not one byte more
    tail = packed[:nbytes].view(torch.float32)[-2 * cout:].cpu()
    assert bool((tail[:cout] == 1.0).all()) and torch.equal(tail[cout:], torch.zeros(cout) if bias is None else bias)
    n_out = len(outs)
    out = torch.full((n_out + 5, cout), SENTINEL, device=dev)
    xdv = x.to(dev)
    rc = lib.shasta_spconv_layer_f32(hip.ptr(xdv), n, cin, hip.ptr(nbr), n_out, K, hip.ptr(packed), nbytes, cout, None, 0, hip.ptr(out),
                                     hip.stream_ptr())
    assert rc == 0, lib.shasta_last_error()
    out = out.cpu()
    assert bool((out[n_out:] == SENTINEL).all())
    got = out[:n_out].double()
    scale = float(ref.abs().max())
    print("%d -> %d %s raw: %d -> %d rows, max err %.3e, range %.3e" % (cin, cout, gname, n, n_out, float((got - ref).abs().max()), scale))
    assert float(ref.min()) < -0.1  # nothing clipped
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-4, atol=2e-5 * max(1.0, scale))


# ---- 5 - 9. the whole backbone in train() mode --------------------------------------------------------------------
CASES = {"41x64x96": ([96, 64, 40], 2, 31, 3, 100), "41x18x26": ([26, 18, 40], 2, 32, 2, 60)}  # input_shape (x, y, z), B, seed, blobs, rows


def _module(seed, **kw):
    from shasta_amd.backbone import SpMiddleResNetFHD
    m = SpMiddleResNetFHD(num_input_features=5, ds_factor=8, batch_statistics=True, **kw).train()
    BT.randomize_train(m, torch.Generator().manual_seed(seed))
    return m


def _bns(m):
    return [bn for _, bn in m._pairs()]


def _buffers(m):
    return [(bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)) for bn in _bns(m)]


@functools.lru_cache(maxsize=None)
def _case(name):
    """Module (train(), batch_statistics=True), input and the CPU references (float64, float32) of one case; computed once, shared and
    left unchanged - every test runs a deep copy of the module."""
    shape, B, seed, blobs, per = CASES[name]
    m = _module(seed)
    grid = (shape[2] + 1, shape[1], shape[0])
    coords = BH.clustered_voxels(np.random.RandomState(seed), B, grid, blobs=blobs, per_blob=per)
    feats = torch.randn(len(coords), 5, generator=torch.Generator().manual_seed(seed + 1))
    r64, l64, s64 = BT.reference_forward_train(m, feats, coords, B, shape, torch.float64)
    r32, l32, _ = BT.reference_forward_train(m, feats, coords, B, shape, torch.float32)
    return dict(m=m, shape=shape, B=B, grid=grid, coords=coords, feats=feats, r64=r64, l64=l64, s64=s64, r32=r32, l32=l32)


def _restatement_errors(l64, r64, l32, r32):
    errs = {k: float((l32[k][0].double() - l64[k][0]).abs().max()) for k in LEVELS}
    errs["ret"] = float((r32.double() - r64).abs().max())
    return errs


@functools.lru_cache(maxsize=None)
def _bars():
    """4 x the float32 restatement's own max error against float64, pooled per level over both cases: test_whole_backbone_vs_float64's bar."""
    pooled = {}
    for name in CASES:
        c = _case(name)
        for k, v in _restatement_errors(c["l64"], c["r64"], c["l32"], c["r32"]).items():
            pooled[k] = max(pooled.get(k, 0.0), v)
    return pooled


def _run(m, c, dev, order=None):
    feats, coords = c["feats"], torch.from_numpy(c["coords"])
    if order is not None:
        feats, coords = feats[order], coords[order]
    with torch.no_grad():
        return m(feats.to(dev), coords.to(dev), c["B"], c["shape"])


def _level_errors(ret, levels, l64, r64, B):
    """Structure checks of one forward against a float64 reference (active sets exactly, inactive cells exactly +0.0, sorted strided
    levels) and max |got - float64| per level."""
    errs = {}
    assert list(levels) == list(LEVELS)
    for k in LEVELS:
        lv = levels[k]
        x64, mask = l64[k]
        assert lv.spatial_shape == list(x64.shape[2:]) and lv.batch_size == B
        rows, lin = TK._sorted_rows(lv.indices, lv.spatial_shape)
        assert np.array_equal(rows, BH.mask_coords(mask)), k
        if k != "conv1":
            assert bool((np.diff(lin) > 0).all()), k
        dense = lv.dense().cpu()
        assert dense.shape == x64.shape
        off = dense[(mask.expand_as(x64) == 0)]
        assert bool((off == 0).all()) and not bool(torch.signbit(off).any()), k
        errs[k] = float((dense.double() - x64).abs().max())
    ret64, mask_ret = l64["ret"]
    got = ret.cpu()
    assert got.shape == r64.shape and got.dtype == torch.float32
    inactive = (mask_ret.expand_as(ret64) == 0).reshape(got.shape)
    assert bool((got[inactive] == 0).all()) and not bool(torch.signbit(got[inactive]).any())  # exactly +0.0
    errs["ret"] = float((got.double() - r64).abs().max())
    return errs


def _check_running(m, want, what):
    """Running statistics against float64 of torch's rule from the reference's statistics, rtol 1e-5; a layer on running statistics
    (want None) must not have moved - the caller compares those bit for bit."""
    worst = 0.0
    for i, (bn, w) in enumerate(zip(_bns(m), want)):
        if w is None:
            continue
        for got, ref in ((bn.running_mean, w[0]), (bn.running_var, w[1])):
            got = got.cpu().double()
            worst = max(worst, float(((got - ref).abs() / ref.abs()).max()))
            np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-5, atol=0, err_msg="%s, pair %d" % (what, i))
    return worst


def test_whole_backbone_train_vs_float64():
    """Active sets exactly; inactive cells exactly +0.0; levels and ret within 4 x the float32 restatement's own max error against
    float64, pooled per level over both cases; the running statistics of all 21 BatchNorm1d modules within rtol 1e-5 of float64;
    every num_batches_tracked = 1; and the result is not the eval forward's.

    Measured on an MI355X (max |got - float64| / fp32 restatement's max error, pooled over both cases): see DESIGN.md section 4."""
    dev = _dev()
    errs = {}
    for name in CASES:
        c = _case(name)
        # conditions on the reference before anything is compared
        ret64, mask_ret = c["l64"]["ret"]
        fill = float(mask_ret.mean())
        active = mask_ret.expand_as(ret64) > 0
        nonzero = float((ret64[active] != 0).double().mean())
        rng = float(c["r64"].abs().max())
        rows = [int(s[2]) for s in c["s64"]]
        print("%s: %d voxels, rows %s, last-level fill %.3f, nonzero share of active outputs %.2f, range %.3g"
              % (name, len(c["coords"]), [int(c["l64"][k][1].sum()) for k in LEVELS + ("ret",)], fill, nonzero, rng))
        if name == "41x64x96":
            assert 0.1 <= fill <= 0.9
        assert nonzero >= 0.25 and 0.1 <= rng <= 100
        assert len(rows) == 21 and min(rows) >= 2  # every layer has batch statistics to take
        want = BT.expected_running(c["m"], c["s64"])
        # the relative bar on a running mean needs (1 - m) r + m mean away from zero: the helper's running means see to that
        assert min(float(w[0].abs().min()) for w in want) >= 0.02 and min(float(w[1].min()) for w in want) >= 0.5

        m = copy.deepcopy(c["m"]).to(dev)
        assert m.training and all(bn.training for bn in _bns(m))
        ret, levels = _run(m, c, dev)
        torch.cuda.synchronize()
        assert torch.equal(levels["conv1"].indices.cpu(), torch.from_numpy(c["coords"]))  # conv1 keeps the input's order
        for k, v in _level_errors(ret, levels, c["l64"], c["r64"], c["B"]).items():
            errs[k] = max(errs.get(k, 0.0), v)
        print("%s: running statistics, worst relative error %.3e" % (name, _check_running(m, want, name)))
        assert all(int(bn.num_batches_tracked) == 1 for bn in _bns(m))
        ev = copy.deepcopy(c["m"]).to(dev).eval()
        ret_eval, _ = _run(ev, c, dev)
        assert float((ret - ret_eval).abs().max()) > 1e-3  # batch statistics, not the running ones
        assert all(int(bn.num_batches_tracked) == 0 for bn in _bns(ev))
    bars = _bars()
    for k in LEVELS + ("ret",):
        print("%s: kernel max|got - f64| = %.3e, fp32 restatement max|f32 - f64| = %.3e, ratio %.2f" % (k, errs[k], bars[k], errs[k] / bars[k]))
    for k in LEVELS + ("ret",):
        assert errs[k] <= 4 * bars[k], (k, errs[k], bars[k])


def test_same_bits_every_run():
    """Two deep copies of one module: equal bits for ret, every level and every running statistic.  For another row ORDER the float64
    sums of a channel are taken in another order, so bit equality is not claimed there: the bar of the whole-backbone test is."""
    dev = _dev()
    c = _case("41x18x26")
    m1, m2, m3 = (copy.deepcopy(c["m"]).to(dev) for _ in range(3))
    r1, l1 = _run(m1, c, dev)
    r2, l2 = _run(m2, c, dev)
    assert torch.equal(r1, r2) and float(r1.abs().max()) > 0
    for k in LEVELS:
        assert torch.equal(l1[k].features, l2[k].features) and torch.equal(l1[k].indices, l2[k].indices)
    for a, b in zip(_buffers(m1), _buffers(m2)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] == 1
    order = torch.randperm(len(c["coords"]), generator=torch.Generator().manual_seed(5))
    r3, l3 = _run(m3, c, dev, order)
    assert torch.equal(l3["conv1"].indices.cpu(), torch.from_numpy(c["coords"])[order])
    errs, bars = _level_errors(r3, l3, c["l64"], c["r64"], c["B"]), _bars()
    for k in LEVELS + ("ret",):
        assert errs[k] <= 4 * bars[k], (k, errs[k], bars[k])
    _check_running(m3, BT.expected_running(c["m"], c["s64"]), "shuffled rows")


def test_per_layer_rule():
    """torch's rule per BatchNorm1d: batch statistics where bn.training, the running ones where not."""
    dev = _dev()
    c = _case("41x18x26")
    # every BatchNorm in eval() inside a train() backbone: the eval forward's bits, no buffer moves
    m = copy.deepcopy(c["m"]).to(dev)
    for bn in _bns(m):
        bn.eval()
    assert m.training
    before = _buffers(m)
    ret, levels = _run(m, c, dev)
    ev = copy.deepcopy(c["m"]).to(dev).eval()
    ret_eval, levels_eval = _run(ev, c, dev)
    assert torch.equal(ret, ret_eval) and all(torch.equal(levels[k].features, levels_eval[k].features) for k in LEVELS)
    for a, b in zip(before, _buffers(m)):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] == 0
    # only conv_input[1] in training mode
    ref_m = copy.deepcopy(c["m"])
    for bn in _bns(ref_m):
        bn.eval()
    ref_m.conv_input[1].train()
    r64, l64, s64 = BT.reference_forward_train(ref_m, c["feats"], c["coords"], c["B"], c["shape"], torch.float64)
    r32, l32, _ = BT.reference_forward_train(ref_m, c["feats"], c["coords"], c["B"], c["shape"], torch.float32)
    assert [s is not None for s in s64] == [True] + [False] * 20
    bars = _restatement_errors(l64, r64, l32, r32)
    m = copy.deepcopy(ref_m).to(dev)
    before = _buffers(m)
    ret, levels = _run(m, c, dev)
    errs = _level_errors(ret, levels, l64, r64, c["B"])
    for k in LEVELS + ("ret",):
        print("%s: one layer on batch statistics: kernel %.3e, fp32 restatement %.3e" % (k, errs[k], bars[k]))
        assert errs[k] <= 4 * bars[k], (k, errs[k], bars[k])
    assert float((ret - ret_eval).abs().max()) > 1e-3 and float((ret.cpu().double() - c["r64"]).abs().max()) > 1e-3
    _check_running(m, BT.expected_running(ref_m, s64), "one layer")
    after = _buffers(m)
    assert after[0][2] == 1 and not torch.equal(after[0][0], before[0][0]) and not torch.equal(after[0][1], before[0][1])
    for a, b in zip(before[1:], after[1:]):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] == 0


def test_eval_packs_follow_the_running_statistics():
    """The kernels write the running statistics through raw pointers (no version bump): an eval forward after a train() forward must
    still fold the UPDATED statistics - also when eval packs of the old ones were cached by an earlier eval forward."""
    dev = _dev()
    c = _case("41x18x26")
    m = _module(CASES["41x18x26"][2], norm_cfg=dict(type="BN1d", eps=1e-3, momentum=0.1))
    m.load_state_dict(c["m"].state_dict())
    m = m.to(dev)
    old64, _ = BH.reference_forward(copy.deepcopy(m).cpu(), c["feats"], c["coords"], c["B"], c["shape"], torch.float64)
    scale = float(old64.abs().max())
    atol = 2e-5 * max(1.0, scale)
    got_old = _run(m.eval(), c, dev)[0].cpu().double()  # caches the eval packs of the old statistics
    np.testing.assert_allclose(got_old.numpy(), old64.numpy(), rtol=1e-4, atol=atol)
    _run(m.train(), c, dev)
    assert all(int(bn.num_batches_tracked) == 1 for bn in _bns(m))
    new64, _ = BH.reference_forward(copy.deepcopy(m).cpu().eval(), c["feats"], c["coords"], c["B"], c["shape"], torch.float64)
    stale = float((new64 - old64).abs().max())
    print("eval result moved by %.3e with the statistics (bar %.3e)" % (stale, atol))
    assert stale > 50 * atol  # a stale pack is off by far more than the bar
    got_new = _run(m.eval(), c, dev)[0].cpu().double()
    np.testing.assert_allclose(got_new.numpy(), new64.numpy(), rtol=1e-4, atol=2e-5 * max(1.0, float(new64.abs().max())))


class _Recorder:
    """The loaded library with the name of every call noted (size queries aside)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.endswith(("_bytes", "_supported")) or name == "shasta_last_error":
            return fn

        def noted(*a):
            self.calls.append(name)
            return fn(*a)
        return noted


def test_what_the_train_mode_refuses(monkeypatch):
    from shasta_amd import hip
    dev = _dev()
    c = _case("41x18x26")
    feats, coords = c["feats"].to(dev), torch.from_numpy(c["coords"]).to(dev)
    m = copy.deepcopy(c["m"]).to(dev)
    with pytest.raises(hip.ShastaHipError, match="autograd"):  # grad mode on, parameters require grad
        m(feats, coords, c["B"], c["shape"])
    assert all(b[2] == 0 for b in _buffers(m))
    m.requires_grad_(False)
    assert m(feats, coords, c["B"], c["shape"])[0].shape == c["r64"].shape  # frozen parameters: served with grad mode on
    with torch.no_grad():
        m.batch_statistics = False
        with pytest.raises(hip.ShastaHipError, match="train"):  # the default module, as before
            m(feats, coords, c["B"], c["shape"])
        cum = _module(3, norm_cfg=dict(type="BN1d", eps=1e-3, momentum=None)).to(dev)
        with pytest.raises(hip.ShastaHipError, match="momentum"):
            cum(feats, coords, c["B"], c["shape"])
        assert all(b[2] == 0 for b in _buffers(cum))
        assert cum.eval()(feats, coords, c["B"], c["shape"])[0].shape == c["r64"].shape  # eval() does not care
        # two voxels six cells apart in z: 2, 2, 3, 2 rows on conv1 .. conv4 and ONE on the last level
        one = copy.deepcopy(c["m"]).to(dev)
        two = torch.tensor([[0, 0, 0, 0], [0, 6, 0, 0]], dtype=torch.int32, device=dev)
        rec = _Recorder(hip.load())
        monkeypatch.setattr(hip, "load", lambda: rec)
        with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
            one(feats[:2].contiguous(), two, 1, c["shape"])
        monkeypatch.undo()
        torch.cuda.synchronize()
        # the raising layer (extra_conv) launched none of its own kernels: its neighbour table, convolution, statistics
        assert rec.calls.count("shasta_spconv_layer_f32") == 20 and rec.calls.count("shasta_bn_rows_stats_f32") == 20
        assert rec.calls.count("shasta_bn_rows_apply_f32") == 20 and rec.calls.count("shasta_spconv_dense_f32") == 0
        assert rec.calls[-1] == "shasta_spconv_out_coords", rec.calls[-3:]  # (its row count is what the refusal reads)
        assert [b[2] for b in _buffers(one)] == [1] * 20 + [0]
        ret, _ = one(feats, coords, c["B"], c["shape"])  # and the module serves the next call
        assert ret.shape == c["r64"].shape and [b[2] for b in _buffers(one)] == [2] * 20 + [1]


# ---- 10. from points to the affinity matrices in train() mode -----------------------------------------------------
@contextlib.contextmanager
def _deterministic_convolutions():
    old = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = old


def test_from_points_to_affinity_matrices_in_train_mode():
    """test_from_points_to_affinity_matrices with the model in train() under no_grad and the backbone built with batch_statistics=True:
    matched1 / matched2 equal, bit for bit, what the same weights give when fed bev_map = neck(backbone(...)) computed outside from
    copies of the same backbone and neck in train() (the neck runs its nn layers there)."""
    import shasta_amd
    from oracle import shasta_oracle as O
    from shasta_amd.backbone import SpMiddleResNetFHD
    from shasta_amd.voxel_generator import VoxelGenerator
    from tests.neck_helpers import SHIPPED, randomize_bn
    dev = _dev()
    N, B, P = 8, 2, 10
    bev = dict(type="BEVFeatureExtractor", pc_start=[-54, -54], voxel_size=[0.5625, 0.5625], out_stride=8)  # 24 x 24 cells over 108 m
    torch.manual_seed(51)
    m = shasta_amd.build_simp_track(dict(type="Shasta", reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5),
                                         backbone=dict(type=SpMiddleResNetFHD, num_input_features=5, ds_factor=8, batch_statistics=True),
                                         neck=dict(type="RPN", **SHIPPED), bev_extractor=bev, max_obj=N, num_feats=7, num_point=5))
    assert m.backbone.batch_statistics is True
    BH.randomize(m.backbone, torch.Generator().manual_seed(52))
    randomize_bn(m.neck, torch.Generator().manual_seed(53))
    plain = shasta_amd.build_simp_track(dict(type="Shasta", reader=None, backbone=None, neck=None, bev_extractor=bev, max_obj=N, num_feats=7,
                                             num_point=5))
    plain.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith(("neck.", "backbone."))})
    m, plain = m.to(dev).train(), plain.to(dev).train()
    assert m.backbone.training and m.neck.training
    outside_backbone, outside_neck = copy.deepcopy(m.backbone), copy.deepcopy(m.neck)

    g = torch.Generator().manual_seed(54)
    clouds = []
    for _ in range(2 * B):  # current and previous cloud of every sample: a few clusters inside the range
        centres = (torch.rand(6, 3, generator=g) - 0.5) * torch.tensor([90.0, 90.0, 5.0]) + torch.tensor([0.0, 0.0, -1.0])
        pts = centres.repeat_interleave(150, 0) + torch.randn(900, 3, generator=g) * torch.tensor([2.0, 2.0, 0.5])
        clouds.append(torch.cat([pts, torch.rand(900, 2, generator=g)], 1).to(dev))
    vg = VoxelGenerator([0.5625, 0.5625, 0.2], [-54, -54, -5, 54, 54, 3], P, max_voxels=4000)
    voxels, coors, num, _, nv = vg.generate_batch_device(clouds)
    nv = nv.cpu().tolist()

    def side(first):  # clouds first, first + 2, ..: one per sample
        vs, cs, ns = [], [], []
        for b in range(B):
            c, k = first + 2 * b, nv[first + 2 * b]
            vs.append(voxels[c, :k])
            ns.append(num[c, :k])
            cs.append(torch.cat([torch.full((k, 1), b, dtype=torch.int32, device=dev), coors[c, :k]], 1))
        return torch.cat(vs), torch.cat(cs), torch.cat(ns)

    (v0, c0, n0), (v1, c1, n1) = side(0), side(1)
    assert min(nv) > 100
    det, prev = O.synth_boxes(g, B, N).to(dev), O.synth_boxes(g, B, N).to(dev)
    shape = [vg.grid_size.tolist()]
    ex = dict(det_boxes=det.clone(), prev_det_boxes=prev.clone(), voxels=v0, prev_voxels=v1, num_points=n0, prev_num_points=n1,
              coordinates=c0, prev_coordinates=c1, points=[None] * B, prev_points=[None] * B, shape=shape, prev_shape=shape)
    with torch.no_grad(), _deterministic_convolutions():
        m1, m2, _ = m(ex, train_mode=False)
        maps = [outside_neck(outside_backbone(m.reader(v, n), c, B, shape[0])[0]) for v, c, n in ((v0, c0, n0), (v1, c1, n1))]
        assert maps[0].shape == (B, 512, 24, 24) and float(maps[0].abs().max()) > 0 and not torch.equal(maps[0], maps[1])
        ex2 = dict(det_boxes=det.clone(), prev_det_boxes=prev.clone(), bev_map=maps[0], prev_bev_map=maps[1])
        r1, r2, _ = plain(ex2, train_mode=False)
    torch.cuda.synchronize()
    assert m1.shape == (B, N, N + 2) and bool(torch.isfinite(m1).all())
    assert torch.equal(m1, r1) and torch.equal(m2, r2)
    # both frames went through every BatchNorm1d of the backbone: two updates each, the same in the model and in the copy
    for a, b in zip(_buffers(m.backbone), _buffers(outside_backbone)):
        assert a[2] == b[2] == 2 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
