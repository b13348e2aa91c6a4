"""GPU: the sparse backbone's kernels (csrc/sparse_conv.hip) through the C ABI and through `SpMiddleResNetFHD`, against the numpy brute
force of the index kernels and the float64 dense restatement of tests/backbone_helpers.py.

Seams of the kernels: the convolution owns 128 output rows per workgroup (rows 1, 127, 128, 129, several tiles); the row-parallel index
kernels run 256 rows (or row x tap pairs) per workgroup; the bitmap scan runs 1024 words = 32 768 cells per workgroup and the block
sums 256 workgroups = 8.4 M cells per trip of the single-workgroup pass (one grid beyond that)."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import backbone_helpers as BH
from tests.backbone_helpers import E_ARG, E_UNSUPPORTED, E_WORKSPACE, GEOMETRIES, SUBM

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
EPS = 1e-3


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda", 0)


def _flat(geom):
    return [v for part in geom for v in part]


def _index_rows(lib, hip, coords, B, grid):
    ws = torch.empty(lib.shasta_spconv_index_workspace_bytes(B, *grid, len(coords)), dtype=torch.uint8, device=coords.device)
    hip.check(lib.shasta_spconv_index_rows(hip.ptr(coords), len(coords), B, *grid, hip.ptr(ws), ws.numel(), hip.stream_ptr()),
              "shasta_spconv_index_rows")
    return ws


def _out_coords(lib, hip, coords, B, grid, geom, cap):
    dev = coords.device
    og = BH.out_grid(grid, geom)
    ws = torch.empty(lib.shasta_spconv_index_workspace_bytes(B, *og, cap), dtype=torch.uint8, device=dev)
    out = torch.full((cap + 3, 4), int(SENTINEL), dtype=torch.int32, device=dev)  # rows beyond the capacity must stay untouched
    count = torch.full((1,), -1, dtype=torch.int32, device=dev)
    hip.check(lib.shasta_spconv_out_coords(hip.ptr(coords), len(coords), B, *grid, *_flat(geom), hip.ptr(out), cap, hip.ptr(count),
                                           hip.ptr(ws), ws.numel(), hip.stream_ptr()), "shasta_spconv_out_coords")
    n = int(count.item())
    assert 0 <= n <= cap and bool((out[n:] == int(SENTINEL)).all())
    return out[:n].contiguous(), ws


def _neighbors(lib, hip, out_coords, in_ws, n_in, B, grid, geom):
    K = int(np.prod(geom[0]))
    nbr = torch.full((len(out_coords) + 2, K), int(SENTINEL), dtype=torch.int32, device=out_coords.device)
    hip.check(lib.shasta_spconv_neighbors(hip.ptr(out_coords), len(out_coords), B, *grid, *_flat(geom), hip.ptr(in_ws), in_ws.numel(), n_in,
                                          hip.ptr(nbr), hip.stream_ptr()), "shasta_spconv_neighbors")
    assert bool((nbr[len(out_coords):] == int(SENTINEL)).all())
    return nbr[:len(out_coords)].contiguous()


def _reach(geom):
    return int(np.prod([-(-k // s) for k, s in zip(geom[0], geom[1])]))


# ---- 1. index kernels ---------------------------------------------------------------------------------------------
def _isolated(rng, B, grid, n):
    """Voxels at odd coordinates at least 4 apart: under k3 s2 p1 each activates 8 output sites of its own (n_out > n_in)."""
    D, H, W = grid
    sites = [(b, z, y, x) for b in range(B) for z in range(1, D - 1, 4) for y in range(1, H - 1, 4) for x in range(1, W - 1, 4)]
    pick = rng.choice(len(sites), size=n, replace=False)
    return np.array([sites[i] for i in pick], np.int32)


INDEX_CASES = {
    # name: (geometry, B, grid, voxels)
    "subm-two-items": ("subm", 2, (5, 6, 7), lambda r, B, g: BH.clustered_voxels(r, B, g, blobs=2, per_blob=30, sigma=(1, 2, 2))),
    "s2p1-odd": ("k3s2p1", 2, (41, 17, 25), lambda r, B, g: BH.clustered_voxels(r, B, g, blobs=3, per_blob=60)),
    "s2p1-even": ("k3s2p1", 1, (8, 12, 10), lambda r, B, g: BH.clustered_voxels(r, B, g, blobs=2, per_blob=40, sigma=(1, 2, 2))),
    "s2p011-odd": ("k3s2p011", 2, (11, 9, 15), lambda r, B, g: BH.clustered_voxels(r, B, g, blobs=2, per_blob=50, sigma=(2, 2, 2))),
    "s2p011-even": ("k3s2p011", 1, (10, 8, 14), lambda r, B, g: BH.clustered_voxels(r, B, g, blobs=2, per_blob=50, sigma=(2, 2, 2))),
    "k311-odd": ("k311s211p0", 2, (5, 9, 7), lambda r, B, g: BH.clustered_voxels(r, B, g, blobs=2, per_blob=40, sigma=(2, 2, 2))),
    "k311-even": ("k311s211p0", 1, (6, 4, 8), lambda r, B, g: BH.clustered_voxels(r, B, g, blobs=2, per_blob=40, sigma=(2, 2, 2))),
    "empty-item": ("k3s2p1", 3, (9, 10, 11), lambda r, B, g: BH.clustered_voxels(r, B, g, blobs=2, per_blob=40, empty_items=(1,))),
    "n_out>n_in": ("k3s2p1", 2, (13, 21, 21), lambda r, B, g: _isolated(r, B, g, 60)),
    "beyond-one-scan-trip": ("k3s2p1", 2, (41, 360, 360), lambda r, B, g: BH.clustered_voxels(r, B, g, blobs=3, per_blob=80)),
}
INDEX_CASES.update({"rows-%d" % n: ("k3s2p1", 2, (9, 20, 24), functools.partial(lambda r, B, g, n: BH.random_voxels(r, B, g, n), n=n))
                    for n in (1, 127, 128, 129, 255, 256, 257, 700)})


@pytest.mark.parametrize("name", list(INDEX_CASES))
def test_index_kernels_vs_brute_force(name):
    """Integers, exact: the submanifold table of the input level (rows in a shuffled order), the output coordinates of the strided
    convolution (sorted by linear index, the count in a device word), its neighbour table, and the submanifold table of the output level
    from the index shasta_spconv_out_coords leaves behind."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    gname, B, grid, make = INDEX_CASES[name]
    geom = GEOMETRIES[gname]
    coords = make(np.random.RandomState(sum(map(ord, name))), B, grid)
    cd = torch.from_numpy(coords).to(dev)
    ws = _index_rows(lib, hip, cd, B, grid)
    got = _neighbors(lib, hip, cd, ws, len(coords), B, grid, SUBM).cpu().numpy()
    want = BH.neighbors_ref(coords, coords, grid, SUBM)
    assert np.array_equal(got, want)
    assert np.array_equal(got[:, 13], np.arange(len(coords)))  # the centre tap is the row itself
    if gname == "subm":
        both = set(map(tuple, coords[coords[:, 0] == 0][:, 1:])) & set(map(tuple, coords[coords[:, 0] == 1][:, 1:]))
        assert both, "the case needs the same (z, y, x) in two batch items"
        return
    want_out = BH.out_coords_ref(coords, B, grid, geom)
    out, ows = _out_coords(lib, hip, cd, B, grid, geom, len(coords) * _reach(geom))
    print("%s: %d rows -> %d" % (name, len(coords), len(want_out)))
    assert np.array_equal(out.cpu().numpy(), want_out)
    if name == "n_out>n_in":
        assert len(want_out) == 8 * len(coords)
    if name == "empty-item":
        assert not (want_out[:, 0] == 1).any() and (want_out[:, 0] == 2).any()
    got = _neighbors(lib, hip, out, ws, len(coords), B, grid, geom).cpu().numpy()
    assert np.array_equal(got, BH.neighbors_ref(want_out, coords, grid, geom))
    og = BH.out_grid(grid, geom)
    got = _neighbors(lib, hip, out, ows, len(want_out), B, og, SUBM).cpu().numpy()
    assert np.array_equal(got, BH.neighbors_ref(want_out, want_out, og, SUBM))


# ---- 2. single layers ---------------------------------------------------------------------------------------------
LAYER_CASES = [
    # cin, cout, geometry, bias + residual (the second convolution of a block), B, grid, input rows
    (5, 16, "subm", False, 2, (6, 10, 12), 300),
    (16, 16, "subm", True, 1, (6, 10, 12), 1), (16, 16, "subm", True, 1, (6, 10, 12), 127), (16, 16, "subm", True, 2, (6, 10, 12), 128),
    (16, 16, "subm", True, 2, (6, 10, 12), 129), (16, 16, "subm", True, 2, (6, 10, 12), 300),
    (32, 32, "subm", True, 1, (6, 10, 12), 129), (64, 64, "subm", True, 2, (5, 8, 9), 200), (128, 128, "subm", True, 1, (5, 8, 9), 257),
    (16, 32, "k3s2p1", False, 2, (9, 12, 13), 200), (32, 64, "k3s2p1", False, 1, (11, 12, 12), 150),
    (64, 128, "k3s2p011", False, 2, (11, 8, 9), 150), (128, 128, "k311s211p0", False, 2, (5, 9, 8), 300),
]


def _pack(lib, hip, cin, cout, K, w, bias, bn, dev):
    nbytes = lib.shasta_spconv_layer_packed_bytes(cin, cout, K)
    assert nbytes > 0
    packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ts = [w.to(dev).contiguous(), None if bias is None else bias.to(dev)] + [t.to(dev) for t in bn]
    hip.check(lib.shasta_spconv_layer_pack_f32(*[hip.ptr(t) for t in ts], EPS, cin, cout, K, hip.ptr(packed), nbytes, hip.stream_ptr()),
              "shasta_spconv_layer_pack_f32")
    return packed


def _layer_tensors(cin, cout, k, with_bias, gen):
    w = torch.randn(cout, *k, cin, generator=gen) / float(np.sqrt(cin * np.prod(k)))
    bias = 0.2 * torch.randn(cout, generator=gen) if with_bias else None
    bn = [0.5 + torch.rand(cout, generator=gen), 0.2 * torch.randn(cout, generator=gen), 0.3 * torch.randn(cout, generator=gen),
          0.5 + torch.rand(cout, generator=gen)]
    return w, bias, bn


@pytest.mark.parametrize("cin,cout,gname,block,B,grid,n", LAYER_CASES, ids=["%d-%d-%s-%d" % (c[0], c[1], c[2], c[6]) for c in LAYER_CASES])
def test_layer_vs_float64(cin, cout, gname, block, B, grid, n):
    """One layer through the C ABI into a sentinel-filled buffer with rows to spare.  Bar: K0's and the neck's, set for the same
    arithmetic - a sequential fp32 chain on the f32 MFMA - at K = 4608; here K <= 3456."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    geom, subm = GEOMETRIES[gname], gname == "subm"
    K = int(np.prod(geom[0]))
    g = torch.Generator().manual_seed(100 * cin + cout + n)
    coords = BH.random_voxels(np.random.RandomState(cin + n), B, grid, n)
    x = torch.randn(n, cin, generator=g) if cin == 5 else torch.relu(torch.randn(n, cin, generator=g))
    w, bias, bn = _layer_tensors(cin, cout, geom[0], block, g)
    # float64: the dense restatement, BatchNorm, residual, ReLU on the rows
    xd, mask = BH.to_dense(x.double(), coords, B, grid)
    yd, mo = BH.dense_conv(xd, mask, w.double(), None if bias is None else bias.double(), geom, subm)
    outs = coords if subm else BH.mask_coords(mo)
    res = torch.randn(len(outs), cout, generator=g) if block else None
    gam, bet, mean, var = [t.double() for t in bn]
    ref = (BH.rows_of(yd, outs) - mean) / torch.sqrt(var + EPS) * gam + bet
    if block:
        ref = ref + res.double()
    ref = torch.relu(ref)

    cd = torch.from_numpy(coords).to(dev)
    ws = _index_rows(lib, hip, cd, B, grid)
    if subm:
        od = cd
    else:
        od, _ = _out_coords(lib, hip, cd, B, grid, geom, n * _reach(geom))
        assert np.array_equal(od.cpu().numpy(), outs)
    nbr = _neighbors(lib, hip, od, ws, n, B, grid, geom)
    packed = _pack(lib, hip, cin, cout, K, w, bias, bn, dev)
    n_out = len(outs)
    out = torch.full((n_out + 5, cout), SENTINEL, device=dev)
    xdv, resd = x.to(dev), None if res is None else res.to(dev)
    rc = lib.shasta_spconv_layer_f32(hip.ptr(xdv), n, cin, hip.ptr(nbr), n_out, K, hip.ptr(packed), packed.numel(), cout, hip.ptr(resd), 1,
                                     hip.ptr(out), hip.stream_ptr())
    assert rc == 0, lib.shasta_last_error()
    out = out.cpu()
    assert bool((out[n_out:] == SENTINEL).all())
    got = out[:n_out].double()
    scale = float(ref.abs().max())
    present = float((nbr >= 0).float().mean())
    print("%d -> %d %s: %d -> %d rows, taps present %.2f, max err %.3e, range %.3e"
          % (cin, cout, gname, n, n_out, present, float((got - ref).abs().max()), scale))
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-4, atol=2e-5 * max(1.0, scale))


def test_layer_without_relu_and_in_place_residual():
    """relu = 0 keeps negative values; out may alias residual (a row is read and written by the same thread)."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    B, grid, n, c = 1, (4, 6, 6), 130, 32
    g = torch.Generator().manual_seed(77)
    coords = BH.random_voxels(np.random.RandomState(77), B, grid, n)
    x = torch.randn(n, c, generator=g)
    w, bias, bn = _layer_tensors(c, c, (3, 3, 3), True, g)
    res = torch.randn(n, c, generator=g)
    xd, mask = BH.to_dense(x.double(), coords, B, grid)
    yd, _ = BH.dense_conv(xd, mask, w.double(), bias.double(), SUBM, True)
    gam, bet, mean, var = [t.double() for t in bn]
    ref = (BH.rows_of(yd, coords) - mean) / torch.sqrt(var + EPS) * gam + bet + res.double()
    cd = torch.from_numpy(coords).to(dev)
    nbr = _neighbors(lib, hip, cd, _index_rows(lib, hip, cd, B, grid), n, B, grid, SUBM)
    packed = _pack(lib, hip, c, c, 27, w, bias, bn, dev)
    buf = res.to(dev)
    xdv = x.to(dev)
    rc = lib.shasta_spconv_layer_f32(hip.ptr(xdv), n, c, hip.ptr(nbr), n, 27, hip.ptr(packed), packed.numel(), c, hip.ptr(buf), 0, hip.ptr(buf),
                                     hip.stream_ptr())
    assert rc == 0, lib.shasta_last_error()
    assert float(ref.min()) < -0.1
    np.testing.assert_allclose(buf.cpu().double().numpy(), ref.numpy(), rtol=1e-4, atol=2e-5 * max(1.0, float(ref.abs().max())))
    assert lib.shasta_spconv_layer_f32(hip.ptr(xdv), n, c, hip.ptr(nbr), n, 27, hip.ptr(packed), packed.numel(), c, None, 0, hip.ptr(xdv),
                                       hip.stream_ptr()) == E_ARG  # out aliasing x is refused


# ---- 3 - 5. the whole backbone ------------------------------------------------------------------------------------
CASES = {"41x64x96": ([96, 64, 40], 2, 11, 3, 100), "41x18x26": ([26, 18, 40], 1, 12, 2, 60)}  # input_shape (x, y, z), B, seed, blobs, rows
LEVELS = ("conv1", "conv2", "conv3", "conv4")


def _module(seed):
    from shasta_amd.backbone import SpMiddleResNetFHD
    m = SpMiddleResNetFHD(num_input_features=5, ds_factor=8).eval()
    BH.randomize(m, torch.Generator().manual_seed(seed))
    return m


@functools.lru_cache(maxsize=None)
def _case(name):
    """Module, input and the CPU references (float64, float32) of one case; computed once, shared and left unchanged."""
    shape, B, seed, blobs, per = CASES[name]
    m = _module(seed)
    grid = (shape[2] + 1, shape[1], shape[0])
    coords = BH.clustered_voxels(np.random.RandomState(seed), B, grid, blobs=blobs, per_blob=per)
    feats = torch.randn(len(coords), 5, generator=torch.Generator().manual_seed(seed + 1))
    r64, l64 = BH.reference_forward(m, feats, coords, B, shape, torch.float64)
    r32, l32 = BH.reference_forward(m, feats, coords, B, shape, torch.float32)
    return dict(m=m, shape=shape, B=B, grid=grid, coords=coords, feats=feats, r64=r64, l64=l64, r32=r32, l32=l32)


def _run(m, c, dev, order=None):
    feats, coords = c["feats"], torch.from_numpy(c["coords"])
    if order is not None:
        feats, coords = feats[order], coords[order]
    with torch.no_grad():
        return m(feats.to(dev), coords.to(dev), c["B"], c["shape"])


def _sorted_rows(coords, grid):
    c = coords.cpu().numpy().astype(np.int64)
    lin = ((c[:, 0] * grid[0] + c[:, 1]) * grid[1] + c[:, 2]) * grid[2] + c[:, 3]
    return c[np.argsort(lin)].astype(np.int32), lin


def test_whole_backbone_vs_float64():
    """Active sets exactly; inactive cells exactly 0.0; values within 4 x the fp32 dense restatement's own max error against float64,
    pooled over both cases, for the result and every densified level.

    Measured on an MI355X (max |got - float64| / fp32 restatement's max error, pooled over both cases): see DESIGN.md section 4."""
    dev = _dev()
    errs, ref_errs = {}, {}
    for name in CASES:
        c = _case(name)
        # conditions on the reference before anything is compared
        ret64, mask_ret = c["l64"]["ret"]
        fill = float(mask_ret.mean())
        active = mask_ret.expand_as(ret64) > 0
        nonzero = float((ret64[active] != 0).double().mean())
        rng = float(c["r64"].abs().max())
        print("%s: %d voxels, rows %s, last-level fill %.3f, nonzero share of active outputs %.2f, range %.3g"
              % (name, len(c["coords"]), [int(c["l64"][k][1].sum()) for k in LEVELS + ("ret",)], fill, nonzero, rng))
        if name == "41x64x96":
            assert 0.1 <= fill <= 0.9
        assert nonzero >= 0.25 and 0.1 <= rng <= 100
        m = copy.deepcopy(c["m"]).to(dev)
        ret, levels = _run(m, c, dev)
        torch.cuda.synchronize()
        assert ret.shape == c["r64"].shape and ret.dtype == torch.float32
        assert list(levels) == list(LEVELS)
        # conv1 keeps the input's order; the strided levels are sorted
        assert torch.equal(levels["conv1"].indices.cpu(), torch.from_numpy(c["coords"]))
        for k in LEVELS:
            lv = levels[k]
            x64, mask = c["l64"][k]
            assert lv.spatial_shape == list(x64.shape[2:]) and lv.batch_size == c["B"]
            rows, lin = _sorted_rows(lv.indices, lv.spatial_shape)
            assert np.array_equal(rows, BH.mask_coords(mask)), k
            if k != "conv1":
                assert bool((np.diff(lin) > 0).all()), k
            dense = lv.dense().cpu()
            assert dense.shape == x64.shape
            assert bool((dense[(mask.expand_as(x64) == 0)] == 0).all())
            errs[k] = max(errs.get(k, 0.0), float((dense.double() - x64).abs().max()))
            ref_errs[k] = max(ref_errs.get(k, 0.0), float((c["l32"][k][0].double() - x64).abs().max()))
        got = ret.cpu()
        inactive = (mask_ret.expand_as(ret64) == 0).reshape(got.shape)
        assert bool((got[inactive] == 0).all()) and not bool(torch.signbit(got[inactive]).any())  # exactly +0.0
        errs["ret"] = max(errs.get("ret", 0.0), float((got.double() - c["r64"]).abs().max()))
        ref_errs["ret"] = max(ref_errs.get("ret", 0.0), float((c["r32"].double() - c["r64"]).abs().max()))
    for k in LEVELS + ("ret",):
        print("%s: kernel max|got - f64| = %.3e, fp32 restatement max|f32 - f64| = %.3e" % (k, errs[k], ref_errs[k]))
    for k in LEVELS + ("ret",):
        assert errs[k] <= 4 * ref_errs[k], (k, errs[k], ref_errs[k])


def test_same_bits_every_run_and_for_every_row_order():
    dev = _dev()
    c = _case("41x18x26")
    m = copy.deepcopy(c["m"]).to(dev)
    r1, l1 = _run(m, c, dev)
    r2, l2 = _run(m, c, dev)
    order = torch.randperm(len(c["coords"]), generator=torch.Generator().manual_seed(5))
    r3, l3 = _run(m, c, dev, order)
    assert torch.equal(r1, r2) and torch.equal(r1, r3) and float(r1.abs().max()) > 0
    for k in LEVELS:
        assert torch.equal(l1[k].features, l2[k].features)
        assert torch.equal(l1[k].dense(), l3[k].dense()), k
    assert torch.equal(l3["conv1"].indices.cpu(), torch.from_numpy(c["coords"])[order])
    for k in LEVELS[1:]:  # the sorted levels do not see the input's order at all
        assert torch.equal(l1[k].indices, l3[k].indices) and torch.equal(l1[k].features, l3[k].features)


def _check_follows(m, c, dev, what):
    """A stale packed layer is off by the size of the values themselves; K0's bar tells that apart from fp32 summation order."""
    ref, _ = BH.reference_forward(copy.deepcopy(m).cpu(), c["feats"], c["coords"], c["B"], c["shape"], torch.float64)
    got = _run(m, c, dev)[0].cpu().double()
    scale = float(ref.abs().max())
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-4, atol=2e-5 * max(1.0, scale), err_msg=what)
    return got


def test_caches_follow_the_parameters():
    dev = _dev()
    c = _case("41x18x26")
    m = copy.deepcopy(c["m"]).to(dev)
    y0 = _check_follows(m, c, dev, "first forward")
    other = _module(99).state_dict()
    m.load_state_dict(other)
    y1 = _check_follows(m, c, dev, "after load_state_dict")
    assert float((y1 - y0).abs().max()) > 1e-3
    with torch.no_grad():
        m.extra_conv[1].running_var.copy_(torch.full((128,), 4.0))
        m.conv2[3].conv2.bias.add_(0.25)
        m.conv_input[0].weight.mul_(1.5)
    y2 = _check_follows(m, c, dev, "after in-place writes into statistics, a bias and a weight")
    assert float((y2 - y1).abs().max()) > 1e-3
    m = m.cpu()
    with torch.no_grad():
        m.conv3[0].weight.mul_(0.5)
    m = m.to(dev)
    y3 = _check_follows(m, c, dev, "after .to()")
    assert float((y3 - y2).abs().max()) > 1e-4
    with torch.no_grad():
        m.conv4[4].bn2.bias.data.add_(0.5)  # (.data: no version bump - the documented case for invalidate_weights_cache)
    m.invalidate_weights_cache()
    y4 = _check_follows(m, c, dev, "after invalidate_weights_cache()")
    assert float((y4 - y3).abs().max()) > 1e-3


# ---- 6. refusals --------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    s = hip.stream_ptr()
    B, grid, n = 1, (6, 10, 12), 140
    geom = GEOMETRIES["k3s2p1"]
    g = torch.Generator().manual_seed(5)
    coords = torch.from_numpy(BH.random_voxels(np.random.RandomState(5), B, grid, n)).to(dev)
    ws = _index_rows(lib, hip, coords, B, grid)
    nbr = _neighbors(lib, hip, coords, ws, n, B, grid, SUBM)
    w, bias, bn = _layer_tensors(16, 32, (3, 3, 3), False, g)
    packed = _pack(lib, hip, 16, 32, 27, w, bias, bn, dev)
    x = torch.ones(n, 16, device=dev)
    out = torch.full((n, 48), SENTINEL, device=dev)

    def layer(cin=16, cout=32, K=27, nbytes=None, o=out, nb=nbr):
        return lib.shasta_spconv_layer_f32(hip.ptr(x), n, cin, hip.ptr(nb), n, K, hip.ptr(packed), packed.numel() if nbytes is None else nbytes,
                                           cout, None, 1, None if o is None else hip.ptr(o), s)

    assert layer(cout=48) == E_UNSUPPORTED                  # channel counts outside the served set
    assert layer(cin=24) == E_UNSUPPORTED
    assert layer(K=125) == E_UNSUPPORTED                    # kernel size 5
    assert layer(nbytes=packed.numel() - 1) == E_WORKSPACE  # one byte short
    assert layer(o=None) == E_ARG
    assert b"null" in lib.shasta_last_error()
    ts = [w.to(dev), None] + [t.to(dev) for t in bn]
    assert lib.shasta_spconv_layer_pack_f32(*[hip.ptr(t) for t in ts], EPS, 16, 48, 27, hip.ptr(packed), packed.numel(), s) == E_UNSUPPORTED
    assert lib.shasta_spconv_layer_pack_f32(*[hip.ptr(t) for t in ts], EPS, 16, 32, 27, hip.ptr(packed), packed.numel() - 1, s) == E_WORKSPACE
    # index calls: kernel size 5, a short workspace
    cap = n * 8
    og = BH.out_grid(grid, geom)
    ows = torch.empty(lib.shasta_spconv_index_workspace_bytes(B, *og, cap), dtype=torch.uint8, device=dev)
    oc = torch.full((cap, 4), int(SENTINEL), dtype=torch.int32, device=dev)
    cnt = torch.full((1,), int(SENTINEL), dtype=torch.int32, device=dev)

    def outc(k=(3, 3, 3), nbytes=None):
        return lib.shasta_spconv_out_coords(hip.ptr(coords), n, B, *grid, *k, *_flat(geom[1:]), hip.ptr(oc), cap, hip.ptr(cnt), hip.ptr(ows),
                                            ows.numel() if nbytes is None else nbytes, s)

    assert outc(k=(5, 5, 5)) == E_UNSUPPORTED
    assert outc(nbytes=ows.numel() - 256) == E_WORKSPACE
    tbl = torch.full((n, 27), int(SENTINEL), dtype=torch.int32, device=dev)
    assert lib.shasta_spconv_neighbors(hip.ptr(coords), n, B, *grid, 5, 3, 3, 1, 1, 1, 1, 1, 1, hip.ptr(ws), ws.numel(), n, hip.ptr(tbl), s) \
        == E_UNSUPPORTED
    assert lib.shasta_spconv_neighbors(hip.ptr(coords), n, B, *grid, *_flat(SUBM), hip.ptr(ws), ws.numel() - 256, n, hip.ptr(tbl), s) == E_WORKSPACE
    assert lib.shasta_spconv_index_rows(hip.ptr(coords), n, B, *grid, hip.ptr(ws), ws.numel() - 256, s) == E_WORKSPACE
    assert lib.shasta_spconv_index_rows(hip.ptr(coords), n, 1 << 12, 1 << 10, 1 << 10, 1 << 10, hip.ptr(ws), ws.numel(), s) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((oc == int(SENTINEL)).all()) and int(cnt) == int(SENTINEL)
    assert bool((tbl == int(SENTINEL)).all())
    out32 = torch.full((n, 32), SENTINEL, device=dev)
    assert layer(o=out32) == 0 and outc() == 0                # and the good calls write
    torch.cuda.synchronize()
    assert bool((out32 >= 0).all()) and 0 < int(cnt) <= cap


def test_no_voxels_give_zeros():
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    m = _module(3).to(dev)
    with torch.no_grad():
        ret, levels = m(torch.empty(0, 5, device=dev), torch.empty(0, 4, dtype=torch.int32, device=dev), 2, [26, 18, 40])
    assert ret.shape == (2, 256, 3, 4) and bool((ret == 0).all())
    assert [tuple(levels[k].features.shape) for k in LEVELS] == [(0, 16), (0, 32), (0, 64), (0, 128)]
    assert levels["conv3"].dense().shape == (2, 64, 11, 5, 7) and bool((levels["conv3"].dense() == 0).all())
    out = torch.full((2, 8 * 3, 4, 5), SENTINEL, device=dev)
    assert lib.shasta_spconv_dense_f32(None, None, 0, 2, 8, 3, 4, 5, hip.ptr(out), hip.stream_ptr()) == 0
    assert bool((out == 0).all())


def test_what_the_module_refuses():
    from shasta_amd import hip
    from shasta_amd.backbone import SpMiddleResNetFHD
    dev = _dev()
    c = _case("41x18x26")
    feats, coords = c["feats"].to(dev), torch.from_numpy(c["coords"]).to(dev)
    m = copy.deepcopy(c["m"]).to(dev)
    with pytest.raises(hip.ShastaHipError, match="autograd"):  # grad mode on, parameters require grad
        m(feats, coords, c["B"], c["shape"])
    m.requires_grad_(False)
    assert m(feats, coords, c["B"], c["shape"])[0].shape == c["r64"].shape  # frozen parameters: served with grad mode on
    with pytest.raises(hip.ShastaHipError, match="autograd"):
        m(feats.clone().requires_grad_(True), coords, c["B"], c["shape"])
    with torch.no_grad():
        with pytest.raises(hip.ShastaHipError, match="train"):
            m.train()(feats, coords, c["B"], c["shape"])
        with pytest.raises(hip.ShastaHipError, match="device"):
            m.eval()(feats.cpu(), coords.cpu(), c["B"], c["shape"])
        gn = SpMiddleResNetFHD(num_input_features=5, norm_cfg=dict(type="GN", num_groups=4)).eval().to(dev)
        with pytest.raises(hip.ShastaHipError, match="BatchNorm1d"):
            gn(feats, coords, c["B"], c["shape"])


# ---- 7. from points to the affinity matrices ----------------------------------------------------------------------
def test_from_points_to_affinity_matrices():
    """Two small clouds per sample -> VoxelGenerator.generate_batch_device (192 x 192 x 40 voxels of 0.5625 m) -> VoxelFeatureExtractorV3 ->
    this backbone -> RPN with the shipped channels -> K0 -> matched1 / matched2 through build_simp_track with the class as `type`; equal,
    bit for bit, to the same weights fed bev_map = neck(backbone(...)) computed outside."""
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
                                         backbone=dict(type=SpMiddleResNetFHD, num_input_features=5, ds_factor=8),
                                         neck=dict(type="RPN", **SHIPPED), bev_extractor=bev, max_obj=N, num_feats=7, num_point=5)).eval()
    assert "backbone.conv4.4.bn2.running_var" in m.state_dict() and "neck.deblocks.1.1.running_mean" in m.state_dict()
    BH.randomize(m.backbone, torch.Generator().manual_seed(52))
    randomize_bn(m.neck, torch.Generator().manual_seed(53))
    plain = shasta_amd.build_simp_track(dict(type="Shasta", reader=None, backbone=None, neck=None, bev_extractor=bev, max_obj=N, num_feats=7,
                                             num_point=5)).eval()
    plain.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith(("neck.", "backbone."))})
    m, plain = m.to(dev), plain.to(dev)

    g = torch.Generator().manual_seed(54)
    clouds = []
    for _ in range(2 * B):  # current and previous cloud of every sample: a few clusters inside the range
        centres = (torch.rand(6, 3, generator=g) - 0.5) * torch.tensor([90.0, 90.0, 5.0]) + torch.tensor([0.0, 0.0, -1.0])
        pts = centres.repeat_interleave(150, 0) + torch.randn(900, 3, generator=g) * torch.tensor([2.0, 2.0, 0.5])
        clouds.append(torch.cat([pts, torch.rand(900, 2, generator=g)], 1).to(dev))
    vg = VoxelGenerator([0.5625, 0.5625, 0.2], [-54, -54, -5, 54, 54, 3], P, max_voxels=4000)
    assert vg.grid_size.tolist() == [192, 192, 40]
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
    with torch.no_grad():
        m1, m2, _ = m(ex, train_mode=False)
        maps = [m.neck(m.backbone(m.reader(v, n), c, B, shape[0])[0]) for v, c, n in ((v0, c0, n0), (v1, c1, n1))]
        assert maps[0].shape == (B, 512, 24, 24) and float(maps[0].abs().max()) > 0 and not torch.equal(maps[0], maps[1])
        ex2 = dict(det_boxes=det.clone(), prev_det_boxes=prev.clone(), bev_map=maps[0], prev_bev_map=maps[1])
        r1, r2, _ = plain(ex2, train_mode=False)
    torch.cuda.synchronize()
    assert m1.shape == (B, N, N + 2) and bool(torch.isfinite(m1).all())
    assert torch.equal(m1, r1) and torch.equal(m2, r2)
