"""GPU: the neck kernels (csrc/neck.hip) through the C ABI and through the registered `RPN` module, against torch's CPU float64.

Tile seams of the kernels: a workgroup owns 4 rows x 32 columns of the pixel domain (output pixels; input pixels for D2) and 64 output
channels (two accumulators of 32); K is walked in chunks of 8 (C3S1), 4 (C3S2) or 32 (C1, D2: the last chunk is zero-padded) input
channels, two chunks per loop trip with a one- or two-chunk tail.  C3S1 on maps up to 256 columns wide: 128 consecutive pixels of the
flattened image per workgroup, chunks of 4 channels, the staged tile sized by the map width."""
import copy

import numpy as np
import pytest
import torch

from tests.neck_helpers import (C1, C3S1, C3S2, D2, E_ARG, E_UNSUPPORTED, E_WORKSPACE, KIND_NAMES, SHIPPED, build_fixture_neck, fixture,
                                layer_ref64, layer_tensors, layers64, randomize_bn)

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
EPS = 1e-3


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda", 0)


def _pack(lib, hip, kind, cin, cout, w, bn, dev):
    nbytes = lib.shasta_neck_layer_packed_bytes(kind, cin, cout)
    assert nbytes > 0
    packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ts = [t.to(dev).contiguous() for t in [w] + bn]
    hip.check(lib.shasta_neck_layer_pack_f32(*[hip.ptr(t) for t in ts], EPS, kind, cin, cout, hip.ptr(packed), nbytes, hip.stream_ptr()),
              "shasta_neck_layer_pack_f32")
    return packed


def _out_hw(kind, H, W):
    return (H // 2, W // 2) if kind == C3S2 else (2 * H, 2 * W) if kind == D2 else (H, W)


def _run_layer(lib, hip, kind, x, packed, cout, total, off):
    B, cin, H, W = x.shape
    oh, ow = _out_hw(kind, H, W)
    out = torch.full((B, total, oh, ow), SENTINEL, device=x.device)
    rc = lib.shasta_neck_layer_f32(hip.ptr(x), B, cin, H, W, hip.ptr(packed), packed.numel(), kind, cout, hip.ptr(out), total, off,
                                   hip.stream_ptr())
    return rc, out


# the issue's shapes, then the seams of this tiling: rows 4 | 5, columns 31 | 32 | 33 | 64 | 65, channel blocks 32 | 64 | 96, K chunks
# 1 .. 5 trips (Cin 8 .. 40), the zero-padded last chunk of the 1x1 kinds (Cin 8, 40, 72); C3S1 up to 256 columns: 128 | 129 flattened
# pixels, one width per staging class of the tile (8, 12, 14, 16, 18 floats per thread: W = 70, 180, 200, 240, 256), a one-column map
# (130-row tile); from 257 columns: the rectangular kernel
LAYER_CASES = [
    (C3S1, 1, 8, 32, 1, 1), (C3S1, 2, 16, 32, 5, 33), (C3S1, 1, 256, 128, 6, 34), (C3S1, 1, 128, 128, 9, 65), (C3S1, 1, 256, 256, 4, 70),
    (C3S1, 1, 24, 96, 4, 32), (C3S1, 1, 32, 64, 5, 31), (C3S1, 1, 40, 32, 8, 64),
    (C3S1, 1, 8, 32, 3, 127), (C3S1, 1, 8, 64, 3, 180), (C3S1, 1, 8, 32, 3, 200), (C3S1, 1, 8, 32, 3, 240), (C3S1, 2, 8, 32, 3, 256),
    (C3S1, 1, 8, 32, 140, 1), (C3S1, 1, 8, 96, 5, 257), (C3S1, 2, 24, 32, 9, 290),
    (C3S2, 1, 8, 32, 2, 2), (C3S2, 2, 128, 256, 6, 34), (C3S2, 1, 16, 64, 10, 66), (C3S2, 1, 32, 32, 14, 130),
    (C3S2, 1, 24, 96, 8, 64), (C3S2, 1, 8, 64, 10, 62),
    (C1, 1, 128, 256, 6, 34), (C1, 2, 8, 32, 3, 65), (C1, 1, 40, 96, 4, 32), (C1, 1, 64, 64, 5, 33),
    (D2, 1, 256, 256, 3, 17), (D2, 2, 16, 32, 5, 33), (D2, 1, 8, 32, 1, 1), (D2, 1, 40, 96, 4, 32), (D2, 1, 72, 64, 9, 31),
]


@pytest.mark.parametrize("kind,B,cin,cout,H,W", LAYER_CASES, ids=["%s-%d-%d-%d-%d-%d" % ((KIND_NAMES[c[0]],) + c[1:]) for c in LAYER_CASES])
def test_layer_vs_float64(kind, B, cin, cout, H, W):
    """One layer through the C ABI into a channel slice of a larger, sentinel-filled output.  Bar: K0's (test_shared_conv_vs_oracle),
    set for the same arithmetic - a sequential fp32 fmaf chain on the f32 MFMA - at K = 4608; here K <= 2304."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    g = torch.Generator().manual_seed(1000 * kind + cin + cout + H + W)
    w, bn = layer_tensors(kind, cin, cout, g)
    x = torch.relu(torch.randn(B, cin, H, W, generator=g))
    ref = layer_ref64(kind, x, w, bn, EPS)
    packed = _pack(lib, hip, kind, cin, cout, w, bn, dev)
    total, off = cout + 9, 5
    rc, out = _run_layer(lib, hip, kind, x.to(dev), packed, cout, total, off)
    assert rc == 0, lib.shasta_last_error()
    out = out.cpu()
    assert out.shape[2:] == ref.shape[2:]
    assert bool((out[:, :off] == SENTINEL).all()) and bool((out[:, off + cout:] == SENTINEL).all())
    got = out[:, off:off + cout].double()
    scale = float(ref.abs().max())
    print("%s %s: max err %.3e, range %.3e" % (KIND_NAMES[kind], (B, cin, cout, H, W), float((got - ref).abs().max()), scale))
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-4, atol=2e-5 * max(1.0, scale))


def test_whole_neck_fixture_vs_reference():
    """The fixture's neck on the kernels against the reference's float64 output.  Bar: 4 x the reference's own max|y32 - y64| (both sides
    sum in fp32 in different orders; the kernel's chain is sequential in K)."""
    fx, dev = fixture(), _dev()
    m = build_fixture_neck().to(dev)
    with torch.no_grad():
        got = m(torch.from_numpy(fx["x"]).to(dev)).cpu().numpy()
    ref_err = float(np.abs(fx["y32"] - fx["y64"]).max())
    err = float(np.abs(got - fx["y64"]).max())
    print("fixture neck: kernel max|got - y64| = %.3e, reference max|y32 - y64| = %.3e, range %.3e" % (err, ref_err, float(np.abs(fx["y64"]).max())))
    assert got.shape == fx["y64"].shape
    assert err <= 4 * ref_err


def test_whole_neck_shipped_channels_vs_float64():
    """256 -> 128 / 256 -> 512 channels, layer_nums [5, 5], on two small maps.  Bar: 4 x the error of forward_layers in fp32 on the CPU
    against forward_layers in float64, pooled over both maps."""
    from shasta_amd import builder
    dev = _dev()
    torch.manual_seed(31)
    m = builder.build_neck(dict(type="RPN", **SHIPPED)).eval()
    g = torch.Generator().manual_seed(32)
    randomize_bn(m, g)
    xs = [torch.relu(torch.randn(1, 256, 6, 34, generator=g)), torch.relu(torch.randn(2, 256, 12, 66, generator=g))]
    refs = [layers64(m, x) for x in xs]
    with torch.no_grad():
        ref_err = max(float((m.forward_layers(x).double() - r).abs().max()) for x, r in zip(xs, refs))
    m = m.to(dev)
    errs = []
    with torch.no_grad():
        for x, r in zip(xs, refs):
            got = m(x.to(dev)).cpu()
            assert got.shape == r.shape and got.shape[1] == 512
            errs.append(float((got.double() - r).abs().max()))
    print("shipped-channel neck: kernel max err %.3e (per map %s), fp32 forward_layers max err %.3e, range %.3e"
          % (max(errs), ["%.3e" % e for e in errs], ref_err, max(float(r.abs().max()) for r in refs)))
    assert max(errs) <= 4 * ref_err


class _CountingLib:
    def __init__(self, lib):
        self._lib, self.calls = lib, 0

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name != "shasta_neck_layer_f32":
            return fn

        def counted(*a):
            self.calls += 1
            return fn(*a)
        return counted


def test_kernel_path_is_taken(monkeypatch):
    from shasta_amd import hip
    fx, dev = fixture(), _dev()
    m = build_fixture_neck().to(dev)
    x = torch.from_numpy(fx["x"]).to(dev)
    ref = copy.deepcopy(m).train()  # (before the wrappers below: an independent module with the same tensors)
    counting = _CountingLib(hip.load())
    monkeypatch.setattr(hip, "load", lambda: counting)
    layer_calls = []
    inner = m.forward_layers
    monkeypatch.setattr(m, "forward_layers", lambda t: (layer_calls.append(1), inner(t))[1])
    with torch.no_grad():
        y = m(x)
    assert counting.calls == 7 and not layer_calls  # 3 + 2 block layers, 2 deblocks: one call per conv + BatchNorm + ReLU
    # requires_grad input in eval mode: the nn layers, differentiable
    xg = x.clone().requires_grad_(True)
    yg = m(xg)
    assert counting.calls == 7 and len(layer_calls) == 1 and yg.requires_grad
    np.testing.assert_allclose(yg.detach().cpu().numpy(), y.cpu().numpy(), rtol=1e-4, atol=2e-5)
    # train() mode: batch statistics, as torch computes them
    m.train()
    with torch.no_grad():
        yt = m(x)
        rt = ref.forward_layers(x)
    assert counting.calls == 7 and len(layer_calls) == 2
    np.testing.assert_allclose(yt.cpu().numpy(), rt.cpu().numpy(), rtol=1e-5, atol=1e-6)
    assert float((yt - y).abs().max()) > 1e-3  # not the running statistics
    assert int(m.blocks[0][2].num_batches_tracked) == 1


def _check_follows(m, x, what):
    """A stale packed layer is off by the size of the values themselves; K0's bar tells that apart from fp32 summation order."""
    ref = layers64(m, x)
    with torch.no_grad():
        got = m(x).cpu().double()
    scale = float(ref.abs().max())
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-4, atol=2e-5 * max(1.0, scale), err_msg=what)
    return got


def test_caches_follow_the_parameters():
    fx, dev = fixture(), _dev()
    m = build_fixture_neck().to(dev)
    x = torch.from_numpy(fx["x"]).to(dev)
    y0 = _check_follows(m, x, "first forward")
    g = torch.Generator().manual_seed(7)
    other = {k: (torch.randn(v.shape, generator=g) * 0.1 if "weight" in k and v.ndim == 4 else
                 0.5 + torch.rand(v.shape, generator=g) if v.ndim == 1 else torch.from_numpy(v.copy())) for k, v in fx["used"].items()}
    m.load_state_dict(other)
    y1 = _check_follows(m, x, "after load_state_dict")
    assert float((y1 - y0).abs().max()) > 1e-3
    with torch.no_grad():
        m.deblocks[1][1].running_var.copy_(torch.full((32,), 9.0))
        m.blocks[0][2].running_mean.copy_(torch.full((32,), -0.5))
    y2 = _check_follows(m, x, "after an in-place copy_ into BatchNorm statistics")
    assert float((y2 - y1).abs().max()) > 1e-3
    m = m.cpu()
    with torch.no_grad():
        m.blocks[1][1].weight.mul_(0.5)
    m = m.to(dev)
    y3 = _check_follows(m, x, "after .to()")
    assert float((y3 - y2).abs().max()) > 1e-4


def test_same_bits_every_run_and_under_graph_replay():
    fx, dev = fixture(), _dev()
    m = build_fixture_neck().to(dev)
    x = torch.from_numpy(fx["x"]).to(dev)
    x2 = torch.relu(torch.randn(x.shape, generator=torch.Generator().manual_seed(3))).to(dev)
    with torch.no_grad():
        e1 = m(x).clone()
        e1b = m(x).clone()
        e2 = m(x2).clone()
        assert torch.equal(e1, e1b) and not torch.equal(e1, e2)
        static = x.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(static)  # warm-up: packed layers and ping-pong buffers exist from here on
        torch.cuda.current_stream().wait_stream(side)
        bufs = [b.data_ptr() for b in m._bufs]
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = m(static)
        assert [b.data_ptr() for b in m._bufs] == bufs
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, e1)
        static.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, e2)


def test_refusals_come_before_any_launch():
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    g = torch.Generator().manual_seed(5)
    w, bn = layer_tensors(C3S2, 16, 32, g)
    packed = _pack(lib, hip, C3S2, 16, 32, w, bn, dev)
    x = torch.ones(1, 16, 6, 34, device=dev)
    out = torch.full((1, 40, 3, 17), SENTINEL, device=dev)
    s = hip.stream_ptr()

    def call(xx=x, cin=16, H=6, W=34, pk=packed, nbytes=None, cout=32, o=out, total=40, off=8):
        return lib.shasta_neck_layer_f32(hip.ptr(xx), 1, cin, H, W, hip.ptr(pk), pk.numel() if nbytes is None else nbytes, C3S2, cout,
                                         None if o is None else hip.ptr(o), total, off, s)

    assert call(H=5) == E_UNSUPPORTED                       # odd H under stride 2
    assert call(W=33) == E_UNSUPPORTED
    assert call(cin=12) == E_UNSUPPORTED
    assert call(cout=48) == E_UNSUPPORTED
    assert call(nbytes=packed.numel() - 1) == E_WORKSPACE   # one byte short
    assert call(o=None) == E_ARG                            # null out
    assert call(off=9) == E_ARG                             # out_channel_offset + Cout > out_channels_total
    assert call(off=-1) == E_ARG
    assert b"slice" in lib.shasta_last_error()
    # the pack refuses alike
    ts = [t.to(dev) for t in [w] + bn]
    small = torch.empty(packed.numel() - 1, dtype=torch.uint8, device=dev)
    assert lib.shasta_neck_layer_pack_f32(*[hip.ptr(t) for t in ts], EPS, C3S2, 16, 32, hip.ptr(small), small.numel(), s) == E_WORKSPACE
    assert lib.shasta_neck_layer_pack_f32(*[hip.ptr(t) for t in ts], EPS, C3S2, 12, 32, hip.ptr(packed), packed.numel(), s) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert call() == 0                                      # and the good call writes channels 8 .. 39 only
    torch.cuda.synchronize()
    assert bool((out[:, :8] == SENTINEL).all()) and bool((out[:, 8:] >= 0).all())


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_c3s1_contains_a_non_finite_pixel(bad):
    """One bad input pixel, next to the tile's column seam (x = 32 | 33) and row seam (y = 3 | 4): every non-finite output lies in its
    3 x 3 neighbourhood, everything outside equals the clean run bit for bit."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    g = torch.Generator().manual_seed(11)
    w, bn = layer_tensors(C3S1, 16, 64, g)
    packed = _pack(lib, hip, C3S1, 16, 64, w, bn, dev)
    x = torch.relu(torch.randn(1, 16, 9, 40, generator=g)).to(dev)
    rc, clean = _run_layer(lib, hip, C3S1, x, packed, 64, 64, 0)
    assert rc == 0 and bool(torch.isfinite(clean).all())
    py, px = 4, 32
    xb = x.clone()
    xb[0, 3, py, px] = bad
    rc, got = _run_layer(lib, hip, C3S1, xb, packed, 64, 64, 0)
    assert rc == 0
    inside = torch.zeros(9, 40, dtype=torch.bool, device=dev)
    inside[py - 1:py + 2, px - 1:px + 2] = True
    nonfinite = ~torch.isfinite(got[0])
    assert bool(nonfinite.any()) and not bool(nonfinite[:, ~inside].any())
    assert torch.equal(got[0][:, ~inside], clean[0][:, ~inside])
    if bad != bad:  # a NaN reaches all nine outputs of every channel (ReLU keeps it, as torch's does)
        assert bool(torch.isnan(got[0][:, inside]).all())


def test_d2_contains_a_nan_pixel():
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    g = torch.Generator().manual_seed(12)
    w, bn = layer_tensors(D2, 40, 64, g)
    packed = _pack(lib, hip, D2, 40, 64, w, bn, dev)
    x = torch.relu(torch.randn(1, 40, 6, 35, generator=g)).to(dev)
    rc, clean = _run_layer(lib, hip, D2, x, packed, 64, 64, 0)
    assert rc == 0 and bool(torch.isfinite(clean).all())
    py, px = 3, 32
    xb = x.clone()
    xb[0, 39, py, px] = float("nan")
    rc, got = _run_layer(lib, hip, D2, xb, packed, 64, 64, 0)
    assert rc == 0
    inside = torch.zeros(12, 70, dtype=torch.bool, device=dev)
    inside[2 * py:2 * py + 2, 2 * px:2 * px + 2] = True
    assert bool(torch.isnan(got[0][:, inside]).all())
    assert bool(torch.isfinite(got[0][:, ~inside]).all()) and torch.equal(got[0][:, ~inside], clean[0][:, ~inside])


class _MapReader(torch.nn.Module):
    """Stub reader: the example's 'voxels' already hold the dense (B, 16, H, W) map."""

    def __init__(self, **kw):
        super().__init__()

    def forward(self, voxels, num_points):
        return voxels


class _MapBackbone(torch.nn.Module):
    def __init__(self, **kw):
        super().__init__()

    def forward(self, features, coordinates, batch_size, input_shape):
        return features, None


def test_through_shasta():
    """Shasta with the neck configured: extract_feat runs reader -> backbone -> neck -> K0; matched1 / matched2 equal, bit for bit, those
    of the same weights fed the neck's own outputs as bev_map / prev_bev_map."""
    import shasta_amd
    from oracle import shasta_oracle as O
    fx, dev = fixture(), _dev()
    for reg, cls in ((shasta_amd.READERS, _MapReader), (shasta_amd.BACKBONES, _MapBackbone)):
        if reg.get(cls.__name__) is None:
            reg.register_module(cls)
    bev = dict(type="BEVFeatureExtractor", pc_start=[-54, -54], voxel_size=[0.5625, 0.5625], out_stride=8)  # 24 x 24 cells over 108 m
    N, B = 8, 2
    torch.manual_seed(41)
    m = shasta_amd.build_simp_track(dict(type="Shasta", reader=dict(type="_MapReader"), backbone=dict(type="_MapBackbone"),
                                         neck=dict(type="RPN", **fx["cfg"]), bev_extractor=bev, max_obj=N, num_feats=7, num_point=5,
                                         in_channels=64)).eval()
    keys = list(m.state_dict().keys())
    assert "neck.blocks.0.1.weight" in keys and "neck.deblocks.1.1.running_mean" in keys
    assert [k[5:] for k in keys if k.startswith("neck.")] == fx["keys"]
    randomize_bn(m.neck, torch.Generator().manual_seed(42))
    plain = shasta_amd.build_simp_track(dict(type="Shasta", reader=None, backbone=None, neck=None, bev_extractor=bev, max_obj=N, num_feats=7,
                                             num_point=5, in_channels=64)).eval()
    plain.load_state_dict({k: v for k, v in m.state_dict().items() if not k.startswith("neck.")})
    m, plain = m.to(dev), plain.to(dev)
    g = torch.Generator().manual_seed(43)
    maps = [torch.relu(torch.randn(B, 16, 24, 24, generator=g)).to(dev) for _ in range(2)]
    det, prev = O.synth_boxes(g, B, N).to(dev), O.synth_boxes(g, B, N).to(dev)
    ex = dict(det_boxes=det.clone(), prev_det_boxes=prev.clone(), voxels=maps[0], prev_voxels=maps[1], num_points=None, prev_num_points=None,
              coordinates=None, prev_coordinates=None, points=[None] * B, prev_points=[None] * B, shape=[None], prev_shape=[None])
    with torch.no_grad():
        m1, m2, _ = m(ex, train_mode=False)
        ex2 = dict(det_boxes=det.clone(), prev_det_boxes=prev.clone(), bev_map=m.neck(maps[0]), prev_bev_map=m.neck(maps[1]))
        assert ex2["bev_map"].shape == (B, 64, 24, 24)
        r1, r2, _ = plain(ex2, train_mode=False)
    torch.cuda.synchronize()
    assert m1.shape == (B, N, N + 2) and bool(torch.isfinite(m1).all())
    assert torch.equal(m1, r1) and torch.equal(m2, r2)


# two chunks (the minimum) with a partial second workgroup whose tile starts mid-row; six chunks: two trips of the steady loop, staging
# class 12; class 18; a 130-row tile; from 257 columns the rectangular kernels: one chunk, and three (one loop trip + the two-chunk tail)
K0_CASES = [(1, 8, 5, 37), (2, 24, 3, 180), (1, 16, 2, 256), (1, 8, 140, 1), (1, 8, 5, 257), (1, 24, 6, 290)]


@pytest.mark.parametrize("B,cin,H,W", K0_CASES, ids=["%d-%d-%d-%d" % c for c in K0_CASES])
def test_c3s1_equals_shared_conv_bits(B, cin, H, W):
    """K0's f32 kernels (csrc/shared_conv.hip, NHWC) and the neck's C3S1 layer at 64 output channels (NCHW) run one convolution body
    (csrc/conv3x3_f32.hpp) with the pixels as the other MFMA operand: the same fp32 chain per output - the same channel pairs, the same
    taps, commutative products - and, with a zero convolution bias, the same epilogue.  So the outputs are equal bit for bit, alone
    and with K0's second map (x_prev / out_prev) in the same launch."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    g = torch.Generator().manual_seed(77 + cin + H + W)
    w, bn = layer_tensors(C3S1, cin, 64, g)
    x, xp = [torch.relu(torch.randn(B, cin, H, W, generator=g)).to(dev) for _ in range(2)]
    packed = _pack(lib, hip, C3S1, cin, 64, w, bn, dev)
    want = []
    for t in (x, xp):
        rc, out = _run_layer(lib, hip, C3S1, t, packed, 64, 64, 0)
        assert rc == 0, lib.shasta_last_error()
        want.append(out.permute(0, 2, 3, 1).contiguous())
    nbytes = lib.shasta_shared_conv_packed_bytes(cin)
    assert nbytes > 0
    k0 = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ts = [t.to(dev).contiguous() for t in [w, torch.zeros(64)] + bn]
    hip.check(lib.shasta_shared_conv_pack_f32(*[hip.ptr(t) for t in ts], EPS, cin, hip.ptr(k0), nbytes, hip.stream_ptr()),
              "shasta_shared_conv_pack_f32")
    alone, got, gotp = [torch.full((B, H, W, 64), SENTINEL, device=dev) for _ in range(3)]
    s = hip.stream_ptr()
    hip.check(lib.shasta_shared_conv_f32(hip.ptr(x), None, B, cin, H, W, hip.ptr(k0), hip.ptr(alone), None, s), "shasta_shared_conv_f32")
    hip.check(lib.shasta_shared_conv_f32(hip.ptr(x), hip.ptr(xp), B, cin, H, W, hip.ptr(k0), hip.ptr(got), hip.ptr(gotp), s),
              "shasta_shared_conv_f32")
    torch.cuda.synchronize()
    assert bool((want[0] > 0).any()) and not torch.equal(want[0], want[1])
    assert torch.equal(alone, want[0])
    assert torch.equal(got, want[0]) and torch.equal(gotp, want[1])
