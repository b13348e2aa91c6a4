"""GPU: the neck in train() mode through the C ABI - the raw instantiation of the convolution kernels (csrc/neck.hip) and the
batch-statistics BatchNorm2d passes of csrc/bn_maps.hip - against float64.

Every tensor is addressed like a neck layer's output, (base, B, C, plane, channels_total, channel_offset); the buffers are filled with a
sentinel, and every test checks the neighbouring channels and the tail untouched.

Seams of the kernels.  Convolution: those of tests/test_neck_kernels.py (the raw kernels are the same code with another epilogue).
Statistics: a plane is cut into slices of at least 4096 floats, 16 at most (one slice up to 4096, 2 .. 16 up to 65536, beyond that the
slices grow), the slice length rounded up to a multiple of 4; planes with plane % 4 == 0 are read 16 bytes at a time, the others - whose
starts are only 4-byte aligned - float by float; a workgroup of 256 threads with four quads / eight floats in flight per thread.  Apply:
a workgroup owns 4096 floats of one plane, with the same two forms."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import test_neck_kernels as TK
from tests.neck_helpers import C1, C3S1, C3S2, D2, E_ARG, E_UNSUPPORTED, E_WORKSPACE, KIND_NAMES, layer_tensors

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
EPS = float(np.float32(1e-3))
E_ALIGN = -4  # include/shasta_hip.h
PIX_MIN, SLICES, APPLY_SEG = 4096, 16, 4096  # csrc/bn_maps.hip: BNM_PIX_MIN, BNM_SLICES, BNM_APPLY_SEG
WIDTHS = (32, 96, 256)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda", 0)


# ---- 1. raw convolution -------------------------------------------------------------------------------------------
# A subset of test_neck_kernels.LAYER_CASES, per kind one case at each seam that file names: rows 4 | 5, columns 31 | 32 | 33, channel
# blocks 32 | 64 | 96, K chunks of one trip and of several, the zero-padded last chunk of the 1x1 kinds (Cin 8, 40, 72), C3S1's flat form
# at 128 flattened pixels (4 x 32) and beyond (5 x 33, 3 x 127), a one-pixel map, and one width above 256 (the rectangular kernel)
RAW_CASES = [
    (C3S1, 1, 8, 32, 1, 1), (C3S1, 2, 16, 32, 5, 33), (C3S1, 1, 24, 96, 4, 32), (C3S1, 1, 32, 64, 5, 31), (C3S1, 1, 8, 32, 3, 127),
    (C3S1, 1, 8, 96, 5, 257),
    (C3S2, 1, 8, 32, 2, 2), (C3S2, 1, 16, 64, 10, 66), (C3S2, 1, 24, 96, 8, 64), (C3S2, 1, 8, 64, 10, 62),
    (C1, 2, 8, 32, 3, 65), (C1, 1, 40, 96, 4, 32), (C1, 1, 64, 64, 5, 33),
    (D2, 2, 16, 32, 5, 33), (D2, 1, 8, 32, 1, 1), (D2, 1, 40, 96, 4, 32), (D2, 1, 72, 64, 9, 31),
]
assert all(c in TK.LAYER_CASES for c in RAW_CASES)
# not in that list: 129 flattened pixels (3 x 43), the first pixel of the flat form's second workgroup
RAW_CASES.append((C3S1, 1, 8, 32, 3, 43))


def _conv64(kind, x, w):
    x, w = x.double(), w.double()
    if kind == C3S1:
        return F.conv2d(x, w, padding=1)
    if kind == C3S2:
        return F.conv2d(F.pad(x, (1, 1, 1, 1)), w, stride=2)
    return F.conv_transpose2d(x, w, stride=1 if kind == C1 else 2)


@pytest.mark.parametrize("kind,B,cin,cout,H,W", RAW_CASES, ids=["%s-%d-%d-%d-%d-%d" % ((KIND_NAMES[c[0]],) + c[1:]) for c in RAW_CASES])
def test_raw_layer_vs_float64(kind, B, cin, cout, H, W):
    """shasta_neck_layer_raw_f32 on the eval call's packed buffer (random alpha / beta' in it: ignored) into a channel slice at offset 5 of
    Cout + 9 channels = float64 conv2d / conv_transpose2d, no affine, no ReLU.  Inputs of both signs: a stray ReLU fails.  Bar: that of
    test_neck_kernels.test_layer_vs_float64 (the same fp32 chain)."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    g = torch.Generator().manual_seed(2000 * kind + cin + cout + H + W)
    w, bn = layer_tensors(kind, cin, cout, g)
    x = torch.randn(B, cin, H, W, generator=g)
    ref = _conv64(kind, x, w)
    assert float((ref < 0).double().mean()) >= 0.25
    packed = TK._pack(lib, hip, kind, cin, cout, w, bn, dev)
    total, off = cout + 9, 5
    oh, ow = TK._out_hw(kind, H, W)
    out = torch.full((B * total * oh * ow + 64,), SENTINEL, device=dev)
    xd = x.to(dev)
    rc = lib.shasta_neck_layer_raw_f32(hip.ptr(xd), B, cin, H, W, hip.ptr(packed), packed.numel(), kind, cout, hip.ptr(out), total, off,
                                       hip.stream_ptr())
    assert rc == 0, lib.shasta_last_error()
    out = out.cpu()
    assert bool((out[B * total * oh * ow:] == SENTINEL).all())
    out = out[:B * total * oh * ow].view(B, total, oh, ow)
    assert out.shape[2:] == ref.shape[2:]
    assert bool((out[:, :off] == SENTINEL).all()) and bool((out[:, off + cout:] == SENTINEL).all())
    got = out[:, off:off + cout].double()
    scale = float(ref.abs().max())
    print("%s %s raw: max err %.3e, range %.3e, negative share %.2f"
          % (KIND_NAMES[kind], (B, cin, cout, H, W), float((got - ref).abs().max()), scale, float((ref < 0).double().mean())))
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-4, atol=2e-5 * max(1.0, scale))


# ---- 2. statistics ------------------------------------------------------------------------------------------------
# (B, C, plane, channels_total - C, channel_offset).  Planes 1, 15, 33 x 5 (not multiples of 4: the scalar form), 64 and 180 x 3 (the
# 16-byte form); B = 1, 2, 3; C = 32, 96, 256; offsets 0 and odd ones; then both sides of every boundary of the division of the work:
# one slice (PIX_MIN and below) | two; SLICES slices exactly filled | the slices grow; in both forms
BIG = SLICES * PIX_MIN
MAP_CASES = [
    (1, 32, 1, 0, 0), (2, 32, 1, 3, 1), (3, 96, 15, 7, 5), (1, 256, 165, 9, 3), (2, 96, 64, 0, 0), (3, 32, 64, 5, 5), (2, 256, 540, 7, 1),
    (1, 32, PIX_MIN, 3, 3), (2, 32, PIX_MIN + 1, 3, 1), (1, 32, PIX_MIN + 4, 0, 0), (1, 32, 3 * PIX_MIN + 2, 1, 1),
    (1, 32, BIG, 2, 1), (1, 32, BIG + 4, 2, 1), (1, 32, BIG + 77, 1, 1),
]
MAP_IDS = ["%d-%d-%d-%d-%d" % c for c in MAP_CASES]


def _maps(B, C, plane, extra, off, g, dev, cancelling=True):
    """A sentinel-filled (B, C + extra, plane) tensor with a 64-float sentinel tail, random values of both signs in the slice (channel 3:
    mean 1e3, standard deviation 0.1).  Returns the slice on the host and the whole buffer on the device."""
    total = C + extra
    y = torch.randn(B, C, plane, generator=g) * (0.5 + torch.rand(C, generator=g))[None, :, None] + torch.randn(C, generator=g)[None, :, None]
    if cancelling:
        y[:, 3] = 1e3 + 0.1 * torch.randn(B, plane, generator=g)  # sum y^2 - (sum y) mean cancels 8 digits
    buf = torch.full((B * total * plane + 64,), SENTINEL)
    buf[:B * total * plane].view(B, total, plane)[:, off:off + C] = y
    return y, buf.to(dev)


def _untouched(buf, before, B, C, plane, extra, off):
    """Everything outside the slice equals `before` bit for bit (neighbouring channels, the tail)."""
    total = C + extra
    a, b = buf.cpu(), before.cpu()
    assert torch.equal(a[B * total * plane:], b[B * total * plane:])
    a, b = a[:B * total * plane].view(B, total, plane), b[:B * total * plane].view(B, total, plane)
    assert torch.equal(a[:, :off], b[:, :off]) and torch.equal(a[:, off + C:], b[:, off + C:])
    return a[:, off:off + C]


def _stats(lib, hip, buf, B, C, plane, extra, off):
    dev = buf.device
    nbytes = lib.shasta_bn_maps_workspace_bytes(B, C, plane)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    mm = torch.full((2 * C + 4,), SENTINEL, device=dev)
    rc = lib.shasta_bn_maps_stats_f32(hip.ptr(buf), B, C, plane, C + extra, off, hip.ptr(mm), hip.ptr(ws), nbytes, hip.stream_ptr())
    assert rc == 0, lib.shasta_last_error()
    mm = mm.cpu()
    assert bool((mm[2 * C:] == SENTINEL).all())
    return mm[:2 * C]


@pytest.mark.parametrize("B,C,plane,extra,off", MAP_CASES, ids=MAP_IDS)
def test_stats_vs_float64(B, C, plane, extra, off):
    """Bars of test_backbone_train_kernels.test_stats_vs_float64, from the float64 accumulation: the mean is one fp32 rounding of a float64
    quotient (2^-24; 2^-22 leaves room for the sum's own error against the channel's rms), M2 = sum y^2 - (sum y) mean carries the sums'
    error n 2^-53 sum y^2 at most, twice."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    assert (PIX_MIN + 1) % 4 and (BIG + 77) % 4 and BIG + 4 > SLICES * PIX_MIN
    g = torch.Generator().manual_seed(1000 * C + plane % 997 + B)
    y, buf = _maps(B, C, plane, extra, off, g, dev)
    before = buf.clone()
    n = B * plane
    y64 = y.double().permute(1, 0, 2).reshape(C, n)
    mean = y64.mean(1)
    m2 = ((y64 - mean[:, None]) ** 2).sum(1)
    sq = (y64 ** 2).sum(1)
    got = _stats(lib, hip, buf, B, C, plane, extra, off).double()
    assert torch.equal(buf, before)  # the pass reads only
    e_mean, e_m2 = (got[:C] - mean).abs(), (got[C:] - m2).abs()
    bar_mean = 2.0 ** -22 * torch.maximum(mean.abs(), (sq / n).sqrt())
    bar_m2 = 2.0 ** -22 * m2 + n * 2.0 ** -52 * sq
    print("B %d C %d plane %d: mean err / bar %.3f, M2 err / bar %.3f (cancelling channel: M2 %.4g, err %.3e, bar %.3e)"
          % (B, C, plane, float((e_mean / bar_mean).max()), float((e_m2 / bar_m2.clamp_min(1e-300)).max()), float(m2[3]), float(e_m2[3]),
             float(bar_m2[3])))
    assert bool((e_mean <= bar_mean).all()) and bool((e_m2 <= bar_m2).all())
    assert bool((got[C:] >= 0).all())
    assert torch.equal(_stats(lib, hip, buf, B, C, plane, extra, off).double(), got)  # the same bits on a second run


# ---- 3. finalize --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", WIDTHS)
def test_finalize_vs_float64(C):
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    g = torch.Generator().manual_seed(C)
    n, mom = 37, 0.1
    mm = torch.cat([0.5 + torch.rand(C, generator=g), 5.0 + 50.0 * torch.rand(C, generator=g)])  # mean > 0, M2 > 0
    rm0, rv0 = 0.2 + torch.rand(C, generator=g), 0.5 + torch.rand(C, generator=g)                  # running mean > 0: no cancellation
    mmd = mm.to(dev)
    stat = torch.full((2 * C + 4,), SENTINEL, device=dev)
    rm, rv = torch.cat([rm0, torch.full((4,), SENTINEL)]).to(dev), torch.cat([rv0, torch.full((4,), SENTINEL)]).to(dev)
    nbt = torch.tensor(5, dtype=torch.int64, device=dev)
    rc = lib.shasta_bn_maps_finalize_f32(hip.ptr(mmd), C, float(n), EPS, mom, hip.ptr(stat), hip.ptr(rm), hip.ptr(rv),
                                         ctypes.c_void_p(nbt.data_ptr()), hip.stream_ptr())
    assert rc == 0, lib.shasta_last_error()
    stat_c = stat.cpu()
    assert bool((stat_c[2 * C:] == SENTINEL).all()) and torch.equal(stat_c[:C], mm[:C])
    assert bool((rm[C:] == SENTINEL).all()) and bool((rv[C:] == SENTINEL).all())
    mean64, m264 = mm[:C].double(), mm[C:].double()
    np.testing.assert_allclose(stat_c[C:2 * C].double().numpy(), (1.0 / torch.sqrt(m264 / n + EPS)).numpy(), rtol=2.0 ** -22, atol=0)
    np.testing.assert_allclose(rm[:C].cpu().double().numpy(), ((1 - mom) * rm0.double() + mom * mean64).numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(rv[:C].cpu().double().numpy(), ((1 - mom) * rv0.double() + mom * m264 / (n - 1)).numpy(), rtol=1e-6, atol=0)
    assert int(nbt) == 6
    # NULL running pointers: nothing but stat is written
    stat2 = torch.full((2 * C + 4,), SENTINEL, device=dev)
    rm1, rv1 = rm.clone(), rv.clone()
    rc = lib.shasta_bn_maps_finalize_f32(hip.ptr(mmd), C, float(n), EPS, mom, hip.ptr(stat2), None, None, None, hip.stream_ptr())
    assert rc == 0, lib.shasta_last_error()
    assert torch.equal(stat2, stat) and torch.equal(rm, rm1) and torch.equal(rv, rv1) and int(nbt) == 6 and torch.equal(mmd.cpu(), mm)


# ---- 4. apply -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,plane,extra,off", MAP_CASES, ids=MAP_IDS)
def test_apply_in_place_vs_float64(B, C, plane, extra, off):
    """ReLU off and on, a planted NaN, in place on the slice; against float64 of the same formula from the same fp32 stat.  Bar of
    test_backbone_train_kernels.test_apply_vs_float64: three roundings on the product chain and one for the addition - 8 ulp of the
    magnitudes added."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    assert 3 * PIX_MIN + 2 > 3 * APPLY_SEG  # (a plane of several apply segments with a partial last one, in the scalar form)
    g = torch.Generator().manual_seed(7 * C + plane % 991 + B)
    y, _ = _maps(B, C, plane, extra, off, g, dev, cancelling=False)
    y = y * 2.0 + 0.5
    y[B // 2, C // 2, plane // 2] = float("nan")  # a NaN stays a NaN through the ReLU
    stat = torch.cat([0.5 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)])
    gamma, beta = 0.5 + torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g)
    t = (y.double() - stat[:C].double()[None, :, None]) * stat[C:].double()[None, :, None] * gamma.double()[None, :, None]
    b64 = beta.double()[None, :, None]
    bar = 8 * 2.0 ** -24 * (t.abs() + b64.abs())
    sd, gd, bd = stat.to(dev), gamma.to(dev), beta.to(dev)
    total = C + extra
    for relu in (0, 1):
        ref = t + b64
        if relu:
            ref = torch.relu(ref)
        buf = torch.full((B * total * plane + 64,), SENTINEL)
        buf[:B * total * plane].view(B, total, plane)[:, off:off + C] = y
        buf = buf.to(dev)
        before = buf.clone()
        rc = lib.shasta_bn_maps_apply_f32(hip.ptr(buf), B, C, plane, total, off, hip.ptr(sd), hip.ptr(gd), hip.ptr(bd), relu, hip.stream_ptr())
        assert rc == 0, lib.shasta_last_error()
        got = _untouched(buf, before, B, C, plane, extra, off).double()
        nan = torch.isnan(ref)
        assert int(nan.sum()) == 1 and bool(torch.isnan(got[nan]).all()) and not bool(torch.isnan(got[~nan]).any())
        err = (got - ref).abs()[~nan]
        ratio = float((err / bar[~nan].clamp_min(1e-300)).max()) if err.numel() else 0.0
        print("B %d C %d plane %d relu %d: worst err / bar %.3f" % (B, C, plane, relu, ratio))
        assert bool((err <= bar[~nan]).all()), (relu, ratio)
        if relu:
            assert bool((got[~nan] >= 0).all())
        if B * C * plane >= 1024:  # enough values for both signs: the ReLU clips a share of them, and only the ReLU does
            assert float((got[~nan] == 0).double().mean()) > 0.05 if relu else float(got[~nan].min()) < -0.1


# ---- 5. refusals --------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch():
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    B, C, plane, extra, off = 2, 32, 64, 8, 3
    g = torch.Generator().manual_seed(9)
    _, buf = _maps(B, C, plane, extra, off, g, dev)
    before = buf.clone()
    total = C + extra
    nbytes = lib.shasta_bn_maps_workspace_bytes(B, C, plane)
    assert nbytes >= B * 2 * C * 8 and lib.shasta_bn_maps_workspace_bytes(B, 48, plane) == 0
    assert lib.shasta_bn_maps_workspace_bytes(B, C, 3 * PIX_MIN) > lib.shasta_bn_maps_workspace_bytes(B, C, PIX_MIN)
    assert lib.shasta_bn_maps_supported(32) == 1 and lib.shasta_bn_maps_supported(48) == 0 and lib.shasta_bn_maps_supported(0) == 0
    ws = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    mm = torch.full((2 * C + 4,), SENTINEL, device=dev)
    stat = torch.cat([torch.zeros(C), torch.ones(C)]).to(dev)
    ones = torch.ones(C, device=dev)
    s = hip.stream_ptr()

    def stats(y=buf, b=B, c=C, p=plane, tot=total, o=off, m=mm, w=ws, nb=nbytes):
        return lib.shasta_bn_maps_stats_f32(hip.ptr(y), b, c, p, tot, o, None if m is None else hip.ptr(m), hip.ptr(w), nb, s)

    def apply(y=buf, b=B, c=C, p=plane, tot=total, o=off, st=stat):
        return lib.shasta_bn_maps_apply_f32(hip.ptr(y), b, c, p, tot, o, None if st is None else hip.ptr(st), hip.ptr(ones), hip.ptr(ones), 1, s)

    for call in (stats, apply):
        assert call(c=48) == E_UNSUPPORTED and call(c=16) == E_UNSUPPORTED and call(c=0) == E_UNSUPPORTED   # widths that are not served
        assert call(b=0) == E_ARG and call(p=0) == E_ARG                                                    # n = 0
        assert call(o=extra + 1) == E_ARG and call(o=-1) == E_ARG and call(tot=C - 1, o=0) == E_ARG         # the slice leaves the tensor
        assert b"slice" in lib.shasta_last_error()
        assert call(b=65536) == E_UNSUPPORTED                                                               # the grid limit
        assert call(y=buf[1:]) == E_ALIGN
    assert stats(nb=nbytes - 1) == E_WORKSPACE and stats(m=None) == E_ARG and apply(st=None) == E_ARG
    assert lib.shasta_bn_maps_finalize_f32(hip.ptr(mm), 48, 10.0, EPS, 0.1, hip.ptr(stat), None, None, None, s) == E_UNSUPPORTED
    assert lib.shasta_bn_maps_finalize_f32(hip.ptr(mm), C, 0.0, EPS, 0.1, hip.ptr(stat), None, None, None, s) == E_ARG
    assert lib.shasta_bn_maps_finalize_f32(None, C, 10.0, EPS, 0.1, hip.ptr(stat), None, None, None, s) == E_ARG
    # the raw layer refuses as the eval call does
    w, bn = layer_tensors(C3S2, 16, 32, g)
    packed = TK._pack(lib, hip, C3S2, 16, 32, w, bn, dev)
    x = torch.ones(1, 16, 6, 34, device=dev)
    out = torch.full((1, 40, 3, 17), SENTINEL, device=dev)

    def raw(cin=16, H=6, nb=None, cout=32, o=out, off_=8):
        return lib.shasta_neck_layer_raw_f32(hip.ptr(x), 1, cin, H, 34, hip.ptr(packed), packed.numel() if nb is None else nb, C3S2, cout,
                                             None if o is None else hip.ptr(o), 40, off_, s)

    assert raw(H=5) == E_UNSUPPORTED and raw(cin=12) == E_UNSUPPORTED and raw(cout=48) == E_UNSUPPORTED
    assert raw(nb=packed.numel() - 1) == E_WORKSPACE and raw(o=None) == E_ARG and raw(off_=9) == E_ARG
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and bool((mm == SENTINEL).all()) and bool((ws == 0x5A).all()) and bool((out == SENTINEL).all())
    assert torch.equal(stat.cpu(), torch.cat([torch.zeros(C), torch.ones(C)]))
    assert stats() == 0 and raw() == 0  # and the good calls write their slices only
    torch.cuda.synchronize()
    assert bool((mm[:2 * C] != SENTINEL).all()) and bool((mm[2 * C:] == SENTINEL).all()) and torch.equal(buf, before)
    assert bool((out[:, :8] == SENTINEL).all()) and bool((out[:, 8:] != SENTINEL).all())
