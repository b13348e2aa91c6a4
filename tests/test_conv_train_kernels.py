"""K0's train-mode kernels (csrc/shared_conv_train.hip) one at a time through the C ABI: every entry gets inputs made on the host and is
compared with a float64 evaluation of those same inputs, so that a failure names the kernel and the shape.  No forward conv kernel is
involved: y is an input.  tests/test_shared_conv_train.py runs the same kernels through the module.

The shapes (CASES) are the smallest that reach each seam of the weight-gradient kernel: its four instantiations (padded row width 64 ...
256), widths with exactly one zero padding column (63, 127, 191, 255) and with a whole round of padding (64, 128, 192), the 16-column
k-step seam (15, 16, 17), fewer rows than the LDS ring holds, the row split and its uneven last slices, channel blocks with 1 / 31 of 32
channels live, x_prev == NULL, workgroup totals below 8, equal to 8 and no multiple of 8.

The ReLU kink: the kernels decide pre > 0 in fp32, the reference in float64.  gout is set to 0 wherever the float64 |pre| < 1e-3 (at most
1 % of it, asserted), so g' = 0 on either branch there and every output is compared in full.

Measured on an MI355X, largest error / bar (the tests print their figures with -s): bn_stats M2 0.06 (5.8e-8 relative), bn_relu_apply
0.008, bn_relu_bwd_reduce sums 0.006, dy pieces 0.15 (4.95 * 2^-24 of the 2^-19 bound_c, bit for bit the fp32 host restatement), conv_wgrad
0.033; per case in the docstrings of test_bn_relu_bwd_dy and test_conv_wgrad.
"""
import ctypes as C
import functools
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from shasta_amd import hip

gpu = pytest.mark.gpu
EPS = 1e-5
E_ARG, E_WORKSPACE = -1, -2  # include/shasta_hip.h
DY_BAR = 2.0 ** -19          # of bound_c: 6 x the 5.3 * 2^-24 an fp32 restatement of the kernel's formula deviates from float64 (a dropped
                             # low piece costs 2^-11)
# key: B, Cin, H, W, single (x_prev NULL), conv_wgrad_kernel<n>, workgroups
CASES = {
    "a": (1, 8, 1, 63, True, 1, 1),      # one pad column; one row; nimg = 1
    "b": (1, 33, 3, 64, False, 2, 4),    # first width of <2>; the second channel block holds one channel
    "c": (2, 40, 17, 127, False, 2, 16),  # two slices 9 + 8, relabelled in full
    "d": (3, 5, 15, 100, False, 2, 12),  # first H that splits; the relabelling covers 8 of 12
    "e": (1, 32, 33, 128, False, 3, 8),  # slices 9, 9, 9, 6
    "f": (2, 31, 31, 191, False, 3, 16),  # slices 8, 8, 8, 7; one pad column
    "g": (1, 64, 16, 192, False, 4, 8),  # first width of <4>
    "h": (1, 16, 2, 255, False, 4, 2),   # widest map; one pad column
    "i": (1, 1, 14, 1, False, 1, 2),     # odd W; one column; largest H that does not split
    "j": (1, 65, 9, 17, False, 1, 6),    # three channel blocks
    "k": (1, 8, 5, 15, False, 1, 2),     # 16-column k-step seam
    "l": (1, 8, 5, 16, False, 1, 2),
}
KEYS = sorted(CASES)


# ---- the float64 reference ------------------------------------------------------------------------------------------------------------
def _bn64(y, gout, gamma, beta, zero_kink=True):
    """One BatchNorm call in float64 from y, gout (.., 64) and gamma, beta (64): everything the kernels compute, and the gout actually
    used (zero within 1e-3 of the ReLU kink)."""
    shape = y.shape
    y2 = y.double().reshape(-1, 64)
    M = y2.shape[0]
    n = float(M)
    ga, be = gamma.double(), beta.double()
    mean = y2.mean(0)
    m2 = (y2 - mean).square().sum(0)
    var = m2 / n
    invstd = 1.0 / torch.sqrt(var + EPS)
    xhat = (y2 - mean) * invstd
    pre = xhat * ga + be
    g = gout.reshape(-1, 64).clone()
    kink = pre.abs() < 1e-3
    if zero_kink:
        g[kink] = 0
    gp = g.double() * (pre > 0)
    s1, s2 = gp.sum(0), (gp * xhat).sum(0)
    a = ga * invstd
    dy = a * (gp - s1 / n - xhat * (s2 / n))
    maxg, maxx = gp.abs().amax(0), xhat.abs().amax(0)
    bound = a.abs() * (maxg + (s1 / n).abs() + maxx * (s2 / n).abs())
    return NS(n=n, M=M, mean=mean, m2=m2, var=var, invstd=invstd, xhat=xhat.reshape(shape), pre=pre.reshape(shape),
              out=torch.relu(pre).reshape(shape), gout=g.reshape(shape), gp=gp.reshape(shape), s1=s1, s2=s2, a=a, dy=dy.reshape(shape),
              maxg=maxg, maxx=maxx, bound=bound, kink_frac=float(kink.double().mean()))


def _dw64(maps, dys):
    """dW[o, c, ky, kx] = sum_p dy[p, o] x[c, p + (ky - 1, kx - 1)] over all maps, zero outside a map; float64."""
    x = torch.cat(maps).double()
    dy = torch.cat([d.double() for d in dys])
    nimg, cin, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1))
    d2 = dy.reshape(-1, 64).t().contiguous()
    dw = torch.zeros(64, cin, 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            dw[:, :, ky, kx] = d2 @ xp[:, :, ky:ky + H, kx:kx + W].permute(0, 2, 3, 1).reshape(-1, cin)
    return dw


def _range_exp(bound):
    """range_exponent_bits (csrc/common.hpp) of each entry: the e with bound * 2^e in [2^13, 2^14), 0 for zero and non-finite bounds."""
    out = []
    for b in bound.tolist():
        out.append(0 if not (0.0 < b < math.inf) else max(-60, min(60, 14 - math.frexp(b)[1])))
    return out


def _stat32(r):
    return torch.cat([r.mean, r.invstd]).float()


def _sums32(r):
    return torch.cat([r.s1, r.s2, r.maxg, r.maxx]).float()


def _dy_f32(y, g, gamma, beta, stat, sums_global, sums_local, n_global):
    """The formula of bn_bwd_dy_kernel restated in fp32 on the host, the two-piece fp16 cut included -> (decoded dy in float64, exponents)."""
    f = torch.float32
    mean, inv = stat[:64], stat[64:]
    a = gamma * inv
    mg = (sums_global[:64].double() / n_global).to(f)
    mgx = (sums_global[64:128].double() / n_global).to(f)
    bound = a.abs() * ((sums_local[128:192] + mg.abs()) + sums_local[192:256] * mgx.abs())
    e = torch.tensor(_range_exp(bound), dtype=torch.int32)
    sc = torch.ldexp(torch.ones(64, dtype=f), e)
    xh = (y - mean) * inv
    pre = xh * gamma + beta
    gp = torch.where(pre > 0, g, torch.zeros_like(g))
    v = (((gp - mg) - xh * mgx) * a) * sc
    hi = v.half()
    lo = (v - hi.float()).half()
    return (hi.double() + lo.double()) * torch.ldexp(torch.ones(64, dtype=torch.float64), -e), e


# ---- the inputs of a case ---------------------------------------------------------------------------------------------------------
def _host(key, variant="base"):
    return _host_cached(key, variant)


@functools.lru_cache(maxsize=None)
def _host_cached(key, variant):
    """Inputs of a case and their float64 reference.  variant: "dead" = channel 3 dead (beta = -50) and channel 9 with gamma = 0;
    "zeroimg" = image 1 all zero."""
    B, cin, H, W, single = CASES[key][:5]
    g = torch.Generator().manual_seed(1000 + ord(key))
    x = torch.relu(torch.randn(B, cin, H, W, generator=g))
    xp = torch.relu(torch.randn(B, cin, H, W, generator=g)) * 1.7
    w = torch.randn(64, cin, 3, 3, generator=g) / math.sqrt(9.0 * cin)
    b = torch.randn(64, generator=g) * 0.3
    gamma = torch.rand(64, generator=g) + 0.5
    beta = torch.rand(64, generator=g) * 0.6 - 0.3
    maps = [x] if single else [x, xp]
    gouts = [torch.randn(B, H, W, 64, generator=g) for _ in maps]
    ys = []
    for m in maps:
        y = F.conv2d(m, w, b, padding=1).permute(0, 2, 3, 1).contiguous()
        # per channel |mean| <= 1.5 std (the few pixels of the smallest maps can leave a channel's bias far outside its spread)
        mean, std = y.reshape(-1, 64).mean(0), y.reshape(-1, 64).std(0, unbiased=False)
        y = (y - (mean - torch.maximum(torch.minimum(mean, 1.5 * std), -1.5 * std))).contiguous()
        assert bool((y.double().reshape(-1, 64).mean(0).abs() <= 2 * y.double().reshape(-1, 64).std(0, unbiased=False)).all())
        ys.append(y)
    if variant == "dead":
        gamma, beta = gamma.clone(), beta.clone()
        beta[3] = -50.0
        gamma[9], beta[9] = 0.0, 0.2
    if variant == "zeroimg":  # (y is an input of its own here: only the weight gradient sees the map)
        maps[0] = maps[0].clone()
        maps[0][1] = 0
    refs = [_bn64(y, go, gamma, beta) for y, go in zip(ys, gouts)]
    for r in refs:
        assert r.kink_frac <= 0.01, r.kink_frac
    xmax = torch.cat([m.abs().amax(dim=(1, 2, 3)) for m in maps]).contiguous().view(torch.int32)
    return NS(B=B, cin=cin, H=H, W=W, single=single, maps=maps, ys=ys, gouts=[r.gout for r in refs], gamma=gamma, beta=beta, refs=refs,
              xmax=xmax, nimg=B * len(maps), dw64=_dw64(maps, [r.dy for r in refs]))


@functools.lru_cache(maxsize=None)
def _rows(M, far=False):
    """(M, 64) activations and gradients for the reduction passes; far: mean = 300 std."""
    g = torch.Generator().manual_seed(77 + M + int(far))
    std = torch.rand(64, generator=g) + 0.5
    mean = (torch.rand(64, generator=g) * 2 - 1) * std
    if far:
        mean = 300.0 * std
    y = (torch.randn(M, 64, generator=g) * std + mean).contiguous()
    gamma = torch.rand(64, generator=g) + 0.5
    beta = torch.rand(64, generator=g) * 0.6 - 0.3
    r = _bn64(y, torch.randn(M, 64, generator=g), gamma, beta)
    assert r.kink_frac <= 0.01
    return NS(y=y, gamma=gamma, beta=beta, ref=r)


# ---- CPU tests ----------------------------------------------------------------------------------------------------------------------
def test_float64_restatement_matches_autograd():
    """The reference the GPU tests compare with (_bn64, _dw64) against torch autograd of relu(batch_norm(conv2d(x))) in float64."""
    g = torch.Generator().manual_seed(4)
    B, cin, H, W = 2, 5, 6, 7
    x = torch.relu(torch.randn(B, cin, H, W, generator=g, dtype=torch.float64))
    w = (torch.randn(64, cin, 3, 3, generator=g, dtype=torch.float64) / 6).requires_grad_(True)
    b = (torch.randn(64, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    gamma = (torch.rand(64, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = (torch.rand(64, generator=g, dtype=torch.float64) * 0.6 - 0.3).requires_grad_(True)
    gout = torch.randn(B, H, W, 64, generator=g, dtype=torch.float64)
    y = F.conv2d(x, w, b, padding=1)
    y.retain_grad()
    r = _bn64(y.detach().permute(0, 2, 3, 1), gout, gamma.detach(), beta.detach())
    out = torch.relu(F.batch_norm(y, None, None, gamma, beta, True, 0.1, EPS)).permute(0, 2, 3, 1)
    (out * r.gout).sum().backward()

    def close(got, want, what):
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), what
    close(r.out, out.detach(), "out")
    close(r.dy, y.grad.permute(0, 2, 3, 1), "dy")
    close(r.s1, beta.grad, "dbeta")
    close(r.s2, gamma.grad, "dgamma")
    close(_dw64([x], [r.dy]), w.grad, "dweight")
    close(r.dy.reshape(-1, 64).sum(0), b.grad, "dbias")
    assert float(r.dy.abs().reshape(-1, 64).amax(0).sub(r.bound).max()) <= 1e-12  # |dy| <= bound_c
    d = float((r.dy - y.grad.permute(0, 2, 3, 1)).abs().max() / y.grad.abs().max())
    print("restatement vs autograd: dy differs by %.1e of its range" % d)


def test_fp32_restatement_of_the_dy_formula_is_within_the_bar():
    """Where DY_BAR comes from: the kernel's formula in fp32 on the host, pieces included, against float64 - no kernel involved."""
    worst = 0.0
    for key in ("a", "b", "c", "i", "j", "k"):
        h = _host(key)
        for y, go, r in zip(h.ys, h.gouts, h.refs):
            dec, _ = _dy_f32(y, go, h.gamma, h.beta, _stat32(r), _sums32(r), _sums32(r), r.n)
            worst = max(worst, float(((dec - r.dy).abs() / r.bound).max()))
    print("fp32 restatement of dy: worst deviation %.2f * 2^-24 of bound_c (bar 2^-19 = 32 * 2^-24)" % (worst * 2.0 ** 24))
    assert worst <= DY_BAR


def _pw_and_workgroups(lib, key):
    B, cin, H, W, single = CASES[key][:5]
    nimg = B if single else 2 * B
    pw = (lib.shasta_conv_dy_bytes(nimg, H, W) // (nimg * H) - 64 * 8) // 256  # 256 bytes of pieces per padded column of a row
    nsplit = lib.shasta_conv_wgrad_workspace_bytes(nimg, cin, H, W) // (64 * cin * 9 * 4)
    return pw, nsplit * ((cin + 31) // 32), nsplit // nimg


def test_case_table_reaches_what_it_claims():
    """From the size queries alone (no GPU): the instantiation and the workgroup total of every case."""
    lib = hip.load()
    inst, totals = set(), set()
    for key in KEYS:
        B, cin, H, W, single, want_inst, want_wgs = CASES[key]
        assert lib.shasta_conv_train_supported(cin, H, W) == 1
        pw, wgs, _ = _pw_and_workgroups(lib, key)
        assert pw % 64 == 0 and pw > W >= pw - 64, (key, pw)
        assert (pw // 64, wgs) == (want_inst, want_wgs), (key, pw, wgs)
        inst.add(pw // 64)
        totals.add(wgs)
    assert inst == {1, 2, 3, 4}
    assert any(t < 8 for t in totals) and 8 in totals and any(t > 8 and t % 8 for t in totals) and any(t > 8 and t % 8 == 0 for t in totals)
    assert {63, 127, 191, 255} <= {CASES[k][3] for k in KEYS}
    assert [_pw_and_workgroups(lib, k)[2] for k in "cdefg"] == [2, 2, 4, 4, 2]  # row slices per image
    assert lib.shasta_conv_train_supported(16, 5, 256) == 0 and lib.shasta_conv_dy_bytes(0, 5, 5) == 0
    assert lib.shasta_conv_wgrad_workspace_bytes(0, 8, 5, 5) == 0 and lib.shasta_bn_workspace_bytes() == 1024 * 4 * 64 * 8


# ---- calling the kernels --------------------------------------------------------------------------------------------------------
def _dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda", 0)


def _up(t):
    return t.contiguous().to(_dev())


def _bn_ws(lib):
    return torch.full((lib.shasta_bn_workspace_bytes() // 8,), float("nan"), dtype=torch.float64, device=_dev())


def _k_stats(lib, y):
    mm = torch.full((128,), float("nan"), device=_dev())
    ws = _bn_ws(lib)
    hip.check(lib.shasta_bn_stats_f32(hip.ptr(y), y.numel() // 64, hip.ptr(mm), hip.ptr(ws), ws.numel() * 8, hip.stream_ptr()), "bn_stats")
    return mm


def _k_finalize(lib, mm, n, mom=0.1, rm=None, rv=None, nbt=None):
    stat = torch.full((128,), float("nan"), device=_dev())
    hip.check(lib.shasta_bn_finalize_f32(hip.ptr(mm), n, EPS, mom, hip.ptr(stat), hip.ptr(rm), hip.ptr(rv),
                                         None if nbt is None else C.c_void_p(nbt.data_ptr()), hip.stream_ptr()), "bn_finalize")
    return stat


def _k_apply(lib, y, stat, gamma, beta):
    out = torch.full_like(y, float("nan"))
    hip.check(lib.shasta_bn_relu_apply_f32(hip.ptr(y), y.numel() // 64, hip.ptr(stat), hip.ptr(gamma), hip.ptr(beta), hip.ptr(out),
                                           hip.stream_ptr()), "bn_relu_apply")
    return out


def _k_reduce(lib, y, g, stat, gamma, beta):
    sums = torch.full((256,), float("nan"), device=_dev())
    ws = _bn_ws(lib)
    hip.check(lib.shasta_bn_relu_bwd_reduce_f32(hip.ptr(y), hip.ptr(g), y.numel() // 64, hip.ptr(stat), hip.ptr(gamma), hip.ptr(beta),
                                                hip.ptr(sums), hip.ptr(ws), ws.numel() * 8, hip.stream_ptr()), "bn_relu_bwd_reduce")
    return sums


def _dy_buffer(lib, nimg_total, H, W):
    return torch.full(((lib.shasta_conv_dy_bytes(nimg_total, H, W) + 3) // 4,), 0x55555555, dtype=torch.int32, device=_dev())


def _k_dy(lib, y, g, img0, nimg_total, stat, gamma, beta, glob, loc, n_global, dy, edy_row, dbias, accumulate):
    nimg, H, W = y.shape[:3]
    return lib.shasta_bn_relu_bwd_dy_f16x2(hip.ptr(y), hip.ptr(g), nimg, img0, nimg_total, H, W, hip.ptr(stat), hip.ptr(gamma), hip.ptr(beta),
                                           hip.ptr(glob), hip.ptr(loc), n_global, hip.ptr(dy), dy.numel() * 4, hip.ptr(edy_row), hip.ptr(dbias),
                                           accumulate, hip.stream_ptr())


def _k_wgrad(lib, x, xp, xmax, dy, edy):
    """-> dweight and the split partials [nimg * rsplit][64][Cin * 9]"""
    B, cin, H, W = x.shape
    nimg = B if xp is None else 2 * B
    wsb = lib.shasta_conv_wgrad_workspace_bytes(nimg, cin, H, W)
    ws = torch.full((wsb // 4,), float("nan"), device=_dev())
    dw = torch.full((64, cin, 3, 3), float("nan"), device=_dev())
    hip.check(lib.shasta_conv_wgrad_f16x2(hip.ptr(x), hip.ptr(xp), B, cin, H, W, hip.ptr(xmax), hip.ptr(dy), hip.ptr(edy), hip.ptr(dw),
                                          hip.ptr(ws), wsb, hip.stream_ptr()), "conv_wgrad")
    return dw, ws.reshape(-1, 64, cin * 9)


def _decode(dy, rows, W):
    """The fragment image on the host: block ((row KS + k) 2 + ob) 2 + piece of 1 KB, lane (m = lane & 31, h = lane >> 5) holds the
    columns 16 k + 8 h .. + 7 of channel 32 ob + m -> bit patterns (piece, row, channel, column) as uint16."""
    pw = (W + 1 + 63) // 64 * 64
    ks = pw // 16
    raw = dy.cpu().numpy().view(np.uint16)[:rows * ks * 2048].reshape(rows, ks, 2, 2, 2, 32, 8)  # row, k, ob, piece, h, m, j
    return np.ascontiguousarray(raw.transpose(3, 0, 2, 5, 1, 4, 6)).reshape(2, rows, 64, pw)


def _values(bits, edy_row, nimg, H, W):
    """decoded dy (nimg, H, W, 64) in float64 from the pieces of these images and the exponents of their BatchNorm call"""
    v = bits.view(np.float16).astype(np.float64)
    v = (v[0] + v[1]) * np.ldexp(1.0, -edy_row.astype(np.int64))[None, :, None]
    return torch.from_numpy(v.reshape(nimg, H, 64, -1)[:, :, :, :W].transpose(0, 1, 3, 2).copy())


def _run(key, variant="base", chain=False):
    return _run_cached(key, variant, chain)


@functools.lru_cache(maxsize=None)
def _run_cached(key, variant, chain):
    """The backward of a case through the C entries, as the module issues them: per BatchNorm call the dy pieces into one image (current
    maps at img0 = 0, previous maps at img0 = B with accumulate_dbias and the second row of edy), then the weight gradient, twice.
    chain = False: every kernel gets the float64 reference's statistics and sums rounded to fp32 (its own error only);
    chain = True: bn_stats -> bn_finalize -> bn_relu_bwd_reduce feed it."""
    lib = hip.load()
    h = _host(key, variant)
    gamma, beta = _up(h.gamma), _up(h.beta)
    dy = _dy_buffer(lib, h.nimg, h.H, h.W)
    edy = torch.full((2, 64), float("nan"), device=_dev())
    dbias = torch.full((64,), float("nan"), device=_dev())
    sums_all, stats = [], []
    for i, (y, go, r) in enumerate(zip(h.ys, h.gouts, h.refs)):
        y, go = _up(y), _up(go)
        if chain:
            stat = _k_finalize(lib, _k_stats(lib, y), r.n)
            sums = _k_reduce(lib, y, go, stat, gamma, beta)
        else:
            stat, sums = _up(_stat32(r)), _up(_sums32(r))
        hip.check(_k_dy(lib, y, go, i * h.B, h.nimg, stat, gamma, beta, sums, sums, r.n, dy, edy[i], dbias, i), "bn_relu_bwd_dy")
        sums_all.append(sums.cpu())
        stats.append(stat.cpu())
    x = _up(h.maps[0])
    xp = None if h.single else _up(h.maps[1])
    xmax = _up(h.xmax)
    dw, ws = _k_wgrad(lib, x, xp, xmax, dy, edy)
    dw2, _ = _k_wgrad(lib, x, xp, xmax, dy, edy)
    torch.cuda.synchronize()
    bits = _decode(dy, h.nimg * h.H, h.W)
    e = edy.cpu().numpy()
    per = h.B * h.H
    dec = [_values(bits[:, i * per:(i + 1) * per], e[i], h.B, h.H, h.W) for i in range(len(h.maps))]
    return NS(bits=bits, edy=e, dec=dec, dbias=dbias.double().cpu(), dw=dw.cpu(), dw2=dw2.cpu(), ws=ws.cpu(), sums=sums_all, stats=stats)


def _check_dy(h, out, what, bounds=None):
    """The assertions on a dy piece image: values, padding, range, exponents."""
    worst = 0.0
    per = h.B * h.H
    for i, r in enumerate(h.refs):
        bound = r.bound if bounds is None else bounds[i]
        err = (out.dec[i] - r.dy).abs()
        live = bound > 0
        assert bool((err[..., ~live] == 0).all()), what
        ratio = float((err[..., live] / bound[live]).max()) if bool(live.any()) else 0.0
        worst = max(worst, ratio)
        assert ratio <= DY_BAR, (what, i, ratio * 2.0 ** 24)
        bits = out.bits[:, i * per:(i + 1) * per]
        assert not bits[:, :, :, h.W:].any(), (what, "padding columns must be the bit pattern 0")
        scaled = np.abs(bits.view(np.float16).astype(np.float64).sum(0)).max()
        assert scaled <= 2.0 ** 14 * (1 + 1e-6), (what, scaled)
        for c, (got, want, b) in enumerate(zip(out.edy[i].tolist(), _range_exp(bound), bound.tolist())):
            near = b > 0 and not 0.5 * (1 + 1e-5) <= math.frexp(b)[0] <= 1 - 1e-5  # the mantissa within 1e-5 of a power of two
            assert got == want or (near and abs(got - want) == 1), (what, i, c, got, want, b)
    return worst


def _dbias_slack(h, want):
    return 2e-5 * float(want.abs().max()) + 1e-6 * float(sum(g.abs().sum() for g in h.gouts)) ** 0.5


# ---- the stages, each on inputs of its own --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("M,far", [(2, False), (255, False), (256, False), (257, False), (4097, False), (4097, True), (262200, False)])
def test_bn_stats(M, far):
    """M = 262200: 1024 slices of 257 rows, the last three empty (beg > M)."""
    lib = hip.load()
    d = _rows(M, far)
    mm = _k_stats(lib, _up(d.y)).double().cpu()
    r = d.ref
    std = torch.sqrt(r.var)
    err = (mm[:64] - r.mean).abs()
    assert bool((err <= 2.0 ** -23 * r.mean.abs() + 1e-10 * std).all()), float((err / r.mean.abs()).max())
    rel = ((mm[64:] - r.m2).abs() / r.m2).max()
    print("bn_stats M=%d far=%s: M2 off by %.2e relative (bar 1e-6)" % (M, far, float(rel)))
    assert float(rel) <= 1e-6


@gpu
def test_bn_finalize():
    """stat, and the running statistics by nn.BatchNorm2d's own rule: two calls with two momenta on the same batch."""
    lib = hip.load()
    r = _rows(257).ref
    y = _rows(257).y
    mm = _up(torch.cat([r.mean, r.m2]).float())
    bn = torch.nn.BatchNorm2d(64, eps=EPS, momentum=0.1).double().train()
    rm, rv = torch.zeros(64, device=_dev()), torch.ones(64, device=_dev())
    nbt = torch.zeros((), dtype=torch.int64, device=_dev())
    for step, mom in enumerate((0.1, 0.25)):
        bn.momentum = mom
        bn(y.double().t().reshape(1, 64, -1, 1))
        stat = _k_finalize(lib, mm, r.n, mom, rm, rv, nbt)
        want = torch.cat([r.mean, r.invstd])
        assert float(((stat.double().cpu() - want).abs() / want.abs()).max()) <= 1e-6
        assert torch.allclose(rm.double().cpu(), bn.running_mean, rtol=1e-6, atol=0)
        assert torch.allclose(rv.double().cpu(), bn.running_var, rtol=1e-6, atol=0)
        assert int(nbt) == step + 1 == int(bn.num_batches_tracked)
    assert torch.equal(_k_finalize(lib, mm, r.n, 0.1), stat)  # no running statistics: the same stat
    assert int(nbt) == 2


@gpu
@pytest.mark.parametrize("M", [63, 4097, 262200])
def test_bn_relu_apply(M):
    """M = 262200: more rows than one pass of the grid (8192 workgroups) covers."""
    lib = hip.load()
    d = _rows(M)
    r = d.ref
    y = d.y.clone()
    y[M // 2, 7] = float("nan")
    out = _k_apply(lib, _up(y), _up(_stat32(r)), _up(d.gamma), _up(d.beta)).double().cpu()
    assert bool(torch.isnan(out[M // 2, 7])) and int(torch.isnan(out).sum()) == 1
    out[M // 2, 7] = r.out[M // 2, 7]
    err = float((out - r.out).abs().max())
    bar = 2e-5 * max(1.0, float(r.out.abs().max()))
    print("bn_relu_apply M=%d: error %.2e, bar %.2e" % (M, err, bar))
    assert err <= bar


@gpu
@pytest.mark.parametrize("M", [63, 257, 4097, 262200])
def test_bn_relu_bwd_reduce(M):
    lib = hip.load()
    d = _rows(M)
    r = d.ref
    sums = _k_reduce(lib, _up(d.y), _up(r.gout), _up(_stat32(r)), _up(d.gamma), _up(d.beta)).double().cpu()
    for k, want in enumerate((r.s1, r.s2)):
        err = float((sums[64 * k:64 * k + 64] - want).abs().max())
        print("bn_relu_bwd_reduce M=%d sums[%d]: error / bar = %.3f" % (M, k, err / (2e-5 * float(want.abs().max()))))
        assert err <= 2e-5 * float(want.abs().max())
    for k, want in ((2, r.maxg), (3, r.maxx)):
        got = sums[64 * k:64 * k + 64]
        assert bool((got >= want * (1 - 1e-6)).all()) and bool((got <= want * (1 + 1e-6)).all()), k


@gpu
@pytest.mark.parametrize("key", KEYS)
def test_bn_relu_bwd_dy(key):
    """The decoded piece image against float64: |decoded - dy64| <= 2^-19 bound_c, zero padding, range, exponents, dbias.
    Measured, in units of 2^-24 bound_c (bar 32), kernel = fp32 host restatement in every case: a 3.08, b 3.20, c 3.57, d 3.81, e 4.59,
    f 3.96, g 4.16, h 3.74, i 3.27, j 3.82, k 3.49, l 4.02; from the kernels' own statistics (case c) 4.76, synchronised 4.95."""
    h, out = _host(key), _run(key)
    worst = _check_dy(h, out, key)
    rest = 0.0
    for y, go, r in zip(h.ys, h.gouts, h.refs):
        dec, _ = _dy_f32(y, go, h.gamma, h.beta, _stat32(r), _sums32(r), _sums32(r), r.n)
        rest = max(rest, float(((dec - r.dy).abs() / r.bound).max()))
    print("bn_relu_bwd_dy %s: kernel %.2f * 2^-24 bound_c, fp32 restatement %.2f * 2^-24 (bar 32)" % (key, worst * 2.0 ** 24, rest * 2.0 ** 24))
    want = sum(r.dy.reshape(-1, 64).sum(0) for r in h.refs)
    assert float((out.dbias - want).abs().max()) <= _dbias_slack(h, want)


@gpu
@pytest.mark.parametrize("key", KEYS)
def test_conv_wgrad(key):
    """dweight against float64 dW from dy64, and from the decoded dy (the weight-gradient kernel's own error); two runs, equal bits.
    Measured error / bar against dy64 (against the decoded dy): a 0.009 (0.005), b 0.009 (0.008), c 0.026 (0.019), d 0.031 (0.024),
    e 0.018 (0.014), f 0.033 (0.024), g 0.023 (0.019), h 0.012 (0.012), i 0.013 (0.011), j 0.013 (0.012), k 0.012 (0.008), l 0.013 (0.010)."""
    h, out = _host(key), _run(key)
    bar = 2e-5 * float(h.dw64.abs().max())
    e1 = float((out.dw.double() - h.dw64).abs().max())
    own = _dw64(h.maps, out.dec)
    e2 = float((out.dw.double() - own).abs().max())
    print("conv_wgrad %s: error / bar = %.3f against dy64, %.3f against the decoded dy" % (key, e1 / bar, e2 / bar))
    assert e1 <= bar and e2 <= 2e-5 * float(own.abs().max())
    assert torch.equal(out.dw, out.dw2)
    assert bool(torch.isfinite(out.ws).all())  # every partial of every split was written


# ---- modes -----------------------------------------------------------------------------------------------------------------------
@gpu
def test_two_calls_into_one_dy_image_from_the_kernels_own_statistics():
    """Case c with bn_stats -> bn_finalize -> bn_relu_bwd_reduce feeding the dy pass of each BatchNorm call (current maps at img0 = 0,
    previous maps at img0 = B, accumulate_dbias = 1, edy row 1) and the weight gradient: against float64 of both calls."""
    h, out = _host("c"), _run("c", chain=True)
    worst = _check_dy(h, out, "c chained")
    print("chained dy: %.2f * 2^-24 bound_c (bar 32)" % (worst * 2.0 ** 24))
    for i, r in enumerate(h.refs):
        want = torch.cat([r.mean, r.invstd])
        assert float(((out.stats[i].double() - want).abs() / want.abs()).max()) <= 1e-6
        for k, w in enumerate((r.s1, r.s2)):
            assert float((out.sums[i][64 * k:64 * k + 64].double() - w).abs().max()) <= 2e-5 * float(w.abs().max())
    want = sum(r.dy.reshape(-1, 64).sum(0) for r in h.refs)
    assert float((out.dbias - want).abs().max()) <= _dbias_slack(h, want)
    assert float((out.dw.double() - h.dw64).abs().max()) <= 2e-5 * float(h.dw64.abs().max())
    # accumulate_dbias = 1 adds to what was there: the second call alone, onto a known value
    lib = hip.load()
    r = h.refs[1]
    dbias = torch.full((64,), 3.0, device=_dev())
    dy = _dy_buffer(lib, h.nimg, h.H, h.W)
    edy = torch.zeros(64, device=_dev())
    s = _up(_sums32(r))
    hip.check(_k_dy(lib, _up(h.ys[1]), _up(h.gouts[1]), h.B, h.nimg, _up(_stat32(r)), _up(h.gamma), _up(h.beta), s, s, r.n, dy, edy, dbias, 1),
              "bn_relu_bwd_dy")
    want1 = r.dy.reshape(-1, 64).sum(0)
    assert float((dbias.double().cpu() - 3.0 - want1).abs().max()) <= _dbias_slack(h, want1) + 3.0 * 2.0 ** -23
    assert bool((_decode(dy, h.nimg * h.H, h.W)[:, :h.B * h.H] == 0x5555).all())  # img0 = B: the first B images keep their bits


@gpu
def test_synchronised_batchnorm_emulated_in_one_process():
    """Case c's batch of two frame pairs as two ranks of one pair each: per-rank bn_stats merged on the host as
    shared_conv_train._batch_stats merges them, bn_finalize with the total count, per-rank reductions, sums_global = the ranks' sum,
    per-rank dy (n_global = total, sums_local its own) and weight gradient.  The ranks' gradients add up to the whole batch's."""
    lib = hip.load()
    h = _host("c")
    gamma, beta = _up(h.gamma), _up(h.beta)
    ranks = range(h.B)
    H, W = h.H, h.W
    dys = [_dy_buffer(lib, 2, H, W) for _ in ranks]
    edys = [torch.full((2, 64), float("nan"), device=_dev()) for _ in ranks]
    dbias = [torch.full((64,), float("nan"), device=_dev()) for _ in ranks]
    dbeta, dgamma = torch.zeros(64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)
    local_bounds = [[None, None] for _ in ranks]
    for i, r in enumerate(h.refs):
        ys = [_up(h.ys[i][k:k + 1]) for k in ranks]
        gs = [_up(h.gouts[i][k:k + 1]) for k in ranks]
        st = torch.stack([torch.cat([_k_stats(lib, y), y.new_full((1,), float(H * W))]) for y in ys])
        ns = st[:, -1:]
        n = ns.sum()
        mean = (st[:, :64] * ns).sum(0) / n
        m2 = (st[:, 64:128] + ns * (st[:, :64] - mean).square()).sum(0)
        stat = _k_finalize(lib, torch.cat([mean, m2]).contiguous(), float(n.item()))
        got = stat.double().cpu()  # (the mean was merged in fp32 on the host: within 1e-6 of the spread, not of itself)
        assert float(((got[64:] - r.invstd).abs() / r.invstd).max()) <= 1e-6
        assert bool(((got[:64] - r.mean).abs() <= 1e-6 * (r.mean.abs() + torch.sqrt(r.var))).all())
        sums = [_k_reduce(lib, y, g, stat, gamma, beta) for y, g in zip(ys, gs)]
        glob = (sums[0][:128] + sums[1][:128]).contiguous()
        for k in ranks:
            hip.check(_k_dy(lib, ys[k], gs[k], i, 2, stat, gamma, beta, glob, sums[k], float(n.item()), dys[k], edys[k][i], dbias[k], i),
                      "bn_relu_bwd_dy")
            dbeta += sums[k][:64].double().cpu()
            dgamma += sums[k][64:128].double().cpu()
            gpk, xk = r.gp[k].reshape(-1, 64), r.xhat[k].reshape(-1, 64)
            local_bounds[k][i] = r.a.abs() * (gpk.abs().amax(0) + (r.s1 / r.n).abs() + xk.abs().amax(0) * (r.s2 / r.n).abs())
    dws = []
    for k in ranks:
        xmax = _up(torch.stack([h.maps[0][k].abs().max(), h.maps[1][k].abs().max()]).view(torch.int32))
        dws.append(_k_wgrad(lib, _up(h.maps[0][k:k + 1]), _up(h.maps[1][k:k + 1]), xmax, dys[k], edys[k])[0].double().cpu())
    torch.cuda.synchronize()
    worst = 0.0
    for k in ranks:  # each rank's dy = the whole batch's at its images, scaled by the rank's own bound
        bits = _decode(dys[k], 2 * H, W)
        e = edys[k].cpu().numpy()
        hk = NS(B=1, H=H, W=W, refs=[NS(dy=r.dy[k:k + 1], bound=r.bound) for r in h.refs])
        outk = NS(bits=bits, edy=e, dec=[_values(bits[:, i * H:(i + 1) * H], e[i], 1, H, W) for i in range(2)])
        worst = max(worst, _check_dy(hk, outk, "rank %d" % k, bounds=local_bounds[k]))
    print("synchronised dy: %.2f * 2^-24 of the rank's bound_c (bar 32)" % (worst * 2.0 ** 24))
    assert float((dws[0] + dws[1] - h.dw64).abs().max()) <= 2e-5 * float(h.dw64.abs().max())
    for got, want in ((dbeta, sum(r.s1 for r in h.refs)), (dgamma, sum(r.s2 for r in h.refs))):
        assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max())
    want = sum(r.dy.reshape(-1, 64).sum(0) for r in h.refs)
    assert float(((dbias[0] + dbias[1]).double().cpu() - want).abs().max()) <= _dbias_slack(h, want)


@gpu
def test_dead_channel_and_zero_scale():
    """beta = -50 (g' = 0 everywhere) and gamma = 0: bound_c = 0 -> exponent 0, dy exactly 0, that row of dweight exactly 0; every other
    output channel keeps its bits."""
    h, out, base = _host("c", "dead"), _run("c", "dead"), _run("c")
    _check_dy(h, out, "dead")
    for c in (3, 9):
        for i, r in enumerate(h.refs):
            assert float(r.bound[c]) == 0.0 and out.edy[i][c] == 0
            assert bool((out.dec[i][..., c] == 0).all())
        assert bool((out.dw[c] == 0).all())
    others = [c for c in range(64) if c not in (3, 9)]
    assert torch.equal(out.dw[others], base.dw[others])
    assert float((out.dw.double() - h.dw64).abs().max()) <= 2e-5 * float(h.dw64.abs().max())


@gpu
def test_all_zero_image():
    """xmax = 0 for one image: its split partials are exactly 0, the other images' keep their bits."""
    h, out, base = _host("c", "zeroimg"), _run("c", "zeroimg"), _run("c")
    assert int(h.xmax[1]) == 0
    rsplit = out.ws.shape[0] // h.nimg
    assert rsplit == 2
    assert bool((out.ws[rsplit:2 * rsplit] == 0).all())
    keep = [s for s in range(out.ws.shape[0]) if not rsplit <= s < 2 * rsplit]
    assert torch.equal(out.ws[keep], base.ws[keep])
    assert float((out.dw.double() - h.dw64).abs().max()) <= 2e-5 * float(h.dw64.abs().max())


@gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_gradient_stays_in_its_channel(bad):
    """A NaN / an inf in one channel of gout (at a pixel the ReLU passes): the non-finite entries of dweight are that output channel's
    rows and nothing else, as in float64."""
    lib = hip.load()
    h = _host("c")
    o = 5
    gouts = [g.clone() for g in h.gouts]
    p = int(torch.nonzero(h.refs[0].pre.reshape(-1, 64)[:, o] > 0.5)[0])
    gouts[0].reshape(-1, 64)[p, o] = bad
    refs = [_bn64(y, g, h.gamma, h.beta, zero_kink=False) for y, g in zip(h.ys, gouts)]
    want = ~torch.isfinite(_dw64(h.maps, [r.dy for r in refs]))
    assert bool(want[o].all()) and int(want.sum()) == want[o].numel()
    gamma, beta = _up(h.gamma), _up(h.beta)
    dy = _dy_buffer(lib, h.nimg, h.H, h.W)
    edy = torch.full((2, 64), float("nan"), device=_dev())
    dbias = torch.full((64,), float("nan"), device=_dev())
    for i, (y, g, r) in enumerate(zip(h.ys, gouts, h.refs)):
        y, g, stat = _up(y), _up(g), _up(_stat32(r))
        sums = _k_reduce(lib, y, g, stat, gamma, beta)
        hip.check(_k_dy(lib, y, g, i * h.B, h.nimg, stat, gamma, beta, sums, sums, r.n, dy, edy[i], dbias, i), "bn_relu_bwd_dy")
    dw, _ = _k_wgrad(lib, _up(h.maps[0]), _up(h.maps[1]), _up(h.xmax), dy, edy)
    got = ~torch.isfinite(dw.cpu())
    assert torch.equal(got, want)
    others = [c for c in range(64) if c != o]
    assert float((dw.cpu()[others].double() - h.dw64[others]).abs().max()) <= 2e-5 * float(h.dw64.abs().max())
    assert bool((~torch.isfinite(dbias.cpu())).nonzero().flatten().eq(o).all())


@gpu
def test_refusals_come_before_any_launch():
    """Every refusal below is decided by SHASTA_REQUIRE / the size checks in front of the launches (csrc/shared_conv_train.hip): the
    error code comes back and sentinel-filled outputs keep their bits."""
    lib = hip.load()
    dev = _dev()
    H, W, cin = 5, 255, 16
    sent = lambda *s: torch.full(s, -7.0, device=dev)  # noqa: E731
    y, g = torch.zeros(1, H, W + 1, 64, device=dev), torch.zeros(1, H, W + 1, 64, device=dev)
    x = torch.zeros(1, cin, H, W + 1, device=dev)
    v64, v128, v256 = torch.ones(64, device=dev), torch.ones(128, device=dev), torch.ones(256, device=dev)
    xmax = torch.zeros(2, dtype=torch.int32, device=dev)
    dyb = lib.shasta_conv_dy_bytes(1, H, W)
    dy = torch.full((dyb // 4,), 0x55555555, dtype=torch.int32, device=dev)
    edy, dbias, dw, mm, stat, sums, out = sent(2, 64), sent(64), sent(64, cin, 3, 3), sent(128), sent(128), sent(256), sent(1, H, W + 1, 64)
    ws = torch.zeros(lib.shasta_bn_workspace_bytes() // 8, dtype=torch.float64, device=dev)
    wsb = lib.shasta_conv_wgrad_workspace_bytes(1, cin, H, W)
    wws = torch.full((wsb // 4,), -7.0, device=dev)
    S = hip.stream_ptr()

    def dy_call(nimg, img0, total, Wc, nbytes):
        return lib.shasta_bn_relu_bwd_dy_f16x2(hip.ptr(y), hip.ptr(g), nimg, img0, total, H, Wc, hip.ptr(v128), hip.ptr(v64), hip.ptr(v64),
                                               hip.ptr(v256), hip.ptr(v256), float(H * Wc), hip.ptr(dy), nbytes, hip.ptr(edy), hip.ptr(dbias), 0, S)

    def wgrad_call(Wc, nbytes):
        return lib.shasta_conv_wgrad_f16x2(hip.ptr(x), None, 1, cin, H, Wc, hip.ptr(xmax), hip.ptr(dy), hip.ptr(edy), hip.ptr(dw), hip.ptr(wws),
                                           nbytes, S)
    # a map of 256 columns
    assert lib.shasta_conv_train_supported(cin, H, 256) == 0
    assert dy_call(1, 0, 1, 256, dyb) == E_ARG and wgrad_call(256, wsb) == E_ARG
    # every buffer four bytes short
    assert dy_call(1, 0, 1, W, dyb - 4) == E_WORKSPACE and wgrad_call(W, wsb - 4) == E_WORKSPACE
    assert lib.shasta_bn_stats_f32(hip.ptr(y), 64, hip.ptr(mm), hip.ptr(ws), ws.numel() * 8 - 4, S) == E_WORKSPACE
    assert lib.shasta_bn_relu_bwd_reduce_f32(hip.ptr(y), hip.ptr(g), 64, hip.ptr(v128), hip.ptr(v64), hip.ptr(v64), hip.ptr(sums), hip.ptr(ws),
                                             ws.numel() * 8 - 4, S) == E_WORKSPACE
    # a count below one, a misaligned y, images past the end of the piece image
    assert lib.shasta_bn_finalize_f32(hip.ptr(v128), 0.5, EPS, 0.1, hip.ptr(stat), None, None, None, S) == E_ARG
    assert lib.shasta_bn_relu_apply_f32(C.c_void_p(y.data_ptr() + 4), 64, hip.ptr(v128), hip.ptr(v64), hip.ptr(v64), hip.ptr(out), S) == E_ARG
    assert b"aligned" in lib.shasta_last_error()
    assert dy_call(1, 1, 1, W, dyb) == E_ARG and dy_call(2, 0, 1, W, dyb) == E_ARG and dy_call(0, 0, 1, W, dyb) == E_ARG
    torch.cuda.synchronize()
    for t in (edy, dbias, dw, mm, stat, sums, out, wws):
        assert bool((t == -7.0).all())
    assert bool((dy == 0x55555555).all())


@gpu
@pytest.mark.parametrize("f16", [False, True])
def test_raw_pack_forward_is_conv_plus_bias(f16):
    """The forward of train() mode: the inference kernels on a RAW pack (shasta_shared_conv_pack_raw_f32 / _f16x2: no BatchNorm folded in,
    no ReLU) give conv + bias, and the fp16 form leaves the image maxima the weight gradient scales by in its workspace."""
    lib = hip.load()
    dev = _dev()
    g = torch.Generator().manual_seed(21)
    B, cin, H, W = 1, 16, 5, 63
    x = torch.relu(torch.randn(B, cin, H, W, generator=g))
    xp = torch.relu(torch.randn(B, cin, H, W, generator=g)) * 1.7
    w = torch.randn(64, cin, 3, 3, generator=g) / 12
    b = torch.randn(64, generator=g)
    want = [F.conv2d(t.double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1) for t in (x, xp)]
    xd, xpd, wd, bd = _up(x), _up(xp), _up(w), _up(b)
    y, yp = torch.full((B, H, W, 64), float("nan"), device=dev), torch.full((B, H, W, 64), float("nan"), device=dev)
    if f16:
        assert lib.shasta_shared_conv_f16x2_supported(cin, H, W) == 1
        nbytes = lib.shasta_shared_conv_f16x2_packed_bytes(cin)
        packed = torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=dev)
        hip.check(lib.shasta_shared_conv_pack_raw_f16x2(hip.ptr(wd), hip.ptr(bd), cin, hip.ptr(packed), nbytes, hip.stream_ptr()), "pack_raw_f16x2")
        ws = torch.zeros((lib.shasta_shared_conv_multi_workspace_bytes(B) + 3) // 4, dtype=torch.int32, device=dev)
        a, c = (C.c_void_p * 1)(y.data_ptr()), (C.c_void_p * 1)(yp.data_ptr())
        hip.check(lib.shasta_shared_conv_multi_f32(hip.ptr(xd), hip.ptr(xpd), B, cin, H, W, hip.ptr(packed), (nbytes + 255) // 256 * 256, 1, a, c,
                                                   hip.ptr(ws), ws.numel() * 4, hip.stream_ptr()), "shared_conv_multi_f32 (raw)")
        xmax = torch.stack([x.abs().max(), xp.abs().max()]).view(torch.int32)
        assert torch.equal(ws[:2 * B].cpu(), xmax)
    else:
        nbytes = lib.shasta_shared_conv_packed_bytes(cin)
        packed = torch.zeros((nbytes + 3) // 4, dtype=torch.int32, device=dev)
        hip.check(lib.shasta_shared_conv_pack_raw_f32(hip.ptr(wd), hip.ptr(bd), cin, hip.ptr(packed), nbytes, hip.stream_ptr()), "pack_raw_f32")
        hip.check(lib.shasta_shared_conv_f32(hip.ptr(xd), hip.ptr(xpd), B, cin, H, W, hip.ptr(packed), hip.ptr(y), hip.ptr(yp), hip.stream_ptr()),
                  "shared_conv_f32 (raw)")
    for got, ref in ((y, want[0]), (yp, want[1])):
        assert float((got.double().cpu() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
    assert bool((want[0] < 0).any())  # no ReLU in a raw pack
