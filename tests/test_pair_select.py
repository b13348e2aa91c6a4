"""pair_f16_kernel<PAIR_SELECT> (F = 256, the "f16x2" default): relu(u + v) = max(v, -u) + u with the fp16 pieces of max(v, -u) PICKED
per pair from words cut once per table row (csrc/pieces.hpp: cut_select_word) and the "+ u" carried through the linear second layers
by a per-row vector (csrc/pair.hip: row_select_kernel).

CPU: cut_select_word itself, compiled for the host from pieces.hpp into a small stand-alone program - the ordering contract that lets
one v_max_f32 pick a word, the reconstruction error, and the selection identity.
GPU: the pair stage at small table sizes against the CPU oracle, on crafted tables against the f32 kernel and a float64 evaluation,
with non-finite rows, and batched against one frame-pair at a time."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import shasta_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shasta_amd", "csrc")

HOST_PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "pieces.hpp"
// argv[1]: n fp32 values (already range-scaled), argv[2]: their n select words
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<float> x;
    float buf[4096];
    size_t n;
    while ((n = fread(buf, sizeof(float), 4096, f)) > 0) x.insert(x.end(), buf, buf + n);
    fclose(f);
    std::vector<uint32_t> w(x.size());
    for (size_t i = 0; i < x.size(); ++i) w[i] = shasta::cut_select_word(x[i]);
    f = fopen(argv[2], "wb");
    if (!f) return 4;
    fwrite(w.data(), sizeof(uint32_t), w.size(), f);
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def words(tmp_path_factory):
    """-> words(x): the select words of a float32 array, from the host build of cut_select_word"""
    from shasta_amd import build as B
    d = tmp_path_factory.mktemp("select_word")
    src, exe = os.path.join(d, "select_word.hip"), os.path.join(d, "select_word")
    with open(src, "w") as f:
        f.write(HOST_PROGRAM)
    r = subprocess.run([B._hipcc(), "--offload-host-only", "-O1", "-std=c++17", "-ffp-contract=off", "-I", CSRC, src, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    count = [0]

    def run(x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        count[0] += 1
        fin, fout = os.path.join(d, "in%d.bin" % count[0]), os.path.join(d, "out%d.bin" % count[0])
        x.tofile(fin)
        r = subprocess.run([exe, fin, fout], capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
        w = np.fromfile(fout, dtype=np.uint32)
        assert w.shape == x.shape
        return w
    return run


def _decode(w):
    """hi + lo of select words, in float64"""
    hi = (w >> np.uint32(16)).astype(np.uint16).view(np.float16).astype(np.float64)
    lo = (w & np.uint32(0xffff)).astype(np.uint16).view(np.float16).astype(np.float64)
    return hi + lo


def _magnitudes(rng, n):
    """n fp32 magnitudes, log-uniform over [2^-20, 2^14]"""
    return np.exp2(rng.uniform(-20.0, 14.0, n)).astype(np.float32)


def test_select_words_order_like_their_values(words):
    """2 x 10^5 sorted fp32 values across both signs, 2^-20 .. 2^14 in magnitude (so the flushed range below 2^-14 and the largest
    scaled magnitude are inside), with zeros, exact powers of two and fp16-representable values among them: read as fp32 the words
    are non-decreasing, never a NaN, an infinity or a denormal, and equal values give equal words."""
    rng = np.random.default_rng(11)
    m = _magnitudes(rng, 199000)
    x = np.concatenate([m[:99500], -m[99500:], np.zeros(8, np.float32), -np.zeros(8, np.float32),
                        np.exp2(np.arange(-20, 15)).astype(np.float32), -np.exp2(np.arange(-20, 15)).astype(np.float32),
                        rng.uniform(-2048, 2048, 458).astype(np.float16).astype(np.float32),
                        np.repeat(m[:228], 2)])                        # equal values
    assert x.size == 200000
    x = np.sort(x)
    w = words(x)
    f = w.view(np.float32)
    assert np.isfinite(f).all()
    expo = (w >> np.uint32(23)) & np.uint32(0xff)
    assert ((expo > 0) | (w == 0)).all(), "an fp32 denormal word"
    assert (np.diff(f.astype(np.float64)) >= 0).all()
    same = np.diff(x) == 0
    assert same.sum() >= 228 and (w[1:][same] == w[:-1][same]).all()
    # the fp16 exponent field of the high piece is never 31, and a low piece has the sign of its high piece (or is zero)
    assert (((w >> np.uint32(26)) & np.uint32(0x1f)) < 31).all()
    lo_mag, lo_sign, hi_sign = w & np.uint32(0x7fff), (w >> np.uint32(15)) & np.uint32(1), w >> np.uint32(31)
    assert ((lo_mag == 0) | (lo_sign == hi_sign)).all()


def test_select_words_reconstruct_their_values(words):
    """|hi + lo - x| <= 2^-22 |x| for |x| >= 2^-3 and <= 2^-25 below, down to the flush at 2^-14; zero (either sign) and everything
    below 2^-14 map to word 0."""
    rng = np.random.default_rng(12)
    m = _magnitudes(rng, 100000)
    x = np.concatenate([m[:50000], -m[50000:], np.float32([0.0, -0.0, 2.0 ** -14, -2.0 ** -14, 16384.0, -16384.0, 2.0 ** -3])])
    w = words(x)
    x64 = x.astype(np.float64)
    err = np.abs(_decode(w) - x64)
    big = np.abs(x64) >= 2.0 ** -3
    assert (err[big] <= 2.0 ** -22 * np.abs(x64[big])).all()
    # below 2^-14 the word is 0 by definition (the flush that keeps every word a normal fp32), so the error there is the value itself,
    # less than 2^-14 of a range whose largest sum is 2^14; the 2^-25 bound is asserted on everything that is not flushed
    small = np.abs(x64) < 2.0 ** -14
    assert small.sum() > 1000 and (w[small] == 0).all()
    keep = ~big & ~small
    assert keep.sum() > 1000 and (err[keep] <= 2.0 ** -25).all()
    assert w[x.size - 7] == 0 and w[x.size - 6] == 0


def test_maximum_of_two_words_is_the_word_of_the_maximum(words):
    """decode(max(word(v), word(-u))) == decode(word(max(v, -u))) with the maximum of the words taken as fp32 - what the kernel's
    v_max_f32 does - for random (u, v) and for u = -v exactly."""
    rng = np.random.default_rng(13)
    n = 100000
    sign = lambda: rng.choice(np.float32([-1.0, 1.0]), n)
    u, v = _magnitudes(rng, n) * sign(), _magnitudes(rng, n) * sign()
    u[n // 2:] = -v[n // 2:]                                              # u = -v exactly
    near = slice(n // 4, n // 2)                                          # -u next to v: one or two fp32 ulps apart, same high piece
    u[near] = -np.nextafter(v[near], np.float32(np.inf) * rng.choice(np.float32([-1.0, 1.0]), n // 4))
    wv, wu, wm = words(v), words(-u), words(np.maximum(v, -u))
    picked = np.maximum(wv.view(np.float32), wu.view(np.float32)).view(np.uint32)
    assert (_decode(picked) == _decode(wm)).all()
    assert (picked[n // 2:] == wv[n // 2:]).all() and (wv[n // 2:] == wu[n // 2:]).all()


# ---- GPU -------------------------------------------------------------------------------------------------------------------------

def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def _model(N, dev, seed=0):
    import shasta_amd
    torch.manual_seed(seed)
    return shasta_amd.build_simp_track(dict(type="Shasta", reader=None, backbone=None, neck=None,
                                            bev_extractor=dict(type="BEVFeatureExtractor", pc_start=[-54, -54], voxel_size=[0.075, 0.075],
                                                               out_stride=8), max_obj=N, num_feats=7, num_point=4)).eval().to(dev)


def _pair_stage(m, mode, pfeat, feat, ptab, dtab):
    """residual (B, T, D) of shasta_pair_residual_f32 on the given feature / box tables (device tensors) in arithmetic `mode`"""
    from shasta_amd import hip
    lib = hip.load()
    B, T, F = feat.shape
    ld = (T + 3) // 4 * 4
    m.arithmetic = mode
    w = m._weights()
    m._ensure_packed(w, feat.device)
    res = torch.full((B, T, ld), 7.0, device=feat.device)
    wsb = lib.shasta_forward_workspace_bytes(B, T - 2, 7, F)
    ws = torch.empty(wsb // 4 + 1, device=feat.device)
    hip.check(lib.shasta_pair_residual_f32(C.byref(w), hip.ptr(m._packed), B, hip.ptr(feat), hip.ptr(pfeat), hip.ptr(dtab), hip.ptr(ptab),
                                           hip.ptr(res), ld, hip.ptr(ws), wsb, hip.stream_ptr()), "pair")
    torch.cuda.synchronize()
    return res[:, :, :T].cpu()


def _tables(B, T, seed, dev):
    g = torch.Generator().manual_seed(seed)
    feat, pfeat = torch.rand(B, T, 256, generator=g), torch.rand(B, T, 256, generator=g)
    dtab, ptab = torch.rand(B, T, 8, generator=g) * 4 + 0.5, torch.rand(B, T, 8, generator=g) * 4 + 0.5
    return [x.to(dev) for x in (pfeat, feat, ptab, dtab)]


def _ref64(m, pfeat, feat, ptab, dtab):
    w64 = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    return O.pair_residual(w64, pfeat.double().cpu(), feat.double().cpu(), ptab[:, :, :7].double().cpu(), dtab[:, :, :7].double().cpu(), 7,
                           chunk=16)


@pytest.mark.gpu
@pytest.mark.parametrize("N,B", [(1, 1), (2, 3), (13, 2), (47, 2), (64, 1), (129, 1)])
def test_select_pair_path_at_small_table_sizes_matches_oracle(N, B):
    """Table sizes from 3 rows (one wave works, seven idle) over T = D = 66 (N = 64: a second tile of two rows) to 131 rows, through
    affinity_from_bev against the CPU oracle: 1e-5, and the arg-max of every decided row - the bar of
    test_fp16_pair_path_at_odd_table_sizes_matches_oracle."""
    dev = _dev()
    m = _model(N, torch.device("cpu"), seed=100 + N)
    w = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(N)
    bev = torch.relu(torch.randn(B, 180, 180, 64, generator=g))
    pbev = torch.relu(torch.randn(B, 180, 180, 64, generator=g))
    det, prev = O.synth_boxes(g, B, N), O.synth_boxes(g, B, N)
    r1, r2 = O.forward_from_bev(w, bev, pbev, det.clone(), prev.clone(), 7, 4)
    m = m.to(dev)
    assert m.arithmetic == "f16x2"
    with torch.no_grad():
        m1, m2 = m.affinity_from_bev(bev.to(dev), pbev.to(dev), det.to(dev), prev.to(dev))
    m1, m2 = m1.cpu(), m2.cpu()
    e1, e2 = float((m1 - r1).abs().max()), float((m2 - r2).abs().max())
    print("N %d B %d: max|m1 - oracle| %.3e  max|m2 - oracle| %.3e" % (N, B, e1, e2))
    assert e1 < 1e-5 and e2 < 1e-5
    top2 = torch.topk(r1, 2, dim=-1).values
    decided = (top2[..., 0] - top2[..., 1]) > 1e-5
    assert bool((m1.argmax(-1) == r1.argmax(-1))[decided].all())


def _crafted(kind, dev):
    """-> model, (pfeat, feat, ptab, dtab) for T = D = 72 (a full tile and one of 8 rows), B = 2"""
    N, B, F, nf = 70, 2, 256, 7
    T = N + 2
    m = _model(N, dev, seed=5)
    pfeat, feat, ptab, dtab = _tables(B, T, 21, dev)
    with torch.no_grad():
        if kind == "all_inactive":        # first-layer biases far below every sum: every hidden unit of every pair is inactive
            for mlp in (m.fuse_shape, m.res_coeff, m.fuse_det):
                mlp[0].bias.fill_(-100.0)
        elif kind == "u_eq_minus_v":      # previous-side columns = minus the current-side ones, no bias, all rows alike: u = -v in every unit
            m.fuse_shape[0].weight[:, :F] = -m.fuse_shape[0].weight[:, F:]
            m.res_coeff[0].weight[:, :F + nf] = -m.res_coeff[0].weight[:, F + nf:]
            m.fuse_det[0].weight[:, :nf] = -m.fuse_det[0].weight[:, nf:]
            for mlp in (m.fuse_shape, m.res_coeff, m.fuse_det):
                mlp[0].bias.zero_()
            feat[:] = feat[:, :1]
            dtab[:] = dtab[:, :1]
            pfeat.copy_(feat)
            ptab.copy_(dtab)
        elif kind == "one_row_1e3":       # one row 10^3 times the others: in the first tile on the detection side, and among the tracks
            feat[:, 5] *= 1e3
            pfeat[:, 70] *= 1e3
        elif kind == "zero_rows":
            feat[:, 3] = 0
            dtab[:, 3] = 0
            pfeat[:, 4] = 0
            ptab[:, 4] = 0
            feat[:, 66:70] = 0
        else:
            raise ValueError(kind)
    return m, (pfeat, feat, ptab, dtab)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["all_inactive", "u_eq_minus_v", "one_row_1e3", "zero_rows"])
def test_select_pair_path_on_crafted_tables(kind):
    """Tables on which max(v, -u) + u has nothing left of its two terms (every unit inactive; u = -v), on which one row sets the
    range of a whole tile, and with all-zero rows; against arithmetic = "f32" on the same tables, both measured on a float64
    evaluation: max error <= 2 x the f32 form's + 1e-7 of the scale (the bound of test_pair_kernels_are_fp32_accurate)."""
    dev = _dev()
    m, tabs = _crafted(kind, dev)
    ref = _ref64(m, *tabs)
    scale = float(ref.abs().max())
    sel = _pair_stage(m, "f16x2", *tabs).double()
    f32 = _pair_stage(m, "f32", *tabs).double()
    e_sel, e_f32 = float((sel - ref).abs().max()), float((f32 - ref).abs().max())
    print("%s: scale %.4g  max err select %.3e  f32 %.3e  bound %.3e" % (kind, scale, e_sel, e_f32, 2.0 * e_f32 + 1e-7 * scale))
    assert torch.isfinite(sel).all()
    assert bool((sel != f32).any()), "the fp16 pair kernel did not run"
    assert e_sel <= 2.0 * e_f32 + 1e-7 * scale


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["prev", "det"])
def test_select_pair_path_keeps_non_finite_rows_non_finite(side):
    """One NaN row and one inf row on one side of the tables.  Every element that is NaN under arithmetic = "f32" is NaN here, and the
    fp16 forms' own contract holds as before: a non-finite track gives NaN for its whole row of every tile, a non-finite detection
    NaN for its whole 64-detection tile - never a finite number; rows and tiles that hold no such value stay finite."""
    dev = _dev()
    N, B = 70, 2
    T = N + 2
    m = _model(N, dev, seed=6)
    pfeat, feat, ptab, dtab = _tables(B, T, 22, dev)
    x = pfeat if side == "prev" else feat
    x[0, 9, 17] = float("nan")
    x[1, 68, 200] = float("inf")
    sel = _pair_stage(m, "f16x2", pfeat, feat, ptab, dtab)
    f32 = _pair_stage(m, "f32", pfeat, feat, ptab, dtab)
    assert bool(torch.isnan(sel)[torch.isnan(f32)].all())
    assert bool((~torch.isfinite(sel))[~torch.isfinite(f32)].all())
    bad = torch.zeros(B, T, T, dtype=torch.bool)
    if side == "prev":
        bad[0, 9, :] = True
        bad[1, 68, :] = True
    else:
        bad[0, :, 0:64] = True       # detection 9: the first tile
        bad[1, :, 64:T] = True       # detection 68: the second
    assert bool(torch.isnan(sel)[bad].all())
    assert bool(torch.isfinite(sel)[~bad].all())


@pytest.mark.gpu
def test_select_pair_path_batched_equals_one_at_a_time():
    """B = 3 in one call against three calls of one frame-pair (another launch geometry, hence other workgroup track ranges and
    scales): <= 1e-6."""
    dev = _dev()
    N, B = 129, 3
    T = N + 2
    m = _model(N, dev, seed=7)
    pfeat, feat, ptab, dtab = _tables(B, T, 23, dev)
    both = _pair_stage(m, "f16x2", pfeat, feat, ptab, dtab)
    for b in range(B):
        one = _pair_stage(m, "f16x2", *[x[b:b + 1].contiguous() for x in (pfeat, feat, ptab, dtab)])
        d = float((one[0] - both[b]).abs().max())
        print("frame-pair %d: max |batched - alone| %.3e (scale %.3g)" % (b, d, float(both[b].abs().max())))
        assert d <= 1e-6
