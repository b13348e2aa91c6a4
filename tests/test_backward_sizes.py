"""The hand-written backward, end to end, against FLOAT64 autograd of the CPU oracle at the table sizes where its kernels change
trips: the tile seams 30 ... 127 on default-init weights, and 254 / 255 / 500 rows on weights whose ReLU decisions carry a margin.

Why two kinds of inputs.  A default-init network above ~1e5 pairs has ReLU units within fp32 rounding of their kink; a correct fp32
backward then takes another branch than float64 and whole tensors move by 1e-3 ... 1e-2 (sums that nearly cancel).  Each committed
(case, seed) of the seam sizes is therefore one on which the float32 oracle itself agrees with the float64 oracle to 1e-5
(`test_seam_inputs_are_stable_under_rounding`, CPU), and the large cases run on `margin_weights`: every ReLU unit - and every argument
of the anchor heads' abs() - is at least 1e-3 of its layer's range away from zero on the case's inputs, asserted in float64 by
`check_margins` before anything is compared."""
import gc

import pytest
import torch

from oracle import shasta_oracle as O
from tests.test_training import _case

N_TENSORS = 2 * (8 + 4 + 8 + 3 + 3 + 6)  # parameters of aug_shape, aug_dets, fuse_shape, res_coeff, fuse_det, aff

# (N, nf, np, B, n_real, seed).  The seeds: counted up from 5, the first whose float32 oracle stays within 7e-6 of the float64 oracle
# (the condition is 1e-5, test_seam_inputs_are_stable_under_rounding; the figure moves by ~15 % with the host's thread count, and
# roughly every second seed has a ReLU unit that flips under rounding: 1e-4 ... 1e-2)
SEAM_CASES = [(30, 7, 4, 2, None, 7), (31, 3, 5, 1, 20, 12), (62, 7, 1, 5, None, 7), (63, 3, 4, 2, 50, 6), (64, 7, 5, 1, None, 14),
              (65, 3, 1, 2, 64, 6), (126, 7, 4, 1, None, 33), (127, 3, 5, 2, 100, 6), (30, 3, 1, 5, 29, 11), (63, 7, 5, 5, None, 27),
              (64, 3, 4, 5, 40, 11), (65, 7, 4, 2, None, 23), (126, 3, 5, 2, 90, 17), (127, 7, 1, 1, None, 6)]
# the headline configuration (F = 256) and the shipped class shape (F = 320, padded rows), and the 256-row seam from both sides
LARGE_CASES = [(254, 7, 4, 2, None, 5), (255, 3, 5, 2, 200, 5), (500, 7, 4, 2, None, 6), (500, 3, 5, 1, 450, 5)]


def oracle_grads(c, w, a, b, det, prev, gt, dtype):
    """Autograd of the oracle in `dtype`: ({parameter: gradient}, d bev, d prev_bev)."""
    wl = {k: v.to(dtype).requires_grad_(v.dtype.is_floating_point and not k.startswith("shared_conv")) for k, v in w.items()}
    a, b = a.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
    m1, m2 = O.forward_from_bev(wl, a, b, det.to(dtype), prev.to(dtype), c["nf"], c["np"], out_stride=c["stride"], grad=True)
    O.affinity_loss(m1, m2, gt.to(dtype)).backward()
    del m1, m2
    return {k: v.grad for k, v in wl.items() if v.grad is not None}, a.grad, b.grad


def deviation(got, want, rows=1 << 22):
    """max |got - want| / max |want| in float64, in slabs (the four 256 M-entry matrices are never held twice in float64)."""
    g, w = got.detach().reshape(-1), want.detach().reshape(-1)
    err = scale = 0.0
    for i in range(0, w.numel(), rows):
        ws = w[i:i + rows].double().cpu()
        err = max(err, float((g[i:i + rows].double().cpu() - ws).abs().max()))
        scale = max(scale, float(ws.abs().max()))
    return err / max(scale, 1e-300), scale


def rounding_deviation(c, w, a, b, det, prev, gt, rows=None):
    """{tensor: deviation of the float32 oracle from the float64 oracle}, and the float64 gradients.  rows: a dict that receives
    {2-D weight gradient: its worst row against that row's own largest entry} (_row_check, without its assertion on the deviation)."""
    g64, a64, b64 = oracle_grads(c, w, a, b, det, prev, gt, torch.float64)
    g32, a32, b32 = oracle_grads(c, w, a, b, det, prev, gt, torch.float32)
    dev = {}
    for k in list(g64):
        g = g32.pop(k)
        dev[k], scale = deviation(g, g64[k])
        if rows is not None and g.dim() == 2 and scale > 0:
            rows[k] = _row_check(k, g, g64[k], scale, bar=float("inf"))
    dev["d bev"], dev["d prev_bev"] = deviation(a32, a64)[0], deviation(b32, b64)[0]
    return dev, (g64, a64, b64)


# ---- margin-certified weights ---------------------------------------------------------------------------------------------------
OFF_STRIDE = 16
LOGIT_RANGE = 4.0
SHRINK = 0.4  # 1 / 2.5: a shifted layer spans 0.5 m ... 2.5 m in magnitude


def _shift_pattern(n, first, m, relu):
    """Bias shifts of a layer whose largest |pre-activation| is m: +1.5 m switches a unit on for every input, -1.5 m off, both with a
    margin of 0.5 m.  Arguments of abs(): three in four up, every fourth down (both signs of the kink's slope in every 4-wide block).
    ReLU layers: a switched-off unit has an all-zero row in its weight gradient, and the row-wise check below admits at most 10 % of
    exempt rows, so one unit in 16 goes off (at most n // 10 of them: layers narrower than 10 keep every unit on)."""
    s = torch.full((n,), 1.5 * m)
    j = torch.arange(first, first + n)
    if relu:
        off = j[j % OFF_STRIDE == 3][: n // 10]
        s[off - first] = -1.5 * m
    else:
        s[j % 4 == 3] = -1.5 * m
    return s


def margin_weights(c, w, a, b, det, prev):
    """Shifts the biases of `w` (float32, IN PLACE) layer by layer in depth order during one no-grad float32 oracle forward on the
    case's inputs, so that no ReLU / abs() argument of that forward is near zero (see _shift_pattern); a shifted layer is scaled by SHRINK,
    back to the range it had - unscaled, the shifts compound to pre-activations of 3e4 in the last aff layer at N = 62."""
    def shift(key, x, cols, kind):
        m = float(x[..., cols].abs().max())
        s = _shift_pattern(x[..., cols].shape[-1], cols.start or 0, m, kind == "relu")
        w[key + ".bias"][cols] = (w[key + ".bias"][cols] + s) * SHRINK
        w[key + ".weight"][cols] *= SHRINK
        x = x.clone()
        x[..., cols] = (x[..., cols] + s) * SHRINK
        return x

    O.KINK_HOOK = shift
    try:
        im = O.forward_from_bev(w, a, b, det.clone(), prev.clone(), c["nf"], c["np"], out_stride=c["stride"], pair_chunk=1 << 30,
                                return_intermediates=True)[2]
    finally:
        O.KINK_HOOK = None
    # The logits: the shifts above scale with the residual's range, which zero-padded rows stretch to 1e2 (their log(1e-10) terms);
    # softmaxes of such logits saturate (entries of 1e-185 measured), the loss's 1 / (m + 1e-10) reaches 1e10 and every gradient is
    # the small difference of huge terms - in any arithmetic.  The last aff layer has no kink behind it: scaled so that |logit| <= 4.
    top = float(im["matched"].abs().max())
    if top > LOGIT_RANGE:
        w["aff.10.weight"] *= LOGIT_RANGE / top
        w["aff.10.bias"] *= LOGIT_RANGE / top
    return w


def check_margins(c, w, a, b, det, prev):
    """THE CERTIFICATE (float64 forward): over every ReLU unit and every abs() argument, |x| >= 1e-3 * (largest |x| of its layer).
    Returns the smallest ratio found."""
    seen = {}

    def look(key, x, cols, kind):
        v = x[..., cols].abs()
        lo, hi = seen.get(key, (float("inf"), 0.0))
        seen[key] = (min(lo, float(v.min())), max(hi, float(v.max())))
        return x

    d = torch.float64
    O.KINK_HOOK = look
    try:
        O.forward_from_bev({k: v.to(d) if v.dtype.is_floating_point else v for k, v in w.items()}, a.to(d), b.to(d), det.to(d), prev.to(d),
                           c["nf"], c["np"], out_stride=c["stride"])
    finally:
        O.KINK_HOOK = None
    assert len(seen) == 8 + 8 + 3 + 2 + 2 + 5, sorted(seen)  # the anchor heads (a ReLU and an abs() each), the pair MLPs, aff
    worst = min(lo / hi for lo, hi in seen.values())
    for key, (lo, hi) in seen.items():
        assert lo >= 1e-3 * hi, "%s: a unit within %.2e of its kink (layer range %.2e)" % (key, lo, hi)
    return worst


def large_case(case):
    N, nf, npnt, B, n_real, seed = case
    c, model, w, a, b, det, prev, gt = _case(N, nf, npnt, B, seed=seed, n_real=n_real)
    gen = torch.Generator().manual_seed(seed)
    gt = (torch.rand(B, N + 2, N + 2, generator=gen) < 0.01).float()  # the density of the headline test
    gt[:, 0, 0] = 1.0
    sd = {k: v.detach() for k, v in model.state_dict().items()}  # the model's own storage: shifted in place
    del w
    margin_weights(c, sd, a, b, det, prev)
    return c, model, sd, a, b, det, prev, gt




def _row_check(name, got, want, scale, slab=1 << 24, bar=1e-3):
    """Every row of a 2-D weight gradient against that row's OWN largest reference entry at 1e-3 (a whole-tensor maximum hides a wrong
    tail row of the 2000 x 128 000 outer products), in slabs of rows; rows below 1e-4 of the tensor's largest entry are exempt, and
    at most 10 % of the rows may be (a property of the reference alone)."""
    rows = max(1, slab // want.shape[1])
    exempt, worst = 0, 0.0
    for r0 in range(0, want.shape[0], rows):
        w = want[r0:r0 + rows].double()
        rmax = w.abs().amax(1)
        live = rmax >= 1e-4 * scale
        exempt += int((~live).sum())
        if got is not None and bool(live.any()):
            err = (got[r0:r0 + rows].double().cpu() - w).abs().amax(1)
            ratio = float((err[live] / rmax[live]).max())
            worst = max(worst, ratio)
            assert ratio <= bar, "%s: a row in [%d, %d) is off by %.3e of its own largest entry" % (name, r0, r0 + rows, ratio)
    assert exempt <= 0.1 * want.shape[0], "%s: %d of %d rows exempt from the row-wise check" % (name, exempt, want.shape[0])
    return worst


def _hip_grads(model, a, b, det, prev, gt, dense=False):
    from shasta_amd import training
    dev = torch.device("cuda:0")
    model = model.to(dev).train()
    model.dense_pair_backward = dense
    model.zero_grad(set_to_none=True)
    ad, bd = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    m1, m2 = training.affinity_train(model, ad, bd, det.to(dev).contiguous(), prev.to(dev).contiguous())
    training.affinity_loss(m1, m2, gt.to(dev)).backward()
    torch.cuda.synchronize()
    model.dense_pair_backward = False
    return {k: p.grad for k, p in model.named_parameters() if p.grad is not None}, ad.grad, bd.grad


def _compare(tag, hip_grads, ref, rows=False):
    """1e-4 of each tensor's largest reference entry (the bar of test_backward_matches_autograd_of_oracle, without its floor on the
    scale: gradients of a default-init net go down to 1e-9), every parameter and both maps; tensor by tensor."""
    got, ga, gb = hip_grads
    g64, a64, b64 = ref
    assert set(got) == set(g64) and len(g64) == N_TENSORS
    worst, worst_row = ("", 0.0), ("", 0.0)
    for k, want in list(g64.items()) + [("d bev", a64), ("d prev_bev", b64)]:
        g = ga if k == "d bev" else gb if k == "d prev_bev" else got[k]
        assert bool(torch.isfinite(g).all()), k
        dev, scale = deviation(g, want)
        assert scale > 0 or not rows, k + ": an all-zero reference gradient checks nothing"  # (default init: a dead narrow layer is possible)
        worst = max(worst, (k, dev), key=lambda t: t[1])
        assert dev <= 1e-4, "%s %s: max |diff| %.3e of the tensor's largest entry %.3e" % (tag, k, dev, scale)
        if rows and want.dim() == 2:
            worst_row = max(worst_row, (k, _row_check(tag + " " + k, g, want, scale)), key=lambda t: t[1])
    print("%s: worst tensor %s %.2e of its range" % (tag, *worst) + (", worst row %s %.2e of its own range" % worst_row if rows else ""))


# ---- the seam sizes on default-init weights -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SEAM_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_seam_inputs_are_stable_under_rounding(case):
    """CPU.  The condition on the committed (case, seed): the float32 oracle agrees with the float64 oracle to 1e-5 of every gradient
    tensor's largest entry, i.e. no ReLU unit of this default-init forward decides differently in fp32 (a flip shows as 1e-4 ... 1e-2,
    see the module docstring; measured on the committed seeds: 3.1e-6 ... 6.9e-6).  A changed oracle or torch cannot void the GPU
    test below unnoticed."""
    N, nf, npnt, B, n_real, seed = case
    c, model, w, a, b, det, prev, gt = _case(N, nf, npnt, B, seed=seed, n_real=n_real)
    dev, _ = rounding_deviation(c, w, a, b, det, prev, gt)
    assert len(dev) == N_TENSORS + 2
    k = max(dev, key=dev.get)
    assert dev[k] <= 1e-5, "%s: the float32 oracle is %.2e of the range away from the float64 oracle" % (k, dev[k])


@pytest.mark.gpu
@pytest.mark.parametrize("case", SEAM_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_backward_at_the_seam_sizes_matches_float64_autograd(case):
    N, nf, npnt, B, n_real, seed = case
    c, model, w, a, b, det, prev, gt = _case(N, nf, npnt, B, seed=seed, n_real=n_real)
    ref = oracle_grads(c, w, a, b, det, prev, gt, torch.float64)
    _compare("N %d nf %d np %d B %d n_real %s" % case[:5], _hip_grads(model, a, b, det, prev, gt), ref)


# ---- 256+ rows and the headline size on margin-certified weights ----------------------------------------------------------------
def _slow(case):
    return pytest.param(case, marks=pytest.mark.slow if case[0] >= 500 else (), id="-".join(str(v) for v in case))


@pytest.mark.parametrize("case", [_slow(c) for c in LARGE_CASES])
def test_large_inputs_carry_their_margin_and_are_stable_under_rounding(case):
    """CPU.  On margin_weights (a) the certificate of check_margins holds, (b) the float32 oracle agrees with the float64 oracle to 2e-5
    of each of the 66 + 2 tensors' largest entry, (c) no gradient tensor is identically zero, (d) at most 10 % of the rows of any
    2-D weight gradient are exempt from the row-wise check.  Measured (smallest margin ratio; worst tensor of (b); 8 threads):
    N 254: 0.201, 8.7e-6 (d bev);  N 255: 0.200, 5.8e-6 (d prev_bev);  N 500 F 256: 0.203, 7.4e-6 (aug_shape.3.0.weight);  N 500 F 320,
    padded: 0.200, 1.0e-5 (fuse_shape.6.weight) - the same 4e-6 ... 1e-5 the float32 oracle shows on the seam cases, i.e. plain fp32
    rounding, so the bar of the HIP backward on these cases is the 1e-4 of the small tests (10 x that and more).  Exempt rows: the
    switched-off units, 6.2 % ... 7.3 %.  The N = 500 cases take about 40 s each and up to 32 GB here.
    Printed, not asserted: the float32 oracle's worst ROW against that row's own range (the HIP backward is held to 1e-3 there):
    1.1e-4, 2.8e-4, 1.7e-4 and 8.9e-4 in the order above.  A row that is small because its terms cancel carries the rounding of the
    terms, so this figure depends on the seed: the headline case has seed 6 because seed 5 gives 1.3e-3 (one row of
    aug_dets.2.0.weight); for the padded F = 320 case, B = 1, seed 5 is the best of 5, 6, 7 (3.2e-3 and 7.3e-3 for the others): there
    the row bar sits at the fp32 floor (HIP kernels: 6.6e-4)."""
    c, model, sd, a, b, det, prev, gt = large_case(case)
    assert check_margins(c, sd, a, b, det, prev) >= 1e-3
    rows = {}
    dev, (g64, a64, b64) = rounding_deviation(c, sd, a, b, det, prev, gt, rows)
    assert len(dev) == N_TENSORS + 2
    k = max(dev, key=dev.get)
    assert dev[k] <= 2e-5, "%s: the float32 oracle is %.2e of the range away from the float64 oracle" % (k, dev[k])
    k = max(rows, key=rows.get)
    print("margin-certified case %s: float32 oracle within %.2e (tensors), %.2e (rows, %s)" % (case, max(dev.values()), rows[k], k))
    for k, g in g64.items():
        scale = float(g.abs().max())
        assert scale > 0, k
        if g.dim() == 2:
            _row_check(k, None, g, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("case", [_slow(c) for c in LARGE_CASES])
def test_backward_at_256_rows_and_the_headline_size_matches_float64_autograd(case):
    """Plain fp32 backward (per pair on chip) on every large case, and the dense formulation (dense_pair_backward) on the headline one;
    whole tensors at 1e-4 and the rows of every 2-D weight gradient at 1e-3 of their own range."""
    c, model, sd, a, b, det, prev, gt = large_case(case)
    assert check_margins(c, sd, a, b, det, prev) >= 1e-3
    ref = oracle_grads(c, sd, a, b, det, prev, gt, torch.float64)
    del sd
    gc.collect()
    tag = "N %d nf %d np %d B %d n_real %s" % case[:5]
    _compare(tag, _hip_grads(model, a, b, det, prev, gt), ref, rows=True)
    if case == LARGE_CASES[2]:
        _compare(tag + " dense", _hip_grads(model, a, b, det, prev, gt, dense=True), ref, rows=True)
