"""The kink-free kernels of the backward (csrc/backward_aux.hip), one by one through the C ABI, against the same formula in torch float64
with autograd - at table sizes T = N + 2 on and around 16, 32, 64, 128, 256, 512 (the trip lengths of these kernels' loops), two
batch sizes, the leading dimension training.py passes and a larger one, NaN in every padding column and in every output before the call.

Bars are derived, not measured (U = 2^-24, the unit roundoff of fp32):
  * an output that is a sum of n fp32 terms:  (n + 16) U A,  A = the float64 sum of the terms' absolute values.  n U A bounds the
    rounding of n - 1 additions in ANY order plus the rounding of each term's last operation; 16 U A covers what goes into a term
    (logf / cosf / sinf / sqrtf at <= 2 ulp each, divisions, the few multiplications and subtractions in front of them).  A dropped
    term is ~A / n: 30 times the bound at n = 600.  Terms that are exactly zero (gt = 0 in the loss) do not count: s + 0 is exact.
  * an elementwise output:  16 U x (the magnitudes it is put together from)  +  its sensitivity to every reduction it depends on
    times that reduction's bound above (`sum g m` of the softmax; `den` and `gs` of the hand-designed residual).
No ReLU, no data-dependent branch other than sign(log p - log q), whose arguments the tests keep apart: nothing here depends on which
side of a kink fp32 rounding falls."""
import pytest
import torch

from oracle import shasta_oracle as O

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SIZES = [1, 2, 13, 14, 29, 30, 31, 62, 63, 126, 127, 253, 254, 255, 256, 257, 500, 509, 510, 600]
BATCHES = (1, 3)
NAN = float("nan")


def _lds(D):
    Dp = (D + 3) // 4 * 4
    return (Dp, Dp + 12)


def _padded(x, ld):
    """(..., D) float64 / float32 CPU -> (rows, ld) fp32 device matrix with NaN in the padding columns [D, ld)."""
    x = x.reshape(-1, x.shape[-1])
    out = torch.full((x.shape[0], ld), NAN)
    out[:, :x.shape[1]] = x.float()
    return out.cuda()


def _within(name, got, want, bound):
    """|got - want| <= bound elementwise (float64); the largest err / bound is returned (how far inside the derived bar the kernel sits)."""
    got, want, bound = got.detach().double().cpu(), want.detach().double().cpu(), bound.detach().double().cpu()
    assert got.shape == want.shape == bound.shape, (name, got.shape, want.shape, bound.shape)
    assert bool(torch.isfinite(got).all()), name + ": not finite"
    err = (got - want).abs()
    bad = err > bound
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    assert not bool(bad.any()), "%s: %d of %d entries outside the derived bound, worst %.2f x the bound (|diff| %.3e, |want| up to %.3e)" % (
        name, int(bad.sum()), bad.numel(), ratio, float(err.max()), float(want.abs().max()))
    return ratio


def _untouched(name, t, cols):
    assert bool(torch.isnan(t[..., cols]).all()), name + ": the kernel wrote into columns it does not own"


# ---- the two softmax backward passes (shasta.py:324-325) ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_softmax_backward_against_float64_autograd(N):
    """gmatched[b, t, d] = [t < N] m1 (g1 - sum_d g1 m1) + [d < N] m2 (g2 - sum_t g2 m2).  The kernels get m = fp32(softmax) of the
    float64 logits the reference differentiates: one more rounding per factor, 2 of the 16 ulp."""
    from shasta_amd import hip
    lib = hip.load()
    T = N + 2
    worst = 0.0
    for B in BATCHES:
        gen = torch.Generator().manual_seed(1000 * N + B)
        z1 = (3 * torch.randn(B, N, T, generator=gen)).double().requires_grad_(True)
        z2 = (3 * torch.randn(B, T, N, generator=gen)).double().requires_grad_(True)
        g1, g2 = torch.randn(B, N, T, generator=gen), torch.randn(B, T, N, generator=gen)
        m1, m2 = torch.softmax(z1, 2), torch.softmax(z2, 1)
        ((m1 * g1.double()).sum() + (m2 * g2.double()).sum()).backward()
        want = torch.zeros(B, T, T, dtype=torch.float64)
        want[:, :N, :] += z1.grad
        want[:, :, :N] += z2.grad
        # the bound: per part 16 U (|m g| + |m s|) + |m| (n + 16) U sum|g m|, n = T terms in either sum
        m1d, m2d, g1d, g2d = m1.detach(), m2.detach(), g1.double(), g2.double()
        s1, a1 = (g1d * m1d).sum(2, keepdim=True), (g1d * m1d).abs().sum(2, keepdim=True)
        s2, a2 = (g2d * m2d).sum(1, keepdim=True), (g2d * m2d).abs().sum(1, keepdim=True)
        bound = torch.zeros(B, T, T, dtype=torch.float64)
        bound[:, :N, :] += 16 * U * m1d * (g1d.abs() + s1.abs()) + m1d * (T + 16) * U * a1
        bound[:, :, :N] += 16 * U * m2d * (g2d.abs() + s2.abs()) + m2d * (T + 16) * U * a2
        dm1, dm2, dg1, dg2 = m1d.float().cuda(), m2d.float().cuda(), g1.cuda(), g2.cuda()
        for ld in _lds(T):
            gm = torch.full((B * T, ld), NAN, device="cuda")
            hip.check(lib.shasta_softmax_bwd_f32(hip.ptr(dm1), hip.ptr(dg1), hip.ptr(dm2), hip.ptr(dg2), B, N, hip.ptr(gm), ld, hip.stream_ptr()),
                      "shasta_softmax_bwd_f32")
            gm = gm.cpu().view(B, T, ld)
            worst = max(worst, _within("gmatched (N %d, B %d, ld %d)" % (N, B, ld), gm[:, :, :T], want, bound))
            assert float(gm[:, N:, N:T].abs().max()) == 0.0  # the anchor x anchor corner belongs to neither softmax
            _untouched("gmatched", gm, slice(T, ld))
    print("softmax backward, N = %d: worst |diff| / bound %.3f" % (N, worst))


# ---- the combine (shasta.py:319) ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_combine_backward_against_float64_autograd(N):
    """residual = coeff_0 fused + coeff_1 dist + coeff_2 shape: six products per pair, each one rounding (bound 16 U |want|)."""
    from shasta_amd import hip
    lib = hip.load()
    T = D = N + 2
    worst = 0.0
    for B in BATCHES:
        gen = torch.Generator().manual_seed(2000 * N + B)
        P = B * T * D
        coeff, fused, shape = torch.randn(P, 3, generator=gen), torch.randn(P, 1, generator=gen), torch.randn(P, 1, generator=gen)
        dist, gres = torch.randn(B, T, D, generator=gen) * 5, torch.randn(B, T, D, generator=gen)
        leaves = [t.double().requires_grad_(True) for t in (coeff, fused, shape, dist)]
        c, f, s, d = leaves
        res = c[:, 0] * f[:, 0] + c[:, 1] * d.reshape(-1) + c[:, 2] * s[:, 0]
        (res * gres.double().reshape(-1)).sum().backward()
        for k, ld in enumerate(_lds(D)):
            ldc, ldf, lds = (3, 1, 1) if k == 0 else (4, 2, 3)  # training.py passes the dense (3, 1, 1); wider: the extra columns are zeroed

            def wide(x, w):
                out = torch.full((P, w), NAN)
                out[:, :x.shape[1]] = x
                return out.cuda()
            dc, df, ds = wide(coeff, ldc), wide(fused, ldf), wide(shape, lds)
            ddist, dgres = _padded(dist, ld), _padded(gres, ld)
            gc_, gf, gs, gd = (torch.full((P, ldc), NAN, device="cuda"), torch.full((P, ldf), NAN, device="cuda"),
                               torch.full((P, lds), NAN, device="cuda"), torch.full((B * T, ld), NAN, device="cuda"))
            hip.check(lib.shasta_combine_bwd_f32(hip.ptr(dgres), hip.ptr(dc), ldc, hip.ptr(df), ldf, hip.ptr(ds), lds, hip.ptr(ddist), B, T, D, ld,
                                                 hip.ptr(gc_), hip.ptr(gf), hip.ptr(gs), hip.ptr(gd), hip.stream_ptr()), "shasta_combine_bwd_f32")
            tag = " (N %d, B %d, ld %d)" % (N, B, ld)
            for name, got, want, w in (("gcoeff", gc_, c.grad, 3), ("gfused", gf, f.grad, 1), ("gshape", gs, s.grad, 1)):
                got = got.cpu()
                worst = max(worst, _within(name + tag, got[:, :w], want, 16 * U * want.abs()))
                assert float(got[:, w:].abs().sum()) == 0.0, name + ": columns behind the payload are zeroed"
            gd = gd.cpu()
            worst = max(worst, _within("gdist" + tag, gd[:, :D], d.grad.reshape(B * T, D), 16 * U * d.grad.abs().reshape(B * T, D)))
            _untouched("gdist", gd, slice(D, ld))
    print("combine backward, N = %d: worst |diff| / bound %.3f" % (N, worst))


# ---- the training loss (tools/nusc_shasta/train.py:200-211) -----------------------------------------------------------------------------
@pytest.mark.parametrize("N", SIZES)
def test_affinity_loss_and_its_gradient_against_float64_autograd(N):
    """sums = (s1, c1, s2, c2, loss); s = sum gt (-log(m + 1e-10)) over the n entries with gt = 1, c = their count (exact in fp32).
    A term's magnitude is counted as at least 1: m + 1e-10 is itself a rounded fp32 sum, i.e. one ulp ABSOLUTE in the logarithm."""
    from shasta_amd import hip
    lib = hip.load()
    T = N + 2
    worst = 0.0
    for B in BATCHES:
        gen = torch.Generator().manual_seed(3000 * N + B)
        m1 = torch.softmax(3 * torch.randn(B, N, T, generator=gen), 2)
        m2 = torch.softmax(3 * torch.randn(B, T, N, generator=gen), 1)
        gt = (torch.rand(B, T, T, generator=gen) < max(0.01, 1.0 / T)).float()
        gt[:, 0, 0] = 1.0
        a1, a2, gtd = m1.double().requires_grad_(True), m2.double().requires_grad_(True), gt.double()  # exact copies of the fp32 inputs
        want = O.affinity_loss(a1, a2, gtd)
        (want * 3.0).backward()
        gt1, gt2 = gtd[:, :N, :], gtd[:, :, :N]
        t1, t2 = gt1 * (-torch.log(a1.detach() + 1e-10)), gt2 * (-torch.log(a2.detach() + 1e-10))
        c1, c2 = float(gt1.sum()), float(gt2.sum())
        A1, A2 = float((gt1 * t1.abs().clamp_min(1.0)).sum()), float((gt2 * t2.abs().clamp_min(1.0)).sum())
        b1, b2 = (c1 + 16) * U * A1, (c2 + 16) * U * A2
        ws_want = torch.tensor([float(t1.sum()), c1, float(t2.sum()), c2, float(want)], dtype=torch.float64)
        q1, q2 = abs(float(t1.sum())) / c1, (abs(float(t2.sum())) / c2 if c2 else 0.0)
        ws_bound = torch.tensor([b1, 0.0, b2, 0.0, 0.5 * (b1 / c1 + (b2 / c2 if c2 else b2)) + 16 * U * 0.5 * (q1 + q2)], dtype=torch.float64)
        d1, d2, dgt = m1.cuda(), m2.cuda(), gt.cuda()
        ws = torch.full((4 * B * T,), NAN, device="cuda")
        sums = torch.full((8,), NAN, device="cuda")
        hip.check(lib.shasta_affinity_loss_f32(hip.ptr(d1), hip.ptr(d2), hip.ptr(dgt), B, N, hip.ptr(ws), hip.ptr(sums), hip.stream_ptr()),
                  "shasta_affinity_loss_f32")
        tag = " (N %d, B %d)" % (N, B)
        worst = max(worst, _within("sums" + tag, sums[:5], ws_want, ws_bound))
        _untouched("sums", sums.cpu(), slice(5, 8))
        g1, g2 = torch.full_like(d1, NAN), torch.full_like(d2, NAN)
        gl = torch.tensor([3.0], device="cuda")
        hip.check(lib.shasta_affinity_loss_bwd_f32(hip.ptr(d1), hip.ptr(d2), hip.ptr(dgt), hip.ptr(sums), hip.ptr(gl), B, N, hip.ptr(g1), hip.ptr(g2),
                                                   hip.stream_ptr()), "shasta_affinity_loss_bwd_f32")
        # elementwise: -gt / (m + 1e-10) * (3 / 2) / c, c exact
        worst = max(worst, _within("d m1" + tag, g1, a1.grad, 16 * U * a1.grad.abs()), _within("d m2" + tag, g2, a2.grad, 16 * U * a2.grad.abs()))
    print("loss, N = %d: worst |diff| / bound %.3f" % (N, worst))


# ---- the hand-designed residual (shasta.py:277-283) and its gradient w.r.t. the anchor rows -------------------------------------------
def _far_yaws(others, k):
    """k yaws in (-pi, pi), each as far as possible (on the circle) from `others` and from the ones chosen before it."""
    cand = (torch.arange(4096, dtype=torch.float64) + 0.5) / 4096 * 2 * torch.pi - torch.pi
    others, out = others.double().flatten(), []
    for _ in range(k):
        gap = (cand[:, None] - others[None, :]).abs()
        gap = torch.minimum(gap, 2 * torch.pi - gap).amin(1)
        out.append(float(cand[gap.argmax()]))
        others = torch.cat([others, torch.tensor(out[-1:], dtype=torch.float64)])
    return torch.tensor(out)


def _hand_case(N, B, n_real, seed, flat=False):
    """Box tables (B, T, 7): rows [n_real, N) zero-padded, the anchor rows N, N + 1 with yaws kept away from every yaw of the other table.
    flat: every row of BOTH tables agrees in x, y, z (zeros) - with nf = 3 every column of d2 is all-equal (zero): the normalisation's
    eps branch."""
    gen = torch.Generator().manual_seed(seed)
    T = N + 2
    p, q = O.synth_boxes(gen, B, T, None)[:, :, :7].contiguous(), O.synth_boxes(gen, B, T, None)[:, :, :7].contiguous()
    if n_real is not None:
        p[:, n_real:N], q[:, n_real:N] = 0.0, 0.0
    if flat:
        p[:, :, :3], q[:, :, :3] = 0.0, 0.0
    for b in range(B):
        p[b, N:, 6] = _far_yaws(q[b, :N, 6], 2).float()
        q[b, N:, 6] = _far_yaws(p[b, :, 6], 2).float()
    # sign(log p - log q) decides a term of the anchor gradient: an anchor size within 1e-4 (in the logarithm) of a size it is compared
    # with moves up by 0.1 % until none is (one pair in 1e5 is that close by chance: one case in five at N = 600)
    for _ in range(50):
        lp, lq = torch.log(p[:, :, 3:6].double() + O.EPS_LOG), torch.log(q[:, :, 3:6].double() + O.EPS_LOG)
        near_p = ((lp[:, N:, None] - lq[:, None, :]).abs() < 1e-4).any(2)   # (B, 2, 3): anchors of p against every row of q
        near_q = ((lq[:, N:, None] - lp[:, None, :]).abs() < 1e-4).any(2)
        if not bool(near_p.any() | near_q.any()):
            break
        p[:, N:, 3:6] = torch.where(near_p, p[:, N:, 3:6] * 1.001, p[:, N:, 3:6])
        q[:, N:, 3:6] = torch.where(near_q, q[:, N:, 3:6] * 1.001, q[:, N:, 3:6])
    return p, q


def _hand_check(N, B, nf, n_real, seed, flat=False):
    from shasta_amd import hip
    lib = hip.load()
    T = D = N + 2
    n = T
    p7, q7 = _hand_case(N, B, n_real, seed, flat)
    gen = torch.Generator().manual_seed(seed + 1)
    g = torch.randn(B, T, D, generator=gen)
    P, Q, G = p7.double(), q7.double(), g.double()
    pa, qa = P[:, N:].clone().requires_grad_(True), Q[:, N:].clone().requires_grad_(True)
    want = O.hand_residual(torch.cat([P[:, :N], pa], 1), torch.cat([Q[:, :N], qa], 1), nf)
    (want * G).sum().backward()
    want = want.detach()
    assert bool(torch.isfinite(pa.grad).all()) and bool(torch.isfinite(qa.grad).all()), "the reference itself must be finite on these inputs"

    # -- the pieces of the formula in float64, for the magnitudes the bounds are made of
    eps = O.EPS_LOG
    diff = P[:, :, None, :nf] - Q[:, None, :, :nf]                       # (B, T, D, nf)
    d2 = (diff ** 2).sum(-1)
    norm = d2.norm(dim=1)                                                  # (B, D)
    den = norm.clamp_min(1e-12)
    rel_den = (n + 16) * U                                                 # sqrt halves the relative error of the n-term sum: an upper bound
    lp, lq = torch.log(P[:, :, None, 3:6] + eps), torch.log(Q[:, None, :, 3:6] + eps)
    cp, sp, cq, sq = torch.cos(P[:, :, None, 6]), torch.sin(P[:, :, None, 6]), torch.cos(Q[:, None, :, 6]), torch.sin(Q[:, None, :, 6])
    dc, ds = cp - cq, sp - sq
    rot = torch.sqrt(dc ** 2 + ds ** 2)
    r = d2 / den[:, None, :]
    mag = r + (lp.abs() + lq.abs()).sum(-1) + (cp.abs() + cq.abs() + sp.abs() + sq.abs())
    dist_bound = 16 * U * mag + r * rel_den
    # sign(log p - log q) must be the same in fp32: apart or exactly equal (two zero-padded rows), on the anchor rows' pairs
    dl = (lp - lq).abs()
    for blk in (dl[:, N:], dl[:, :, N:]):
        assert bool(((blk == 0) | (blk > 1e-5)).all()), "an anchor size within fp32 rounding of a size it is compared with (_hand_case keeps them apart)"
    assert float(torch.minimum(rot[:, N:].min(), rot[:, :, N:].min())) > 1e-4, "anchor yaws must stay apart from every row's"
    gs, a_gs = (G * d2).sum(1), (G * d2).abs().sum(1)                      # (B, D): the column sums behind the normalisation's gradient
    gs_bound = (n + 16) * U * a_gs
    live = (norm > 1e-12)[:, None, :]
    t_a = G.abs() / den[:, None, :]
    t_b = torch.where(live, gs[:, None, :].abs() * d2 / den[:, None, :] ** 3, torch.zeros_like(d2))
    # error of gd2 = g / den - gs d2 / den^3 from its two reductions
    e_gd2 = t_a * rel_den + t_b * 3 * rel_den + torch.where(live, d2 / den[:, None, :] ** 3 * gs_bound[:, None, :], torch.zeros_like(d2))
    A = torch.zeros(2, B, 2, 7, dtype=torch.float64)                       # side, batch, anchor row, component
    E = torch.zeros(2, B, 2, 7, dtype=torch.float64)
    for side, sl, dim_o in ((0, (slice(None), slice(N, T), slice(None)), 2), (1, (slice(None), slice(None), slice(N, T)), 1)):
        def over(x):  # sum over the other table's rows -> (B, 2)
            return x[sl].sum(dim_o)
        for k in range(nf):
            A[side, :, :, k] += over((2 * diff[..., k]).abs() * (t_a + t_b))
            E[side, :, :, k] += over((2 * diff[..., k]).abs() * e_gd2)
        own = P[:, :, None, 3:6] if side == 0 else Q[:, None, :, 3:6]
        for k in range(3):
            A[side, :, :, 3 + k] += over(G.abs() * (dl[..., k] > 0) / (own[..., k] + eps).expand_as(dl[..., k]))
        s_own, c_own = (sp, cp) if side == 0 else (sq, cq)
        A[side, :, :, 6] += over(G.abs() * ((dc * s_own).abs() + (ds * c_own).abs()) / rot)
        # cosf / sinf carry ABSOLUTE errors (2 ulp of 1): dc, ds are off by ~5 U, numerator and rot by ~7 U each -> 16 U / rot per term
        E[side, :, :, 6] += over(G.abs() * 16 * U / rot)
    grad_bound = (n + 16) * U * A + E

    worst = 0.0
    ptab, qtab = torch.full((B, T, 8), NAN), torch.full((B, T, 8), NAN)    # column 7 is padding: never read
    ptab[:, :, :7], qtab[:, :, :7] = p7, q7
    ptab, qtab = ptab.cuda(), qtab.cuda()
    for ld in _lds(D):
        tag = " (N %d, B %d, nf %d, n_real %s, ld %d)" % (N, B, nf, n_real, ld)
        dist = torch.full((B * T, ld), NAN, device="cuda")
        denom = torch.full((2 * B * D,), NAN, device="cuda")
        hip.check(lib.shasta_hand_dist_f32(hip.ptr(ptab), hip.ptr(qtab), B, T, D, nf, hip.ptr(dist), ld, hip.ptr(denom), hip.stream_ptr()),
                  "shasta_hand_dist_f32")
        distc = dist.cpu().view(B, T, ld)
        worst = max(worst, _within("dist" + tag, distc[:, :, :D], want, dist_bound))
        _untouched("dist", distc, slice(D, ld))
        worst = max(worst, _within("denom" + tag, denom[:B * D].view(B, D), den, rel_den * den))
        _untouched("denom's second half", denom.cpu(), slice(B * D, 2 * B * D))
        gd = _padded(g, ld)
        dp, dq = torch.full((B, T, 8), NAN, device="cuda"), torch.full((B, T, 8), NAN, device="cuda")
        dp[:, N:, :7], dq[:, N:, :7] = 0.0, 0.0                           # the kernel ADDS to the anchor rows' seven components
        hip.check(lib.shasta_hand_dist_bwd_f32(hip.ptr(gd), ld, hip.ptr(ptab), hip.ptr(qtab), hip.ptr(denom), B, T, D, nf, N, 2, hip.ptr(dp),
                                               hip.ptr(dq), hip.stream_ptr()), "shasta_hand_dist_bwd_f32")
        worst = max(worst, _within("gs" + tag, denom[B * D:].view(B, D), gs, gs_bound))
        worst = max(worst, _within("d prev anchors" + tag, dp[:, N:, :7], pa.grad, grad_bound[0]))
        worst = max(worst, _within("d det anchors" + tag, dq[:, N:, :7], qa.grad, grad_bound[1]))
        for name, t in (("dprev_tab", dp.cpu()), ("ddet_tab", dq.cpu())):
            assert bool(torch.isnan(t[:, :N]).all()) and bool(torch.isnan(t[:, N:, 7]).all()), name + ": only the anchor rows' seven components are written"
    return worst


@pytest.mark.parametrize("nf", [3, 7])
@pytest.mark.parametrize("N", SIZES)
def test_hand_dist_and_anchor_gradient_against_float64_autograd(N, nf):
    worst = max(_hand_check(N, B, nf, None, 4000 * N + 10 * B + nf) for B in BATCHES)
    print("hand-designed residual, N = %d, nf = %d: worst |diff| / bound %.3f" % (N, nf, worst))


@pytest.mark.parametrize("N,n_real,nf,flat", [(14, 9, 7, False), (62, 40, 3, False), (254, 3, 7, False), (255, 0, 3, False), (500, 450, 3, False), (600, 599, 7, False),
                                              (30, 0, 3, True), (257, 100, 3, True), (510, 0, 3, True)])
def test_hand_dist_with_zero_padded_rows(N, n_real, nf, flat):
    """n_real < N: rows of zeros - log(0 + 1e-10) in the size terms, yaw 0 on a whole block of rows, pairs of identical rows (rot = 0,
    sign 0) - and, `flat`, tables whose first three components all agree: every column of d2 is zero and `den` is the eps of the
    normalisation (d2 / max(||d2||, 1e-12)), whose gradient w.r.t. d2 is then g / 1e-12 times 2 (p - q) = 0."""
    worst = max(_hand_check(N, B, nf, n_real, 5000 * N + 10 * B + nf, flat) for B in BATCHES)
    print("hand-designed residual, zero-padded, N = %d: worst |diff| / bound %.3f" % (N, worst))
