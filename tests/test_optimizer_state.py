"""FusedAdam through checkpoint, resume and graph replay: the update kernels at any step number against a float64 restatement of Adam,
state_dict() as a checkpoint, a resumed run against the uninterrupted one, and the books of a step replayed from a hipGraph.

The measure of float32 accuracy everywhere: torch.optim.Adam(foreach=False) on float32 CPU tensors with the same inputs.  Its largest
error against the float64 restatement, per quantity (p normalised by max(1, |p|max) of its tensor, m and v by the tensor's own maximum), is
the yardstick Y of a case; a tensor of FusedAdam passes when its error is at most 2 Y scale + one float32 ulp of the scale (the factor 2:
this project's margin for "a different float32 evaluation of the same formula").  Y is measured on every run; nothing is calibrated on
FusedAdam.  Each case prints `FusedAdam error / Y` per quantity (run with -s)."""
import copy
import functools
import io
import json
import math

import numpy as np
import pytest
import torch

LR, EPS = 3e-3, 1e-8


# ------------------------------------------------------------------------------------------------------------------ the float64 reference
def adam64(p, m, v, t, g, lr, betas, eps, wd):
    """One Adam step in float64 from the state after t steps: L2 weight decay added to the gradient, bias corrections 1 - beta^t, no
    amsgrad (the rule adam_one states in csrc/adam.hip).  Returns the state after t + 1 steps."""
    b1, b2 = betas
    t = t + 1
    g = g + wd * p
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - (lr / (1.0 - b1 ** t)) * m / (v.sqrt() / math.sqrt(1.0 - b2 ** t) + eps)
    return p, m, v, t


def _torch_adam_from(ps, ms, vs, t, lr, betas, wd, dtype):
    """torch.optim.Adam(foreach=False) on CPU tensors of `dtype`, its state put at step t with the given moments."""
    params = [torch.nn.Parameter(p.to(dtype).clone()) for p in ps]
    opt = torch.optim.Adam(params, lr=lr, betas=betas, eps=EPS, weight_decay=wd, foreach=False)
    if ms is not None:
        sd = opt.state_dict()
        sd["state"] = {i: dict(step=torch.tensor(float(t)), exp_avg=m.to(dtype).clone(), exp_avg_sq=v.to(dtype).clone())
                       for i, (m, v) in enumerate(zip(ms, vs))}
        opt.load_state_dict(sd)
    return params, opt


def _pmv(params, opt):
    return [(p.detach().cpu(), opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu()) for p in params]


def _ulp32(x):
    return float(np.spacing(np.float32(x))) if x > 0 else 0.0


def _errors(got, ref):
    """Per tensor and quantity: (max |got - ref|, normalising scale)."""
    out = []
    for g3, r3 in zip(got, ref):
        row = []
        for k, (a, r) in enumerate(zip(g3, r3)):
            scale = float(r.abs().max())
            row.append((float((a.double() - r).abs().max()), max(1.0, scale) if k == 0 else scale))
        out.append(row)
    return out


def _within_twice_the_yardstick(name, fused, yard, ref):
    """fused, yard: lists of (p, m, v) float32; ref: the same in float64.  Returns the ratios FusedAdam error / Y for p, m, v."""
    ef, ey = _errors(fused, ref), _errors(yard, ref)
    ratios = []
    for k in range(3):
        Y = max((e / s for e, s in (row[k] for row in ey) if s > 0), default=0.0)
        worst = max((e / s for e, s in (row[k] for row in ef) if s > 0), default=0.0)
        ratios.append(worst / Y if Y > 0 else float("inf") if worst > 0 else 0.0)
    print("%s: FusedAdam error / yardstick  p %.2f  m %.2f  v %.2f" % ((name,) + tuple(ratios)))
    for k, q in enumerate("pmv"):
        Y = max((e / s for e, s in (row[k] for row in ey) if s > 0), default=0.0)
        for i, row in enumerate(ef):
            e, s = row[k]
            assert e <= 2.0 * Y * s + _ulp32(s), "%s: %s of tensor %d: error %.3e, bar 2 x %.3e x %.3e + %.3e" % (name, q, i, e, Y, s, _ulp32(s))
    return ratios


def _same_between_modes(name, a, b):
    """The tolerance test_capturable_adam_and_the_graphed_step_equal_the_eager_loop uses between the plain and the device-argument mode."""
    for i, (x3, y3) in enumerate(zip(a, b)):
        for q, x, y in zip("pmv", x3, y3):
            assert float((x - y).abs().max()) <= 1e-6 * max(1.0, float(y.abs().max())), "%s: %s of tensor %d" % (name, q, i)


def test_the_float64_restatement_is_torch_adam():
    """adam64 against torch.optim.Adam on float64 CPU tensors, 5 steps from a fresh optimizer, to 1e-14 relative."""
    for wd in (0.0, 0.01):
        gen = torch.Generator().manual_seed(5)
        p0 = [torch.randn(n, generator=gen, dtype=torch.float64) for n in (1, 37, 1000)]
        params, opt = _torch_adam_from(p0, None, None, 0, LR, (0.9, 0.999), wd, torch.float64)
        ref = [(p.clone(), torch.zeros_like(p), torch.zeros_like(p), 0) for p in p0]
        for _ in range(5):
            gs = [torch.randn(p.shape, generator=gen, dtype=torch.float64) for p in p0]
            for p, g in zip(params, gs):
                p.grad = g.clone()
            opt.step()
            ref = [adam64(*r, g, LR, (0.9, 0.999), EPS, wd) for r, g in zip(ref, gs)]
            for p, r in zip(params, ref):
                st = opt.state[p]
                assert r[3] == int(st["step"])
                for got, want in ((p.detach(), r[0]), (st["exp_avg"], r[1]), (st["exp_avg_sq"], r[2])):
                    assert float((got - want).abs().max()) <= 1e-14 * max(1.0, float(want.abs().max()))


# --------------------------------------------------------------------------------------------------------- A. the kernels at any step number
# above MULTI_MAX_NUMEL with n % 4 = 3, 2, 1, 0 (adam_kernel's vector body and scalar tail); the last one is the all-zero tensor
LARGE = [(262147,), (262146,), (262145,), (600, 500), (263000,)]
# (512, 512) is exactly MULTI_MAX_NUMEL; with the 50 small ones 51 tensors = two launches of adam_multi, 48 + 3
SMALL = [(512, 512), (1,), (7,), (33, 5), (1000, 129)] + [(3, 5)] * 46
SHAPES = LARGE + SMALL
ZERO = len(LARGE) - 1
STEPS = (1, 2, 11, 1000, 100000)


@functools.lru_cache(maxsize=None)
def _seeded_inputs():
    """p ~ N(0,1), m ~ 0.1 N(0,1), v = (0.1 N(0,1))^2, g ~ N(0,1) with 10 % exact zeros (padded anchor rows send exact zeros); one tensor with
    g = m = v = 0 everywhere.  float32 on the host, made once and left unchanged."""
    gen = torch.Generator().manual_seed(20)
    ps, ms, vs, gs = [], [], [], []
    for i, s in enumerate(SHAPES):
        ps.append(torch.randn(*s, generator=gen))
        ms.append(0.1 * torch.randn(*s, generator=gen))
        vs.append((0.1 * torch.randn(*s, generator=gen)) ** 2)
        g = torch.randn(*s, generator=gen)
        g[torch.rand(*s, generator=gen) < 0.1] = 0.0
        if i == ZERO:
            ms[-1].zero_(), vs[-1].zero_(), g.zero_()
        gs.append(g)
    return ps, ms, vs, gs


def _hand_built_state(ms, vs, step, lr, betas, wd):
    return dict(state={i: dict(step=step, exp_avg=m.clone(), exp_avg_sq=v.clone()) for i, (m, v) in enumerate(zip(ms, vs))},
                param_groups=[dict(lr=lr, betas=betas, eps=EPS, weight_decay=wd, params=list(range(len(ms))))])


def _misaligned(g, dev):
    """A gradient that is a view at a 4-byte offset (csrc/pair_bwd.hip's image), as in test_fused_adam_matches_torch_adam."""
    odd = torch.empty(g.numel() + 1, device=dev)
    odd[1:].copy_(g.flatten())
    return odd[1:].view(g.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("t,wd,betas", [(t, wd, (0.9, 0.999)) for t in STEPS for wd in (0.0, 0.01)] + [(11, 0.01, (0.85, 0.95))])
def test_step_from_seeded_state_at_any_step_number(t, wd, betas, monkeypatch):
    """shasta_adam_step_f32 and shasta_adam_multi_f32 through FusedAdam.step(), with the launch arguments from the host and from device
    memory (capturable=True), at step t from a state put in with load_state_dict at step t - 1: the device-argument mode reaches step t
    only because the load seeds its counter.  (0.85, 0.95): the other end of OneCycleLR's cycle."""
    from shasta_amd import hip
    from shasta_amd.training import FusedAdam
    dev = torch.device("cuda:0")
    ps, ms, vs, gs = _seeded_inputs()
    ref = [adam64(p.double(), m.double(), v.double(), t - 1, g.double(), LR, betas, EPS, wd)[:3] for p, m, v, g in zip(ps, ms, vs, gs)]
    yp, yo = _torch_adam_from(ps, ms, vs, t - 1, LR, betas, wd, torch.float32)
    for p, g in zip(yp, gs):
        p.grad = g.clone()
    yo.step()
    yard = _pmv(yp, yo)
    lib = hip.load()
    calls = dict(single=[], multi=[])
    single, multi = lib.shasta_adam_step_f32, lib.shasta_adam_multi_f32
    monkeypatch.setattr(lib, "shasta_adam_step_f32", lambda *a: (calls["single"].append(int(a[4])), single(*a))[1])
    monkeypatch.setattr(lib, "shasta_adam_multi_f32", lambda *a: (calls["multi"].append(int(a[0])), multi(*a))[1])
    got = {}
    for capturable in (False, True):
        params = [torch.nn.Parameter(p.to(dev)) for p in ps]
        opt = FusedAdam(params, lr=1.0, betas=(0.5, 0.5), weight_decay=0.5, capturable=capturable)  # the loaded group's values are the ones used
        opt.load_state_dict(_hand_built_state(ms, vs, t - 1, LR, betas, wd))
        for p, g in zip(params, gs):
            p.grad = _misaligned(g, dev)
        calls["single"].clear(), calls["multi"].clear()
        opt.step()
        torch.cuda.synchronize()
        assert sorted(calls["single"]) == sorted(int(np.prod(s)) for s in LARGE), "one launch per tensor above MULTI_MAX_NUMEL"
        assert calls["multi"] == [len(SMALL)] and FusedAdam.MULTI_MAX_NUMEL == 512 * 512, "(512, 512) goes with the small ones: 48 + 3"
        assert all(opt.state[p]["step"] == t for p in params)
        if capturable:
            assert opt.device_step(0) == t
        got[capturable] = _pmv(params, opt)
        name = "step/multi %s t=%d wd=%g betas=%s" % ("d_dyn" if capturable else "host", t, wd, betas)
        _within_twice_the_yardstick(name, got[capturable], yard, ref)
        if wd == 0.0:
            for x, x0 in zip(got[capturable][ZERO], (ps[ZERO], ms[ZERO], vs[ZERO])):
                assert torch.equal(x, x0), "g = m = v = 0 and no weight decay: nothing moves"
    _same_between_modes("t=%d" % t, got[True], got[False])


def _prepared_dyn(lib, hip, t, lr, betas, dev):
    """What FusedAdam(capturable=True) hands the kernels at step t: shasta_adam_prepare_f32 on a counter that stands at t - 1."""
    step = torch.full((1,), t - 1, dtype=torch.int32, device=dev)
    hyper = torch.tensor([lr, betas[0], betas[1]], dtype=torch.float64).to(dev)
    dyn = torch.zeros(6, device=dev)
    hip.check(lib.shasta_adam_prepare_f32(hip.ptr(step), hip.ptr(hyper), hip.ptr(dyn), hip.stream_ptr()), "prepare")
    assert int(step) == t
    return dyn


@pytest.mark.gpu
@pytest.mark.parametrize("H,K,R,Rdx", [(33, 260, 3, 8), (33, 260, 16, 8), (33, 260, 24, 8), (33, 260, 64, 8), (131, 1032, 8, 5), (131, 1032, 40, 12)])
def test_lowrank_entries_from_seeded_state_at_any_step_number(H, K, R, Rdx):
    """shasta_adam_lowrank_f32 (at 33 x 260, R = 3, 16, 24, 64: the <8,2>, <16,4>, <32,1> and <64,1> instantiations) and
    shasta_adam_lowrank_dx_f32 (all six cases) with the `step` argument and with d_dyn, p, m and v only: the dx form's Y is pinned by
    test_adam_lowrank_with_the_product_in_the_same_pass, and the large-matrix instantiations (H K > 2^26) are left to
    test_adam_from_gradient_factors_small_and_large_matrices_agree, which holds them equal to the small ones.  The reference forms the
    gradient G^T X in float64, the yardstick in float32 with torch.matmul."""
    from shasta_amd import hip
    lib = hip.load()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(R * 1000 + H)
    p0, m0 = torch.randn(H, K, generator=gen), 0.1 * torch.randn(H, K, generator=gen)
    v0 = (0.1 * torch.randn(H, K, generator=gen)) ** 2
    G, X, Gdx = torch.randn(R, H, generator=gen), torch.randn(R, K, generator=gen), torch.randn(Rdx, H, generator=gen)
    G[:, torch.rand(H, generator=gen) < 0.1] = 0.0  # rows of the gradient that are exactly zero
    g64, g32 = G.double().t() @ X.double(), torch.matmul(G.t(), X)
    Gd, Xd, Gdxd = G.to(dev), X.to(dev), Gdx.to(dev)
    nb = lib.shasta_adam_lowrank_dx_workspace_bytes(H, K, Rdx)
    ws, y = torch.empty((nb + 3) // 4, device=dev), torch.empty(Rdx, K, device=dev)
    forms = ["lowrank", "lowrank_dx"] if (H, K) == (33, 260) else ["lowrank_dx"]
    for t, wd, betas in [(t, wd, (0.9, 0.999)) for t in STEPS for wd in (0.0, 0.01)] + [(11, 0.01, (0.85, 0.95))]:
        ref = [adam64(p0.double(), m0.double(), v0.double(), t - 1, g64, LR, betas, EPS, wd)[:3]]
        yp, yo = _torch_adam_from([p0], [m0], [v0], t - 1, LR, betas, wd, torch.float32)
        yp[0].grad = g32.clone()
        yo.step()
        yard = _pmv(yp, yo)
        for form in forms:
            got = {}
            for mode in ("host", "d_dyn"):
                p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
                dyn = _prepared_dyn(lib, hip, t, LR, betas, dev) if mode == "d_dyn" else None
                # d_dyn given: lr, the betas and step are ignored (deliberately wrong here)
                hyper = (LR, betas[0], betas[1], EPS, wd, t, None) if dyn is None else (1.0, 0.5, 0.5, EPS, wd, 0, hip.ptr(dyn))
                if form == "lowrank":
                    hip.check(lib.shasta_adam_lowrank_f32(hip.ptr(p), hip.ptr(m), hip.ptr(v), H, K, hip.ptr(Gd), H, hip.ptr(Xd), K, R, *hyper,
                                                          hip.stream_ptr()), form)
                else:
                    hip.check(lib.shasta_adam_lowrank_dx_f32(hip.ptr(p), hip.ptr(m), hip.ptr(v), H, K, hip.ptr(Gd), H, hip.ptr(Xd), K, R, hip.ptr(Gdxd), H,
                                                             Rdx, hip.ptr(y), K, 0, hip.ptr(ws), nb, *hyper, hip.stream_ptr()), form)
                torch.cuda.synchronize()
                got[mode] = [(p.cpu(), m.cpu(), v.cpu())]
                _within_twice_the_yardstick("%s R=%d %dx%d %s t=%d wd=%g betas=%s" % (form, R, H, K, mode, t, wd, betas), got[mode], yard, ref)
            _same_between_modes("%s t=%d" % (form, t), got["d_dyn"], got["host"])


# ------------------------------------------------------------------------------------------------------------ B. state_dict() is a checkpoint
GROUP_KEYS = {"lr", "betas", "eps", "weight_decay", "params"}
ONE_CYCLE_KEYS = {"initial_lr", "max_lr", "min_lr", "base_momentum", "max_momentum"}


def _is_plain_data(x):
    if isinstance(x, (list, tuple)):
        return all(_is_plain_data(y) for y in x)
    return isinstance(x, (int, float, bool, str)) or x is None


def _check_is_a_checkpoint(sd, scheduled):
    for g in sd["param_groups"]:
        assert GROUP_KEYS <= set(g) <= GROUP_KEYS | (ONE_CYCLE_KEYS if scheduled else set()), sorted(g)
        assert all(_is_plain_data(x) for x in g.values()), "numbers only: no tensor in param_groups"
    json.dumps(sd["param_groups"])
    for st in sd["state"].values():
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert isinstance(st["step"], int)


@pytest.mark.parametrize("capturable", [False, True])
def test_state_dict_holds_numbers_and_moments_only(capturable):
    """Host only (CPU parameters, no kernel): what state_dict() of either mode contains, with and without a scheduler."""
    from shasta_amd.training import FusedAdam
    ps = [torch.nn.Parameter(torch.randn(3, 5)), torch.nn.Parameter(torch.randn(7))]
    opt = FusedAdam([dict(params=ps[:1]), dict(params=ps[1:], lr=1e-4)], lr=LR, weight_decay=0.01, capturable=capturable)
    _check_is_a_checkpoint(opt.state_dict(), False)
    assert opt.state_dict()["state"] == {}
    torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-2, total_steps=13)
    sd = opt.state_dict()
    sd["state"] = {i: dict(step=4, exp_avg=torch.randn_like(p), exp_avg_sq=torch.rand_like(p)) for i, p in enumerate(ps)}
    opt.load_state_dict(sd)
    out = opt.state_dict()
    _check_is_a_checkpoint(out, True)
    assert [st["step"] for st in out["state"].values()] == [4, 4]
    assert all(torch.equal(out["state"][i][k], sd["state"][i][k]) for i in (0, 1) for k in ("exp_avg", "exp_avg_sq"))
    assert not any(k.startswith("_") for g in opt.param_groups for k in g), "nothing private in the live groups either"


def _round_trip(obj):
    buf = io.BytesIO()
    torch.save(obj, buf)
    buf.seek(0)
    return torch.load(buf, map_location="cpu")


def _assert_same_state_dict(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert set(a["state"]) == set(b["state"])
    for i in a["state"]:
        assert a["state"][i]["step"] == b["state"][i]["step"]
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(a["state"][i][k].cpu(), b["state"][i][k].cpu()), (i, k)


# ----------------------------------------------------------------------------------------- the tiny model case of tests/test_training.py
def _tiny(total):
    """_case(12, 7, 4, 3, seed=23) on the device, make(capturable) and the eager loop of
    test_capturable_adam_and_the_graphed_step_equal_the_eager_loop (first layers stepped inside the backward, OneCycleLR)."""
    from shasta_amd import training
    from tests.test_training import _case
    c, model, w, a, b, det, prev, gt = _case(12, 7, 4, 3, seed=23)
    dev = torch.device("cuda:0")
    base = model.to(dev).train()
    ad, bd, gtd, detd, prevd = a.to(dev), b.to(dev), gt.to(dev), det.to(dev).contiguous(), prev.to(dev).contiguous()

    def make(capturable):
        m = copy.deepcopy(base)
        opt = training.FusedAdam(m.parameters(), lr=1e-3, weight_decay=0.01, lowrank_first_layers=m, in_backward=True, capturable=capturable)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=5e-3, total_steps=total + 1)
        return m, opt, sched

    def one(m, opt):
        opt.zero_grad(set_to_none=True)
        m1, m2 = training.affinity_train(m, ad, bd, detd.clone(), prevd)
        loss = training.affinity_loss(m1, m2, gtd)
        loss.backward()
        opt.step()
        return loss.detach()

    def eager(m, opt, sched, steps, losses):
        for _ in range(steps):
            losses.append(float(one(m, opt)))
            sched.step()

    def graphed(m, opt):
        return training.GraphedTrainStep(m, opt, ad, bd, detd, prevd, gtd, warmup=3), (ad, bd, detd, prevd, gtd)
    return make, one, eager, graphed


def _stepped(opt):
    return [p for g in opt.param_groups for p in g["params"] if opt.state.get(p)]


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["eager", "graphed"])
def test_a_snapshot_of_state_dict_stays_at_its_step(how):
    """deepcopy(opt.state_dict()) taken at step k of a capturable optimizer says step k and holds that step's moments after three more
    steps (nothing in it is aliased to the running optimizer, and its step is the counter's value then - replays included), and goes
    through torch.save / torch.load(map_location='cpu') unchanged."""
    make, one, eager, graphed = _tiny(12)
    m, opt, sched = make(True)
    if how == "eager":
        k = 4
        eager(m, opt, sched, k, [])
        more = lambda: eager(m, opt, sched, 3, [])  # noqa: E731
    else:
        step, batch = graphed(m, opt)
        k = 3 + 2
        for _ in range(2):
            step(*batch)
            sched.step()

        def more():
            for _ in range(3):
                step(*batch)
                sched.step()
    assert opt.device_step(0) == k
    snap = copy.deepcopy(opt.state_dict())
    _check_is_a_checkpoint(snap, True)
    assert len(snap["state"]) == len(_stepped(opt)) > 10 and all(st["step"] == k for st in snap["state"].values())
    loaded = _round_trip(snap)
    assert all(not t.is_cuda for st in loaded["state"].values() for t in (st["exp_avg"], st["exp_avg_sq"]))
    more()
    torch.cuda.synchronize()
    assert all(st["step"] == k for st in snap["state"].values())
    _assert_same_state_dict(snap, loaded)
    now = opt.state_dict()
    assert all(st["step"] == k + 3 for st in now["state"].values()) and opt.device_step(0) == k + 3
    assert any(not torch.equal(now["state"][i]["exp_avg"], snap["state"][i]["exp_avg"]) for i in snap["state"]), "the optimizer went on"


# ------------------------------------------------------------------------------------------------ C. resume equals the uninterrupted run
C_STEPS, C_TOTAL, C_MAX_LR = 12, 13, 1e-2


@functools.lru_cache(maxsize=None)
def _c_inputs():
    gen = torch.Generator().manual_seed(31)
    ps = [torch.randn(*s, generator=gen) for s in SHAPES]
    gs = [[torch.randn(*s, generator=gen) for s in SHAPES] for _ in range(C_STEPS)]
    return ps, gs


def _c_new(ps, capturable, dev):
    from shasta_amd.training import FusedAdam
    params = [torch.nn.Parameter(p.to(dev)) for p in ps]
    opt = FusedAdam(params, lr=LR, weight_decay=0.01, capturable=capturable)
    return params, opt, torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=C_MAX_LR, total_steps=C_TOTAL)


def _c_run(params, opt, sched, gs, dev):
    for step_grads in gs:
        for p, g in zip(params, step_grads):
            p.grad = g.to(dev)
        opt.step()
        sched.step()


_C_UNINTERRUPTED = {}


def _c_uninterrupted(capturable):
    """The 12-step run of one mode, made once and shared."""
    if capturable not in _C_UNINTERRUPTED:
        dev = torch.device("cuda:0")
        ps, gs = _c_inputs()
        params, opt, sched = _c_new(ps, capturable, dev)
        _c_run(params, opt, sched, gs, dev)
        _C_UNINTERRUPTED[capturable] = _pmv(params, opt)
    return _C_UNINTERRUPTED[capturable]


@pytest.mark.gpu
@pytest.mark.parametrize("before,after", [(False, False), (True, True), (False, True), (True, False)])
def test_resumed_run_equals_the_uninterrupted_run(before, after):
    """Six steps under OneCycleLR, optimizer + scheduler + parameters through torch.save / torch.load(map_location='cpu') into fresh
    objects, six more steps: the same mode before and after gives the bits of the uninterrupted 12-step run (elementwise kernels, the same
    input bits, nothing reorders); a change of mode (capturable or not: `before` -> `after`) stays within the tolerance between the modes.
    Teeth: a counter that restarts at 1 after six steps scales the first resumed update by (1 - 0.9^7) / (1 - 0.9), about 5: p moves by
    more than lr (3e-3 and up here), orders of magnitude outside 1e-6 max(1, |p|) and certainly not the same bits."""
    dev = torch.device("cuda:0")
    ps, gs = _c_inputs()
    params, opt, sched = _c_new(ps, before, dev)
    _c_run(params, opt, sched, gs[:6], dev)
    ckpt = _round_trip(dict(opt=opt.state_dict(), sched=sched.state_dict(), params=[p.detach() for p in params]))
    _check_is_a_checkpoint(ckpt["opt"], True)
    params, opt, sched = _c_new([torch.zeros_like(p) for p in ps], after, dev)
    with torch.no_grad():
        for p, q in zip(params, ckpt["params"]):
            p.copy_(q)
    opt.load_state_dict(ckpt["opt"])
    sched.load_state_dict(ckpt["sched"])
    _c_run(params, opt, sched, gs[6:], dev)
    got, want = _pmv(params, opt), _c_uninterrupted(before)
    assert all(opt.state[p]["step"] == C_STEPS for p in params)
    if before == after:
        bit_exact = all(torch.equal(x, y) for x3, y3 in zip(got, want) for x, y in zip(x3, y3))
        print("resume %s -> %s bit-exact: %s" % (before, after, bit_exact))
        assert bit_exact
    else:
        _same_between_modes("resume %s -> %s" % (before, after), got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("capturable", [False, True])
def test_twelve_uninterrupted_steps_are_fp32_accurate(capturable):
    """The uninterrupted 12-step run against the float64 restatement driven by the same schedule; the yardstick is torch's float32 Adam
    over the same 12 steps."""
    ps, gs = _c_inputs()
    yp, yo = _torch_adam_from(ps, None, None, 0, LR, (0.9, 0.999), 0.01, torch.float32)
    ys = torch.optim.lr_scheduler.OneCycleLR(yo, max_lr=C_MAX_LR, total_steps=C_TOTAL)
    ref = [(p.double(), torch.zeros_like(p, dtype=torch.float64), torch.zeros_like(p, dtype=torch.float64), 0) for p in ps]
    for step_grads in gs:
        lr, betas = yo.param_groups[0]["lr"], yo.param_groups[0]["betas"]
        ref = [adam64(*r, g.double(), lr, betas, EPS, 0.01) for r, g in zip(ref, step_grads)]
        for p, g in zip(yp, step_grads):
            p.grad = g.clone()
        yo.step()
        ys.step()
    _within_twice_the_yardstick("12 steps capturable=%s" % capturable, _c_uninterrupted(capturable), _pmv(yp, yo), [r[:3] for r in ref])


@pytest.mark.gpu
@pytest.mark.parametrize("capturable", [False, True])
def test_resumed_training_of_the_model_gives_the_same_bits(capturable):
    """The tiny model, first layers stepped inside the backward from the factors of their gradient, weight decay, OneCycleLR: four steps,
    model + optimizer + scheduler through torch.save / torch.load(map_location='cpu') into a fresh copy of the base model, four more.
    Losses 5 to 8 and every parameter have the bits of the uninterrupted 8-step run (the step is bit-reproducible:
    test_backward_at_the_headline_size_twice_the_same_bits)."""
    make, one, eager, graphed = _tiny(8)
    whole, lw = make(capturable), []
    eager(*whole, 8, lw)
    first, l1 = make(capturable), []
    eager(*first, 4, l1)
    ckpt = _round_trip(dict(model=first[0].state_dict(), opt=first[1].state_dict(), sched=first[2].state_dict()))
    second, l2 = make(capturable), []
    second[0].load_state_dict(ckpt["model"])
    second[1].load_state_dict(ckpt["opt"])
    second[2].load_state_dict(ckpt["sched"])
    eager(*second, 4, l2)
    assert l1 + l2 == lw, (l1 + l2, lw)
    for (k, p), (_, q) in zip(whole[0].named_parameters(), second[0].named_parameters()):
        assert torch.equal(p, q), k
    assert all(second[1].state[p]["step"] == 8 for p in _stepped(second[1]))


# -------------------------------------------------------------------------------------------------------- D. graph replay keeps the books
@pytest.mark.gpu
def test_graphed_steps_are_counted_and_resume_eagerly():
    """GraphedTrainStep(warmup=3): state['step'] is 3 after construction (the capture pass applies no update and does not count), 8 after
    five replays, and equal to the device counter.  The checkpoint written then, loaded into a fresh model with an eager capturable
    optimizer and stepped three more times, follows the loop that never used a graph (three eager steps without moving the schedule, then
    eight with one scheduler step each - the `ref` of test_capturable_adam_and_the_graphed_step_equal_the_eager_loop) within that test's
    tolerances."""
    total = 9
    make, one, eager, graphed = _tiny(total)
    ref, lr_ = make(True), []
    for _ in range(3):
        one(ref[0], ref[1])
    eager(*ref, 8, lr_)
    m, opt, sched = make(True)
    step, batch = graphed(m, opt)
    assert {opt.state[p]["step"] for p in _stepped(opt)} == {3} and opt.device_step(0) == 3
    lg = []
    for _ in range(5):
        lg.append(float(step(*batch)))
        sched.step()
    assert {opt.state[p]["step"] for p in _stepped(opt)} == {8} and opt.device_step(0) == 8
    ckpt = _round_trip(dict(model=m.state_dict(), opt=opt.state_dict(), sched=sched.state_dict()))
    m2, opt2, sched2 = make(True)
    m2.load_state_dict(ckpt["model"])
    opt2.load_state_dict(ckpt["opt"])
    sched2.load_state_dict(ckpt["sched"])
    eager(m2, opt2, sched2, 3, lg)
    assert opt2.device_step(0) == 11
    assert len(lg) == len(lr_) == 8
    for x, y in zip(lr_, lg):
        assert abs(x - y) <= 1e-6 * max(1.0, abs(x)), (lr_, lg)
    for (k, p), (_, q) in zip(ref[0].named_parameters(), m2.named_parameters()):
        assert float((p - q).detach().abs().max()) <= 1e-6 * max(1.0, float(p.detach().abs().max())), k


@pytest.mark.gpu
def test_load_state_dict_under_a_live_graph():
    """Five replays, a snapshot of model + optimizer + scheduler, three more replays (weights W1); the snapshot loaded back into the SAME
    objects and three more replays give W1 again, bit for bit: load_state_dict writes into the counter, the schedule values and the
    moments that the captured graph points at instead of replacing them.  The books read 8 after the load and 11 after the replays."""
    make, one, eager, graphed = _tiny(12)
    m, opt, sched = make(True)
    step, batch = graphed(m, opt)

    def replay(n):
        for _ in range(n):
            step(*batch)
            sched.step()
    replay(5)
    snap = copy.deepcopy((m.state_dict(), opt.state_dict(), sched.state_dict()))
    replay(3)
    torch.cuda.synchronize()
    W1 = {k: p.detach().clone() for k, p in m.named_parameters()}
    M1 = copy.deepcopy(opt.state_dict())
    m.load_state_dict(snap[0])
    opt.load_state_dict(snap[1])
    sched.load_state_dict(snap[2])
    assert {opt.state[p]["step"] for p in _stepped(opt)} == {8} and opt.device_step(0) == 8
    replay(3)
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        assert torch.equal(p, W1[k]), k
    assert {opt.state[p]["step"] for p in _stepped(opt)} == {11} and opt.device_step(0) == 11
    _assert_same_state_dict(opt.state_dict(), M1)


# --------------------------------------------------------------------------------------------------------------------- E. one counter per group
@pytest.mark.gpu
def test_capturable_group_refuses_parameters_at_different_steps():
    """A parameter that had no gradient for two steps stands at another step number than its group.  The plain mode corrects every tensor by
    its own count, like torch; one device-side counter cannot, so step() of a capturable optimizer raises, names the parameter and
    changes nothing."""
    from shasta_amd import hip
    from shasta_amd.training import FusedAdam
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(41)
    shapes = [(33, 5), (7,), (600, 500)]
    p0 = [torch.randn(*s, generator=gen) for s in shapes]
    gs = [[torch.randn(*s, generator=gen) for s in shapes] for _ in range(4)]
    params = [torch.nn.Parameter(p.to(dev)) for p in p0]
    opt = FusedAdam(params, lr=LR, weight_decay=0.01)
    for it in range(3):
        for i, (p, g) in enumerate(zip(params, gs[it])):
            p.grad = None if (i == 1 and it > 0) else g.to(dev)
        opt.step()
    assert [opt.state[p]["step"] for p in params] == [3, 1, 3]
    ckpt = _round_trip(dict(opt=opt.state_dict(), params=[p.detach() for p in params]))

    def resumed(capturable):
        ps = [torch.nn.Parameter(q.to(dev)) for q in ckpt["params"]]
        o = FusedAdam(ps, lr=LR, weight_decay=0.01, capturable=capturable)
        o.load_state_dict(ckpt["opt"])
        for p, g in zip(ps, gs[3]):
            p.grad = g.to(dev)
        return ps, o
    ps, o = resumed(True)
    before = _pmv(ps, o)
    with pytest.raises(hip.ShastaHipError, match=r"param_groups\[0\]\['params'\]\[1\] \(shape \(7,\)\) is at step 1.*step 3"):
        o.step()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x3, y3 in zip(_pmv(ps, o), before) for x, y in zip(x3, y3)) and o.state[ps[0]]["step"] == 3
    # the plain mode: every tensor by its own count, against the float64 restatement and torch's float32 Adam from the same state
    ps, o = resumed(False)
    o.step()
    assert [o.state[p]["step"] for p in ps] == [4, 2, 4]
    st = ckpt["opt"]["state"]
    ref = [adam64(q.double(), st[i]["exp_avg"].double(), st[i]["exp_avg_sq"].double(), st[i]["step"], g.double(), LR, (0.9, 0.999), EPS, 0.01)[:3]
           for i, (q, g) in enumerate(zip(ckpt["params"], gs[3]))]
    yard = []
    for i, (q, g) in enumerate(zip(ckpt["params"], gs[3])):
        yp, yo = _torch_adam_from([q], [st[i]["exp_avg"]], [st[i]["exp_avg_sq"]], st[i]["step"], LR, (0.9, 0.999), 0.01, torch.float32)
        yp[0].grad = g.clone()
        yo.step()
        yard += _pmv(yp, yo)
    _within_twice_the_yardstick("plain mode, steps 4 / 2 / 4", _pmv(ps, o), yard, ref)
