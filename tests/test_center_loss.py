"""CenterPoint head losses with their gradient (csrc/center_loss.hip, shasta_amd/head_loss.py) against float64 torch autograd of the same
formulas on the CPU.  The bar of every figure is 4 x the error of torch's own fp32 CPU composite against float64 on the same inputs, with
the floors the loss values (16 u sum|term|) and the gradient entries (16 u |g| + u max|g|) get from fp32 rounding alone, u = 2^-24.
The largest error / bar ratios are printed; DESIGN.md section 4 records them."""
import numpy as np
import pytest
import torch

from . import center_targets_helpers as H

U = 2.0 ** -24
WEIGHT, CODE_WEIGHTS = 0.25, [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0]
HEADS = ("hm", "reg", "height", "dim", "vel", "rot")
WIDTH = dict(reg=2, height=1, dim=3, vel=2, rot=2)


# ---- CPU: the composite by hand ---------------------------------------------------------------------------------------------------
def test_composite_matches_hand_computed_values_on_a_2x2_map():
    from shasta_amd import head_loss
    x = torch.tensor([[[[0.0, 2.0], [-1.0, 30.0]]]], dtype=torch.float64)          # (1, 1, 2, 2); 30: beyond the upper clamp bound
    target = torch.tensor([[[[1.0, 0.5], [0.0, 0.0]]]], dtype=torch.float64)
    ind, mask, cat = torch.tensor([[0, 3, 1]]), torch.tensor([[1, 1, 0]], dtype=torch.uint8), torch.zeros(1, 3, dtype=torch.int64)
    pd = dict(hm=x.clone().requires_grad_(True))
    for i, (n, w) in enumerate(WIDTH.items()):
        pd[n] = torch.full((1, w, 2, 2), 0.5 * (i + 1), dtype=torch.float64)
    anno = torch.zeros(1, 3, 10, dtype=torch.float64)
    anno[0, 0] = torch.arange(10, dtype=torch.float64) * 0.1
    anno[0, 2] = 100.0  # masked out
    out = head_loss.composite_task_loss(pd, target, anno, ind, mask, cat, WEIGHT, CODE_WEIGHTS)
    p = [1 / (1 + np.exp(-0.0)), 1 / (1 + np.exp(-2.0)), 1 / (1 + np.exp(1.0)), 1 - 1e-4]
    t = [1.0, 0.5, 0.0, 0.0]
    neg = sum(np.log(1 - pi) * pi ** 2 * (1 - ti) ** 4 for pi, ti in zip(p, t))
    pos = np.log(p[0]) * (1 - p[0]) ** 2 + np.log(p[3]) * (1 - p[3]) ** 2
    assert abs(float(out["hm_loss"].detach()) - (-(pos + neg) / 2)) < 1e-12 and float(out["num_positive"]) == 2
    pred = [0.5, 0.5, 1.0, 1.5, 1.5, 1.5, 2.0, 2.0, 2.5, 2.5]
    elem = [(abs(pred[c] - 0.1 * c) + abs(pred[c])) / (2 + 1e-4) for c in range(10)]
    np.testing.assert_allclose(out["loc_loss_elem"].numpy(), elem, rtol=1e-12)
    loc = sum(e * w for e, w in zip(elem, CODE_WEIGHTS))
    assert abs(float(out["loc_loss"]) - loc) < 1e-12 and abs(float(out["loss"]) - (-(pos + neg) / 2 + WEIGHT * loc)) < 1e-12
    out["loss"].backward()
    assert float(pd["hm"].grad[0, 0, 1, 1]) == 0.0  # the clamp is active: no gradient
    # d/dx of -(log(p) (1 - p)^2) / 2 at x = 0 (target 1: no negative term): -((1 - p)^3 - 2 p (1 - p)^2 log p) / 2
    assert abs(float(pd["hm"].grad[0, 0, 0, 0]) - (-(0.125 - 2 * 0.5 * 0.25 * np.log(0.5)) / 2)) < 1e-12
    # no positives: -neg
    out0 = head_loss.composite_task_loss(dict(pd, hm=x), target, anno, ind, torch.zeros_like(mask), cat, WEIGHT, CODE_WEIGHTS)
    assert abs(float(out0["hm_loss"]) + neg) < 1e-12 and float(out0["loc_loss"]) == 0.0
    # CPU tensors take the composite through the public entry too
    ex = dict(hm=[target], anno_box=[anno], ind=[ind], mask=[mask], cat=[cat])
    assert float(head_loss.center_loss([dict(pd, hm=x)], ex, WEIGHT, CODE_WEIGHTS)[0]["loss"]) == float(out["loss"])


def test_head_loss_refusals_without_a_device():
    from tests import head_helpers as HH
    from shasta_amd import builder
    head = builder.build_head(dict(type="CenterHead", in_channels=[8], tasks=HH.TWO_TASKS, dataset="waymo", code_weights=CODE_WEIGHTS))
    with pytest.raises(NotImplementedError):
        head.loss({}, [{}, {}])
    head = builder.build_head(dict(type="CenterHead", in_channels=[8], tasks=HH.TWO_TASKS, code_weights=CODE_WEIGHTS))
    with pytest.raises(NotImplementedError, match="targets"):
        head.loss(dict(metadata=[]), [{}, {}])
    with pytest.raises(ValueError):
        head.loss({}, [{}])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _dev():
    return torch.device("cuda")


_CASE = {}


def _case():
    """B = 2 on the 24 x 20 map of the target tests: targets from assign_targets (task 0 has no positive: the -neg branch; task 1 holds two
    slots on one pixel and class), logits random in [-6, 6] with +-12 and +-30 planted on four background pixels and on four positive
    pixels of every task that has them.  Computed once and left unchanged."""
    if _CASE:
        return _CASE
    from shasta_amd import targets
    dev = _dev()
    cfg = H.GEOM_A
    special, first8 = H.special_sample(cfg), (H.special_sample(cfg)[0][:8], H.special_sample(cfg)[1][:8])
    boxes = [torch.from_numpy(b).to(dev) for b, _ in (special, first8)]
    ex = targets.assign_targets(boxes, [special[1], first8[1]], H.TASKS, dict(cfg, gt_boxes_and_cls=False))
    g = torch.Generator().manual_seed(5)
    preds = []
    for t, nc in enumerate(H.TASKS):
        pd = dict(hm=(torch.rand(2, nc, H.MAP_H, H.MAP_W, generator=g) * 12 - 6))
        for n, w in WIDTH.items():
            pd[n] = torch.randn(2, w, H.MAP_H, H.MAP_W, generator=g)
        planted = [(0, 0, 3, 3), (1, nc - 1, 17, 2), (0, nc - 1, 5, 20), (1, 0, 11, 11)]
        mask, ind, cat = ex["mask"][t].cpu(), ex["ind"][t].cpu(), ex["cat"][t].cpu()
        pos = [(b, int(cat[b, k]), int(ind[b, k]) // H.MAP_W, int(ind[b, k]) % H.MAP_W) for b in range(2) for k in range(H.MAX_OBJS) if mask[b, k]]
        for where in (planted, pos[2:6]):  # (slots 0 and 1 of task 1 share a pixel and keep their random logit)
            for (b, c, y, x), v in zip(where, (12.0, -12.0, 30.0, -30.0)):
                pd["hm"][b, c, y, x] = v
        pd["_planted"] = planted + pos[2:6]
        preds.append(pd)
    assert int(ex["mask"][0].sum()) == 0 and int(ex["mask"][1].sum()) > 4 and int(ex["ind"][1][0, 0]) == int(ex["ind"][1][0, 1])
    _CASE.update(example=ex, preds=preds)
    return _CASE


def _composite(dtype, device):
    """The torch composite with autograd at `dtype` on `device`: (per-task results, per-task gradients of the task's loss)."""
    from shasta_amd import head_loss
    c = _case()
    ex = {k: [v.to(device) for v in c["example"][k]] for k in ("hm", "anno_box", "ind", "mask", "cat")}
    pds = [{n: pd[n].detach().clone().to(device, dtype).requires_grad_(True) for n in HEADS} for pd in c["preds"]]
    outs = head_loss.center_loss(pds, ex, WEIGHT, CODE_WEIGHTS, force_composite=True)
    grads = []
    for pd, o in zip(pds, outs):
        gs = torch.autograd.grad(o["loss"], [pd[n] for n in HEADS], allow_unused=True)
        grads.append({n: (torch.zeros_like(pd[n]) if g is None else g).double().cpu() for n, g in zip(HEADS, gs)})
    return outs, grads


def _kernel(scale=1.0):
    from shasta_amd import head_loss
    c = _case()
    dev = _dev()
    pds = [{n: pd[n].detach().clone().to(dev).requires_grad_(True) for n in HEADS} for pd in c["preds"]]
    outs = head_loss.center_loss(pds, c["example"], WEIGHT, CODE_WEIGHTS)
    assert all(o["loss"].requires_grad and not o["hm_loss"].requires_grad for o in outs)
    (sum(o["loss"] for o in outs) * scale).backward()
    return outs, [{n: pd[n].grad.cpu() for n in HEADS} for pd in pds]


def _sum_abs_terms():
    """float64 sum |term| of every loss value, for the floors."""
    c = _case()
    floors = []
    for t, pd in enumerate(c["preds"]):
        p = torch.clamp(torch.sigmoid(pd["hm"].double()), 1e-4, 1 - 1e-4)
        thm = c["example"]["hm"][t].cpu().double()
        m, ind, cat = c["example"]["mask"][t].cpu().double(), c["example"]["ind"][t].cpu(), c["example"]["cat"][t].cpu()
        neg = (torch.log(1 - p) * p ** 2 * (1 - thm) ** 4).abs().sum()
        q = torch.stack([p[b, cat[b], ind[b] // H.MAP_W, ind[b] % H.MAP_W] for b in range(2)])
        pos = ((torch.log(q) * (1 - q) ** 2).abs() * m).sum()
        npos = float(m.sum())
        floors.append(float((pos + neg) / max(npos, 1.0)))
    return floors


@pytest.mark.gpu
def test_loss_values_against_float64():
    o64, _ = _composite(torch.float64, "cpu")
    o32, _ = _composite(torch.float32, "cpu")
    ok, _ = _kernel()
    hm_abs = _sum_abs_terms()
    worst = 0.0
    for t in range(len(H.TASKS)):
        assert float(ok[t]["num_positive"]) == float(o64[t]["num_positive"])
        elem64 = o64[t]["loc_loss_elem"]
        loc_abs = float((elem64.detach() * torch.tensor(CODE_WEIGHTS, dtype=torch.float64)).sum())
        figures = [("hm_loss", ok[t]["hm_loss"], o32[t]["hm_loss"], o64[t]["hm_loss"], hm_abs[t]),
                   ("loss", ok[t]["loss"], o32[t]["loss"], o64[t]["loss"], hm_abs[t] + WEIGHT * loc_abs),
                   ("loc_loss", ok[t]["loc_loss"], o32[t]["loc_loss"], o64[t]["loc_loss"], loc_abs)]
        figures += [("loc_loss_elem[%d]" % c, ok[t]["loc_loss_elem"][c], o32[t]["loc_loss_elem"][c], elem64[c], float(elem64[c])) for c in range(10)]
        for name, got, own, want, terms in figures:
            err, bar = abs(float(got) - float(want)), max(4 * abs(float(own) - float(want)), 16 * U * terms)
            print("task %d %-17s %.9g  error %.3g  torch fp32 %.3g  bar %.3g" % (t, name, float(got), err, abs(float(own) - float(want)), bar))
            assert err <= bar, (t, name)
            worst = max(worst, err / bar) if bar > 0 else worst
    print("loss values: largest error / bar %.3f" % worst)
    assert float(o64[0]["num_positive"]) == 0 and float(ok[0]["loc_loss"]) == 0.0  # the -neg branch


@pytest.mark.gpu
def test_gradient_entries_against_float64_autograd():
    _, g64 = _composite(torch.float64, "cpu")
    _, g32 = _composite(torch.float32, "cpu")
    _, gk = _kernel()
    _, again = _kernel()
    _, tripled = _kernel(3.0)
    c = _case()
    worst = 0.0
    for t in range(len(H.TASKS)):
        for n in HEADS:
            want, own, got = g64[t][n], g32[t][n], gk[t][n].double()
            assert torch.equal(gk[t][n], again[t][n]), "two runs, the same bits"
            assert torch.equal(tripled[t][n], gk[t][n] * 3.0), "linear in grad_output"
            nz = want != 0
            R = float(((own - want).abs()[nz] / want.abs()[nz]).max()) if nz.any() else 0.0
            bar = torch.maximum(4 * R * want.abs(), 16 * U * want.abs() + U * want.abs().max())
            err = (got - want).abs()
            ratio = float((err / bar.clamp_min(1e-300)).max()) if float(want.abs().max()) > 0 else 0.0
            print("task %d %-6s torch fp32 largest relative error %.3g, largest error / bar %.3g" % (t, n, R, ratio))
            assert (err <= bar).all(), (t, n)
            worst = max(worst, ratio)
        for b, cc, y, x in c["preds"][t]["_planted"]:  # the clamp is active: exactly zero
            assert float(gk[t]["hm"][b, cc, y, x]) == 0.0 and float(g64[t]["hm"][b, cc, y, x]) == 0.0
        m, ind = c["example"]["mask"][t].cpu().bool(), c["example"]["ind"][t].cpu()
        touched = torch.zeros(2, H.MAP_H * H.MAP_W, dtype=torch.bool)
        for b in range(2):
            touched[b, ind[b][m[b]]] = True
        for n in WIDTH:
            g = gk[t][n].reshape(2, -1, H.MAP_H * H.MAP_W)
            assert not g[~touched[:, None, :].expand_as(g)].any(), "box-head pixels no object points to"
    print("gradient: largest error / bar %.3f" % worst)


def _head(dtype=torch.float32):
    from shasta_amd import builder
    from tests.neck_helpers import randomize_bn
    torch.manual_seed(31)
    tasks = [dict(num_class=n, class_names=["c%d" % i for i in range(n)]) for n in H.TASKS]
    head = builder.build_head(dict(type="CenterHead", in_channels=[16], tasks=tasks, weight=WEIGHT, code_weights=CODE_WEIGHTS, share_conv_channel=32))
    randomize_bn(head, torch.Generator().manual_seed(32))
    return head


@pytest.mark.gpu
def test_center_head_loss_backward_through_forward_layers():
    """`CenterHead.loss` on `forward_layers` outputs in train() mode: parameter gradients against a float64 copy on the composite path, by
    the gradient rule, with the fp32 composite path of the same module as the yardstick."""
    import copy
    from shasta_amd import head_loss
    dev = _dev()
    ex = _case()["example"]
    x = torch.randn(2, 16, H.MAP_H, H.MAP_W, generator=torch.Generator().manual_seed(33))

    def run(head, xin, composite):
        head.train()
        head.zero_grad()
        preds = head(xin)
        if composite:
            outs = head_loss.center_loss(preds, ex, head.weight, head.code_weights, force_composite=True)
        else:
            outs = head.loss(ex, preds)
        sum(o["loss"] for o in outs).backward()
        return outs, {n: p.grad.double().cpu() for n, p in head.named_parameters()}

    base = _head()
    ok, gk = run(copy.deepcopy(base).to(dev), x.to(dev), False)
    _, g32 = run(copy.deepcopy(base).to(dev), x.to(dev), True)
    _, g64 = run(copy.deepcopy(base).double().to(dev), x.double().to(dev), True)
    assert sorted(ok[0]) == ["hm_loss", "loc_loss", "loc_loss_elem", "loss", "num_positive"] and ok[0]["loss"].is_cuda
    worst = 0.0
    largest = max(float(w.abs().max()) for w in g64.values())
    for n, want in g64.items():
        if float(want.abs().max()) <= 1e-9 * largest:
            # a convolution bias in front of a batch-statistics BatchNorm: the mean removes it, the true gradient is zero (float64 leaves
            # 1e-16 of the others) and a relative rule has nothing to hold on to.  What fp32 leaves there is the rounding noise of the
            # convolution backward, which both paths take from torch: the yardstick is the fp32 composite's own noise.
            assert float(gk[n].abs().max()) <= 4 * float(g32[n].abs().max()) + U * largest, n
            continue
        nz = want != 0
        R = float(((g32[n] - want).abs()[nz] / want.abs()[nz]).max()) if nz.any() else 0.0
        bar = torch.maximum(4 * R * want.abs(), 16 * U * want.abs() + U * want.abs().max())
        err = (gk[n] - want).abs()
        assert (err <= bar).all(), n
        if float(want.abs().max()) > 0:
            worst = max(worst, float((err / bar.clamp_min(1e-300)).max()))
    print("parameter gradients: largest error / bar %.3f" % worst)
    # eval(): the kernel-path forward's channel slices are served as they are
    head = copy.deepcopy(base).to(dev).eval()
    with torch.no_grad():
        a = head.loss(ex, head(x.to(dev)))
        b = head.loss(ex, head.forward_layers(x.to(dev)))
    for t in range(len(H.TASKS)):
        assert abs(float(a[t]["loss"]) - float(b[t]["loss"])) <= 1e-4 * abs(float(b[t]["loss"]))


@pytest.mark.gpu
def test_voxelnet_forward_return_loss():
    import shasta_amd
    from shasta_amd import targets
    from shasta_amd.backbone import SpMiddleResNetFHD
    from shasta_amd.voxel_generator import VoxelGenerator
    from tests import head_helpers as HH
    dev = _dev()
    torch.manual_seed(71)
    m = shasta_amd.build_detector(dict(
        type="VoxelNet", reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5),
        backbone=dict(type=SpMiddleResNetFHD, num_input_features=5, ds_factor=8),
        neck=dict(type="RPN", layer_nums=[1, 1], ds_layer_strides=[1, 2], ds_num_filters=[32, 64], us_layer_strides=[1, 2], us_num_filters=[32, 32],
                  num_input_features=256),
        bbox_head=dict(type="CenterHead", in_channels=[64], tasks=HH.TWO_TASKS, weight=WEIGHT, code_weights=CODE_WEIGHTS)), test_cfg=None).eval().to(dev)
    g = torch.Generator().manual_seed(75)
    clouds = []
    for _ in range(2):
        centres = (torch.rand(6, 3, generator=g) - 0.5) * torch.tensor([22.0, 22.0, 5.0]) + torch.tensor([0.0, 0.0, -1.0])
        pts = centres.repeat_interleave(150, 0) + torch.randn(900, 3, generator=g) * torch.tensor([1.0, 1.0, 0.5])
        clouds.append(torch.cat([pts, torch.rand(900, 2, generator=g)], 1).to(dev))
    vg = VoxelGenerator([0.5625, 0.5625, 0.2], [-13.5, -13.5, -5, 13.5, 13.5, 3], 10, max_voxels=4000)
    voxels, coors, num, _, nv = vg.generate_batch_device(clouds)
    nv = nv.cpu().tolist()
    vs = torch.cat([voxels[b, :nv[b]] for b in range(2)])
    ns = torch.cat([num[b, :nv[b]] for b in range(2)])
    cs = torch.cat([torch.cat([torch.full((nv[b], 1), b, dtype=torch.int32, device=dev), coors[b, :nv[b]]], 1) for b in range(2)])
    example = dict(voxels=vs, num_points=ns, coordinates=cs, points=[None] * 2, shape=[vg.grid_size.tolist()], metadata=[dict(token="a"), dict(token="b")])
    boxes = [torch.tensor([H._box(-6.0, 3.0, 2.0, 4.5, 0.3), H._box(8.2, -7.1, 2.8, 9.0, -1.0), H._box(1.0, 1.0, 2.5, 7.0, 2.0)], device=dev),
             torch.tensor([H._box(4.0, -2.0, 2.0, 4.4, 1.3)], device=dev)]
    tcfg = dict(pc_range=[-13.5, -13.5, -5.0, 13.5, 13.5, 3.0], voxel_size=[0.5625, 0.5625, 0.2], out_size_factor=8, gaussian_overlap=0.1, max_objs=8,
                min_radius=2)
    example.update({k: v for k, v in targets.assign_targets(boxes, [np.array([1, 3, 2]), np.array([2])], HH.TWO_TASKS, tcfg).items()
                    if k in ("hm", "anno_box", "ind", "mask", "cat", "gt_boxes_and_cls")})
    with torch.no_grad():
        losses = m(example, return_loss=True)
    assert isinstance(losses, list) and len(losses) == 2
    for o, npos in zip(losses, (1.0, 3.0)):
        assert sorted(o) == ["hm_loss", "loc_loss", "loc_loss_elem", "loss", "num_positive"]
        assert all(v.is_cuda for v in o.values()) and o["loc_loss_elem"].shape == (10,) and float(o["num_positive"]) == npos
        assert np.isfinite(float(o["loss"])) and float(o["hm_loss"]) > 0
