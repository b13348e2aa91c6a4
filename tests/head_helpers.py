"""Shared by tests/test_head_kernels.py (GPU), tests/test_head_module.py and tests/test_detections.py: float64 oracles of the CenterPoint
head (torch's CPU float64 nn functions), the error bars, and the synthetic inputs.

Bars (u = 2^-24; gamma_n <= n u / (1 - n u) of an n-term fmaf chain, any summation order; each entry on its own):
  final convs               |y - y64| <= (9 * 64 + 8) u (sum|w||x| + |b|)
  bias + BN + ReLU layers   |y - y64| <= (9 Cin + 16) u (|A| (sum|w||x| + |b| + |mean|) + |beta|),  A = gamma / sqrt(var + eps) in float64
  decode x, y               6 u E, E = |pc_range| + W out_size_factor voxel_size (four fp32 roundings of quantities <= E + the fp32 images
                            of the constants); z and vel bit-equal
  decode score, dim, rot    `transcendental_bars`: 4 x the largest error of torch's CPU fp32 sigmoid / exp / atan2 on the same inputs, in
                            ulps (fp32 spacing at the float64 value; rot modulo 2 pi), at least 4 ulp - the device library is another
                            implementation.  Measured on the decode tests' inputs (9 x 130 maps, two classes): torch CPU at most 1.78 / 0.55 /
                            1.10 ulp for score / dim / rot, so the device bars are 5.5 .. 7.5 / 4 / 4 .. 4.4 ulp by input; the device's own
                            largest errors there (MI355X, printed by the tests): 1.38 / 0.74 / 1.89 ulp."""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
NUSC_TASKS = [dict(num_class=1, class_names=["car"]), dict(num_class=2, class_names=["truck", "construction_vehicle"]),
              dict(num_class=2, class_names=["bus", "trailer"]), dict(num_class=1, class_names=["barrier"]),
              dict(num_class=2, class_names=["motorcycle", "bicycle"]), dict(num_class=2, class_names=["pedestrian", "traffic_cone"])]
TWO_TASKS = [dict(num_class=1, class_names=["car"]), dict(num_class=2, class_names=["bus", "trailer"])]
TEST_CFG = dict(post_center_limit_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], max_per_img=500,
                nms=dict(use_rotate_nms=True, use_multi_class_nms=False, nms_pre_max_size=1000, nms_post_max_size=83, nms_iou_threshold=0.2),
                score_threshold=0.1, pc_range=[-54, -54], out_size_factor=8, voxel_size=[0.075, 0.075])


def make_head(in_channels, tasks, seed):
    """A CenterHead in eval mode with non-trivial BatchNorm tensors and convolution biases from a seeded generator."""
    from shasta_amd import builder
    torch.manual_seed(seed)
    head = builder.build_head(dict(type="CenterHead", in_channels=[in_channels], tasks=tasks, share_conv_channel=64))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in head.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                n = mod.num_features
                mod.weight.copy_(0.5 + torch.rand(n, generator=g))
                mod.bias.copy_(0.2 * torch.randn(n, generator=g))
                mod.running_mean.copy_(0.3 * torch.randn(n, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(n, generator=g))
            elif isinstance(mod, torch.nn.Conv2d):
                mod.bias.add_(0.3 * torch.randn(mod.out_channels, generator=g))
    return head.eval()


def head_layers(head):
    """(shared (conv, bn), per task [(name, conv0, bn, conv3)])."""
    return (head.shared_conv[0], head.shared_conv[1]), [[(n, getattr(t, n)[0], getattr(t, n)[1], getattr(t, n)[3]) for n in t.heads] for t in head.tasks]


def bn_layer_ref(conv, bn, x):
    """float64 Conv2d(3, padding 1, bias) -> eval BatchNorm2d -> ReLU of the fp32 input x, and the per-entry bar."""
    w, b = conv.weight.detach().double(), conv.bias.detach().double()
    g, beta, mean, var = (t.detach().double() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
    x = x.detach().cpu().double()
    y = F.relu(F.batch_norm(F.conv2d(x, w, b, padding=1), mean, var, g, beta, training=False, eps=bn.eps))
    A = (g / torch.sqrt(var + bn.eps)).abs()
    s = F.conv2d(x.abs(), w.abs(), padding=1)
    v = lambda t: t.abs()[None, :, None, None]
    bar = (9 * conv.in_channels + 16) * U * (v(A) * (s + v(b) + v(mean)) + v(beta))
    return y, bar


def final_ref(conv, x):
    """float64 Conv2d(3, padding 1, bias) of the fp32 input x (64 channels), and the per-entry bar."""
    w, b = conv.weight.detach().double(), conv.bias.detach().double()
    x = x.detach().cpu().double()
    y = F.conv2d(x, w, b, padding=1)
    bar = (9 * 64 + 8) * U * (F.conv2d(x.abs(), w.abs(), padding=1) + b.abs()[None, :, None, None])
    return y, bar


def assert_inside(got, ref, bar, what):
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), what + ": an entry was not written (NaN poison) or is not finite"
    err = (got - ref).abs()
    worst = float((err / bar.clamp_min(1e-300)).max())
    print("%s: max err %.3e, largest err / bar %.3f" % (what, float(err.max()), worst))
    assert bool((err <= bar).all()), "%s: %d entries outside the bar, worst err / bar %.3f" % (what, int((err > bar).sum()), worst)


def check_chain(head, x, run_bn_layer, run_final):
    """Every layer of the head against float64 ON ITS OWN fp32 INPUT (the previous stage's fp32 output as the implementation under test
    produced it).  run_bn_layer(convs, bns, x) -> fp32 (B, sum Cout, H, W); run_final(convs, x (B, 64 heads, H, W)) -> fp32 (B, C_task, H, W).
    Returns the tasks' raw tensors."""
    (sc, sbn), tasks = head_layers(head)
    s = run_bn_layer([sc], [sbn], x)
    assert_inside(s, *bn_layer_ref(sc, sbn, x), "shared_conv")
    raws = []
    for t, heads in enumerate(tasks):
        f = run_bn_layer([h[1] for h in heads], [h[2] for h in heads], s)
        raw = run_final([h[3] for h in heads], f)
        at = 0
        for i, (name, c0, bn, c3) in enumerate(heads):
            assert_inside(f[:, 64 * i:64 * i + 64], *bn_layer_ref(c0, bn, s), "task %d %s.0-2" % (t, name))
            k = c3.out_channels
            assert_inside(raw[:, at:at + k], *final_ref(c3, f[:, 64 * i:64 * i + 64]), "task %d %s.3" % (t, name))
            at += k
        assert at == raw.shape[1]
        raws.append(raw)
    return raws


def torch_bn_layer(convs, bns, x):
    """torch's own fp32 layers on the CPU."""
    with torch.no_grad():
        return torch.cat([F.relu(bn(c(x.cpu()))) for c, bn in zip(convs, bns)], 1)


def torch_final(convs, x):
    with torch.no_grad():
        return torch.cat([c(x.cpu()[:, 64 * i:64 * i + 64]) for i, c in enumerate(convs)], 1)


# ---- decode ---------------------------------------------------------------------------------------------------------

def channel_offsets(num_class):
    return dict(reg=0, height=2, dim=3, rot=6, vel=8, hm=10, num_class=num_class)


def decode_cfg(num_class, test_cfg):
    from shasta_amd import hip
    import ctypes
    c = hip.HeadDecodeCfg()
    for k, v in channel_offsets(num_class).items():
        setattr(c, k, v)
    c.out_size_factor, c.voxel_x, c.voxel_y = float(test_cfg["out_size_factor"]), float(test_cfg["voxel_size"][0]), float(test_cfg["voxel_size"][1])
    c.pc_x, c.pc_y, c.score_threshold = float(test_cfg["pc_range"][0]), float(test_cfg["pc_range"][1]), float(test_cfg["score_threshold"])
    c.range = (ctypes.c_float * 6)(*[float(v) for v in test_cfg["post_center_limit_range"]])
    return c


def decode_oracle(raw, num_class, test_cfg):
    """float64 decode of ONE image's fp32 raw maps (C, H, W) -> dict(pixel (n,) ascending, box (n, 9), score, label, all_score (HW,),
    margin_score, margin_range): the smallest distance of a score to the threshold and of a centre to a range limit over ALL pixels."""
    C, H, W = raw.shape
    r = raw.detach().cpu().double().reshape(C, H * W)
    o = channel_offsets(num_class)
    sc = torch.sigmoid(r[o["hm"]:o["hm"] + num_class])
    score = sc.max(0)[0]
    label = torch.zeros(H * W, dtype=torch.int64)
    for k in reversed(range(num_class)):  # the FIRST class holding the maximum
        label[sc[k] == score] = k
    p = torch.arange(H * W)
    ix, iy = (p % W).double(), (p // W).double()
    f = float(test_cfg["out_size_factor"])
    x = (ix + r[o["reg"]]) * f * float(test_cfg["voxel_size"][0]) + float(test_cfg["pc_range"][0])
    y = (iy + r[o["reg"] + 1]) * f * float(test_cfg["voxel_size"][1]) + float(test_cfg["pc_range"][1])
    z = r[o["height"]]
    dim = torch.exp(r[o["dim"]:o["dim"] + 3])
    rot = torch.atan2(r[o["rot"]], r[o["rot"] + 1])
    box = torch.stack([x, y, z, dim[0], dim[1], dim[2], r[o["vel"]], r[o["vel"] + 1], rot], 1)
    lim = torch.tensor([float(v) for v in test_cfg["post_center_limit_range"]], dtype=torch.float64)
    xyz = box[:, :3]
    thr = float(test_cfg["score_threshold"])
    keep = (score > thr) & (xyz >= lim[:3]).all(1) & (xyz <= lim[3:]).all(1)
    m_range = float(torch.minimum((xyz - lim[:3]).abs(), (xyz - lim[3:]).abs()).min())
    return dict(pixel=p[keep], box=box[keep], score=score[keep], label=label[keep], all_score=score, margin_score=float((score - thr).abs().min()),
                margin_range=m_range)


def ulps(got32, ref64, modulo=None):
    """|got - ref| in fp32 spacings at the float64 value (rot: modulo 2 pi)."""
    d = got32.detach().cpu().double() - ref64
    if modulo is not None:
        d = torch.remainder(d + modulo / 2, modulo) - modulo / 2
    a = ref64.abs().clamp_min(2.0 ** -126)
    spacing = torch.pow(2.0, torch.floor(torch.log2(a)) - 23)
    return d.abs() / spacing


def transcendental_bars(raw, num_class):
    """Largest error of torch's CPU fp32 sigmoid / exp / atan2 against float64 on these inputs, in ulps -> (measured, device bars =
    max(4 x measured, 4)), each a dict over score / dim / rot."""
    r = raw.detach().cpu().float()
    r = r.reshape(-1, r.shape[-3], r.shape[-2] * r.shape[-1]) if r.dim() == 4 else r.reshape(1, r.shape[0], -1)
    o = channel_offsets(num_class)
    hm, dim, r0, r1 = r[:, o["hm"]:o["hm"] + num_class], r[:, o["dim"]:o["dim"] + 3], r[:, o["rot"]], r[:, o["rot"] + 1]
    measured = dict(score=float(ulps(torch.sigmoid(hm), torch.sigmoid(hm.double())).max()),
                    dim=float(ulps(torch.exp(dim), torch.exp(dim.double())).max()),
                    rot=float(ulps(torch.atan2(r0, r1), torch.atan2(r0.double(), r1.double()), modulo=2 * math.pi).max()))
    return measured, {k: max(4.0 * v, 4.0) for k, v in measured.items()}


DECODE_CFG = dict(TEST_CFG, pc_range=[-39.0, -2.7], post_center_limit_range=[-37.0, -2.0, -5.0, 37.0, 2.0, 3.0])   # a 9 x 130 map of 0.6 m pixels
DECODE_CFG_ALL = dict(DECODE_CFG, post_center_limit_range=[-100.0, -100.0, -10.0, 100.0, 100.0, 10.0])          # every pixel inside


def decode_input(count, H, W, num_class, seed, test_cfg):
    """One image's raw maps (C, H, W) fp32 with exactly `count` candidates: `count` hot pixels well inside the limits, a few hot pixels
    outside them (border columns / rows, or a height out of range), every other pixel cold.  Re-drawn (seed + 1000 k) until no score lies
    within 1e-4 of the threshold and no centre within 1e-3 m of a limit; the caller asserts both on the oracle."""
    npix, C = H * W, 10 + num_class
    for k in range(50):
        g = torch.Generator().manual_seed(seed + 1000 * k)
        raw = torch.randn(C, npix, generator=g)
        raw[0:2] = torch.rand(2, npix, generator=g)                        # reg in [0, 1)
        raw[2] = -1.0 + 0.5 * torch.randn(npix, generator=g)                # height
        raw[3:6] = 0.5 * torch.randn(3, npix, generator=g)                  # log dim
        raw[10:] = -5.0 + 0.4 * torch.randn(num_class, npix, generator=g)   # cold: score < 0.03
        o = decode_oracle(raw.reshape(C, H, W), num_class, dict(test_cfg, score_threshold=-1.0))  # (which pixels lie inside the limits)
        inside = torch.zeros(npix, dtype=torch.bool)
        inside[o["pixel"]] = True
        ins, outs = torch.nonzero(inside)[:, 0], torch.nonzero(~inside)[:, 0]
        if count > len(ins):
            raise AssertionError("decode_input: %d candidates asked, %d pixels inside the limits" % (count, len(ins)))
        hot = ins[torch.randperm(len(ins), generator=g)[:count]]
        hot_out = outs[torch.randperm(len(outs), generator=g)[:7]]
        for idx in (hot, hot_out):
            raw[10:, idx] = 0.5 + 2.5 * torch.rand(num_class, len(idx), generator=g)
        if count < len(ins) and count > 0:  # a hot pixel inside in x, y whose height leaves the range: not a candidate
            spare = ins[~torch.isin(ins, hot)][:3]
            raw[10:, spare] = 2.0
            raw[2, spare] = 50.0
        raw = raw.reshape(C, H, W).contiguous()
        o = decode_oracle(raw, num_class, test_cfg)
        if o["margin_score"] > 1e-4 and o["margin_range"] > 1e-3:
            assert len(o["pixel"]) == count, (len(o["pixel"]), count)
            return raw, o
    raise AssertionError("decode_input: no draw with the margins")


# ---- predict: planted objects --------------------------------------------------------------------------------------

PLANT_STEP = 6  # lattice pitch in pixels: clusters are further apart than two half diagonals


def planted_maps(peaks, num_class, H, W, seed, duplicates=True, tie=False):
    """One image's raw maps (C, H, W) with `peaks` clusters on a lattice: a main peak and - for every third cluster - a second, weaker peak
    on the neighbouring pixel with nearly the same box (IoU ~ 0.4 - 0.8: suppressed).  Clusters do not touch each other (IoU 0).
    tie: the first two clusters get the same heat-map logit (equal scores; the lower pixel must come first)."""
    C = 10 + num_class
    g = torch.Generator().manual_seed(seed)
    raw = torch.zeros(C, H, W)
    raw[10:] = -5.0 + 0.3 * torch.randn(num_class, H, W, generator=g)
    raw[0:2] = 0.4 + 0.2 * torch.rand(2, H, W, generator=g)
    raw[2] = -1.0 + 0.3 * torch.randn(H, W, generator=g)
    raw[3:6] = torch.log(torch.tensor(1.6)) + math.log(1.5) * torch.rand(3, H, W, generator=g)  # sizes 1.6 .. 2.4
    raw[6:10] = torch.randn(4, H, W, generator=g)
    cells = [(iy, ix) for iy in range(2, H - 2, PLANT_STEP) for ix in range(2, W - 2, PLANT_STEP)]
    assert peaks <= len(cells), (peaks, len(cells))
    pick = torch.randperm(len(cells), generator=g)[:peaks].tolist()
    for n, ci in enumerate(pick):
        iy, ix = cells[ci]
        cls = int(torch.randint(num_class, (1,), generator=g))
        logit = 0.2 + 3.0 * float(torch.rand(1, generator=g))
        if tie and n < 2:
            logit = 1.25
        raw[10 + cls, iy, ix] = logit
        if duplicates and n % 3 == 2:
            raw[:10, iy, ix + 1] = raw[:10, iy, ix]
            raw[0:2, iy, ix + 1] = 0.4 + 0.2 * torch.rand(2, generator=g)
            raw[10 + cls, iy, ix + 1] = logit - 1.0 - float(torch.rand(1, generator=g))  # weaker: sigmoid(-0.8 - 1) > 0.1 still
    return raw


def iou_near(boxes7):
    """nms_oracle's IoU matrix, pairs further apart than both half diagonals left at 0 (they cannot touch)."""
    from oracle import nms_oracle as O
    n = len(boxes7)
    m = np.zeros((n, n))
    r = 0.5 * np.hypot(boxes7[:, 3], boxes7[:, 4])
    for i in range(n):
        d = np.hypot(boxes7[i + 1:, 0] - boxes7[i, 0], boxes7[i + 1:, 1] - boxes7[i, 1])
        for j in np.nonzero(d <= r[i] + r[i + 1:])[0] + i + 1:
            m[i, j] = m[j, i] = O.iou_bev(boxes7[i], boxes7[j])
    return m


def predict_oracle(raws, num_classes, test_cfg):
    """The oracle chain for one sample: per task the float64 decode, a stable sort by descending score cut to nms_pre_max_size,
    nms_oracle on the converted boxes, the cut to nms_post_max_size; tasks concatenated.  raws: per task (C, H, W) fp32.
    -> dict(box (n, 9) float64, score, label (offset by the earlier tasks' classes), iou_margin: the smallest distance of a pair's IoU
    (pairs inside the pre-NMS cut) to the threshold, score_gap: the smallest gap between two consecutive sorted scores of a task)."""
    from oracle import nms_oracle as O
    nms = test_cfg["nms"]
    thr = float(nms["nms_iou_threshold"])
    boxes, scores, labels, margin, gap = [], [], [], float("inf"), float("inf")
    for t, raw in enumerate(raws):
        d = decode_oracle(raw, num_classes[t], test_cfg)
        order = np.argsort(-d["score"].numpy(), kind="stable")[:int(nms["nms_pre_max_size"])]
        b, s, l = d["box"].numpy()[order], d["score"].numpy()[order], d["label"].numpy()[order]
        if len(s) > 1:
            gap = min(gap, float(np.min(s[:-1] - s[1:])))
        b7 = b[:, [0, 1, 2, 4, 3, 5, 8]].copy()
        b7[:, 6] = -b7[:, 6] - np.pi / 2
        iou = iou_near(b7)
        if len(b7) > 1:
            margin = min(margin, float(np.abs(iou[np.triu_indices(len(b7), 1)] - thr).min()))
        keep, _ = O.nms_sorted(b7, thr, iou)
        keep = np.asarray(keep, dtype=np.int64)[:int(nms["nms_post_max_size"])]
        boxes.append(b[keep].reshape(-1, 9)), scores.append(s[keep]), labels.append(l[keep] + sum(num_classes[:t]))
    return dict(box=np.concatenate(boxes), score=np.concatenate(scores), label=np.concatenate(labels), iou_margin=margin, score_gap=gap)


def xy_bar(W, H, test_cfg):
    f = float(test_cfg["out_size_factor"])
    ex = abs(float(test_cfg["pc_range"][0])) + W * f * float(test_cfg["voxel_size"][0])
    ey = abs(float(test_cfg["pc_range"][1])) + H * f * float(test_cfg["voxel_size"][1])
    return 6 * U * ex, 6 * U * ey


def assert_boxes(got_box, got_score, ref_box, ref_score, bars, W, H, test_cfg, what):
    """Decoded rows against the float64 rows: z, vel bit-equal (they identify the pixel), x / y within 6 u E, dim / rot / score in ulps."""
    got = got_box.detach().cpu()
    ref = torch.as_tensor(ref_box, dtype=torch.float64).reshape(-1, 9)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if len(ref) == 0:
        return
    assert torch.equal(got[:, [2, 6, 7]].double(), ref[:, [2, 6, 7]]), what + ": z / vel are not the oracle's (another pixel, or not passed through)"
    bx, by = xy_bar(W, H, test_cfg)
    ex, ey = float((got[:, 0].double() - ref[:, 0]).abs().max()), float((got[:, 1].double() - ref[:, 1]).abs().max())
    e_dim = float(ulps(got[:, 3:6], ref[:, 3:6]).max())
    e_rot = float(ulps(got[:, 8], ref[:, 8], modulo=2 * math.pi).max())
    e_score = float(ulps(got_score, torch.as_tensor(ref_score, dtype=torch.float64)).max())
    print("%s: x err %.3e (bar %.3e), y err %.3e (bar %.3e), dim %.2f ulp, rot %.2f ulp, score %.2f ulp (bars %s)" % (what, ex, bx, ey, by, e_dim, e_rot, e_score, bars))
    assert ex <= bx and ey <= by, what
    assert e_dim <= bars["dim"] and e_rot <= bars["rot"] and e_score <= bars["score"], what
