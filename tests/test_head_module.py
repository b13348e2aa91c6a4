"""`CenterHead` and `VoxelNet`: registry, state_dict layout, the kernel-path forward against float64, `predict` against the oracle chain
(float64 decode, stable sort, oracle/nms_oracle.py), and the detector from voxels to detections.  CPU tests are unmarked."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import head_helpers as HH


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda", 0)


# ---- CPU ----------------------------------------------------------------------------------------------------------------

def test_registries_and_builders():
    import shasta_amd
    from shasta_amd import builder, registry
    assert registry.HEADS.get("CenterHead") is shasta_amd.CenterHead and registry.DETECTORS.get("VoxelNet") is shasta_amd.VoxelNet
    assert builder.build_head(None) is None and builder.build_detector(None) is None
    head = builder.build_head(dict(type="CenterHead", in_channels=sum([256, 256]), tasks=HH.NUSC_TASKS, dataset="nuscenes", weight=0.25,
                                   code_weights=[1.0] * 10, common_heads={"reg": (2, 2), "height": (1, 2), "dim": (3, 2), "rot": (2, 2), "vel": (2, 2)},
                                   share_conv_channel=64, dcn_head=False))
    assert head.in_channels == 512 and head.num_classes == [1, 2, 2, 1, 2, 2] and head.code_weights == [1.0] * 10
    assert [n for n, _ in head.named_children()] == ["shared_conv", "tasks"]
    assert list(head.tasks[1].heads) == ["reg", "height", "dim", "rot", "vel", "hm"]
    with pytest.raises(NotImplementedError):
        builder.build_head(dict(type="CenterHead", in_channels=[8], tasks=HH.TWO_TASKS, dcn_head=True))
    with pytest.raises(KeyError):
        builder.build_head(dict(type="NoSuchHead"))
    default = builder.build_head(dict(type="CenterHead", in_channels=[8], tasks=HH.TWO_TASKS))
    assert list(default.common_heads.items()) == [("reg", (2, 2)), ("height", (1, 2)), ("dim", (3, 2)), ("rot", (2, 2)), ("vel", (2, 2))]


def test_state_dict_keys_and_permissive_round_trip():
    from shasta_amd.shasta import load_state_dict_permissive
    head = HH.make_head(8, HH.TWO_TASKS, 3)
    keys = list(head.state_dict().keys())
    want = ["shared_conv.0.weight", "shared_conv.0.bias"] + ["shared_conv.1." + n for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    for t in range(2):
        for name in ("reg", "height", "dim", "rot", "vel", "hm"):
            p = "tasks.%d.%s." % (t, name)
            want += [p + "0.weight", p + "0.bias"] + [p + "1." + n for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
            want += [p + "3.weight", p + "3.bias"]
    assert keys == want
    sd = head.state_dict()
    assert sd["tasks.1.hm.3.weight"].shape == (2, 64, 3, 3) and sd["tasks.0.hm.3.bias"].shape == (1,) and sd["tasks.0.dim.3.weight"].shape == (3, 64, 3, 3)
    fresh = HH.make_head(8, HH.TWO_TASKS, 4)
    assert float(fresh.tasks[0].hm[3].bias.detach().abs().sum()) > 0

    class Det(torch.nn.Module):  # a detector's key layout: bbox_head.*
        def __init__(self, h):
            super().__init__()
            self.bbox_head = h

    det = Det(fresh)
    skipped, missing = load_state_dict_permissive(det, dict({"bbox_head." + k: v.clone() for k, v in sd.items()}, **{"bbox_head.nothing": torch.zeros(1)}))
    assert [s[0] for s in skipped] == ["bbox_head.nothing"] and missing == []
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), sd.values()))
    # hm's last bias starts at init_bias; nothing else is claimed about the initial values
    from shasta_amd import builder
    raw = builder.build_head(dict(type="CenterHead", in_channels=[8], tasks=HH.TWO_TASKS, init_bias=-2.19))
    assert bool((raw.tasks[1].hm[3].bias == -2.19).all()) and bool((raw.tasks[1].reg[3].bias == 0).all()) and bool((raw.shared_conv[0].bias == 0).all())


def test_torch_fp32_layers_stay_inside_the_bars():
    """torch's own fp32 layers on the CPU against float64, on the kernel tests' inputs, at the kernel tests' bars."""
    for in_channels, B, H, W in ((8, 1, 3, 5), (24, 3, 5, 33), (24, 1, 9, 130), (512, 1, 9, 130)):
        seed = 32 if in_channels == 512 else 100 * H + W + B + in_channels
        head = HH.make_head(in_channels, HH.TWO_TASKS, seed)
        x = torch.relu(torch.randn(B, in_channels, H, W, generator=torch.Generator().manual_seed(seed + 7)))
        raws = HH.check_chain(head, x, HH.torch_bn_layer, HH.torch_final)
        with torch.no_grad():
            nn_out = head(x)  # the CPU forward is forward_layers
        for raw, d in zip(raws, nn_out):
            assert list(d) == ["reg", "height", "dim", "rot", "vel", "hm"]
            np.testing.assert_allclose(torch.cat([d[n] for n in d], 1).numpy(), raw.numpy(), rtol=1e-5, atol=1e-6)


def test_forward_layers_serves_train_mode_and_autograd_on_the_cpu():
    head = HH.make_head(8, HH.TWO_TASKS, 5).train()
    x = torch.randn(2, 8, 4, 6, requires_grad=True)
    out = head(x)
    sum(v.sum() for d in out for v in d.values()).backward()
    assert x.grad is not None and head.shared_conv[0].weight.grad is not None and int(head.shared_conv[1].num_batches_tracked) == 1


def test_predict_refuses_what_it_does_not_serve():
    head = HH.make_head(8, HH.TWO_TASKS, 6)
    with torch.no_grad():
        preds = head(torch.randn(1, 8, 4, 4))
    from shasta_amd import hip
    for nms in (dict(HH.TEST_CFG["nms"], use_rotate_nms=False), dict(HH.TEST_CFG["nms"], use_multi_class_nms=True)):
        with pytest.raises(NotImplementedError):
            head.predict({}, preds, dict(HH.TEST_CFG, nms=nms))
    with pytest.raises(hip.ShastaHipError):  # CPU tensors: there is no CPU path
        head.predict({}, preds, HH.TEST_CFG)


# ---- GPU ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("tasks,in_channels,B,H,W", [(HH.TWO_TASKS, 24, 3, 5, 33), (HH.NUSC_TASKS, 8, 1, 9, 130)], ids=["two-tasks", "nuscenes"])
def test_forward_on_the_kernels_against_forward_layers_float64(tasks, in_channels, B, H, W):
    """The module's kernel path end to end against forward_layers in float64.  Each layer's bar holds on its own input; through the chain
    the earlier layers' errors are carried by the later weights, so the comparison is layer by layer on the kernel path's own
    intermediates (head_helpers.check_chain with the module's buffers), and the dict `forward` returns must be those raw tensors."""
    from shasta_amd import hip
    dev = _dev()
    head = HH.make_head(in_channels, tasks, 40 + in_channels).to(dev)
    x = torch.relu(torch.randn(B, in_channels, H, W, generator=torch.Generator().manual_seed(41)))
    with torch.no_grad():
        out = head(x.to(dev))
        again = head(x.to(dev))
    assert head._packed is not None, "the kernel path was not taken"
    host = copy.deepcopy(head).cpu()

    def from_module_bn(convs, bns, xin):  # the kernel path's own intermediate for these layers: re-run through the module's packing
        lib = hip.load()
        packed = head._pack_bn_layer(lib, convs, bns, dev)
        xd = xin.to(dev).contiguous()
        cout = sum(c.out_channels for c in convs)
        o = torch.empty(xd.shape[0], cout, H, W, device=dev)
        hip.check(lib.shasta_neck_layer_f32(hip.ptr(xd), xd.shape[0], xd.shape[1], H, W, hip.ptr(packed), packed.numel(), 0, cout, hip.ptr(o), cout, 0,
                                            hip.stream_ptr()), "layer")
        return o.cpu()

    it = iter(out)

    def from_forward(convs, xin):
        d = next(it)
        return torch.cat([d[n] for n in d], 1).cpu()

    raws = HH.check_chain(host, x, lambda convs, bns, xin: from_module_bn([_twin(head, host, c) for c in convs], [_twin(head, host, b) for b in bns], xin),
                          from_forward)
    assert len(raws) == len(tasks)
    for d, d2, t in zip(out, again, tasks):
        assert list(d) == ["reg", "height", "dim", "rot", "vel", "hm"] and d["hm"].shape == (B, t["num_class"], H, W) and d["dim"].shape == (B, 3, H, W)
        assert all(torch.equal(d[n], d2[n]) for n in d), "two runs differ"
    # forward_layers in float64 end to end: the same numbers at a loose, chain-wide tolerance (the strict bars are the per-layer ones)
    ref = copy.deepcopy(host).double().forward_layers(x.double())
    for d, r in zip(out, ref):
        for n in d:
            np.testing.assert_allclose(d[n].cpu().double().numpy(), r[n].detach().numpy(), rtol=1e-4, atol=1e-4)
    # in-place weight edits and .to() are followed
    with torch.no_grad():
        head.tasks[0].hm[3].bias.add_(1.0)
        shifted = head(x.to(dev))
    assert torch.allclose(shifted[0]["hm"], out[0]["hm"] + 1.0, atol=1e-5) and torch.equal(shifted[0]["reg"], out[0]["reg"])


@pytest.mark.gpu
def test_widths_outside_the_kernels_run_forward_layers():
    """A four-class task (final width 4) and train() mode are served by the nn form on the device, not refused and not mis-served."""
    dev = _dev()
    wide = HH.make_head(8, [dict(num_class=4, class_names=list("abcd"))], 50).to(dev)
    x = torch.randn(2, 8, 5, 7, device=dev)
    with torch.no_grad():
        out = wide(x)
        ref = wide.forward_layers(x)
    assert wide._packed is None and out[0]["hm"].shape == (2, 4, 5, 7) and all(torch.allclose(out[0][n], ref[0][n], rtol=1e-5, atol=1e-6) for n in ref[0])
    head = HH.make_head(8, HH.TWO_TASKS, 51).to(dev).train()
    with torch.no_grad():
        head(x)
    assert head._packed is None and int(head.shared_conv[1].num_batches_tracked) == 1


def _twin(dev_module, host_module, host_layer):
    """The device module's layer that corresponds to a layer of its host copy."""
    for (_, a), (_, b) in zip(dev_module.named_modules(), host_module.named_modules()):
        if b is host_layer:
            return a
    raise KeyError


def _predict_case(peaks, tasks, B, cfg, seed, empty=(), tie=False, H=36, W=40):
    """Planted raw maps -> (device predict output, per-sample oracle chain, bars)."""
    dev = _dev()
    head = HH.make_head(8, tasks, 7)
    ncs = [t["num_class"] for t in tasks]
    raws = [[HH.planted_maps(0 if b in empty else peaks, nc, H, W, seed + 10 * t + b, tie=tie) for b in range(B)] for t, nc in enumerate(ncs)]
    preds = []
    for t, nc in enumerate(ncs):
        raw = torch.stack(raws[t]).to(dev)
        preds.append(dict(reg=raw[:, 0:2], height=raw[:, 2:3], dim=raw[:, 3:6], rot=raw[:, 6:8], vel=raw[:, 8:10], hm=raw[:, 10:]))
    example = dict(metadata=[dict(token="t%d" % b) for b in range(B)])
    got = head.predict(example, preds, cfg)
    again = head.predict(example, preds, cfg)
    torch.cuda.synchronize()
    assert len(got) == B
    for b in range(B):
        o = HH.predict_oracle([raws[t][b] for t in range(len(ncs))], ncs, cfg)
        # the oracle's own conditions: every pair's exact IoU at least 0.02 from the threshold (the pinned IoU error bar of 0.016 with a
        # margin), scores distinct (but for the planted tie)
        assert o["iou_margin"] >= 0.02, o["iou_margin"]
        assert tie or o["score_gap"] > 1e-6, o["score_gap"]
        g = got[b]
        assert g["metadata"] == dict(token="t%d" % b)
        assert g["box3d_lidar"].dtype == torch.float32 and g["scores"].dtype == torch.float32 and g["label_preds"].dtype == torch.int64
        assert g["label_preds"].cpu().tolist() == o["label"].tolist(), "sample %d: selection" % b
        per_task = [HH.transcendental_bars(raws[t][b], nc)[1] for t, nc in enumerate(ncs)]
        bars = {k: max(p[k] for p in per_task) for k in per_task[0]}
        HH.assert_boxes(g["box3d_lidar"], g["scores"], o["box"], o["score"], bars, W, H, cfg, "sample %d" % b)
        assert all(torch.equal(g[k], again[b][k]) for k in ("box3d_lidar", "scores", "label_preds")), "two runs differ"
        yield g, o


PLANT_CFG = dict(HH.TEST_CFG, pc_range=[-12.0, -10.8])  # a 36 x 40 map of 0.6 m pixels around the origin


@pytest.mark.gpu
@pytest.mark.parametrize("peaks", [1, 5, 120])
def test_predict_on_planted_objects(peaks):
    """box3d_lidar rows, scores and label_preds equal the oracle chain's selection index for index."""
    H, W = (72, 66) if peaks == 120 else (36, 40)
    cfg = dict(HH.TEST_CFG, pc_range=[-0.3 * W, -0.3 * H])
    for g, o in _predict_case(peaks, HH.TWO_TASKS, 2, cfg, 300 + peaks, H=H, W=W):
        want = 2 * min(peaks, cfg["nms"]["nms_post_max_size"])  # the main peaks stay, the second peaks go; 120 peaks meet the cut to 83
        assert len(o["label"]) == want and g["box3d_lidar"].shape == (want, 9)


@pytest.mark.gpu
def test_predict_cuts_offsets_ties_and_an_empty_sample():
    three = HH.TWO_TASKS + [dict(num_class=2, class_names=["pedestrian", "traffic_cone"])]
    # nms_pre_max_size 8 with 20 candidates (15 clusters, 5 second peaks), nms_post_max_size 3, three tasks, sample 1 empty
    cfg = dict(PLANT_CFG, nms=dict(PLANT_CFG["nms"], nms_pre_max_size=8, nms_post_max_size=3))
    res = list(_predict_case(15, three, 3, cfg, 400, empty=(1,)))
    for b, (g, o) in enumerate(res):
        assert len(g["scores"]) == (0 if b == 1 else 9), len(g["scores"])  # 3 per task
        if b != 1:
            lab = g["label_preds"].cpu()
            assert bool((lab[:3] == 0).all()) and bool(((lab[3:6] >= 1) & (lab[3:6] <= 2)).all()) and bool(((lab[6:] >= 3) & (lab[6:] <= 4)).all())
    assert res[1][0]["box3d_lidar"].shape == (0, 9) and res[1][0]["label_preds"].shape == (0,)
    # the pre-NMS cut alone: 8 of 20 candidates enter, the post cut is wide
    cfg8 = dict(PLANT_CFG, nms=dict(PLANT_CFG["nms"], nms_pre_max_size=8))
    for g, o in _predict_case(15, HH.TWO_TASKS, 1, cfg8, 410):
        assert 2 <= len(g["scores"]) <= 16 and len(g["scores"]) == len(o["score"])
    # two equal scores: the lower pixel first
    for g, o in _predict_case(5, [HH.TWO_TASKS[0]], 1, PLANT_CFG, 420, tie=True):
        s = g["scores"].cpu()
        same = torch.nonzero(s[:-1] == s[1:])[:, 0]
        assert len(same) == 1, "the planted tie"
        i = int(same[0])
        xy = g["box3d_lidar"][i:i + 2, :2].cpu().double()
        pix = torch.floor((xy[:, 1] - PLANT_CFG["pc_range"][1]) / 0.6) * 40 + torch.floor((xy[:, 0] - PLANT_CFG["pc_range"][0]) / 0.6)
        assert float(pix[0]) < float(pix[1]), "ties: the lower pixel first"


# ---- the detector -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _detector():
    import shasta_amd
    from shasta_amd.backbone import SpMiddleResNetFHD
    from tests import backbone_helpers as BH
    from tests.neck_helpers import randomize_bn
    torch.manual_seed(71)
    cfg = dict(HH.TEST_CFG, pc_range=[-13.5, -13.5], voxel_size=[0.5625, 0.5625], post_center_limit_range=[-20.0, -20.0, -10.0, 20.0, 20.0, 10.0],
               score_threshold=0.05)
    m = shasta_amd.build_detector(dict(
        type="VoxelNet", reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5),
        backbone=dict(type=SpMiddleResNetFHD, num_input_features=5, ds_factor=8),
        neck=dict(type="RPN", layer_nums=[1, 1], ds_layer_strides=[1, 2], ds_num_filters=[32, 64], us_layer_strides=[1, 2], us_num_filters=[32, 32],
                  num_input_features=256),
        bbox_head=dict(type="CenterHead", in_channels=[64], tasks=HH.TWO_TASKS)), test_cfg=cfg).eval()
    BH.randomize(m.backbone, torch.Generator().manual_seed(72))
    randomize_bn(m.neck, torch.Generator().manual_seed(73))
    randomize_bn(m.bbox_head, torch.Generator().manual_seed(74))
    with torch.no_grad():
        for t in m.bbox_head.tasks:
            t.hm[3].bias.fill_(0.0)  # (scores around 0.5: there are detections)
    return m.to(_dev()), cfg


@pytest.mark.gpu
def test_voxelnet_from_voxels_to_detections():
    from shasta_amd.voxel_generator import VoxelGenerator
    m, cfg = _detector()
    dev = _dev()
    assert [n for n, _ in m.named_children()] == ["reader", "backbone", "neck", "bbox_head"]
    assert any(k.startswith("bbox_head.tasks.1.hm.3.") for k in m.state_dict()) and any(k.startswith("neck.blocks.0.") for k in m.state_dict())
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
    with torch.no_grad():
        dets = m(example)
        again = m(example)
        x = m.neck(m.backbone(m.reader(vs, ns), cs, 2, example["shape"][0])[0])
        by_hand = m.bbox_head.predict(example, m.bbox_head(x), cfg)
    assert x.shape == (2, 64, 6, 6) and len(dets) == 2
    for d, d2, d3, tok in zip(dets, again, by_hand, "ab"):
        n = d["scores"].shape[0]
        assert n > 0 and d["box3d_lidar"].shape == (n, 9) and d["label_preds"].shape == (n,) and d["metadata"] == dict(token=tok)
        assert int(d["label_preds"].min()) >= 0 and int(d["label_preds"].max()) <= 2
        for k in ("box3d_lidar", "scores", "label_preds"):
            assert torch.equal(d[k], d2[k]) and torch.equal(d[k], d3[k])
    with pytest.raises(NotImplementedError):
        m(example, return_loss=True)
