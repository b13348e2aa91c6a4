"""CenterPoint training targets on the device (csrc/center_targets.hip, shasta_amd/targets.py) against the numpy / float64 restatement
of tests/center_targets_helpers.py.  Integer outputs, the slot layout and the copied columns must be equal; the heatmap within 1 fp32
ulp (the count of entries that differ at all is printed; DESIGN.md section 4 records it); log / sin / cos within 4 x what numpy's fp32
functions reach on the same inputs and at least 4 ulp of the float64 value, the rule of tests/test_head_kernels.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from . import center_targets_helpers as H

F = np.float32


def _dev():
    return torch.device("cuda")


# ---- CPU: the restatement itself, refusals ----------------------------------------------------------------------------------------
def test_restatement_pins():
    # radius of l' = 8, w' = 4 cells at overlap 0.1, by hand: r3 = (-2.4 + sqrt(5.76 + 1.6 * 28.8)) / 2 = 2.39999..; r1 = 10.47.., r2 = 5.29..
    r = H.gaussian_radius_ref((F(8.0), F(4.0)), 0.1)
    assert isinstance(r, np.floating) and r.dtype == np.float32  # fp32 throughout under numpy >= 2 promotion
    assert abs(float(r) - (-2.4 + np.sqrt(5.76 + 1.6 * 28.8)) / 2) < 1e-5 and int(r) == 2
    # one gaussian row, radius 2: sigma = 5 / 6, centre row = exp(-x^2 / (2 sigma^2)) = exp(-0.72 x^2)
    g = H.gaussian_ref(2)
    assert g.dtype == np.float64 and g.shape == (5, 5)
    np.testing.assert_allclose(g[2], np.exp(-0.72 * np.array([4.0, 1.0, 0.0, 1.0, 4.0])), rtol=1e-15)
    assert g.min() > np.exp(-9.0)  # exp(-36 r^2 / (2r + 1)^2): the eps cut never fires
    # limit_period wraps: 4.0 -> 4 - 2 pi, -5.5 -> -5.5 + 2 pi, 7.0 -> 7 - 2 pi, in fp32
    v = H.limit_period_ref(np.array([4.0, -5.5, 7.0, 1.0], dtype=F), 0.5, np.pi * 2)
    assert v.dtype == np.float32
    np.testing.assert_allclose(v, [4.0 - 2 * np.pi, -5.5 + 2 * np.pi, 7.0 - 2 * np.pi, 1.0], atol=1e-6)
    # the rectangle's test puts a point on an edge outside
    keep = H.filter_ref(H.filter_exact_set([-7.2, -6.0, 7.2, 6.0]), [-7.2, -6.0, 7.2, 6.0])
    assert keep.tolist() == [False, True, False, True, False, False, True]
    # a flip's heading: -rot + fp32(pi) in fp32
    e = dict(flip_x=True, flip_y=False, angle=0.0, c=1.0, s=0.0, scale=1.0, translate=None)
    b = H.augment_ref(np.array([H._box(1.0, 2.0, 1.0, 2.0, 0.25)], dtype=F), e)
    assert b[0, 1] == -2.0 and b[0, 7] == F(0.2) and b[0, 8] == F(F(-0.25) + F(np.pi))
    # slots: stable partition, a hole, truncation
    boxes, cls = H.truncation_sample(H.GEOM_A)
    ref = H.assign_ref(boxes, cls, H.GEOM_A, with_gtbc=False)
    assert ref["mask"][1].sum() == 8 and ref["cat"][1].tolist() == [0] * 5 + [1] * 3 and ref["mask"][0].sum() == 2
    boxes, cls = H.special_sample(H.GEOM_A)
    ref = H.assign_ref(boxes, cls, H.GEOM_A, with_gtbc=False)
    assert ref["mask"][0].sum() == 0 and ref["mask"][2].tolist() == [1, 1, 1, 1, 0, 1, 0, 0]  # slot 4: the centre outside the map
    assert ref["ind"][1][0] == ref["ind"][1][1] == 9 * H.MAP_W + 10 and max(int(r) for r in ref["radius"]) >= 9
    assert ref["mask"][1].tolist() == [1, 1, 1, 1, 1, 1, 0, 0]  # slot 6: w = 0


def test_input_sets_keep_their_margins():
    for cfg in (H.GEOM_A, H.GEOM_B):
        for make in (H.special_sample, H.truncation_sample):
            boxes, cls = make(cfg)
            H.assert_margins(boxes, cls, cfg)
            for e in H.ENTRIES_ROTATION:
                from shasta_amd.sweeps import augment_entry
                H.assert_margins(H.augment_ref(boxes, augment_entry(**e)), cls, cfg)
    rng = [-7.2, -6.0, 7.2, 6.0]
    H.assert_corner_margins(H.filter_set(rng), rng)
    boxes, _ = H.special_sample(H.GEOM_A)
    H.assert_corner_margins(boxes, rng)


def test_cpu_use_and_waymo_are_refused():
    from shasta_amd import hip, targets
    boxes, cls = H.special_sample(H.GEOM_A)
    t = torch.from_numpy(boxes)
    with pytest.raises(hip.ShastaHipError):
        targets.assign_targets([t], [cls], H.TASKS, H.GEOM_A)
    with pytest.raises(hip.ShastaHipError):
        targets.filter_gt_box_outside_range(t, [-7.2, -6.0, 7.2, 6.0])
    with pytest.raises(hip.ShastaHipError):
        targets.augment_boxes(t, None)
    step = targets.AssignLabel(cfg=dict(H.GEOM_A, target_assigner=dict(tasks=[dict(num_class=n) for n in H.TASKS])))
    res = dict(mode="train", type="WaymoDataset", lidar=dict(annotations=dict(gt_boxes=t, gt_classes=cls)))
    with pytest.raises(NotImplementedError):
        step(res, {})
    res = dict(mode="train", type="NuScenesDataset", lidar=dict(annotations=dict(gt_boxes=t, gt_classes=cls)))
    with pytest.raises(hip.ShastaHipError):
        step(res, {})
    res = dict(mode="val", type="NuScenesDataset", lidar={})
    assert step(res, {})[0]["lidar"]["targets"] == {}
    with pytest.raises(NotImplementedError):
        targets.LoadPointCloudAnnotations()(dict(type="WaymoDataset", lidar={}), dict(gt_boxes=boxes))
    from shasta_amd import PIPELINES
    assert PIPELINES.get("AssignLabel") is targets.AssignLabel and PIPELINES.get("LoadPointCloudAnnotations") is targets.LoadPointCloudAnnotations


def test_shapes_beyond_the_limits_are_refused_before_a_launch():
    """No GPU here: a call that reached a memset or a launch would fail differently (SHASTA_E_LAUNCH) or crash on the fake pointers."""
    from shasta_amd import hip
    lib = hip.load()
    assert lib.shasta_center_targets_workspace_bytes(64, 16, 1024) > 0 and lib.shasta_center_loss_workspace_bytes(16, 64) > 0
    for B, T, M in ((65, 6, 500), (0, 6, 500), (4, 17, 500), (4, 0, 500), (4, 6, 1025), (4, 6, 0)):
        assert lib.shasta_center_targets_workspace_bytes(B, T, M) == 0
    assert lib.shasta_center_loss_workspace_bytes(17, 4) == 0 and lib.shasta_center_loss_workspace_bytes(6, 65) == 0
    buf = (C.c_double * 64)()
    fake = C.cast(buf, C.c_void_p)

    def call(B=1, T=1, max_objs=8, W=24, H_=20, ncls=2, counts=(3,)):
        k = hip.CenterTargetCfg()
        k.num_tasks, k.max_objs, k.min_radius, k.map_w, k.map_h = T, max_objs, 2, W, H_
        for t in range(min(T, 16)):
            k.num_class[t] = ncls
        k.pc_x, k.pc_y, k.voxel_x, k.voxel_y, k.out_size_factor, k.gaussian_overlap = -7.2, -6.0, 0.075, 0.075, 8.0, 0.1
        off = (C.c_int32 * (len(counts) + 1))(*np.concatenate([[0], np.cumsum(counts)]).tolist())
        return lib.shasta_center_targets_f32(fake, fake, off, B, C.byref(k), None, None, fake, fake, fake, fake, fake, fake, fake, None, fake,
                                             1 << 30, None)

    assert call(W=513) == hip.E_UNSUPPORTED and call(H_=0) == hip.E_UNSUPPORTED
    assert call(ncls=5) == hip.E_UNSUPPORTED and call(T=17) == hip.E_UNSUPPORTED and call(max_objs=1025) == hip.E_UNSUPPORTED
    assert call(counts=(4097,)) == hip.E_UNSUPPORTED
    assert call(B=65, counts=(1,) * 65) == hip.E_UNSUPPORTED
    task = (hip.CenterLossTask * 1)()
    cw = (C.c_float * 10)(*([1.0] * 10))
    assert lib.shasta_center_loss_f32(task, 1, 2, 513, 24, 8, 0.25, cw, fake, fake, 1 << 30, None) == hip.E_UNSUPPORTED
    assert lib.shasta_center_loss_f32(task, 1, 2, 20, 24, 1025, 0.25, cw, fake, fake, 1 << 30, None) == hip.E_UNSUPPORTED
    assert lib.shasta_center_loss_f32(task, 1, 2, 20, 24, 8, 0.25, cw, fake, fake, 1 << 30, None) == hip.E_UNSUPPORTED  # num_class = 0
    from shasta_amd import build
    assert "center_targets.hip" in build.SOURCES and "center_loss.hip" in build.SOURCES


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _run(samples, cfg, augment=None, bv_range=None, gtbc=True):
    from shasta_amd import targets
    dev = _dev()
    boxes = [torch.from_numpy(np.ascontiguousarray(b)).to(dev) for b, _ in samples]
    out = targets.assign_targets(boxes, [c for _, c in samples], H.TASKS, dict(cfg, gt_boxes_and_cls=gtbc), augment=augment, bv_range=bv_range)
    torch.cuda.synchronize()
    return out


def _close_fn(got, arg64, fn, what):
    """tests/test_head_kernels.py's rule: 4 x numpy's own fp32 error on these inputs, at least 4 ulp of the float64 value."""
    want = fn(arg64.astype(np.float64))
    own = H.ulps(fn(arg64.astype(F)), want).max() if len(want) else 0.0
    err = H.ulps(got, want).max() if len(want) else 0.0
    print("%s: largest error %.2f ulp, numpy fp32 %.2f ulp, bar %.2f" % (what, err, own, max(4.0, 4 * own)))
    assert err <= max(4.0, 4 * own), what
    return err


def _compare(out, samples, cfg, gtbc, rotated=False):
    """Every output of a batch against the restatement, sample by sample.  `samples` are the boxes AFTER augmentation and range filter
    as the restatement computes them.  Returns the number of heatmap entries that differ at all."""
    differ = 0
    for b, (boxes, cls) in enumerate(samples):
        ref = H.assign_ref(boxes, cls, cfg, with_gtbc=gtbc)
        for t in range(len(H.TASKS)):
            for key in ("ind", "mask", "cat"):
                got = out[key][t][b].cpu().numpy()
                assert got.dtype == ref[key][t].dtype and np.array_equal(got, ref[key][t]), (key, b, t)
            hm, want = out["hm"][t][b].cpu().numpy(), ref["hm"][t]
            assert hm.shape == want.shape == (H.TASKS[t], H.MAP_H, H.MAP_W) and hm.dtype == np.float32
            assert np.array_equal(hm == 0, want == 0), ("exact zeros", b, t)
            differ += int((hm != want).sum())
            assert (np.abs(hm.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)) <= 1).all(), ("hm within 1 ulp", b, t)
            anno, wanno = out["anno_box"][t][b].cpu().numpy(), ref["anno_box"][t]
            m = ref["mask"][t].astype(bool)
            assert not anno[~m].any()
            for col in (0, 1, 2, 6, 7):
                assert np.array_equal(anno[m, col].view(np.int32), wanno[m, col].view(np.int32)), ("anno_box column", col, b, t)
            lim = ref["limited"][t][:H.MAX_OBJS][m[:len(ref["limited"][t])]] if m.any() else np.zeros((0, 9), F)
            _close_fn(anno[m, 3:6].reshape(-1), lim[:, 3:6].reshape(-1), np.log, "log w/l/h")
            _close_fn(anno[m, 8], lim[:, 8], np.sin, "sin rot")
            _close_fn(anno[m, 9], lim[:, 8], np.cos, "cos rot")
        if gtbc:
            got = out["gt_boxes_and_cls"][b].cpu().numpy()
            assert np.array_equal(got.view(np.int32), ref["gt_boxes_and_cls"].view(np.int32)), ("gt_boxes_and_cls", b)
    return differ


def _batch_nogtbc(cfg):
    return [H.truncation_sample(cfg), (np.zeros((0, 9), F), np.zeros(0, np.int32)), H.special_sample(cfg)]


def _batch_gtbc(cfg):
    boxes, cls = H.special_sample(cfg)
    eb, ec = H.exact_sample(cfg)
    return [(boxes[:8], cls[:8]), (np.zeros((0, 9), F), np.zeros(0, np.int32)), (np.concatenate([boxes[8:], eb[:3]]), np.concatenate([cls[8:], ec[:3]]))]


@pytest.mark.gpu
@pytest.mark.parametrize("geom", ["A", "B"])
def test_assign_targets_matches_the_restatement(geom):
    cfg = H.GEOM_A if geom == "A" else H.GEOM_B
    differ = 0
    for gtbc, samples in ((False, _batch_nogtbc(cfg)), (True, _batch_gtbc(cfg)), (True, [H.exact_sample(cfg)])):
        out = _run(samples, cfg, gtbc=gtbc)
        assert [tuple(h.shape) for h in out["hm"]] == [(len(samples), n, H.MAP_H, H.MAP_W) for n in H.TASKS]
        assert out["ind"][0].dtype == torch.int64 and out["cat"][0].dtype == torch.int64 and out["mask"][0].dtype == torch.uint8
        assert ("gt_boxes_and_cls" in out) == gtbc and bool(out["keep"].all())
        differ += _compare(out, samples, cfg, gtbc)
        again = _run(samples, cfg, gtbc=gtbc)
        for key in ("hm", "anno_box", "ind", "mask", "cat"):
            assert all(torch.equal(a, b) for a, b in zip(out[key], again[key])), key
    print("geometry %s: heatmap entries that differ from the restatement: %d" % (geom, differ))


@pytest.mark.gpu
def test_packed_form_and_device_classes_give_the_same():
    from shasta_amd import targets
    cfg, dev = H.GEOM_A, _dev()
    samples = _batch_gtbc(cfg)
    a = _run(samples, cfg)
    packed = torch.from_numpy(np.concatenate([b for b, _ in samples])).to(dev)
    cls = torch.from_numpy(np.concatenate([c for _, c in samples])).to(dev)
    off = np.concatenate([[0], np.cumsum([len(b) for b, _ in samples])]).tolist()
    b = targets.assign_targets((packed, off), cls, [dict(num_class=n) for n in H.TASKS], cfg)
    for key in ("hm", "anno_box", "ind", "mask", "cat"):
        assert all(torch.equal(x, y) for x, y in zip(a[key], b[key])), key
    assert torch.equal(a["gt_boxes_and_cls"], b["gt_boxes_and_cls"])


@pytest.mark.gpu
def test_more_boxes_than_max_objs_is_a_value_error():
    from shasta_amd import targets
    dev = _dev()
    boxes, cls = H.truncation_sample(H.GEOM_A)
    t = torch.from_numpy(boxes).to(dev)
    with pytest.raises(ValueError, match="max_objs"):
        targets.assign_targets([t], [cls], H.TASKS, H.GEOM_A)
    with pytest.raises(ValueError, match="max_objs"):
        targets.assign_targets([t], [torch.from_numpy(cls).to(dev)], H.TASKS, H.GEOM_A)
    # 14 boxes in the tasks' classes, 9 of them inside a narrow range: the limit is checked on what the filter keeps
    keep = H.filter_ref(boxes, [-7.2, -6.0, 7.2, 0.9])
    n_in = int((keep & (cls <= 5)).sum())
    assert n_in != 14
    if n_in > 8:
        with pytest.raises(ValueError, match="max_objs"):
            targets.assign_targets([t], [cls], H.TASKS, H.GEOM_A, bv_range=[-7.2, -6.0, 7.2, 0.9])
    else:
        targets.assign_targets([t], [cls], H.TASKS, H.GEOM_A, bv_range=[-7.2, -6.0, 7.2, 0.9])


@pytest.mark.gpu
def test_range_filter_kept_set_is_equal():
    from shasta_amd import targets
    dev = _dev()
    rng = [-7.2, -6.0, 7.2, 6.0]
    for boxes in (H.filter_set(rng), H.filter_exact_set(rng), H.special_sample(H.GEOM_A)[0], np.zeros((0, 9), F)):
        got = targets.filter_gt_box_outside_range(torch.from_numpy(boxes).to(dev), rng)
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), H.filter_ref(boxes, rng))
    kept = H.filter_ref(H.filter_set(rng), rng)
    assert 5 < kept.sum() < len(kept) - 5  # both outcomes occur
    # as a stage of the batched call: the kept boxes are assigned, the others leave no trace
    boxes, cls = H.special_sample(H.GEOM_A)
    narrow = [-7.2, -6.0, 4.9, 3.1]
    H.assert_corner_margins(boxes, narrow)
    k = H.filter_ref(boxes, narrow)
    assert 0 < k.sum() < len(k)
    out = _run([(boxes, cls)], H.GEOM_A, bv_range=narrow, gtbc=False)
    assert np.array_equal(out["keep"].cpu().numpy(), k)
    _compare(out, [(boxes[k], cls[k])], H.GEOM_A, False)


@pytest.mark.gpu
def test_box_augmentation_without_rotation_is_bit_equal():
    from shasta_amd import targets
    from shasta_amd.sweeps import augment_entry
    dev, cfg = _dev(), H.GEOM_A
    boxes, cls = H.special_sample(cfg)
    eb, ec = H.exact_sample(cfg)
    boxes, cls = np.concatenate([boxes, eb]), np.concatenate([cls, ec])
    entries = [augment_entry(**e) for e in H.ENTRIES_NO_ROTATION]
    for e in entries:
        got = targets.augment_boxes(torch.from_numpy(boxes).to(dev), e).cpu().numpy()
        assert np.array_equal(got.view(np.int32), H.augment_ref(boxes, e).view(np.int32))
    # inside the batched call: every decision and every copied column equal
    samples = [(boxes, cls)] * 3
    out = _run(samples, cfg, augment=entries, gtbc=False)
    want = [(H.augment_ref(boxes, e), cls) for e in entries]
    assert np.array_equal(out["gt_boxes"].cpu().numpy().view(np.int32), np.concatenate([w for w, _ in want]).view(np.int32))
    _compare(out, want, cfg, False)


@pytest.mark.gpu
def test_box_augmentation_with_rotation_keeps_the_dot_product_bound():
    from shasta_amd import targets
    from shasta_amd.sweeps import augment_entry
    dev, cfg = _dev(), H.GEOM_A
    boxes, cls = H.special_sample(cfg)
    u = 2.0 ** -24
    entries = [augment_entry(**e) for e in H.ENTRIES_ROTATION]
    for e in entries:
        got = targets.augment_boxes(torch.from_numpy(boxes).to(dev), e).cpu().numpy()
        flips = H.augment_ref(boxes, dict(e, angle=0.0, c=1.0, s=0.0, scale=1.0, translate=None))  # exact steps before the rotation
        only_rot = targets.augment_boxes(torch.from_numpy(flips).to(dev), dict(e, flip_x=False, flip_y=False, scale=1.0, translate=None)).cpu().numpy()
        val, mag = H.rotate64(flips, e)
        for col in (0, 1, 6, 7):
            assert (np.abs(only_rot[:, col].astype(np.float64) - val[col]) <= 4 * u * mag[col]).all(), col
        ref = H.augment_ref(boxes, e)
        for col in (2, 3, 4, 5):  # z and the sizes: bit-equal
            assert np.array_equal(got[:, col].view(np.int32), ref[:, col].view(np.int32)), col
        assert np.array_equal(only_rot[:, 8].view(np.int32), (flips[:, 8] + F(e["angle"])).view(np.int32))
        assert np.array_equal(got[:, 8].view(np.int32), ref[:, 8].view(np.int32))
    # the batched call on rotated boxes: the inputs keep their margins (test_input_sets_keep_their_margins), so every decision is equal
    out = _run([(boxes, cls)] * 3, cfg, augment=entries, gtbc=False)
    got = out["gt_boxes"].cpu().numpy().reshape(3, -1, 9)
    for i, e in enumerate(entries):
        ref = H.assign_ref(H.augment_ref(boxes, e), cls, cfg, with_gtbc=False)
        for t in range(len(H.TASKS)):
            for key in ("ind", "mask", "cat"):
                assert np.array_equal(out[key][t][i].cpu().numpy(), ref[key][t]), (key, i, t)
        _compare({k: [v[i:i + 1] for v in out[k]] for k in ("hm", "anno_box", "ind", "mask", "cat")}, [(got[i], cls)], cfg, False)


@pytest.mark.gpu
def test_preprocess_gives_points_and_boxes_the_same_entry():
    from shasta_amd import sweeps, targets
    dev, cfg = _dev(), H.GEOM_A
    boxes, cls = H.special_sample(cfg)
    names = np.array(["car", "truck", "bus", "trailer", "barrier"])[cls - 1]
    names = np.concatenate([names, ["DontCare", "animal"]])
    boxes = np.concatenate([boxes, boxes[:2]])
    pts = torch.from_numpy(np.random.RandomState(3).randn(500, 5).astype(F)).to(dev)
    pcfg = dict(mode="train", shuffle_points=True, global_rot_noise=[0.0, 0.0], global_scale_noise=[0.95, 1.05], global_translate_std=0.5,
                class_names=["car", "truck", "bus", "trailer", "barrier"], db_sampler=None)
    step = sweeps.Preprocess(cfg=pcfg)

    def run(with_anno):
        np.random.seed(11)
        res = dict(type="NuScenesDataset", lidar=dict(combined=pts.clone()))
        if with_anno:
            res["lidar"]["annotations"] = dict(boxes=boxes.copy(), names=names)
        return step(res, {})[0]

    a, b = run(True), run(False)
    assert torch.equal(a["lidar"]["points"], b["lidar"]["points"])  # the points do not depend on the annotations
    assert "annotations" not in b["lidar"] and a["lidar"]["augment"] == b["lidar"]["augment"]
    np.random.seed(11)
    entry = sweeps.draw_augment([0.0, 0.0], [0.95, 1.05], 0.5)
    assert entry == a["lidar"]["augment"]
    gt = a["lidar"]["annotations"]
    assert gt["gt_names"].tolist() == names[:13].tolist() and np.array_equal(gt["gt_classes"], cls) and gt["gt_classes"].dtype == np.int32
    assert gt["gt_boxes"].is_cuda
    assert np.array_equal(gt["gt_boxes"].cpu().numpy().view(np.int32), H.augment_ref(boxes[:13], entry).view(np.int32))
    # no_augmentation: classes are selected and numbered only (DontCare is no class name either)
    res = dict(type="NuScenesDataset", lidar=dict(combined=pts.clone(), annotations=dict(boxes=boxes.copy(), names=names)))
    gt = sweeps.Preprocess(cfg=dict(pcfg, no_augmentation=True, shuffle_points=False))(res, {})[0]["lidar"]["annotations"]
    assert np.array_equal(gt["gt_boxes"].cpu().numpy(), boxes[:13]) and np.array_equal(gt["gt_classes"], cls)
    # ... and AssignLabel behind it, both branches of the grid geometry
    tasks = [dict(num_class=1, class_names=["car"]), dict(num_class=2, class_names=["truck", "bus"]), dict(num_class=2, class_names=["trailer", "barrier"])]
    acfg = dict(cfg, target_assigner=dict(tasks=tasks), max_objs=16)
    for voxels in (False, True):
        res = dict(type="NuScenesDataset", mode="train", lidar=dict(annotations=dict(gt)))
        if voxels:
            res["lidar"]["voxels"] = dict(shape=np.array([192, 160, 40]), range=np.array(cfg["pc_range"], dtype=F), size=np.array(cfg["voxel_size"], dtype=F))
            step2 = targets.AssignLabel(cfg={k: v for k, v in acfg.items() if k not in ("pc_range", "voxel_size")})
        else:
            step2 = targets.AssignLabel(cfg=acfg)
        ex = step2(res, {})[0]["lidar"]["targets"]
        ref = H.assign_ref(boxes[:13], cls, dict(cfg, max_objs=16))
        for t in range(3):
            assert ex["hm"][t].shape == (H.TASKS[t], H.MAP_H, H.MAP_W)
            for key in ("ind", "mask", "cat"):
                assert np.array_equal(ex[key][t].cpu().numpy(), ref[key][t])
        assert np.array_equal(ex["gt_boxes_and_cls"].cpu().numpy().view(np.int32), ref["gt_boxes_and_cls"].view(np.int32))
