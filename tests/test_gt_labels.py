"""Ground-truth label construction (shasta_amd/gt_labels.py, csrc/gt_labels.hip) against the reference's
preprocessing/make_gt_shasta.py + gt_association/associate.py, recorded in tests/golden/gt_labels_golden.json.gz
(tests/golden/make_gt_labels_golden.py): every index equal - which ground-truth box each detection takes, the false negatives, the
one-hot column of every previous detection, the newborn flags.  No mask, no tolerance: the fixture holds equal scores, equal
distances and distances exactly at the threshold, where only the reference's tie rules and strict comparisons give its answer."""
import gzip
import json
import os
import random

import numpy as np
import pytest

from tests.gt_label_scenes import synth_scene

HERE = os.path.dirname(os.path.abspath(__file__))
_cache = {}


def _golden():
    """{scene name: (frames as gt_labels takes them, the recorded frames)} - read once."""
    if not _cache:
        with gzip.open(os.path.join(HERE, "golden", "gt_labels_golden.json.gz"), "rt") as f:
            g = json.load(f)
        _cache["threshold"] = g["threshold"]
        _cache["scenes"] = {}
        for name, rec in g["scenes"].items():
            frames = [dict(det_xy=np.array([r["det_x"], r["det_y"]], dtype=np.float64).T.reshape(-1, 2), det_score=np.array(r["det_score"], dtype=np.float64),
                           det_types=[g["det_names"][i] for i in r["det_type"]],
                           gt_xy=np.array([r["gt_x"], r["gt_y"]], dtype=np.float64).T.reshape(-1, 2), gt_types=[g["gt_names"][i] for i in r["gt_type"]],
                           gt_ids=r["gt_id"], emit=bool(r["emit"]), has_prev=bool(r["has_prev"])) for r in rec]
            _cache["scenes"][name] = (frames, rec)
    return _cache["scenes"], _cache["threshold"]


def _want_labels(rec):
    """The reference's (matched, newborn) of the emitted frames, dense, from the recorded columns."""
    out = []
    for t, r in enumerate(rec):
        if not r["emit"]:
            continue
        matched = None
        if r["col_of_prev"] is not None:
            N, K = len(rec[t - 1]["det_score"]), len(r["det_score"])
            matched = np.zeros((N, K + 2))
            matched[np.arange(N), np.array(r["col_of_prev"], dtype=int)] = 1.0
        out.append((matched, np.array(r["newborn"], dtype=np.float64)))
    return out


def _same_labels(got, want):
    assert len(got) == len(want)
    for (gm, gn), (wm, wn) in zip(got, want):
        assert (gm is None) == (wm is None)
        if wm is not None:
            assert gm.dtype == np.float64 and gm.shape == wm.shape and np.array_equal(gm, wm)
        assert gn.dtype == np.float64 and gn.shape == wn.shape and np.array_equal(gn, wn)


def _check_against_golden(device):
    from shasta_amd import gt_labels
    scenes, thr = _golden()
    rows = 0
    for name, (frames, rec) in scenes.items():
        assoc = gt_labels.frame_associations(frames, thr, device=device)
        assert len(assoc) == len(rec)
        for (tp, fn), r in zip(assoc, rec):
            assert tp == {k: g for k, g in r["tp_ind_pairs"]}, name
            assert fn == r["fn_inds"], name
        want = _want_labels(rec)
        _same_labels(gt_labels.scene_labels(frames, thr, device=device), want)
        rows += sum(m.shape[0] for m, _ in want if m is not None)
    assert rows > 2000


def test_host_path_equals_the_reference_golden():
    _check_against_golden(device=False)


def test_golden_holds_the_cases_that_need_the_tie_rules():
    """What the generator asserted from the reference alone, visible from the recorded data: all four label kinds, the seam sizes,
    frames that are not emitted."""
    scenes, _ = _golden()
    kinds = dict(match=0, dead=0, fn=0, newborn=0)
    for frames, rec in scenes.values():
        for r in rec:
            if not r["emit"]:
                continue
            K = len(r["det_score"])
            kinds["newborn"] += sum(r["newborn"])
            for c in r["col_of_prev"] or []:
                kinds["match" if c < K else "dead" if c == K else "fn"] += 1
    assert min(kinds.values()) >= 50, kinds
    assert [(len(r["det_score"]), len(r["gt_id"])) for r in scenes["seam"][1]] == [(0, 0), (0, 5), (5, 0), (1, 1), (63, 64), (64, 65), (65, 64), (130, 90), (90, 130)]
    assert [r["emit"] for r in scenes["skipped"][1]].count(0) == 2


def test_associate_equals_the_live_reference():
    import sys
    saved_modules, saved_path = dict(sys.modules), list(sys.path)  # the reference's packages and the stubs stay out of later tests
    try:
        _associate_against_the_live_reference()
    finally:
        ref_root = getattr(sys.modules.get("ref_import"), "REF_ROOT", None)
        sys.path[:] = saved_path
        for name in set(sys.modules) - set(saved_modules):
            file = getattr(sys.modules[name], "__file__", None)
            if name == "ref_import" or file is None or (ref_root and file.startswith(ref_root)):  # (the stubs have no file)
                del sys.modules[name]


def _associate_against_the_live_reference():
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import ref_import
    if not os.path.isfile(os.path.join(ref_import.REF_ROOT, "preprocessing", "gt_association", "associate.py")):
        pytest.skip("reference tree absent")
    import importlib.util
    ref_import._install_stubs()
    if ref_import.REF_ROOT not in sys.path:
        sys.path.insert(0, ref_import.REF_ROOT)
    spec = importlib.util.spec_from_file_location("_ref_gt_associate_live", os.path.join(ref_import.REF_ROOT, "preprocessing", "gt_association", "associate.py"))
    A = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(A)
    from mot_3d.data_protos import BBox
    from shasta_amd import gt_labels

    def boxes(xy, score=None):
        out = []
        for i, p in enumerate(xy):
            b = BBox(x=float(p[0]), y=float(p[1]), z=0.0, h=1.5, w=2.0, l=4.0, o=0.0)
            if score is not None:
                b.s = float(score[i])
            out.append(b)
        return out
    pairs = 0
    for seed in range(20):
        f = synth_scene(1000 + seed, n_frames=3, quant=seed % 2 == 0, half=40.0 if seed % 4 < 2 else 10.0)[1]
        if seed == 7:
            f = dict(f, gt_xy=np.zeros((0, 2)), gt_types=[], gt_ids=[])  # an empty side returns the inputs themselves
        gt, det = boxes(f["gt_xy"]), boxes(f["det_xy"], f["det_score"])
        want = A.associate(gt, f["gt_types"], det, f["det_types"], 2.0)
        got = gt_labels.associate(gt, f["gt_types"], det, f["det_types"], 2.0)
        assert len(got) == len(want) == 10
        for i in (0, 1, 2, 3):  # lists of the very box objects that went in
            assert len(got[i]) == len(want[i]) and all(a is b for a, b in zip(got[i], want[i])), (seed, i)
        for i in (4, 5, 6, 8, 9):
            assert list(got[i]) == list(want[i]), (seed, i)
        assert got[7] == want[7] and list(got[7]) == list(want[7])  # the same pairs, entered in the same order
        pairs += len(want[7])
        rows = [[b.x, b.y, b.z, b.o, b.l, b.w, b.h, b.s] for b in det]  # rows [x, y, ..., score] give the same indices
        assert gt_labels.associate([[b.x, b.y] for b in gt], f["gt_types"], rows, f["det_types"], 2.0)[7] == want[7]
    assert pairs > 200


def test_written_label_files_load_like_the_references(tmp_path):
    """write_labels -> frames.FramePairs.load: the same `gt` as from label files holding the golden's matrices."""
    from shasta_amd import frames as fr_mod
    from shasta_amd import gt_labels
    scenes, thr = _golden()
    frames, rec = scenes["quant0"]
    tokens = ["tok%02d" % t for t in range(len(frames))]
    det_path, cls_path = tmp_path / "dets", tmp_path / "cls"
    det_path.mkdir()
    cls_path.mkdir()
    info = {}
    for t, (tok, f) in enumerate(zip(tokens, frames)):
        rows = [[float(x), float(y), 0.0, 2.0, 4.0, 1.5, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, float(s)] for (x, y), s in zip(f["det_xy"], f["det_score"])]
        (det_path / (tok + ".json")).write_text(json.dumps(rows))
        (cls_path / (tok + ".json")).write_text(json.dumps([dict(detection_name=n, detection_score=float(s)) for n, s in zip(f["det_types"], f["det_score"])]))
        info[tok] = dict(prev=tokens[t - 1] if t else "", timestamp=500000 * (t + 1), prev_timestamp=500000 * t)
    (tmp_path / "frame_info.json").write_text(json.dumps(info))
    gt_labels.write_labels(str(tmp_path / "ours"), tokens, gt_labels.scene_labels(frames, thr, device=False))
    os.makedirs(tmp_path / "golden")
    for tok, (matched, newborn) in zip(tokens, _want_labels(rec)):
        np.savez_compressed(str(tmp_path / "golden" / (tok + ".npz")), matched=matched, newborn=newborn)
    loaded = {}
    for which in ("ours", "golden"):
        fp = fr_mod.FramePairs(str(det_path), str(cls_path), str(tmp_path / "frame_info.json"), labels_path=str(tmp_path / which), max_objects=24)
        random.seed(11)
        loaded[which] = [fp.load(tok) for tok in tokens]
    ones = 0
    for a, b in zip(loaded["ours"], loaded["golden"]):
        assert np.array_equal(a["gt"], b["gt"]) and a["num_det_boxes"] == b["num_det_boxes"] and a["num_prev_det_boxes"] == b["num_prev_det_boxes"]
        ones += int(a["gt"].sum())
    assert ones > 100
    lab = np.load(str(tmp_path / "ours" / (tokens[0] + ".npz")), allow_pickle=True)
    assert lab["matched"].shape == () and lab["matched"].item() is None  # a first frame: `matched = None`, as the reference saves it


def test_frames_from_box_lists_give_the_same_labels():
    """gt_labels.frame: objects with .x .y .s and rows [x, y, ..., score] describe the same frame as the arrays."""
    from types import SimpleNamespace
    from shasta_amd import gt_labels
    scene = synth_scene(5, n_frames=4, not_emitted=(2,))
    want = gt_labels.scene_labels(scene, device=False)
    rows = [gt_labels.frame([[x, y, 0.0, s] for (x, y), s in zip(f["det_xy"], f["det_score"])], f["det_types"], [[x, y, 0.0] for x, y in f["gt_xy"]],
                            f["gt_types"], f["gt_ids"], emit=f["emit"]) for f in scene]
    objs = [gt_labels.frame([SimpleNamespace(x=x, y=y, s=s) for (x, y), s in zip(f["det_xy"], f["det_score"])], f["det_types"],
                            [SimpleNamespace(x=x, y=y, s=None) for x, y in f["gt_xy"]], f["gt_types"], f["gt_ids"], emit=f["emit"]) for f in scene]
    assert len(want) == 3 and want[0][0] is None and sum(int(m[:, :-2].sum()) for m, _ in want[1:]) > 10
    _same_labels(gt_labels.scene_labels(rows, device=False), want)
    _same_labels(gt_labels.scene_labels(objs, device=False), want)


def test_error_cases():
    from shasta_amd import gt_labels
    f = synth_scene(3, n_frames=2)
    with pytest.raises(NotImplementedError, match="3D-IOU"):
        gt_labels.associate([[0.0, 0.0]], ["vehicle.car"], [[0.0, 0.0, 0.5]], ["car"], 2.0, distance_type="3D-IOU")
    twice = [dict(f[0]), dict(f[1], gt_ids=[f[1]["gt_ids"][0]] * len(f[1]["gt_ids"]))]
    with pytest.raises(ValueError, match="list order"):
        gt_labels.scene_labels(twice, device=False)
    for key, bad in (("det_score", np.nan), ("det_xy", np.inf), ("gt_xy", np.nan)):
        arr = f[1][key].copy()
        arr.reshape(-1)[0] = bad
        with pytest.raises(ValueError, match="finite"):
            gt_labels.scene_labels([f[0], dict(f[1], **{key: arr})], device=False)
    with pytest.raises(ValueError, match="finite"):
        gt_labels.associate([[0.0, 0.0]], ["vehicle.car"], [[np.nan, 0.0, 0.5]], ["car"], 2.0)
    with pytest.raises(ValueError, match="previous"):
        gt_labels.scene_labels([dict(f[0], has_prev=True)], device=False)


def test_device_path_without_a_gpu_raises(monkeypatch):
    import torch
    from shasta_amd import gt_labels, hip
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(hip.ShastaHipError, match="GPU"):
        gt_labels.scene_labels(synth_scene(3, n_frames=2), device=True)


def test_capacity_is_refused_by_the_c_entry_before_any_launch():
    """No GPU needed: the size check comes first (null pointers would be the next complaint, a launch the last)."""
    from shasta_amd import gt_labels, hip
    lib = hip.load()
    assert (gt_labels.MAX_DET, gt_labels.MAX_GT) == (1024, 512)
    for max_det, max_gt in ((1025, 1), (1, 513)):
        assert lib.shasta_gt_labels_f64(*([None] * 9), 0, None, None, 1, 0, 0, max_det, max_gt, 2.0, None, None, None, None) == hip.E_UNSUPPORTED
        assert b"1024" in lib.shasta_last_error() and b"512" in lib.shasta_last_error()
    assert lib.shasta_gt_labels_f64(*([None] * 9), 0, None, None, 0, 0, 0, 1024, 512, 2.0, None, None, None, None) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_path_equals_the_reference_golden():
    _check_against_golden(device=True)


@pytest.mark.gpu
def test_one_launch_for_all_scenes_equals_scene_by_scene():
    from shasta_amd import gt_labels
    scenes, thr = _golden()
    names = list(scenes)
    together = gt_labels.split_labels([scenes[n][0] for n in names], thr, device=True)
    assert len(together) == len(names)
    for n, got in zip(names, together):
        _same_labels(got, gt_labels.scene_labels(scenes[n][0], thr, device=True))
        _same_labels(got, _want_labels(scenes[n][1]))


@pytest.mark.gpu
def test_device_equals_host_on_further_scenes_with_frames_left_out():
    from shasta_amd import gt_labels
    scenes = [synth_scene(2000 + s, quant=s % 2 == 0, skip_frac=0.2, half=40.0 if s < 6 else 8.0) for s in range(8)]
    left_out = sum(1 for sc in scenes for f in sc if not f["emit"])
    assert 8 <= left_out <= 40
    dev, host = gt_labels.split_labels(scenes, 2.0, device=True), gt_labels.split_labels(scenes, 2.0, device=False)
    for sc, d, h in zip(scenes, dev, host):
        assert len(d) == sum(1 for f in sc if f["emit"])
        _same_labels(d, h)
        assert gt_labels.frame_associations(sc, 2.0, device=True) == gt_labels.frame_associations(sc, 2.0, device=False)


@pytest.mark.gpu
def test_full_capacity_runs_and_one_more_is_refused():
    """1024 detections x 512 ground-truth boxes equals the host path; one more on either side raises before any kernel starts."""
    from shasta_amd import gt_labels, hip
    full = synth_scene(50, counts=[(1024, 512), (1000, 512)], half=60.0)
    _same_labels(gt_labels.scene_labels(full, 2.0, device=True), gt_labels.scene_labels(full, 2.0, device=False))
    for counts in ([(1025, 512)], [(1024, 513)]):
        with pytest.raises(hip.ShastaHipError, match="1024 detections and 512"):
            gt_labels.scene_labels(synth_scene(51, counts=counts, half=60.0), 2.0, device=True)
