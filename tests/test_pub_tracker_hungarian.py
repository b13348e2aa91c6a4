"""`hungarian=True` on the device: the per-frame trackers (distance kernel -> clip -> batched solver, csrc/lsap.hip), the whole-scene
kernel (shasta_track_merged_lsap_f64) and association's mode='bipartite' with device=True, against the reference's own Hungarian
output (the two tracker goldens hold it at max_age=2) and against the host paths.  scipy's solver is made to raise wherever the
device path is under test."""
import copy
import gzip
import json
import os
import random

import numpy as np
import pytest

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    with gzip.open(os.path.join(G, name), "rt") as f:
        return json.load(f)


def _snapshot(ret):
    return [dict(uid=t["uid"], tracking_id=int(t["tracking_id"]), age=int(t["age"]), active=int(t["active"]),
                 ref_detection_score=float(t["ref_detection_score"]), ct=[float(t["ct"][0]), float(t["ct"][1])]) for t in ret]


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g["uid"], g["tracking_id"], g["age"], g["active"]) == (w["uid"], w["tracking_id"], w["age"], w["active"])
        assert abs(g["ref_detection_score"] - w["ref_detection_score"]) <= 1e-12
        assert np.allclose(g["ct"], w["ct"], rtol=0, atol=1e-12)


def _hungarian_cases():
    """[(constructor arguments, expected[scene][frame], plain)]: the Hungarian case of either golden."""
    g, m = _load("pub_tracker_golden.json.gz"), _load("pub_tracker_merged_golden.json.gz")
    runs = [(case, g["expected"][ci], True) for ci, case in enumerate(g["cases"]) if case["hungarian"]]
    runs += [(case, m["expected"][ci], False) for ci, case in enumerate(m["cases"]) if case["hungarian"]]
    assert len(runs) == 2 and all(case["max_age"] == 2 for case, _, _ in runs)
    return g["scenes"], runs


@pytest.fixture
def no_scipy(monkeypatch):
    """The host solver raises: whatever passes under this fixture was solved on the device."""
    import scipy.optimize
    from shasta_amd import association

    def refuse(*a, **k):
        raise AssertionError("scipy.optimize.linear_sum_assignment was called: the assignment left the device")
    monkeypatch.setattr(scipy.optimize, "linear_sum_assignment", refuse)
    monkeypatch.setattr(association, "linear_sum_assignment", refuse)


def test_the_hungarian_goldens_are_a_workout():
    """CPU: with the greedy rule the oracle's frames differ from the Hungarian goldens in at least 10 of the 24 frames of either
    tracker - the goldens pin the solver, not only the bookkeeping around it."""
    from oracle import tracker_oracle as TO
    scenes, runs = _hungarian_cases()
    for case, expected, plain in runs:
        differ = frames_seen = 0
        for si, frames in enumerate(scenes):
            trk = (TO.PubTrackerOracle if plain else TO.PubTrackerMergedOracle)(**dict(case, hungarian=False))
            for fi, dets in enumerate(copy.deepcopy(frames)):
                got = [(t["uid"], int(t["tracking_id"]), int(t["age"]), int(t["active"])) for t in trk.step_centertrack(dets, 0.5)]
                want = [(t["uid"], t["tracking_id"], t["age"], t["active"]) for t in expected[si][fi]]
                differ += got != want
                frames_seen += 1
        assert frames_seen == 24 and differ >= 10, (case, differ)


@pytest.mark.gpu
def test_per_frame_trackers_equal_the_reference_hungarian_output(no_scipy):
    from shasta_amd.pub_tracker import PubTracker, PubTrackerMerged, step_batch, step_batch_merged
    scenes, runs = _hungarian_cases()
    for case, expected, plain in runs:
        cls, batch = (PubTracker, step_batch) if plain else (PubTrackerMerged, step_batch_merged)
        for si, frames in enumerate(scenes):
            trk = cls(**case)
            for fi, dets in enumerate(copy.deepcopy(frames)):
                _same(_snapshot(trk.step_centertrack(dets, 0.5)), expected[si][fi])
        trackers = [cls(**case) for _ in scenes]
        work = copy.deepcopy(scenes)
        for fi in range(len(work[0])):
            outs = batch(trackers, [s[fi] for s in work], [0.5] * len(work))
            for si, ret in enumerate(outs):
                _same(_snapshot(ret), expected[si][fi])


@pytest.mark.gpu
def test_whole_scene_kernel_equals_the_reference_hungarian_output(no_scipy):
    from shasta_amd.pub_tracker import track_scenes_merged_device
    scenes, runs = _hungarian_cases()
    checked = 0
    for case, expected, plain in runs:
        work = copy.deepcopy(scenes)
        keep = copy.deepcopy(work)
        kw = dict(refine_confidence=case["refine_confidence"], alpha=case.get("alpha", 0.5), beta=case.get("beta", 0.5)) if plain else {}
        res = track_scenes_merged_device([[(dets, 0.5) for dets in frames] for frames in work], max_age=case["max_age"], plain=plain,
                                         hungarian=True, **kw)
        assert work == keep  # the kernel path leaves the detection dicts alone
        for si, frames in enumerate(res):
            assert frames is not None
            for fi, rows in enumerate(frames):
                want = [t for t in expected[si][fi] if t["active"] > 0]
                assert [(d["uid"], tid) for d, tid, _ in rows] == [(t["uid"], t["tracking_id"]) for t in want], (case, si, fi)
                for (_, _, sc), t in zip(rows, want):
                    assert abs(sc - t["ref_detection_score"]) <= 1e-12
                checked += len(rows)
    assert checked > 400


@pytest.mark.gpu
@pytest.mark.parametrize("merged", [True, False])
@pytest.mark.parametrize("max_age", [0, 2])
def test_run_tracking_whole_scenes_equals_the_per_frame_hungarian_path(tmp_path, no_scipy, merged, max_age):
    from shasta_amd import pipeline, scenes
    paths, sc = scenes.write_synthetic_split(str(tmp_path), n_scenes=4, frames_per_scene=[8, 2, 11, 5], seed=33, drop=0.3, clutter=3)
    meta = json.load(open(paths["frames_meta_path"]))["frames"]
    rnd = random.Random(8)
    preds = {}
    for _, toks in sc:
        for t in toks:
            rows = json.load(open(os.path.join(paths["cls_info_path"], t + ".json")))
            for d in rows:
                d["ref_detection_score"] = rnd.random()
                if rnd.random() < 0.25:
                    d["newborn"] = True
                if rnd.random() < 0.25:
                    d["dead"] = True
            preds[t] = rows
    preds[sc[2][1][4]] = []  # an empty frame drops every track
    kw = dict(max_age=max_age, merged=merged, hungarian=True)
    keep = copy.deepcopy(preds)
    fast = pipeline.run_tracking(preds, meta, whole_scenes=True, **kw)
    assert preds == keep
    slow = pipeline.run_tracking(copy.deepcopy(preds), meta, **kw)
    assert fast == slow and sum(len(v) for v in fast["results"].values()) > 50
    # capacity: 513 detections in one frame -> the per-frame path serves the call, same contract
    big = copy.deepcopy(preds)
    tok = sc[0][1][2]
    big[tok] = [dict(big[tok][0], translation=[float(i), 0.0, 0.0]) for i in range(513)]
    ref = pipeline.run_tracking(copy.deepcopy(big), meta, **kw)
    keep = copy.deepcopy(big)
    assert pipeline.run_tracking(big, meta, whole_scenes=True, **kw) == ref and big == keep


@pytest.mark.gpu
@pytest.mark.parametrize("asso", ["iou", "giou", "euler", "m_dis", "affinity"])
def test_bipartite_association_on_the_device_equals_the_host_solver(monkeypatch, asso):
    import scipy.optimize
    from shasta_amd import association as A
    rng = np.random.default_rng(11)
    host_solver = A.linear_sum_assignment
    for nd, nt in ((7, 5), (5, 7), (70, 66)):
        base = np.concatenate([rng.uniform(-30, 30, (max(nd, nt), 2)), rng.uniform(-1, 1, (max(nd, nt), 1)), rng.uniform(-3, 3, (max(nd, nt), 1)),
                               rng.uniform(1.5, 4.5, (max(nd, nt), 1)), rng.uniform(1.0, 2.0, (max(nd, nt), 2))], axis=1)
        dets = list(base[:nd])
        trks = list((base + rng.normal(0, 0.15, base.shape) * np.array([1, 1, 1, 0.2, 0.2, 0.2, 0.2]))[rng.permutation(max(nd, nt))[:nt]])
        inn = None
        if asso == "m_dis":
            inn = []
            for _ in range(nt):
                a = rng.normal(size=(7, 7))
                inn.append(a @ a.T + 7 * np.eye(7))
        aff = rng.uniform(0, 1, (nt + 2, nd + 3)) if asso == "affinity" else None
        args = (dets, trks, "bipartite", asso)
        kw = dict(dist_threshold=0.9, trk_innovation_matrix=inn, affinity=aff)
        want = A.associate_dets_to_tracks(*args, **kw)

        def refuse(*a, **k):
            raise AssertionError("the host solver was called with device=True")
        monkeypatch.setattr(A, "linear_sum_assignment", refuse)
        monkeypatch.setattr(scipy.optimize, "linear_sum_assignment", refuse)
        got = A.associate_dets_to_tracks(*args, device=True, **kw)
        monkeypatch.setattr(A, "linear_sum_assignment", host_solver)
        monkeypatch.setattr(scipy.optimize, "linear_sum_assignment", host_solver)
        assert len(got[0]) == len(want[0]) and all(np.array_equal(a, b) for a, b in zip(got[0], want[0]))
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert len(want[0]) + len(want[1]) == nd
