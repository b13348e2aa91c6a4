"""CPU tests of the host-side mirror: decode loop, association surface, scene sharding + 2-process gloo gather."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import shasta_oracle as O
from shasta_amd import association as A
from shasta_amd import decode as Dm
from shasta_amd import replica


def _boxes(n, tag):
    return [dict(sample_token=tag, translation=[float(i), float(-i), 0.5], size=[2, 4, 1.5], rotation=[1, 0, 0, 0],
                 velocity=[0.5 * i, -0.25 * i], detection_name="car", detection_score=0.5 + 0.01 * i) for i in range(n)]


def _known_answer_matrices(N=6, n_prev=4, n_cur=3):
    """Hand-built matrices: prev0->det1 match, prev1 dead (0.9), prev2 FN (0.8), prev3 weak; det0 newborn (0.6),
    det2 FP (0.75)."""
    m1 = np.full((N, N + 2), 0.01, np.float32)
    m1[0, 1] = 0.9
    m1[1, N] = 0.9       # dead column  (index -2)
    m1[2, N + 1] = 0.8   # FN column    (index -1)
    m1[3, 0] = 0.3
    m2 = np.full((N + 2, N), 0.01, np.float32)
    m2[0, 1] = 0.9
    m2[N, 0] = 0.6       # newborn row (index -2)
    m2[N + 1, 2] = 0.75  # FP row      (index -1)
    return m1, m2


def test_decode_known_answer():
    m1, m2 = _known_answer_matrices()
    cur, prev = _boxes(3, "t1"), _boxes(4, "t0")
    annos, dead_prev, keep = Dm.decode_frame(m1, m2, cur, prev, "t1", 0.5)
    assert dead_prev == [1]
    assert keep == [0, 1]                      # det2 dropped as FP
    assert cur[0].get("newborn") is True and "newborn" not in cur[1]
    assert annos[0] is cur[0] and annos[1] is cur[1]
    fn = annos[2]                              # the propagated previous box comes last
    assert fn is prev[2] and fn["FN"] is True and fn["token"] == "t1"
    assert fn["translation"][:2] == [2.0 + 0.5 * 1.0, -2.0 + 0.5 * -0.5]
    assert abs(fn["ref_detection_score"] - (1 - 0.01)) < 1e-6
    assert abs(cur[0]["ref_detection_score"] - (1 - 0.01)) < 1e-6


def test_decode_matches_oracle_on_random_matrices():
    rng = np.random.default_rng(0)
    for trial in range(20):
        N = 8
        n_prev, n_cur = int(rng.integers(0, N + 1)), int(rng.integers(0, N + 1))
        m1 = rng.dirichlet(np.full(N + 2, 0.15), size=N).astype(np.float32)
        m2 = rng.dirichlet(np.full(N + 2, 0.15), size=N).astype(np.float32).T.copy()
        c1, p1, c2, p2 = _boxes(n_cur, "a"), _boxes(n_prev, "b"), _boxes(n_cur, "a"), _boxes(n_prev, "b")
        got = Dm.decode_frame(torch.from_numpy(m1), torch.from_numpy(m2), c1, p1, "tok", 0.5)
        ref = O.decode_frame(m1, m2, c2, p2, "tok", 0.5)
        assert got[1] == ref[1] and got[2] == ref[2] and got[0] == ref[0]


def test_decoder_dead_postpass_and_empty_frames():
    dec = Dm.AffinityDecoder()
    m1, m2 = _known_answer_matrices()
    f0 = dict(metadata=[{"token": "t0"}], prev_metadata=[{"token": "none"}], cls_det_boxes=[_boxes(4, "t0")],
              prev_cls_det_boxes=[[]], prev_det_boxes=torch.zeros(1, 6, 11))
    e = np.full((6, 8), 1 / 8, np.float32)
    dec.add(e[None], np.full((8, 6), 1 / 8, np.float32)[None], f0)
    pb = torch.zeros(1, 6, 11)
    pb[0, 0, 9] = 0.5
    f1 = dict(metadata=[{"token": "t1"}], prev_metadata=[{"token": "t0"}], cls_det_boxes=[_boxes(3, "t1")],
              prev_cls_det_boxes=[_boxes(4, "t0")], prev_det_boxes=pb)
    dec.add(m1[None], m2[None], f1)
    out = dec.finalize()
    assert out["results"]["t0"][1].get("dead") is True      # prev index 1 was kept in frame t0 and died in t1
    assert all("dead" not in a for i, a in enumerate(out["results"]["t0"]) if i != 1)
    assert out["meta"]["use_lidar"] is True


def test_association_affinity_and_euler_modes():
    rng = np.random.default_rng(1)
    dets = [rng.normal(size=7) for _ in range(5)]
    trks = [d + rng.normal(scale=0.01, size=7) for d in dets[:4]][::-1]
    m, ud, ut = A.associate_dets_to_tracks(dets, trks, "greedy", "euler", dist_threshold=0.5)
    assert sorted((int(a), int(b)) for a, b in m) == [(0, 3), (1, 2), (2, 1), (3, 0)]
    assert list(ud) == [4] and len(ut) == 0
    m2, _, _ = A.associate_dets_to_tracks(dets, trks, "bipartite", "euler", dist_threshold=0.5)
    assert sorted((int(a), int(b)) for a, b in m2) == [(0, 3), (1, 2), (2, 1), (3, 0)]
    aff = np.full((6, 8), 0.02)
    aff[0, 2], aff[1, 0], aff[2, 1] = 0.9, 0.8, 0.05  # tracks are rows of matched1, detections columns
    m3, ud3, ut3 = A.associate_dets_to_tracks(dets[:3], trks[:3], "greedy", "affinity", dist_threshold=0.5, affinity=aff)
    assert sorted((int(a), int(b)) for a, b in m3) == [(0, 1), (2, 0)]
    assert sorted(int(x) for x in ud3) == [1] and sorted(int(x) for x in ut3) == [2]
    if not torch.cuda.is_available():  # the IoU modes run on the GPU only: loud failure on a CPU-only box
        from shasta_amd import hip
        with pytest.raises(hip.ShastaHipError):
            A.associate_dets_to_tracks(dets, trks, "greedy", "iou")


def test_association_matches_reference_module():
    """Against the reference's mot_3d.association on seeded boxes (tests/golden/association_golden.json, made by
    tests/golden/make_association_golden.py): the same matches and unmatched lists, in the same order."""
    import json
    from types import SimpleNamespace
    with open(os.path.join(os.path.dirname(__file__), "golden", "association_golden.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) == 4

    def bbox(a):  # the attributes mot_3d's BBox.array2bbox sets
        return SimpleNamespace(**dict(zip(("x", "y", "z", "o", "l", "w", "h"), a)))
    for c in cases:
        dets, trks = [bbox(d) for d in c["dets"]], [bbox(t) for t in c["trks"]]
        inn = None if c["innovation"] is None else [np.array(m, np.float64) for m in c["innovation"]]
        g = A.associate_dets_to_tracks(dets, trks, c["mode"], c["asso"], c["dist_threshold"], inn)
        assert [tuple(x) for x in c["matches"]] == [tuple(int(v) for v in x) for x in g[0]], (c["mode"], c["asso"])
        assert c["unmatched_dets"] == [int(v) for v in g[1]] and c["unmatched_trks"] == [int(v) for v in g[2]], (c["mode"], c["asso"])


def test_shard_scenes_is_a_balanced_partition():
    scenes = [("s%d" % i, 35 + (i * 7) % 9) for i in range(150)]
    parts = [replica.shard_scenes(scenes, r, 8) for r in range(8)]
    assert sorted(sum(parts, [])) == sorted(s for s, _ in scenes)
    loads = [sum(dict(scenes)[s] for s in p) for p in parts]
    assert max(loads) - min(loads) <= 43
    assert replica.shard_scenes(scenes, 0, 1) == [s for s, _ in scenes]


def _gloo_worker(rank, world, port, out_path):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    scenes = [("scene%d" % i, 2) for i in range(4)]
    mine = replica.shard_scenes(scenes, rank, world)
    dec = Dm.AffinityDecoder()
    m1, m2 = _known_answer_matrices()
    for s in mine:  # two frames per scene: t0 (no prev), t1
        e = np.full((6, 8), 1 / 8, np.float32)
        f0 = dict(metadata=[{"token": s + "_t0"}], prev_metadata=[{"token": "none"}], cls_det_boxes=[_boxes(4, s)],
                  prev_cls_det_boxes=[[]], prev_det_boxes=torch.zeros(1, 6, 11))
        dec.add(e[None], np.full((8, 6), 1 / 8, np.float32)[None], f0)
        pb = torch.zeros(1, 6, 11)
        pb[0, 0, 9] = 0.5
        f1 = dict(metadata=[{"token": s + "_t1"}], prev_metadata=[{"token": s + "_t0"}], cls_det_boxes=[_boxes(3, s)],
                  prev_cls_det_boxes=[_boxes(4, s)], prev_det_boxes=pb)
        dec.add(m1[None], m2[None], f1)
    out = replica.gather_decoded(dec, dst=0)
    if rank == 0:
        torch.save(out, out_path)
    else:
        assert out is None
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gloo_gather_equals_single_process(tmp_path):
    import torch.multiprocessing as mp
    port = 29500 + (os.getpid() % 2000)
    out_path = str(tmp_path / "merged.pt")
    mp.spawn(_gloo_worker, args=(2, port, out_path), nprocs=2, join=True)
    merged = torch.load(out_path, weights_only=False)
    # single-process run over all scenes
    dec = Dm.AffinityDecoder()
    m1, m2 = _known_answer_matrices()
    for s in ["scene%d" % i for i in range(4)]:
        e = np.full((6, 8), 1 / 8, np.float32)
        f0 = dict(metadata=[{"token": s + "_t0"}], prev_metadata=[{"token": "none"}], cls_det_boxes=[_boxes(4, s)],
                  prev_cls_det_boxes=[[]], prev_det_boxes=torch.zeros(1, 6, 11))
        dec.add(e[None], np.full((8, 6), 1 / 8, np.float32)[None], f0)
        pb = torch.zeros(1, 6, 11)
        pb[0, 0, 9] = 0.5
        f1 = dict(metadata=[{"token": s + "_t1"}], prev_metadata=[{"token": s + "_t0"}], cls_det_boxes=[_boxes(3, s)],
                  prev_cls_det_boxes=[_boxes(4, s)], prev_det_boxes=pb)
        dec.add(m1[None], m2[None], f1)
    single = dec.finalize()
    assert merged["results"].keys() == single["results"].keys()
    for k in single["results"]:
        assert merged["results"][k] == single["results"][k]
    assert any(a.get("dead") for a in merged["results"]["scene3_t0"])


def test_scene_runs_split_where_a_frame_does_not_follow_its_predecessor():
    """pipeline._scene_runs: runs are consecutive frames of one scene; a token list that skips a frame, or a frame whose `prev` is not part
    of the split (eval.py falls back to the frame itself), starts a new run instead of raising - with or without `python -O`."""
    from shasta_amd import pipeline
    info = {"a": {"prev": ""}, "b": {"prev": "a"}, "c": {"prev": "b"}, "d": {"prev": "c"}, "e": {"prev": "d"}, "f": {"prev": "zz"}, "g": {"prev": "f"}}
    scenes = [("s0", ["a", "b", "d", "e", "f", "g"]), ("s1", ["c"])]
    known = {"a", "b", "c", "d", "e", "f", "g"}
    runs = list(pipeline._scene_runs(scenes, {"s0", "s1"}, known, info, 8))
    assert runs == [[("a", ""), ("b", "a")], [("d", "c"), ("e", "d")], [("f", ""), ("g", "f")], [("c", "b")]]
    for run in runs:  # the invariant the stacked maps rely on
        assert all(run[j][1] == run[j - 1][0] for j in range(1, len(run)))
    # the run length is still capped, and scenes of other ranks are skipped
    assert [len(r) for r in pipeline._scene_runs([("s", list("abc"))], {"s"}, known, info, 2)] == [2, 1]
    assert list(pipeline._scene_runs(scenes, {"s1"}, known, info, 8)) == [[("c", "b")]]
