"""From the head's detection dicts to the per-frame files `frames.FramePairs` reads (shasta_amd/detections.py)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from shasta_amd import detections, frames

NAMES = ["car", "truck", "construction_vehicle", "bus", "trailer", "barrier", "motorcycle", "bicycle", "pedestrian", "traffic_cone"]


def _det(n, seed, token="tok"):
    g = torch.Generator().manual_seed(seed)
    box = torch.randn(n, 9, generator=g)
    box[:, 3:6] = 0.5 + 4.0 * torch.rand(n, 3, generator=g)
    box[:, 8] = (torch.rand(n, generator=g) * 2 - 1) * math.pi
    if n >= 4:  # yaw = -rot - pi/2 at the ends of the range and across the wrap
        box[:4, 8] = torch.tensor([math.pi, -math.pi, math.pi / 2, -math.pi / 2 + 1e-3])
    return dict(box3d_lidar=box, scores=torch.rand(n, generator=g), label_preds=torch.randint(len(NAMES), (n,), generator=g), metadata=dict(token=token))


def _wrap(a):  # into (-pi, pi]
    return math.pi - ((math.pi - a) % (2 * math.pi))


def test_sensor_rows_through_det_rows():
    det = _det(12, 1)
    rows, cls = detections.sensor_rows(det, NAMES)
    assert len(rows) == len(cls) == 12 and all(len(r) == 13 and all(type(v) is float for v in r) for r in rows)
    assert [c["detection_name"] for c in cls] == [NAMES[i] for i in det["label_preds"].tolist()] and {c["sample_token"] for c in cls} == {"tok"}
    box, sc = det["box3d_lidar"].double().numpy(), det["scores"].double().numpy()
    out, keep, kept_cls, n = frames.det_rows(rows, cls, None, 0.5, 20)
    assert n == 12 and keep == list(range(12)) and kept_cls == cls
    assert np.array_equal(out[:12, :6], box[:, :6]) and np.array_equal(out[:12, 7:9], box[:, 6:8]) and np.array_equal(out[:12, 10], sc)  # exact
    assert bool((out[:12, 9] == 0.5).all()) and bool((out[12:] == 0).all())
    for i in range(12):
        assert abs(out[i, 6] - _wrap(-box[i, 8] - math.pi / 2)) <= 1e-12, i
        assert -math.pi < out[i, 6] <= math.pi
    q = np.array(rows)[:, 6:10]
    assert np.allclose((q ** 2).sum(1), 1.0, atol=1e-15) and bool((q[:, 1:3] == 0).all())
    assert [c["detection_score"] for c in cls] == sc.tolist()
    # det_type filtering goes through the class dicts
    want = [i for i, l in enumerate(det["label_preds"].tolist()) if NAMES[l] in ("car", "bus")]
    _, keep2, kept2, n2 = frames.det_rows(rows, cls, ["car", "bus"], 0.5, 20)
    assert keep2 == want and n2 == len(want) and all(c["detection_name"] in ("car", "bus") for c in kept2)
    # an empty detection dict gives empty lists
    assert detections.sensor_rows(_det(0, 2), NAMES) == ([], [])
    assert detections.sensor_rows(dict(det, metadata=None), NAMES, token="x")[1][0]["sample_token"] == "x"


def test_written_files_load_through_frame_pairs(tmp_path):
    det_dir, cls_dir = str(tmp_path / "det"), str(tmp_path / "cls")
    dets = {"a": _det(7, 3, "a"), "b": _det(0, 4, "b"), "c": _det(5, 5, "c")}
    for tok, d in dets.items():
        assert detections.write_frame_files(d, tok, det_dir, cls_dir, NAMES) == d["scores"].shape[0]
    info = {"a": dict(prev="", timestamp=1000000), "b": dict(prev="a", timestamp=1500000, prev_timestamp=1000000),
            "c": dict(prev="b", timestamp=2000000, prev_timestamp=1500000)}
    fi = str(tmp_path / "frame_info.json")
    with open(fi, "w") as f:
        json.dump(info, f)
    fp = frames.FramePairs(det_dir, cls_dir, fi, max_objects=10, test_mode=True)
    c = fp.load("c")
    assert c["num_det_boxes"] == 5 and c["num_prev_det_boxes"] == 0 and len(c["cls_det_boxes"]) == 5
    want = dets["c"]["box3d_lidar"].double().numpy()
    assert np.array_equal(c["det_boxes"][:5, :6], want[:, :6]) and np.array_equal(c["det_boxes"][:5, 7:9], want[:, 6:8])
    assert np.array_equal(c["det_boxes"][:5, 10], dets["c"]["scores"].double().numpy()) and np.allclose(c["det_boxes"][:5, 9], 0.5)
    b = fp.load("b")
    assert b["num_det_boxes"] == 0 and b["num_prev_det_boxes"] == 7
    assert np.array_equal(b["prev_det_boxes"][:7, :3], dets["a"]["box3d_lidar"].double().numpy()[:, :3])
    assert sorted(os.listdir(det_dir)) == ["a.json", "b.json", "c.json"] == sorted(os.listdir(cls_dir))


class _FakeHead:
    class_names = [["car"], ["bus", "trailer"]]


class _FakeModel:
    training = False
    bbox_head = _FakeHead()

    def __call__(self, example):
        return [dict(_det(int(p.shape[0]), 9, m["token"]), label_preds=torch.arange(int(p.shape[0])) % 3) for p, m in zip(example["points"], example["metadata"])]


def test_detected_frames_groups_tokens_and_writes_every_file(tmp_path):
    clouds = {"t%d" % i: np.zeros((i + 1, 5), np.float32) for i in range(5)}
    df = detections.DetectedFrames(_FakeModel(), clouds.__getitem__, max_clouds=2)
    assert df.class_names == ["car", "bus", "trailer"]
    done = df.write(list(clouds), str(tmp_path / "d"), str(tmp_path / "c"), device="cpu")
    assert done == {"t%d" % i: i + 1 for i in range(5)}
    with open(str(tmp_path / "c" / "t3.json")) as f:
        assert [c["detection_name"] for c in json.load(f)] == ["car", "bus", "trailer", "car"]
    with pytest.raises(ValueError):
        detections.DetectedFrames(_FakeModel(), clouds.__getitem__, max_clouds=0)


@pytest.mark.gpu
def test_detected_frames_on_the_detector(tmp_path):
    """Point clouds -> VoxelNet on the kernels -> files -> FramePairs rows."""
    import shasta_amd
    from shasta_amd.backbone import SpMiddleResNetFHD
    from tests import head_helpers as HH
    dev = torch.device("cuda", 0)
    torch.manual_seed(81)
    cfg = dict(HH.TEST_CFG, pc_range=[-13.5, -13.5], voxel_size=[0.5625, 0.5625], score_threshold=0.05)
    m = shasta_amd.build_detector(dict(
        type="VoxelNet", reader=dict(type="DynamicVoxelEncoder", pc_range=[-13.5, -13.5, -5, 13.5, 13.5, 3], voxel_size=[0.5625, 0.5625, 0.2]),
        backbone=dict(type=SpMiddleResNetFHD, num_input_features=5, ds_factor=8),
        neck=dict(type="RPN", layer_nums=[1, 1], ds_layer_strides=[1, 2], ds_num_filters=[32, 64], us_layer_strides=[1, 2], us_num_filters=[32, 32],
                  num_input_features=256),
        bbox_head=dict(type="CenterHead", in_channels=[64], tasks=HH.TWO_TASKS)), test_cfg=cfg).eval().to(dev)
    with torch.no_grad():
        for t in m.bbox_head.tasks:
            t.hm[3].bias.fill_(0.0)
    g = torch.Generator().manual_seed(82)
    clouds = {}
    for tok in ("p", "q", "r"):
        pts = (torch.rand(600, 3, generator=g) - 0.5) * torch.tensor([24.0, 24.0, 6.0]) + torch.tensor([0.0, 0.0, -1.0])
        clouds[tok] = torch.cat([pts, torch.rand(600, 2, generator=g)], 1).numpy()
    df = detections.DetectedFrames(m, clouds.__getitem__, max_clouds=2)
    done = df.write(["p", "q", "r"], str(tmp_path / "d"), str(tmp_path / "c"), device=dev)
    assert set(done) == {"p", "q", "r"} and all(v > 0 for v in done.values())
    fi = str(tmp_path / "fi.json")
    with open(fi, "w") as f:
        json.dump({"q": dict(prev="p", timestamp=500000, prev_timestamp=0)}, f)
    out = frames.FramePairs(str(tmp_path / "d"), str(tmp_path / "c"), fi, max_objects=600, test_mode=True).load("q")
    assert out["num_det_boxes"] == done["q"] and out["num_prev_det_boxes"] == done["p"]
    with torch.no_grad():
        direct = m(dict(points=[torch.from_numpy(clouds["q"]).to(dev)], metadata=[dict(token="q")]))[0]
    assert direct["scores"].shape[0] == done["q"]
    assert np.allclose(out["det_boxes"][:done["q"], :6], direct["box3d_lidar"][:, :6].cpu().double().numpy(), atol=1e-3)
