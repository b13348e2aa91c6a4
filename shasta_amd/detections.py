"""From the head's output to the per-frame detection files `frames.FramePairs` reads: the last link between a point cloud and `det_boxes`.

A detection dict is `CenterHead.predict`'s `{box3d_lidar (n, 9) [x, y, z, w, l, h, vx, vy, rot], scores, label_preds, metadata}` - the dict
det3d/datasets/nuscenes/nusc_common.py:160-178 (`_second_det_to_nusc_box`) takes.  `sensor_rows` makes the 13-float rows of
`<det_path>/<token>.json` (frames.py:5-9): `[x, y, z, w, l, h, qw, qx, qy, qz, vx, vy, score]` in the LiDAR frame with
`yaw = -rot - pi/2` (nusc_common.py:164) and `q = [cos(yaw/2), 0, 0, sin(yaw/2)]` (pyquaternion's `Quaternion(axis=[0, 0, 1], radians=yaw)`),
and the class dicts of `<cls_info_path>/<token>.json` (`sample_token`, `detection_name`, `detection_score`).  The fp32 values are widened
to float64 exactly; the yaw and the quaternion are computed in float64.  Nothing in frames.py or pipeline.py changes: the files are the
interface."""
import json
import math
import os

import numpy as np
import torch


def _np(v, dtype):
    if torch.is_tensor(v):
        v = v.detach().cpu().numpy()
    return np.asarray(v, dtype=dtype)


def sensor_rows(det, class_names, token=None):
    """-> (rows: list of 13-float lists, class dicts).  `class_names`: the flat list of names `label_preds` indexes (the tasks' names in
    task order).  `token` defaults to det["metadata"]["token"] when there is one, else ""."""
    box = _np(det["box3d_lidar"], np.float64).reshape(-1, 9)
    scores = _np(det["scores"], np.float64).reshape(-1)
    labels = _np(det["label_preds"], np.int64).reshape(-1)
    if token is None:
        meta = det.get("metadata")
        token = meta.get("token", "") if isinstance(meta, dict) else ""
    rows, cls = [], []
    for b, s, l in zip(box, scores, labels):
        yaw = -float(b[8]) - math.pi / 2
        rows.append([float(b[0]), float(b[1]), float(b[2]), float(b[3]), float(b[4]), float(b[5]), math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2),
                     float(b[6]), float(b[7]), float(s)])
        cls.append(dict(sample_token=token, detection_name=class_names[int(l)], detection_score=float(s)))
    return rows, cls


def write_frame_files(det, token, det_dir, cls_dir, class_names):
    """Write `<det_dir>/<token>.json` and `<cls_dir>/<token>.json` for one frame; returns the number of detections."""
    rows, cls = sensor_rows(det, class_names, token=token)
    os.makedirs(det_dir, exist_ok=True)
    os.makedirs(cls_dir, exist_ok=True)
    with open(os.path.join(det_dir, token + ".json"), "w") as f:
        json.dump(rows, f)
    with open(os.path.join(cls_dir, token + ".json"), "w") as f:
        json.dump(cls, f)
    return len(rows)


class DetectedFrames:
    """Detection files of frames from their point clouds: `model` a detector (detector.VoxelNet) in eval mode whose forward takes
    dict(points=[...]) and returns one detection dict per cloud; `clouds` as in `bevmap.CloudMaps` (sweeps.SweepClouds: `batch(tokens,
    device)`, or a callable token -> (P, ndim) array or tensor).  `write(tokens, det_dir, cls_dir, device)` runs the tokens through the
    model in groups of at most `max_clouds` and writes both files per token; returns {token: number of detections}."""

    def __init__(self, model, clouds, class_names=None, max_clouds=8):
        if max_clouds < 1:
            raise ValueError("DetectedFrames: max_clouds must be at least 1")
        self.model, self.clouds, self.max_clouds = model, clouds, int(max_clouds)
        if class_names is None:
            class_names = [n for names in model.bbox_head.class_names for n in names]
        self.class_names = list(class_names)

    def _cloud(self, token, device):
        c = self.clouds(token)
        if not torch.is_tensor(c):
            c = torch.from_numpy(np.ascontiguousarray(c, np.float32))
        return c.to(device=device, dtype=torch.float32)

    def write(self, tokens, det_dir, cls_dir, device="cuda"):
        if self.model.training:
            raise RuntimeError("DetectedFrames: the model must be in eval() mode")
        done = {}
        with torch.no_grad():
            for i in range(0, len(tokens), self.max_clouds):
                group = list(tokens[i:i + self.max_clouds])
                pts = list(self.clouds.batch(group, device)) if hasattr(self.clouds, "batch") else [self._cloud(t, device) for t in group]
                dets = self.model(dict(points=pts, metadata=[dict(token=t) for t in group]))
                for t, det in zip(group, dets):
                    done[t] = write_frame_files(det, t, det_dir, cls_dir, self.class_names)
        return done
