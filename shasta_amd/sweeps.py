"""Multi-sweep cloud assembly on the device: sweep files -> the reader's input (csrc/sweeps.hip).

Mirror of det3d/datasets/pipelines/loading.py:45-69,111-148 (`LoadPointCloudFromFile`, the nuScenes branch) and of the point half of
det3d/datasets/pipelines/preprocess.py:28-158 (`Preprocess`).  The host reads the files and draws the random numbers, in the
reference's order from the global numpy stream (`np.random.seed(s)` reproduces the reference's sweep order, augmentation parameters
and shuffle); every per-point step - column cut, close-point filter, float64 transform, time column, concatenation, flips, rotation,
scaling, translation - is one call of `shasta_sweeps_assemble_f32`.  The result equals the reference's bit for bit, except through a
rotation by a non-zero angle, which the reference leaves to its BLAS.

  * `assemble_clouds(infos, nsweeps, device)` - up to 32 frames in one call: all files into one reused pinned buffer, one
    host-to-device copy, one kernel chain, one host read (the n + 1 prefix words).  Returns `(points, offsets)`, the form
    `dynamic_voxelize` and `points_to_voxel_batch_device` take.
  * `LoadPointCloudFromFile`, `Preprocess` - registered in `registry.PIPELINES` with the reference's `__call__(res, info)` contract.
  * `SweepClouds` - a `clouds` object for `bevmap.CloudMaps` (which calls its `batch`).

Deviations, all deliberate:
  * the reference's hard-coded `.replace('tsadja', 'ubuntu')` on every path is not copied: pass `path_map`, a callable str -> str.
  * `WaymoDataset`, `res["virtual"]`, a `db_sampler` and `min_points_in_gt > 0` raise NotImplementedError.
  * `Preprocess` works on the ground-truth boxes only when res["lidar"]["annotations"] is present (targets.py applies the drawn entry
    to them); without annotations it handles the points alone, as the tracker's pipeline needs.
There is no CPU path: CPU use raises ShastaHipError."""
import ctypes as C
import os

import numpy as np
import torch

from . import hip
from .registry import PIPELINES

ROWS_PER_BLOCK = 256  # include/shasta_hip.h SHASTA_SWEEPS_BLOCK_ROWS
MAX_CLOUDS = 32       # SHASTA_SWEEPS_MAX_CLOUDS
MAX_SEGMENTS = 1024   # SHASTA_SWEEPS_MAX_SEGMENTS
SWEEP_TRANSFORM, SWEEP_DROP_CLOSE = 1, 2
AUG_NEG_Y, AUG_NEG_X, AUG_TRANSLATE = 1, 2, 4
RAW_NDIM, KEEP = 5, 4   # read_file: (n, 5) float32 rows, the first four columns are kept
CLOSE_RADIUS = 1.0      # read_sweep: min_distance


class Segment(C.Structure):
    """shasta_sweep_segment"""
    _fields_ = [("rows", C.c_int32), ("cloud", C.c_int32), ("flags", C.c_int32), ("reserved", C.c_int32),
                ("transform", C.c_double * 12), ("time_lag", C.c_double)]


class Augment(C.Structure):
    """shasta_sweep_augment"""
    _fields_ = [("flags", C.c_int32), ("c", C.c_float), ("s", C.c_float), ("reserved", C.c_int32), ("scale", C.c_double),
                ("translate", C.c_double * 3)]


def segment_table(segments):
    """segments: sequence of (rows, cloud, transform, drop_close, time_lag); transform None or an array whose first three rows are
    the 3 x 4 float64 matrix (a 4 x 4 `transform_matrix` as the info files hold it).  -> ctypes array of `Segment`."""
    table = (Segment * max(len(segments), 1))()
    for g, (rows, cloud, transform, drop, lag) in zip(table, segments):
        g.rows, g.cloud, g.time_lag = int(rows), int(cloud), float(lag)
        g.flags = (SWEEP_DROP_CLOSE if drop else 0) | (SWEEP_TRANSFORM if transform is not None else 0)
        if transform is not None:
            g.transform[:] = np.asarray(transform, np.float64)[:3, :4].reshape(-1).tolist()
    return table


def augment_entry(flip_x=False, flip_y=False, angle=0.0, scale=1.0, translate=None):
    """One cloud's augmentation as the reference applies it to fp32 points.  flip_x / flip_y are `random_flip_both`'s two draws ("x
    flip" negates y, "y flip" negates x); c, s are rounded to fp32 as `rotation_points_single_angle` rounds its matrix; the scale is
    rounded to fp32 (`points[:, :3] *= noise_scale` multiplies in fp32); `translate` is a float64 triple or None (step skipped)."""
    return dict(flip_x=bool(flip_x), flip_y=bool(flip_y), angle=float(angle), c=float(np.float32(np.cos(angle))),
                s=float(np.float32(np.sin(angle))), scale=float(np.float32(scale)),
                translate=None if translate is None else [float(v) for v in np.asarray(translate, np.float64).reshape(-1)[:3]])


def augment_table(entries, n):
    """entries: None, or n items of `augment_entry` (None = identity) -> ctypes array of `Augment`, or None."""
    if entries is None:
        return None
    if len(entries) != n:
        raise ValueError("sweeps: one augmentation entry per cloud (%d for %d clouds)" % (len(entries), n))
    table = (Augment * n)()
    for a, e in zip(table, entries):
        e = e or augment_entry()
        a.flags = (AUG_NEG_Y if e["flip_x"] else 0) | (AUG_NEG_X if e["flip_y"] else 0) | (AUG_TRANSLATE if e["translate"] is not None else 0)
        a.c, a.s, a.scale = e["c"], e["s"], e["scale"]
        if e["translate"] is not None:
            a.translate[:] = e["translate"]
    return table


def _need_device(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise hip.ShastaHipError("sweep assembly runs on the device only; there is no CPU path (got device %s)" % device)
    return device


def assemble_rows(raw, segments, n_clouds, keep=KEEP, radius=CLOSE_RADIUS, augment=None):
    """raw: (total_rows, raw_ndim) fp32 device tensor, the rows of all segments back to back; segments: a `segment_table` or the
    sequence it takes; augment: None or one `augment_entry` per cloud.  -> (out (total_rows, keep + 1) fp32, of which the first
    prefix[n] rows are written, prefix (n + 1,) int32 device tensor).  Nothing is read back."""
    if not (torch.is_tensor(raw) and raw.is_cuda):
        raise hip.ShastaHipError("sweep assembly needs a device tensor; there is no CPU path")
    if raw.dim() != 2 or raw.dtype != torch.float32:
        raise ValueError("sweeps: raw rows must be a (total_rows, raw_ndim) fp32 tensor")
    lib = hip.load()
    table = segments if isinstance(segments, C.Array) else segment_table(segments)
    nseg = len(segments)
    total, raw_ndim = int(raw.shape[0]), int(raw.shape[1])
    wsb = lib.shasta_sweeps_workspace_bytes(nseg, total)
    if wsb == 0:
        raise hip.ShastaHipError("sweep assembly serves 1 to %d segments per call (got %d)" % (MAX_SEGMENTS, nseg))
    dev = raw.device
    out = torch.empty(max(total, 1), keep + 1, device=dev)
    prefix = torch.empty(n_clouds + 1, dtype=torch.int32, device=dev)
    ws = torch.empty((wsb + 3) // 4, dtype=torch.int32, device=dev)
    hip.check(lib.shasta_sweeps_assemble_f32(hip.ptr(raw.contiguous()), total, raw_ndim, table, nseg, n_clouds, keep, float(radius),
                                             augment_table(augment, n_clouds), hip.ptr(out), int(out.shape[0]), hip.ptr(prefix),
                                             hip.ptr(ws), wsb, hip.stream_ptr()), "shasta_sweeps_assemble_f32")
    return out, prefix


_pinned = None  # one pinned staging buffer for the raw rows of a call, grown on demand and reused


def _staging(nbytes):
    global _pinned
    if _pinned is None or _pinned.numel() < nbytes:
        _pinned = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, pin_memory=True)
    return _pinned


def _rows_of(path):
    size = os.path.getsize(path)
    if size % (4 * RAW_NDIM):
        raise ValueError("%s: %d bytes are no whole number of (n, %d) float32 rows" % (path, size, RAW_NDIM))
    return size // (4 * RAW_NDIM)


def assemble_clouds(infos, nsweeps, device, path_map=None, augment=None):
    """infos: 1 to 32 frame infos (`lidar_path`, `sweeps[i]{lidar_path, transform_matrix, time_lag}`).  Per frame, in order, the sweep
    order is drawn as the reference draws it (`np.random.choice(len(sweeps), nsweeps - 1, replace=False)`, global numpy stream).
    -> (points (N, 5) fp32 device tensor: x, y, z, intensity, time lag - the reference's `combined` of every frame back to back,
    offsets: n + 1 ints, rows before each frame)."""
    device = _need_device(device)
    if not 1 <= len(infos) <= MAX_CLOUDS:
        raise ValueError("assemble_clouds: 1 to %d frames per call (got %d)" % (MAX_CLOUDS, len(infos)))
    pm = path_map or (lambda p: p)
    files, segments = [], []
    for c, info in enumerate(infos):
        assert (nsweeps - 1) == len(info["sweeps"]), "nsweeps {} should equal to list length {}.".format(nsweeps, len(info["sweeps"]))
        path = pm(str(info["lidar_path"]))
        files.append(path)
        segments.append((_rows_of(path), c, None, False, 0.0))
        for i in np.random.choice(len(info["sweeps"]), nsweeps - 1, replace=False):
            sweep = info["sweeps"][i]
            path = pm(str(sweep["lidar_path"]))
            files.append(path)
            segments.append((_rows_of(path), c, sweep["transform_matrix"], True, sweep["time_lag"]))
    total = sum(g[0] for g in segments)
    nbytes = total * 4 * RAW_NDIM
    stage = _staging(nbytes)
    view, at = memoryview(stage.numpy()), 0
    for path, g in zip(files, segments):
        want = g[0] * 4 * RAW_NDIM
        with open(path, "rb") as f:
            if f.readinto(view[at:at + want]) != want:
                raise IOError("%s changed size while it was read" % path)
        at += want
    with torch.cuda.device(device):
        raw = torch.empty(total, RAW_NDIM, device=device)
        if nbytes:
            raw.view(-1).copy_(stage[:nbytes].view(torch.float32), non_blocking=True)
        out, prefix = assemble_rows(raw, segments, len(infos), augment=augment)
        offsets = [int(v) for v in prefix.cpu()]  # the one host read; the pinned buffer is free again after it
    return out[:offsets[-1]], offsets


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


@PIPELINES.register_module
class LoadPointCloudFromFile(object):
    """loading.py:111-148.  `__call__(res, info)` fills res["lidar"]["combined"] ((N, 5) fp32 device tensor), ["points"] (its first
    four columns) and ["times"] (its last column, (N, 1)) - the latter two are views of the first.  Keywords beyond the reference's:
    `device` (default "cuda") and `path_map` (a callable str -> str applied to every path, in place of the reference's hard-coded
    `.replace('tsadja', 'ubuntu')`).  The default dataset is the one that is served (the reference's default, "KittiDataset", raises in
    its `__call__` too)."""

    def __init__(self, dataset="NuScenesDataset", **kwargs):
        self.type = dataset
        self.random_select = kwargs.get("random_select", False)
        self.npoints = kwargs.get("npoints", 16834)
        self.device = kwargs.get("device", "cuda")
        self.path_map = kwargs.get("path_map")

    def __call__(self, res, info):
        res["type"] = self.type
        if self.type != "NuScenesDataset":
            raise NotImplementedError("LoadPointCloudFromFile: only NuScenesDataset is served (got %s)" % self.type)
        if res.get("virtual"):
            raise NotImplementedError("LoadPointCloudFromFile: virtual (painted) points are out of scope (DESIGN.md 8)")
        combined, _ = assemble_clouds([info], res["lidar"]["nsweeps"], self.device, path_map=self.path_map)
        res["lidar"]["points"] = combined[:, :KEEP]
        res["lidar"]["times"] = combined[:, KEEP:]
        res["lidar"]["combined"] = combined
        return res, info


def draw_augment(rot_noise, scale_noise, translate_std):
    """The draws of preprocess.py:126-136 in the reference's order: the two flips (`random_flip_both`), the rotation angle
    (`global_rotation`), the scale (`global_scaling_v2`) and - only when a std is non-zero - three normals (`global_translate_`, which
    draws z with the x std, as the reference does).  -> `augment_entry`."""
    flip_x = np.random.choice([False, True], replace=False, p=[0.5, 0.5])
    flip_y = np.random.choice([False, True], replace=False, p=[0.5, 0.5])
    rotation = rot_noise if isinstance(rot_noise, list) else [-rot_noise, rot_noise]
    angle = np.random.uniform(rotation[0], rotation[1])
    scale = np.random.uniform(scale_noise[0], scale_noise[1])
    std = translate_std
    if not isinstance(std, (list, tuple, np.ndarray)):
        std = np.array([std, std, std])
    translate = None
    if not all([e == 0 for e in std]):
        translate = np.array([np.random.normal(0, std[0], 1), np.random.normal(0, std[1], 1), np.random.normal(0, std[0], 1)]).T
    return augment_entry(flip_x, flip_y, angle, scale, translate)


@PIPELINES.register_module
class Preprocess(object):
    """preprocess.py:28-158.  In train mode (without `no_augmentation`) the parameters are drawn by `draw_augment` and
    applied by the assembly kernels' write pass to res["lidar"]["combined"]; with `shuffle_points` the permutation is drawn with
    `np.random.shuffle` on an index array - the same permutation as shuffling the rows - and applied as a row gather.  Result in
    res["lidar"]["points"], as in the reference; the drawn parameters are kept in res["lidar"]["augment"].
    With res["lidar"]["annotations"] (`LoadPointCloudAnnotations`) in train mode the boxes follow the reference too: `DontCare / ignore /
    UNKNOWN` are dropped, the `class_names` mask and the 1-based `gt_classes` are built on the host, the SAME drawn entry is applied to the
    boxes on the device (`targets.augment_boxes`), and `gt_dict` (`gt_boxes` a device tensor, `gt_names`, `gt_classes`) replaces
    res["lidar"]["annotations"]; with `no_augmentation` the classes are selected and numbered only.  The draws and the points do not
    depend on the presence of annotations."""

    def __init__(self, cfg=None, **kwargs):
        self.shuffle_points = _get(cfg, "shuffle_points")
        self.min_points_in_gt = _get(cfg, "min_points_in_gt", -1)
        self.mode = _get(cfg, "mode")
        if self.mode == "train":
            self.global_rotation_noise = _get(cfg, "global_rot_noise")
            self.global_scaling_noise = _get(cfg, "global_scale_noise")
            self.global_translate_std = _get(cfg, "global_translate_std", 0)
            self.class_names = _get(cfg, "class_names")
            if _get(cfg, "db_sampler") is not None:
                raise NotImplementedError("Preprocess: a db_sampler (ground-truth pasting) is out of scope (DESIGN.md 8)")
            self.db_sampler = None
            self.npoints = _get(cfg, "npoints", -1)
        if self.min_points_in_gt > 0:
            raise NotImplementedError("Preprocess: min_points_in_gt > 0 is out of scope (DESIGN.md 8)")
        self.no_augmentation = _get(cfg, "no_augmentation", False)

    def __call__(self, res, info):
        res["mode"] = self.mode
        if res["type"] not in ["NuScenesDataset"]:
            raise NotImplementedError
        points = res["lidar"]["combined"]
        if not (torch.is_tensor(points) and points.is_cuda):
            raise hip.ShastaHipError("Preprocess needs the device tensor LoadPointCloudFromFile leaves; there is no CPU path")
        gt_dict = None
        if self.mode == "train" and "annotations" in res["lidar"]:
            anno = res["lidar"]["annotations"]
            gt_dict = {"gt_boxes": anno["boxes"], "gt_names": np.array(anno["names"]).reshape(-1)}
            if not self.no_augmentation:
                self._select(gt_dict, np.array([n not in ("DontCare", "ignore", "UNKNOWN") for n in gt_dict["gt_names"]], dtype=np.bool_))
            self._select(gt_dict, np.array([n in self.class_names for n in gt_dict["gt_names"]], dtype=np.bool_))
            gt_dict["gt_classes"] = np.array([self.class_names.index(n) + 1 for n in gt_dict["gt_names"]], dtype=np.int32)
            boxes = gt_dict["gt_boxes"]
            if not torch.is_tensor(boxes):
                boxes = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float32))
            gt_dict["gt_boxes"] = boxes.to(points.device, torch.float32).reshape(-1, 9)
        if self.mode == "train" and not self.no_augmentation:
            entry = draw_augment(self.global_rotation_noise, self.global_scaling_noise, self.global_translate_std)
            n, w = int(points.shape[0]), int(points.shape[1])
            out, _ = assemble_rows(points, [(n, 0, None, False, 0.0)], 1, keep=w, augment=[entry])  # no row is dropped
            points = out[:n, :w].contiguous()
            res["lidar"]["augment"] = entry
            if gt_dict is not None:
                from .targets import augment_boxes
                gt_dict["gt_boxes"] = augment_boxes(gt_dict["gt_boxes"], entry)
        if self.shuffle_points:
            index = np.arange(int(points.shape[0]))
            np.random.shuffle(index)
            points = points[torch.from_numpy(index).to(points.device)]
        res["lidar"]["points"] = points
        if gt_dict is not None:
            res["lidar"]["annotations"] = gt_dict
        return res, info

    @staticmethod
    def _select(gt_dict, keep):
        """_dict_select on the host arrays (the boxes are still the loader's numpy array or a tensor of any device)."""
        boxes = gt_dict["gt_boxes"]
        gt_dict["gt_boxes"] = boxes[torch.from_numpy(keep).to(boxes.device)] if torch.is_tensor(boxes) else boxes[keep]
        gt_dict["gt_names"] = gt_dict["gt_names"][keep]


class SweepClouds:
    """`clouds` for `bevmap.CloudMaps`: token -> the frame's assembled multi-sweep cloud.  `batch(tokens, device)` assembles up to 32
    frames in one call and returns their device tensors; `__call__(token)` is a batch of one."""

    def __init__(self, infos_by_token, nsweeps, path_map=None, device="cuda"):
        self.infos, self.nsweeps, self.path_map, self.device = infos_by_token, int(nsweeps), path_map, device

    def batch(self, tokens, device=None):
        points, off = assemble_clouds([self.infos[t] for t in tokens], self.nsweeps, device or self.device, path_map=self.path_map)
        return [points[off[i]:off[i + 1]] for i in range(len(tokens))]

    def __call__(self, token):
        return self.batch([token])[0]
