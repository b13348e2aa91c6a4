"""CenterPoint training targets on the device: ground-truth boxes -> heatmaps, anno_box, ind, mask, cat (csrc/center_targets.hip).

Mirror of the box half of det3d/datasets/pipelines/preprocess.py:28-158 (`Preprocess`; det3d/core/sampler/preprocess.py:771-839, 940-962),
of `filter_gt_box_outside_range` (sampler/preprocess.py:108-122, the reference's `Voxelization` applies it in train mode) and of
`AssignLabel` (datasets/pipelines/preprocess.py:273-458), the nuScenes branch.  Boxes are (n, 9) fp32 rows [x, y, z, w, l, h, vx, vy, rot].

  * `augment_boxes(boxes, entry)` - one `sweeps.augment_entry` applied to a cloud's boxes in the reference's order and fp32 arithmetic:
    flips (`rot -> -rot + pi`, `-rot + 2 pi` with the fp32-rounded constants numpy uses), rotation (the points' operation order; the
    reference rotates the velocities through a float64 matrix and rounds once, here they take the points' fp32 form - equal within the
    bound of a two-term fp32 dot product), `rot += fp32(angle)`, the scale on ALL columns but the last (the velocities too), the
    translation as fp32(float64 sum).
  * `filter_gt_box_outside_range(boxes, bv_range)` -> bool device tensor: a box stays when one of its four BEV corners is strictly inside
    the rectangle; a corner exactly on an edge is outside (`cross >= 0` fails the reference's convex-polygon test).
  * `assign_targets(boxes, classes, tasks, cfg, augment=None, bv_range=None)` - a batch of B samples and all tasks in ONE call of
    `shasta_center_targets_f32`, no host read: augmentation and range filter (both optional), the stable partition by task and class,
    slots, truncation to `max_objs`, holes for centres outside the map, gaussian radius and heatmap.  `gaussian_radius` runs in fp32
    THROUGHOUT: under numpy >= 2 promotion a Python float next to an fp32 scalar stays fp32, so the reference's `w, l` (fp32 scalars) keep
    every intermediate in fp32; `1 - min_overlap` and the like are formed in float64 first and then rounded.  Returns the reference's
    `example` entries stacked over the batch - what `collate` builds: `hm`, `anno_box`, `ind`, `mask`, `cat` as lists over tasks of
    (B, ...) tensors and `gt_boxes_and_cls` (B, max_objs, 10) - plus `gt_boxes` (the augmented boxes, packed), `keep` (the range
    filter's mask) and `offsets`.
  * `AssignLabel`, `LoadPointCloudAnnotations` - registered in `registry.PIPELINES` with the reference's `__call__(res, info)` contract.

Deviations, all deliberate:
  * `assert num_obj <= max_objs` on `gt_boxes_and_cls` is a ValueError raised before any launch.  It needs the classes on the host:
    pass them as numpy arrays or CPU tensors (what `Preprocess` leaves); device classes are copied to the host only for a sample with
    more than `max_objs` boxes, and so is the range filter's mask.  `cfg["gt_boxes_and_cls"] = False` leaves the entry out (and with
    it the limit: a task's boxes beyond `max_objs` are then dropped, `num_objs = min(n, max_objs)`).
  * `AssignLabel` leaves `gt_dict` as `Preprocess` wrote it; the reference regroups `gt_boxes / gt_classes / gt_names` by task there
    (host lists nothing reads afterwards).  The range filter, which the reference's `Voxelization` step applies, is an option of this
    step: `cfg["bv_range"]`.
  * `WaymoDataset` raises NotImplementedError.
There is no CPU path: CPU boxes raise ShastaHipError."""
import ctypes as C

import numpy as np
import torch

from . import hip
from .registry import PIPELINES
from .sweeps import AUG_NEG_X, AUG_NEG_Y, AUG_TRANSLATE, augment_entry

MAX_BATCH, MAX_TASKS, MAX_TASK_CLASSES, MAX_OBJS, MAX_BOXES, MAX_MAP = 64, 16, 4, 1024, 4096, 512  # include/shasta_hip.h SHASTA_CENTER_*


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


def _fill_augment(a, e):
    e = e or augment_entry()
    a.flags = (AUG_NEG_Y if e["flip_x"] else 0) | (AUG_NEG_X if e["flip_y"] else 0) | (AUG_TRANSLATE if e["translate"] is not None else 0)
    a.c, a.s, a.angle, a.scale = e["c"], e["s"], float(np.float32(e["angle"])), e["scale"]
    if e["translate"] is not None:
        a.translate[:] = e["translate"]


def _need_boxes(boxes, what):
    if not (torch.is_tensor(boxes) and boxes.is_cuda):
        raise hip.ShastaHipError("%s runs on the device only; there is no CPU path" % what)
    if boxes.dim() != 2 or boxes.shape[1] != 9 or boxes.dtype != torch.float32:
        raise ValueError("%s: boxes must be an (n, 9) fp32 tensor [x, y, z, w, l, h, vx, vy, rot]" % what)
    return boxes.contiguous()


def augment_boxes(boxes, entry):
    """boxes (n, 9) fp32 device tensor, entry: a `sweeps.augment_entry` (None = identity) -> the augmented boxes, a new tensor."""
    boxes = _need_boxes(boxes, "augment_boxes")
    a = hip.BoxAugment()
    _fill_augment(a, entry)
    out = torch.empty_like(boxes)
    hip.check(hip.load().shasta_center_box_augment_f32(hip.ptr(boxes), int(boxes.shape[0]), C.byref(a), hip.ptr(out), hip.stream_ptr()),
              "shasta_center_box_augment_f32")
    return out


def _range4(bv_range):
    r = np.ascontiguousarray(np.asarray(bv_range, dtype=np.float32).reshape(-1))
    if r.shape[0] != 4:
        raise ValueError("bv_range must be [x0, y0, x1, y1]")
    return r


def filter_gt_box_outside_range(boxes, bv_range):
    """boxes (n, 9) fp32 device tensor, bv_range [x0, y0, x1, y1] (rounded to fp32, as the voxel generator's range is) -> (n,) bool."""
    boxes = _need_boxes(boxes, "filter_gt_box_outside_range")
    r = _range4(bv_range)
    keep = torch.empty(boxes.shape[0], dtype=torch.uint8, device=boxes.device)
    hip.check(hip.load().shasta_center_range_filter_f32(hip.ptr(boxes), int(boxes.shape[0]), r.ctypes.data_as(C.c_void_p), hip.ptr(keep),
                                                        hip.stream_ptr()), "shasta_center_range_filter_f32")
    return keep.bool()


def feature_map_size(cfg):
    """[W_map, H_map] as AssignLabel derives it: `cfg["grid_size"]` (the voxel generator's) or round((pc_range[3:] - pc_range[:3]) /
    voxel_size) in fp32, floor-divided by out_size_factor."""
    grid = _get(cfg, "grid_size")
    if grid is None:
        pc, vs = np.array(_get(cfg, "pc_range"), dtype=np.float32), np.array(_get(cfg, "voxel_size"), dtype=np.float32)
        grid = np.round((pc[3:] - pc[:3]) / vs).astype(np.int64)
    fms = np.asarray(grid)[:2] // int(_get(cfg, "out_size_factor"))
    return int(fms[0]), int(fms[1])


def _num_classes(tasks):
    return [int(t) if isinstance(t, (int, np.integer)) else int(_get(t, "num_class", len(_get(t, "class_names", [])))) for t in tasks]


def _host_classes(c):
    if torch.is_tensor(c):
        return None if c.is_cuda else c.numpy().astype(np.int32).reshape(-1)
    return np.asarray(c, dtype=np.int32).reshape(-1)


def assign_targets(boxes, classes, tasks, cfg, augment=None, bv_range=None):
    """boxes: a list of B per-sample (n_b, 9) fp32 device tensors, or (packed (N, 9) tensor, offsets: B + 1 ints) - the form
    `sweeps.assemble_clouds` returns; classes: the 1-based classes over all tasks in the same form (host arrays or tensors of any
    integer type; 0 or a class beyond the tasks' belongs to no task); tasks: per task a class count or a dict / object with `num_class`
    or `class_names`; cfg: `out_size_factor, gaussian_overlap, max_objs, min_radius, pc_range, voxel_size` (and optionally `grid_size`,
    `gt_boxes_and_cls`); augment: None or one `sweeps.augment_entry` per sample; bv_range: None or [x0, y0, x1, y1]."""
    if isinstance(boxes, (list,)):
        per = [_need_boxes(b, "assign_targets") for b in boxes]
        offsets = [0]
        for b in per:
            offsets.append(offsets[-1] + int(b.shape[0]))
        if not per:
            raise ValueError("assign_targets: an empty batch")
        packed = torch.cat(per, 0) if len(per) > 1 else per[0]
        cls_list = list(classes)
        if len(cls_list) != len(per):
            raise ValueError("assign_targets: one class array per sample")
        host = [_host_classes(c) for c in cls_list]
        if all(h is not None for h in host):
            cls_host, cls_dev = np.concatenate(host) if host else np.zeros(0, np.int32), None
        else:
            cls_host, cls_dev = None, torch.cat([torch.as_tensor(c).reshape(-1).to(packed.device, torch.int32) for c in cls_list])
    else:
        packed, offsets = boxes
        packed = _need_boxes(packed, "assign_targets")
        offsets = [int(v) for v in offsets]
        cls_host = _host_classes(classes)
        cls_dev = None if cls_host is not None else classes.reshape(-1).to(torch.int32)
    B, N, dev = len(offsets) - 1, int(packed.shape[0]), packed.device
    if offsets[0] != 0 or offsets[-1] != N or any(b < a for a, b in zip(offsets, offsets[1:])):
        raise ValueError("assign_targets: offsets must rise from 0 to the number of boxes")
    if (cls_host if cls_host is not None else cls_dev).shape[0] != N:
        raise ValueError("assign_targets: one class per box")
    if _get(cfg, "dataset", "NuScenesDataset") not in ("NuScenesDataset", "nuscenes"):
        raise NotImplementedError("assign_targets: only NuScenesDataset is served")
    ncls = _num_classes(tasks)
    T, max_objs = len(ncls), int(_get(cfg, "max_objs"))
    W, H = feature_map_size(cfg)
    lib = hip.load()
    wsb = lib.shasta_center_targets_workspace_bytes(B, T, max_objs)
    if (wsb == 0 or any(not 1 <= c <= MAX_TASK_CLASSES for c in ncls) or not (1 <= W <= MAX_MAP and 1 <= H <= MAX_MAP)
            or any(b - a > MAX_BOXES for a, b in zip(offsets, offsets[1:]))):
        raise hip.ShastaHipError("assign_targets serves 1..%d samples, 1..%d tasks of 1..%d classes, max_objs <= %d, %d boxes per sample and "
                                 "maps up to %d x %d (got B %d, classes %s, max_objs %d, map %d x %d)"
                                 % (MAX_BATCH, MAX_TASKS, MAX_TASK_CLASSES, MAX_OBJS, MAX_BOXES, MAX_MAP, MAX_MAP, B, ncls, max_objs, W, H))
    if augment is not None and len(augment) != B:
        raise ValueError("assign_targets: one augmentation entry per sample (%d for %d)" % (len(augment), B))
    with_gtbc = bool(_get(cfg, "gt_boxes_and_cls", True))
    rng = None if bv_range is None else _range4(bv_range)
    if with_gtbc and any(b - a > max_objs for a, b in zip(offsets, offsets[1:])):
        # the reference's `assert num_obj <= max_objs`; only a sample with more boxes than max_objs can fail it
        ch = cls_host if cls_host is not None else cls_dev.cpu().numpy()
        in_task = (ch >= 1) & (ch <= sum(ncls))
        if rng is not None:
            ab = packed
            if augment is not None:
                ab = torch.cat([augment_boxes(packed[a:b], e) for a, b, e in zip(offsets, offsets[1:], augment)])
            in_task &= filter_gt_box_outside_range(ab, rng).cpu().numpy()
        for s, (a, b) in enumerate(zip(offsets, offsets[1:])):
            if int(in_task[a:b].sum()) > max_objs:
                raise ValueError("assign_targets: sample %d has %d boxes in the tasks' classes, gt_boxes_and_cls holds max_objs = %d"
                                 % (s, int(in_task[a:b].sum()), max_objs))
    if cls_dev is None:
        cls_dev = torch.from_numpy(np.ascontiguousarray(cls_host, dtype=np.int32)).to(dev)
    cls_dev = cls_dev.contiguous()

    pc, vs = _get(cfg, "pc_range"), _get(cfg, "voxel_size")
    k = hip.CenterTargetCfg()
    k.num_tasks, k.max_objs, k.min_radius, k.map_w, k.map_h = T, max_objs, int(_get(cfg, "min_radius")), W, H
    k.num_class[:T] = ncls
    k.pc_x, k.pc_y, k.voxel_x, k.voxel_y = float(pc[0]), float(pc[1]), float(vs[0]), float(vs[1])
    k.out_size_factor, k.gaussian_overlap = float(_get(cfg, "out_size_factor")), float(_get(cfg, "gaussian_overlap"))
    table = None
    if augment is not None:
        table = (hip.BoxAugment * B)()
        for a, e in zip(table, augment):
            _fill_augment(a, e)
    off = (C.c_int32 * (B + 1))(*offsets)
    with torch.cuda.device(dev):
        hm = torch.empty(B * sum(ncls) * H * W, dtype=torch.float32, device=dev)
        anno = torch.empty(T, B, max_objs, 10, dtype=torch.float32, device=dev)
        ind = torch.empty(T, B, max_objs, dtype=torch.int64, device=dev)
        cat = torch.empty(T, B, max_objs, dtype=torch.int64, device=dev)
        mask = torch.empty(T, B, max_objs, dtype=torch.uint8, device=dev)
        gtbc = torch.empty(B, max_objs, 10, dtype=torch.float32, device=dev) if with_gtbc else None
        out_boxes = torch.empty(max(N, 1), 9, dtype=torch.float32, device=dev)
        keep = torch.empty(max(N, 1), dtype=torch.uint8, device=dev)
        ws = torch.empty((wsb + 3) // 4, dtype=torch.int32, device=dev)
        hip.check(lib.shasta_center_targets_f32(hip.ptr(packed) if N else None, hip.ptr(cls_dev) if N else None, off, B, C.byref(k), table,
                                                None if rng is None else rng.ctypes.data_as(C.c_void_p), hip.ptr(out_boxes), hip.ptr(keep),
                                                hip.ptr(hm), hip.ptr(anno), C.c_void_p(ind.data_ptr()), hip.ptr(mask), C.c_void_p(cat.data_ptr()),
                                                hip.ptr(gtbc), hip.ptr(ws), wsb, hip.stream_ptr()), "shasta_center_targets_f32")
    hms, at = [], 0
    for c in ncls:
        hms.append(hm[at:at + B * c * H * W].view(B, c, H, W))
        at += B * c * H * W
    ret = dict(hm=hms, anno_box=list(anno.unbind(0)), ind=list(ind.unbind(0)), mask=list(mask.unbind(0)), cat=list(cat.unbind(0)),
               gt_boxes=out_boxes[:N], keep=keep[:N].bool(), offsets=offsets)
    if with_gtbc:
        ret["gt_boxes_and_cls"] = gtbc
    return ret


@PIPELINES.register_module
class LoadPointCloudAnnotations(object):
    """loading.py:186-209: the info's boxes (float32, NaN -> 0), names, tokens and velocities into res["lidar"]["annotations"]."""

    def __init__(self, with_bbox=True, **kwargs):
        pass

    def __call__(self, res, info):
        if res["type"] in ["NuScenesDataset"] and "gt_boxes" in info:
            gt_boxes = info["gt_boxes"].astype(np.float32)
            gt_boxes[np.isnan(gt_boxes)] = 0
            res["lidar"]["annotations"] = {
                "boxes": gt_boxes,
                "names": info["gt_names"],
                "tokens": info["gt_boxes_token"],
                "velocities": info["gt_boxes_velocity"].astype(np.float32),
            }
        elif res["type"] == "WaymoDataset":
            raise NotImplementedError("LoadPointCloudAnnotations: only NuScenesDataset is served")
        return res, info


@PIPELINES.register_module
class AssignLabel(object):
    """preprocess.py:273-458 as a batch of one.  `cfg`: `out_size_factor, target_assigner.tasks, gaussian_overlap, max_objs, min_radius`
    and, for the branch without res["lidar"]["voxels"], `pc_range, voxel_size`; optional `bv_range` (the range filter as a stage of the
    call).  Fills res["lidar"]["targets"] with `hm, anno_box, ind, mask, cat` (lists over tasks, no batch axis) and `gt_boxes_and_cls`;
    for `mode != "train"` with {}."""

    def __init__(self, **kwargs):
        cfg = kwargs["cfg"]
        self.out_size_factor = _get(cfg, "out_size_factor")
        self.tasks = _get(_get(cfg, "target_assigner"), "tasks")
        self.gaussian_overlap = _get(cfg, "gaussian_overlap")
        self._max_objs = _get(cfg, "max_objs")
        self._min_radius = _get(cfg, "min_radius")
        self.bv_range = _get(cfg, "bv_range")
        self.cfg = cfg

    def __call__(self, res, info):
        example = {}
        if res["mode"] == "train":
            if res["type"] != "NuScenesDataset":
                raise NotImplementedError("AssignLabel: only NuScenesDataset is served (got %s)" % res["type"])
            k = dict(out_size_factor=self.out_size_factor, gaussian_overlap=self.gaussian_overlap, max_objs=self._max_objs,
                     min_radius=self._min_radius)
            if "voxels" in res["lidar"]:
                v = res["lidar"]["voxels"]
                k.update(grid_size=[int(s) for s in v["shape"]], pc_range=[float(s) for s in v["range"]], voxel_size=[float(s) for s in v["size"]])
            else:
                k.update(pc_range=_get(self.cfg, "pc_range"), voxel_size=_get(self.cfg, "voxel_size"))
            gt = res["lidar"]["annotations"]
            boxes = gt["gt_boxes"]
            if not (torch.is_tensor(boxes) and boxes.is_cuda):
                raise hip.ShastaHipError("AssignLabel needs the device boxes Preprocess leaves; there is no CPU path")
            out = assign_targets([boxes], [gt["gt_classes"]], self.tasks, k, bv_range=self.bv_range)
            for key in ("hm", "anno_box", "ind", "mask", "cat"):
                example[key] = [t[0] for t in out[key]]
            example["gt_boxes_and_cls"] = out["gt_boxes_and_cls"][0]
        res["lidar"]["targets"] = example
        return res, info
