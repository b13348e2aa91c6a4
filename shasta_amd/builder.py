"""`build_*` entry points of det3d/models/builder.py:20-75 for the registries this path uses.

A None config builds nothing (returns None).  NECKS holds `RPN` (shasta_amd/neck.py: the reference's neck on the kernels of
csrc/neck.hip).  BACKBONES is empty at import: the sparse backbone `SpMiddleResNetFHD` (shasta_amd/backbone.py, eval-mode forward on
csrc/sparse_conv.hip, no spconv) is passed as a class - `backbone=dict(type=shasta_amd.backbone.SpMiddleResNetFHD, ...)` - or
registered under its name by `shasta_amd.backbone.register()` for the reference's string configs; the Shasta module calls it
exactly like the reference.  BEV holds `SingleStageBEV` and `BEVMap` (shasta_amd/bevmap.py), the stand-alone reader -> backbone -> neck
module whose weights are `bev_map.pth`.  HEADS holds `CenterHead` (shasta_amd/head.py), DETECTORS `VoxelNet` (shasta_amd/detector.py): the
detector that ends in detections.  A list of configs becomes an nn.Sequential, like the reference."""
from torch import nn

from . import registry as R


def build(cfg, registry, default_args=None):
    if cfg is None:
        return None
    if isinstance(cfg, (list, tuple)):
        return nn.Sequential(*(R.build_from_cfg(one, registry, default_args) for one in cfg))
    return R.build_from_cfg(cfg, registry, default_args)


def _plain(registry):
    return lambda cfg: build(cfg, registry)


def _with_run_cfgs(registry):
    return lambda cfg, train_cfg=None, test_cfg=None: build(cfg, registry, {"train_cfg": train_cfg, "test_cfg": test_cfg})


build_reader = _plain(R.READERS)
build_backbone = _plain(R.BACKBONES)
build_neck = _plain(R.NECKS)
build_head = _plain(R.HEADS)  # builder.py:46-47: CenterHead (shasta_amd/head.py)
build_second_stage_module = _plain(R.SECOND_STAGE)
build_simp_track = _with_run_cfgs(R.TRACK)
build_track = _with_run_cfgs(R.TRACK)
build_detector = _with_run_cfgs(R.DETECTORS)  # builder.py:62-63: VoxelNet (shasta_amd/detector.py)
build_bev = _with_run_cfgs(R.BEV)  # builder.py:66: BEVMap / SingleStageBEV (shasta_amd/bevmap.py)
