"""`BEVMap`: the stand-alone reader -> backbone -> neck module that produces the maps `shared_conv` reads; its weights are `bev_map.pth`.

Mirror of det3d/models/bev/base.py:11-64 (`BaseBEV`), single_stage.py:10-59 (`SingleStageBEV`) and bevmap.py:7-57 (`BEVMap`), built by
`build_bev` (det3d/models/builder.py:66):
  * same constructor keywords, same child creation order (reader, backbone, neck), so the `state_dict` keys `backbone.*` / `neck.*` are
    those of `Shasta` and a reference checkpoint loads through `load_state_dict_permissive`;
  * `BEVMap.extract_feat(data)` has both reference branches: dynamic (`data['points']` -> DynamicVoxelEncoder) and hard-voxel
    (`data['voxels']`, `data['num_points']`, `data['coordinates']`, `data['shape'][0]`); `forward` returns the map.
Every compute step runs on this package's kernels: csrc/dynvox.hip or voxelize.hip, sparse_conv.hip, neck.hip.  The backbone
`SpMiddleResNetFHD` is not registered at import: pass the class as `type`, or its name after `shasta_amd.backbone.register()`.

Deviation: `freeze()` sets requires_grad = False and eval() but does NOT swap BatchNorm2d for the reference's FrozenBatchNorm2d
(single_stage.py:55-59): the neck kernels take eval-mode BatchNorm2d modules, whose arithmetic is the same running-statistics affine.

`CloudMaps` feeds `pipeline.run_split` from point clouds: `neck_batch(tokens, device)` is the protocol `pipeline._run_features` accepts."""
import numpy as np
import torch
import torch.nn as nn

from . import builder
from .registry import BEV
from .shasta import load_state_dict_permissive


class BaseBEV(nn.Module):
    """det3d/models/bev/base.py:11-64."""

    def __init__(self):
        super().__init__()
        self.fp16_enabled = False

    @property
    def with_reader(self):
        return hasattr(self, "reader") and self.reader is not None

    @property
    def with_neck(self):
        return hasattr(self, "neck") and self.neck is not None

    def extract_feat(self, data):
        raise NotImplementedError

    def extract_feats(self, datas):
        assert isinstance(datas, list)
        for data in datas:
            yield self.extract_feat(data)

    def init_weights(self, pretrained=None):
        """A local checkpoint file: a bare state dict or a {'state_dict': ...} wrapper.  Like the reference, a missing or broken file is
        reported and does not abort construction."""
        if pretrained is None:
            return
        try:
            checkpoint = torch.load(pretrained, map_location="cpu")
            sd = checkpoint.get("state_dict", checkpoint) if isinstance(checkpoint, dict) else checkpoint
            load_state_dict_permissive(self, sd)
            print("init weight from {}".format(pretrained))
        except Exception as e:  # noqa: BLE001
            print("no pretrained model at {} ({})".format(pretrained, e))

    def forward(self, example, return_loss=True, **kwargs):
        pass


@BEV.register_module
class SingleStageBEV(BaseBEV):
    def __init__(self, reader, backbone, neck, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__()
        self.reader = builder.build_reader(reader)
        self.backbone = builder.build_backbone(backbone)
        self.neck = builder.build_neck(neck)
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg
        self.init_weights(pretrained=pretrained)

    def extract_feat(self, data):
        x = self.backbone(self.reader(data))
        if self.with_neck:
            x = self.neck(x)
        return x

    def aug_test(self, example, rescale=False):
        raise NotImplementedError

    def predict(self, example, preds_dicts):
        pass

    def freeze(self):
        for p in self.parameters():
            p.requires_grad = False
        self.eval()
        return self


@BEV.register_module
class BEVMap(SingleStageBEV):
    def extract_feat(self, data):
        if "voxels" not in data:
            voxels, coors, shape = self.reader(data["points"])
            input_features, batch_size = voxels, len(data["points"])
        else:
            input_features = self.reader(data["voxels"], data["num_points"])
            coors, batch_size, shape = data["coordinates"], len(data["points"]), data["shape"][0]
        x, voxel_feature = self.backbone(input_features, coors, batch_size, shape)
        if self.with_neck:
            x = self.neck(x)
        return x, voxel_feature

    def forward(self, example, return_loss=True, **kwargs):
        x, _ = self.extract_feat(example)
        return x


class CloudMaps:
    """Neck outputs of frames from their point clouds: `clouds(token)` -> (P, ndim) fp32 array or tensor, `model` a BEVMap in eval mode.
    A `clouds` object with a `batch(tokens, device)` method (sweeps.SweepClouds) is asked for a whole group's device tensors at once.
    `neck_batch(tokens, device)` -> (n, C, H, W) fp32, the tokens run through the model in groups of at most `max_clouds`."""

    def __init__(self, model, clouds, max_clouds=8):
        if max_clouds < 1:
            raise ValueError("CloudMaps: max_clouds must be at least 1")
        self.model, self.clouds, self.max_clouds = model, clouds, int(max_clouds)

    def _cloud(self, token, device):
        c = self.clouds(token)
        if not torch.is_tensor(c):
            c = torch.from_numpy(np.ascontiguousarray(c, np.float32))
        return c.to(device=device, dtype=torch.float32)

    def neck_batch(self, tokens, device):
        if self.model.training:
            raise RuntimeError("CloudMaps: the model must be in eval() mode (BEVMap.freeze())")
        outs = []
        with torch.no_grad():
            for i in range(0, len(tokens), self.max_clouds):
                group = tokens[i:i + self.max_clouds]
                pts = list(self.clouds.batch(group, device)) if hasattr(self.clouds, "batch") else [self._cloud(t, device) for t in group]
                outs.append(self.model(dict(points=pts)))
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
