"""`VoxelNet`: reader -> backbone -> neck -> bbox_head, the detector whose output is the detections `Shasta` consumes.

The reference keeps the socket (`DETECTORS`, `build_detector`, det3d/models/builder.py:62-63) without a detector class; this is
CenterPoint's `VoxelNet` on this package's modules.  Children are created in the order reader, backbone, neck, bbox_head, so a CenterPoint
checkpoint's `reader.* / backbone.* / neck.* / bbox_head.*` keys load through `load_state_dict_permissive`.  `extract_feat` is `BEVMap`'s
(both reader branches).  `forward(example, return_loss=False)` returns `bbox_head.predict(example, preds, test_cfg)`: one dict per sample
`{box3d_lidar, scores, label_preds, metadata}`; `return_loss=True` raises NotImplementedError - there is no head loss here."""
from . import builder
from .bevmap import BEVMap
from .registry import DETECTORS


@DETECTORS.register_module
class VoxelNet(BEVMap):
    def __init__(self, reader, backbone, neck=None, bbox_head=None, train_cfg=None, test_cfg=None, pretrained=None):
        super().__init__(reader, backbone, neck, train_cfg=train_cfg, test_cfg=test_cfg, pretrained=None)
        self.bbox_head = builder.build_head(bbox_head)
        self.init_weights(pretrained=pretrained)

    def forward(self, example, return_loss=False, **kwargs):
        if return_loss:
            raise NotImplementedError("VoxelNet: the head's losses and target assignment are not part of this package")
        x, _ = self.extract_feat(example)
        preds = self.bbox_head(x)
        return self.bbox_head.predict(example, preds, self.test_cfg)
