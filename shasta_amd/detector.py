"""`VoxelNet`: reader -> backbone -> neck -> bbox_head, the detector whose output is the detections `Shasta` consumes.

The reference keeps the socket (`DETECTORS`, `build_detector`, det3d/models/builder.py:62-63) without a detector class; this is
CenterPoint's `VoxelNet` on this package's modules.  Children are created in the order reader, backbone, neck, bbox_head, so a CenterPoint
checkpoint's `reader.* / backbone.* / neck.* / bbox_head.*` keys load through `load_state_dict_permissive`.  `extract_feat` is `BEVMap`'s
(both reader branches).  `forward(example, return_loss=False)` returns `bbox_head.predict(example, preds, test_cfg)`: one dict per sample
`{box3d_lidar, scores, label_preds, metadata}`; `return_loss=True` returns `bbox_head.loss(example, preds, test_cfg)`: one dict per task
`{loss, hm_loss, loc_loss, loc_loss_elem, num_positive}`.  The loss needs the targets of `targets.AssignLabel` / `targets.assign_targets`
in the example (`hm, anno_box, ind, mask, cat`); an example without them is refused with NotImplementedError before any stage runs."""
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
        if return_loss and any(k not in example for k in ("hm", "anno_box", "ind", "mask", "cat")):
            raise NotImplementedError("VoxelNet: return_loss=True needs the targets hm, anno_box, ind, mask, cat in the example "
                                      "(targets.AssignLabel / targets.assign_targets make them)")
        x, _ = self.extract_feat(example)
        preds = self.bbox_head(x)
        if return_loss:
            return self.bbox_head.loss(example, preds, self.test_cfg)
        return self.bbox_head.predict(example, preds, self.test_cfg)
