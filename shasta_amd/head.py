"""`CenterHead`: the CenterPoint detection head behind the neck map - the stage that produces the detections `Shasta` consumes.

The reference ships the head's sockets (`HEADS`, `build_head`, the configs' `tasks` and `test_cfg`, `_second_det_to_nusc_box`) but not its
source; this module restates CenterPoint's `CenterHead` / `SepHead` / `predict` / `post_processing` as its nuScenes voxel configuration
uses them.  Parameter names are the `bbox_head.*` keys of a CenterPoint checkpoint: `shared_conv.{0,1}.*`, `tasks.<t>.<head>.{0,1,3}.*`
with the heads `reg, height, dim, rot, vel` (the order of `common_heads`) and `hm` last.  Initialisation: `hm`'s last bias is `init_bias`,
every other convolution gets kaiming-normal weights and a zero bias; NO random-number parity with CenterPoint's construction is claimed
(a checkpoint overwrites every tensor).  The loss arguments (`weight`, `code_weights`, `dataset`) feed `loss`.

`forward(x)` -> one dict per task, `{head name: (B, channels, H, W) fp32}`.  Two paths, `RPN`'s arrangement (neck.py):
  * the kernel path - `eval()` mode, fp32 device tensors, autograd off, `in_channels % 8 == 0`, `share_conv_channel % 32 == 0`, head width
    64, final widths 1 .. 3, `num_conv == 2`: `shared_conv` is one `shasta_neck_layer_f32` call (the convolution bias folded into the
    BatchNorm mean on the host), the first convolutions of a task's heads are ONE such call with 64 x heads output channels, the last
    convolutions one `shasta_head_final_f32` call (csrc/head.hip) into the task's (B, C_task, H, W) tensor; the dict entries are channel
    slices of it.  2 x tasks + 1 launches, no host synchronisation; packed weights are cached and follow in-place writes, optimizer
    steps, `load_state_dict` and `.to()` (pointer + version keys).
  * `forward_layers` - the module's own nn layers - for everything else: CPU, autograd, `train()` mode, other widths.

`predict(example, preds_dicts, test_cfg)` -> one dict per sample `{box3d_lidar (n, 9) [x, y, z, w, l, h, vx, vy, rot], scores (n,),
label_preds (n,) int64, metadata}`; device tensors only.  Per task: `shasta_head_decode_f32` (candidates in pixel order, counts on the
device), a stable descending `torch.sort` of the scores (ties: the lower pixel first) cut to `nms_pre_max_size`; then ONE
`shasta_nms_rotated_batch_f32` call for all tasks and samples on `[x, y, z, w, l, h, rot]` converted as `nms.rotate_nms_pcdet` converts,
one copy of the counts to the host, and the cut to `nms_post_max_size`.  Tasks are concatenated in order, `label_preds` = label + the
class count of the earlier tasks.  `max_per_img` is read and NOT applied: tasks x nms_post_max_size (6 x 83 = 498) stays below the
nuScenes value of 500, as in CenterPoint.  `use_rotate_nms=False`, `use_multi_class_nms=True` and `dcn_head=True` raise
NotImplementedError.  Circle NMS, the double-flip merge and graph capture are outside this module.

`loss(example, preds_dicts, test_cfg=None)` -> one dict per task `{loss, hm_loss, loc_loss, loc_loss_elem (10,), num_positive}`, device
tensors: FastFocalLoss on `hm` and the masked L1 RegLoss on (reg, height, dim, vel, rot) against the targets of `targets.assign_targets`
/ `AssignLabel` in `example` (`hm, anno_box, ind, mask, cat`), `loss = hm_loss + weight * loc_loss` (head_loss.py).  Both forms `forward`
returns are accepted; fp32 device tensors take ONE `shasta_center_loss_f32` call for all tasks, which also leaves the gradient with respect
to the raw outputs (head_loss.CenterLoss), everything else the torch composite.  In `train()` mode the convolutions run `forward_layers`
under autograd: there is no convolution backward on the kernels.  nuScenes only."""
import ctypes
import math
from collections import OrderedDict

import torch
from torch import nn

from . import frozen, hip
from .registry import HEADS

NUSC_COMMON_HEADS = OrderedDict([("reg", (2, 2)), ("height", (1, 2)), ("dim", (3, 2)), ("rot", (2, 2)), ("vel", (2, 2))])
_BOX_HEADS = ("reg", "height", "dim", "rot", "vel")  # what predict decodes, besides hm


class SepHead(nn.Module):
    """One nn.Sequential per head name: (num_conv - 1) x [Conv2d(3, bias), BatchNorm2d, ReLU], then Conv2d(3, bias) to the head's channels."""

    def __init__(self, in_channels, heads, head_conv=64, final_kernel=3, bn=True, init_bias=-2.19, **kwargs):
        super().__init__()
        self.heads = OrderedDict((k, tuple(v)) for k, v in heads.items())
        for name, (classes, num_conv) in self.heads.items():
            layers, cin = [], in_channels
            for _ in range(num_conv - 1):
                layers.append(nn.Conv2d(cin, head_conv, final_kernel, stride=1, padding=final_kernel // 2, bias=True))
                if bn:
                    layers.append(nn.BatchNorm2d(head_conv))
                layers.append(nn.ReLU())
                cin = head_conv
            layers.append(nn.Conv2d(cin, classes, final_kernel, stride=1, padding=final_kernel // 2, bias=True))
            fc = nn.Sequential(*layers)
            for m in fc.modules():
                if isinstance(m, nn.Conv2d):
                    nn.init.kaiming_normal_(m.weight)
                    nn.init.constant_(m.bias, 0)
            if name == "hm":
                fc[-1].bias.data.fill_(init_bias)
            setattr(self, name, fc)

    def forward(self, x):
        return {name: getattr(self, name)(x) for name in self.heads}


def _get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default)


@HEADS.register_module
class CenterHead(frozen.FrozenStage):
    def __init__(self, in_channels=[512], tasks=[], dataset="nuscenes", weight=0.25, code_weights=[], common_heads=dict(), logger=None,
                 init_bias=-2.19, share_conv_channel=64, num_hm_conv=2, dcn_head=False):
        super().__init__()
        if dcn_head:
            raise NotImplementedError("CenterHead: dcn_head is not part of this package")
        self.in_channels = int(in_channels[0] if isinstance(in_channels, (list, tuple)) else in_channels)
        self.num_classes = [int(t["num_class"]) for t in tasks]
        self.class_names = [list(t["class_names"]) for t in tasks]
        self.dataset, self.weight, self.code_weights = dataset, weight, list(code_weights)  # loss arguments
        self.common_heads = OrderedDict((k, tuple(v)) for k, v in (common_heads if len(common_heads) else NUSC_COMMON_HEADS).items())
        self.share_conv_channel, self.num_hm_conv = int(share_conv_channel), int(num_hm_conv)

        self.shared_conv = nn.Sequential(nn.Conv2d(self.in_channels, self.share_conv_channel, 3, padding=1, bias=True),
                                         nn.BatchNorm2d(self.share_conv_channel), nn.ReLU())
        nn.init.kaiming_normal_(self.shared_conv[0].weight)
        nn.init.constant_(self.shared_conv[0].bias, 0)
        self.tasks = nn.ModuleList()
        for num_cls in self.num_classes:
            heads = OrderedDict(self.common_heads)
            heads["hm"] = (num_cls, self.num_hm_conv)
            self.tasks.append(SepHead(self.share_conv_channel, heads, head_conv=64, final_kernel=3, bn=True, init_bias=init_bias))
        if logger is not None:
            logger.info("Finish CenterHead Initialization")

        # HIP-side state (not parameters, not in state_dict); `_cache` (frozen.py) holds the packed layers, slots "shared" and the task index
        self._packed = None      # (shared layer, [per task (first-convs layer, final convs, widths array, names, channel counts)]) of this forward
        self._bufs = None        # the shared map and the tasks' 64 x heads map

    # ---- the nn form --------------------------------------------------------------------------------------------
    def forward_layers(self, x):
        x = self.shared_conv(x)
        return [task(x) for task in self.tasks]

    # ---- kernel path --------------------------------------------------------------------------------------------
    def _layout(self):
        """None when a layer is outside what the kernels serve; else per task [(name, first conv, bn, last conv)]."""
        def bn_ok(bn):
            return frozen.servable_norm(bn, nn.BatchNorm2d)

        sc = self.shared_conv
        if not (isinstance(sc[0], nn.Conv2d) and bn_ok(sc[1])):
            return None
        lay = []
        for task in self.tasks:
            heads = []
            for name in task.heads:
                fc = getattr(task, name)
                if len(fc) != 4 or not (isinstance(fc[0], nn.Conv2d) and bn_ok(fc[1]) and isinstance(fc[3], nn.Conv2d)):
                    return None
                if fc[0].out_channels != 64 or not 1 <= fc[3].out_channels <= 3:
                    return None
                heads.append((name, fc[0], fc[1], fc[3]))
            if not 1 <= len(heads) <= 16:
                return None
            lay.append(heads)
        return lay if lay else None

    @staticmethod
    def _bn_tensors(conv, bn):
        return [conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]

    def _task_tensors(self, heads):
        return [t for _, c0, bn, c3 in heads for t in self._bn_tensors(c0, bn) + [c3.weight, c3.bias]]

    def _kernel_path(self, x, lay):
        if self.training or lay is None or x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda:
            return False
        params = self._bn_tensors(self.shared_conv[0], self.shared_conv[1]) + [t for heads in lay for t in self._task_tensors(heads)]
        return frozen.all_fp32(params) and not frozen.wants_autograd(x, params)

    @staticmethod
    def _pack_bn_layer(lib, convs, bns, dev):
        """One SHASTA_NECK_C3S1 layer from the (concatenated) convolutions and BatchNorms, the bias folded into the mean."""
        cat = (lambda ts: (ts[0].detach() if len(ts) == 1 else torch.cat([t.detach() for t in ts], 0)).to(dev))
        w = cat([c.weight for c in convs]).contiguous()
        mean = (cat([b.running_mean for b in bns]) - cat([c.bias for c in convs])).contiguous()
        gamma, beta, var = (cat([getattr(b, n) for b in bns]).contiguous() for n in ("weight", "bias", "running_var"))
        eps = {float(b.eps) for b in bns}
        if len(eps) != 1:
            raise hip.ShastaHipError("CenterHead: the heads of a task must share one BatchNorm eps")
        cout, cin = w.shape[0], w.shape[1]
        nbytes = lib.shasta_neck_layer_packed_bytes(0, cin, cout)
        if nbytes == 0:
            raise hip.ShastaHipError("CenterHead: layer %d -> %d channels is not served by shasta_neck_layer_f32" % (cin, cout))
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        hip.check(lib.shasta_neck_layer_pack_f32(hip.ptr(w), hip.ptr(gamma), hip.ptr(beta), hip.ptr(mean), hip.ptr(var), eps.pop(), 0, cin, cout,
                                                 hip.ptr(buf), nbytes, hip.stream_ptr()), "shasta_neck_layer_pack_f32")
        return buf

    @staticmethod
    def _pack_final(convs, dev):
        """include/shasta_hip.h shasta_head_final_f32: per head [cc 16][tap 9][kq 4][i 4] weights, bias[4]."""
        out = torch.zeros(len(convs), 576 * 4 + 4, dtype=torch.float32, device=dev)
        for h, c in enumerate(convs):
            k = c.out_channels
            w4 = torch.zeros(4, 64, 9, dtype=torch.float32, device=dev)
            w4[:k] = c.weight.detach().to(dev).reshape(k, 64, 9)
            out[h, :2304] = w4.reshape(4, 16, 4, 9).permute(1, 3, 2, 0).reshape(-1)  # [i][cc][kq][tap] -> [cc][tap][kq][i]
            out[h, 2304:2304 + k] = c.bias.detach().to(dev)
        return out

    def _ensure_packed(self, lay, dev):
        """The shared layer and one entry per task, each packed for its own tensors as they are."""
        lib = hip.load()
        sc = self.shared_conv

        def task(heads):
            first = self._pack_bn_layer(lib, [h[1] for h in heads], [h[2] for h in heads], dev)
            widths = (ctypes.c_int * len(heads))(*[h[3].out_channels for h in heads])
            return first, self._pack_final([h[3] for h in heads], dev), widths, [h[0] for h in heads], [h[3].out_channels for h in heads]

        shared = self._cache.get("shared", self._bn_tensors(sc[0], sc[1]), dev, lambda: self._pack_bn_layer(lib, [sc[0]], [sc[1]], dev))
        self._packed = (shared, [self._cache.get(t, self._task_tensors(heads), dev, lambda: task(heads)) for t, heads in enumerate(lay)])
        return self._packed

    def forward_raw(self, x):
        """Kernel path only: one (B, C_task, H, W) tensor per task (the heads' channels in head order), or None when `forward` would
        take `forward_layers`."""
        lay = self._layout()
        if not self._kernel_path(x, lay):
            return None
        B, cin, H, W = x.shape
        if cin != self.in_channels:
            raise ValueError("CenterHead: expected %d input channels, got %d" % (self.in_channels, cin))
        lib = hip.load()
        share = self.share_conv_channel
        for heads in lay:
            widths = (ctypes.c_int * len(heads))(*[h[3].out_channels for h in heads])
            if any(h[1].in_channels != share for h in heads) or not lib.shasta_head_supported(cin, share, len(heads), widths, H, W):
                return None
        dev = x.device
        shared, tasks = self._ensure_packed(lay, dev)
        x = x.contiguous()
        hmax = max(len(heads) for heads in lay)
        need = (B * share * H * W, B * 64 * hmax * H * W)
        if self._bufs is None or self._bufs[0].device != dev or any(b.numel() < n for b, n in zip(self._bufs, need)):
            self._bufs = None
            self._bufs = [torch.empty(n, dtype=torch.float32, device=dev) for n in need]
        s_map, t_map = self._bufs
        stream = hip.stream_ptr()
        hip.check(lib.shasta_neck_layer_f32(hip.ptr(x), B, cin, H, W, hip.ptr(shared), shared.numel(), 0, share, hip.ptr(s_map), share, 0, stream),
                  "shasta_neck_layer_f32")
        outs = []
        for first, final, widths, names, chans in tasks:
            nh = len(names)
            hip.check(lib.shasta_neck_layer_f32(hip.ptr(s_map), B, share, H, W, hip.ptr(first), first.numel(), 0, 64 * nh, hip.ptr(t_map), 64 * nh, 0,
                                                stream), "shasta_neck_layer_f32")
            out = torch.empty(B, sum(chans), H, W, dtype=torch.float32, device=dev)
            hip.check(lib.shasta_head_final_f32(hip.ptr(t_map), B, nh, widths, H, W, hip.ptr(final), final.numel() * 4, hip.ptr(out), stream),
                      "shasta_head_final_f32")
            outs.append(out)
        return outs

    def forward(self, x):
        raws = self.forward_raw(x)
        if raws is None:
            return self.forward_layers(x)
        rets = []
        for raw, (_, _, _, names, chans) in zip(raws, self._packed[1]):
            d, at = {}, 0
            for name, k in zip(names, chans):
                d[name] = raw[:, at:at + k]
                at += k
            rets.append(d)
        return rets

    # ---- losses -------------------------------------------------------------------------------------------------
    def loss(self, example, preds_dicts, test_cfg=None, **kwargs):
        from . import head_loss
        if str(self.dataset).lower() not in ("nuscenes", "nuscenesdataset"):
            raise NotImplementedError("CenterHead.loss: only nuScenes is served (dataset=%r)" % (self.dataset,))
        if len(preds_dicts) != len(self.tasks):
            raise ValueError("CenterHead.loss: %d prediction dicts for %d tasks" % (len(preds_dicts), len(self.tasks)))
        missing = [k for k in ("hm", "anno_box", "ind", "mask", "cat") if k not in example]
        if missing:
            raise NotImplementedError("CenterHead.loss: a loss without targets is not served - the example lacks %s (targets.AssignLabel / "
                                      "targets.assign_targets make them)" % missing)
        if len(self.code_weights) != 10:
            raise ValueError("CenterHead.loss: code_weights must hold ten values, one per anno_box channel (got %d)" % len(self.code_weights))
        return head_loss.center_loss(preds_dicts, example, self.weight, self.code_weights)

    # ---- detections ---------------------------------------------------------------------------------------------
    @torch.no_grad()
    def predict(self, example, preds_dicts, test_cfg):
        nms_cfg = _get(test_cfg, "nms")
        if not _get(nms_cfg, "use_rotate_nms", True):
            raise NotImplementedError("CenterHead.predict: only rotated NMS is served (use_rotate_nms=False)")
        if _get(nms_cfg, "use_multi_class_nms", False):
            raise NotImplementedError("CenterHead.predict: use_multi_class_nms is not served")
        if _get(test_cfg, "circular_nms", False) or _get(test_cfg, "double_flip", False):
            raise NotImplementedError("CenterHead.predict: circle NMS and the double-flip merge are not served")
        pre_max, post_max = int(_get(nms_cfg, "nms_pre_max_size")), int(_get(nms_cfg, "nms_post_max_size"))
        iou_thr = float(_get(nms_cfg, "nms_iou_threshold"))
        _ = _get(test_cfg, "max_per_img")  # read, not applied (see the module docstring)
        rng = [float(v) for v in _get(test_cfg, "post_center_limit_range")]
        pc, vs = _get(test_cfg, "pc_range"), _get(test_cfg, "voxel_size")
        if len(preds_dicts) != len(self.tasks):
            raise ValueError("CenterHead.predict: %d prediction dicts for %d tasks" % (len(preds_dicts), len(self.tasks)))
        for n in _BOX_HEADS:
            if n not in self.common_heads:
                raise NotImplementedError("CenterHead.predict: the decode needs the heads %s" % (_BOX_HEADS,))
        for t, pd in enumerate(preds_dicts):
            if not all(pd[n].is_cuda for n in self.tasks[t].heads):
                raise hip.ShastaHipError("CenterHead.predict needs device tensors; there is no CPU path")
        lib = hip.load()
        stream = hip.stream_ptr()
        per_task, B, dev = [], None, None
        for t, pd in enumerate(preds_dicts):
            names = list(self.tasks[t].heads)
            raw = torch.cat([pd[n].float() for n in names], 1).contiguous()
            B, C, H, W = raw.shape
            dev = raw.device
            cfg = hip.HeadDecodeCfg()
            at = 0
            for n in names:
                setattr(cfg, n, at)
                at += pd[n].shape[1]
            cfg.num_class = self.num_classes[t]
            cfg.out_size_factor, cfg.voxel_x, cfg.voxel_y = float(_get(test_cfg, "out_size_factor")), float(vs[0]), float(vs[1])
            cfg.pc_x, cfg.pc_y, cfg.score_threshold = float(pc[0]), float(pc[1]), float(_get(test_cfg, "score_threshold"))
            cfg.range = (ctypes.c_float * 6)(*rng)
            cand = decode_candidates(raw, cfg)
            pre = min(pre_max, H * W)
            order = torch.sort(cand["score"], dim=1, descending=True, stable=True)[1][:, :pre]  # ties: the lower pixel first
            box = torch.gather(cand["box"], 1, order[..., None].expand(-1, -1, 9))
            score = torch.gather(cand["score"], 1, order)
            label = torch.gather(cand["label"], 1, order).long() + sum(self.num_classes[:t])
            if pre < pre_max:  # (maps smaller than the cut: pad the segment rows to one width)
                pad = pre_max - pre
                box, score, label = (torch.cat([v, v.new_zeros((B, pad) + v.shape[2:])], 1) for v in (box, score, label))
            per_task.append((box, score, label, cand["count"].clamp(max=pre)))
        T = len(per_task)
        S = T * B
        box = torch.stack([p[0] for p in per_task]).reshape(S * pre_max, 9)      # segment s = t * B + b
        score = torch.stack([p[1] for p in per_task]).reshape(S * pre_max)
        label = torch.stack([p[2] for p in per_task]).reshape(S * pre_max)
        n = torch.stack([p[3] for p in per_task]).reshape(S)
        # the segments' valid rows to the front, order kept: a stable sort on the invalid flag
        invalid = (torch.arange(pre_max, device=dev)[None, :] >= n[:, None]).reshape(-1).to(torch.uint8)
        perm = torch.sort(invalid, stable=True)[1]
        box, score, label = box[perm], score[perm], label[perm]
        offsets = torch.zeros(S + 1, dtype=torch.int32, device=dev)
        offsets[1:] = torch.cumsum(n, 0)
        nb = box[:, [0, 1, 2, 4, 3, 5, 8]]  # nms.rotate_nms_pcdet's conversion
        nb[:, -1] = -nb[:, -1] - math.pi / 2
        nb = nb.contiguous()
        keep = torch.empty(S, pre_max, dtype=torch.int32, device=dev)
        num_keep = torch.zeros(S, dtype=torch.int32, device=dev)
        ws_bytes = lib.shasta_nms_batch_workspace_bytes(S, pre_max)
        ws = torch.empty((ws_bytes + 7) // 8, dtype=torch.float64, device=dev)
        hip.check(lib.shasta_nms_rotated_batch_f32(hip.ptr(nb), hip.ptr(offsets), S, pre_max, iou_thr, hip.ptr(ws), ws_bytes, hip.ptr(keep),
                                                   hip.ptr(num_keep), stream), "shasta_nms_rotated_batch_f32")
        counts = torch.stack([num_keep, n.to(torch.int32)]).cpu().tolist()  # the one copy to the host
        first = [0]
        for v in counts[1]:
            first.append(first[-1] + v)
        meta = example.get("metadata") if hasattr(example, "get") else None
        rets = []
        for b in range(B):
            sel = [keep[t * B + b, :min(counts[0][t * B + b], post_max)].long() + first[t * B + b] for t in range(T)]
            sel = torch.cat(sel)
            rets.append(dict(box3d_lidar=box[sel], scores=score[sel], label_preds=label[sel], metadata=None if meta is None else meta[b]))
        return rets


def decode_candidates(raw, cfg, cap=None):
    """`shasta_head_decode_f32` on one task's raw (B, C, H, W) maps: dict(box (B, cap, 9), score (B, cap) - rows past the count hold -inf -,
    label (B, cap) int32, pixel (B, cap) int32, count (B,) int32), everything on the device.  `cap` defaults to H * W."""
    lib = hip.load()
    B, C, H, W = raw.shape
    cap = H * W if cap is None else int(cap)
    dev = raw.device
    box = torch.zeros(B, cap, 9, dtype=torch.float32, device=dev)
    score = torch.full((B, cap), float("-inf"), dtype=torch.float32, device=dev)
    label = torch.zeros(B, cap, dtype=torch.int32, device=dev)
    pixel = torch.full((B, cap), -1, dtype=torch.int32, device=dev)
    count = torch.zeros(B, dtype=torch.int32, device=dev)
    ws_bytes = lib.shasta_head_decode_workspace_bytes(B, H, W)
    ws = torch.empty(max(ws_bytes, 4) // 4, dtype=torch.int32, device=dev)
    hip.check(lib.shasta_head_decode_f32(hip.ptr(raw), B, C, H, W, ctypes.byref(cfg), cap, hip.ptr(box), hip.ptr(score), hip.ptr(label),
                                         hip.ptr(pixel), hip.ptr(count), hip.ptr(ws), ws_bytes, hip.stream_ptr()), "shasta_head_decode_f32")
    return dict(box=box, score=score, label=label, pixel=pixel, count=count)
