"""`RPN`: the neck between the backbone and K0, with the reference's module API, computed layer by layer by csrc/neck.hip.

Mirror of det3d/models/necks/rpn.py:24-163 (`RPN`): same constructor keywords and asserts (:25-65), same sub-module creation
order (module creation order = RNG order, so a seeded default init gives the reference's tensors), same `state_dict` keys
(`blocks.<i>.<j>.*` with the ZeroPad2d at index 0, `deblocks.<i>.<j>.*`): a reference checkpoint's `neck.*` entries load as they are.

`forward` has two paths:
  * the kernel path - device tensors, `eval()` mode, autograd off, every layer served by `shasta_neck_layer_f32` (BatchNorm2d norm,
    ds strides 1 / 2, us strides 1 / 2, fp32): one `shasta_neck_layer_f32` call per conv + BatchNorm + ReLU on the current stream,
    intermediates in two ping-pong buffers the module owns, the two deblocks writing their channel slices of the result in place
    (no pass for `torch.cat`).  After a warm-up call there is no host synchronisation and no allocation but the result: the call can
    be captured in `torch.cuda.graph`.  A CPU tensor on this path raises: there is no CPU fallback.
  * `forward_layers` - the module's own nn layers, the reference's `forward` restated - for everything outside that set: `train()`
    mode by default (the reference keeps the frozen neck's BatchNorms on batch statistics while training,
    tools/nusc_shasta/train.py:193), autograd on, other norms, other strides, other dtypes.  The same arrangement as shared_conv's
    documented exceptions.

TRAIN() MODE ON THE KERNELS (`batch_statistics=True`, or the attribute set later; the default keeps `forward_layers`): with autograd
off or nothing requiring grad, a `train()`-mode call takes the kernel path too.  torch's rule per layer: where `bn.training` is true
the layer is four calls into its destination (a ping-pong buffer or the output slice) - `shasta_neck_layer_raw_f32` (the eval kernels
without the epilogue's affine and ReLU, reading the weight section of the SAME packed buffer: nothing is re-packed per step),
`shasta_bn_maps_stats_f32` (float64 sums, fixed tree: the same bits on every run), `shasta_bn_maps_finalize_f32` (updates
`running_mean`, `running_var`, `num_batches_tracked` of the module in place: momentum, unbiased variance) and `shasta_bn_maps_apply_f32`
(in place); where it is false the layer is the eval one.  The kernels write the running statistics through raw pointers, which bumps no
version counter, so a forward marks the alpha / beta' of the layers it updated as stale and the next eval use re-packs them.  The
statistics workspace and the `stat` buffers live with the ping-pong buffers: no host synchronisation, no allocation but the result,
capturable.  `n = B * OH * OW < 2` raises ValueError as torch does; `momentum=None` raises `ShastaHipError`.

SYNCHRONISED STATISTICS: the plan follows the modules (`_plan`), so after `sync_bn.convert_syncbn_model` - the reference's training run,
tools/nusc_shasta/train.py:155-156 - the layers read the new `SyncBatchNorm` modules and their `training` flags.  A `SyncBatchNorm`
layer on batch statistics whose process group has more than one rank normalises with the statistics of ALL ranks' maps: the stats
kernel writes the front of the local record, one all-gather, `shasta_bn_sync_finalize_f32` (csrc/bn_sync.hip: the merge on the device,
no host read), apply - `sync_bn.RankStats`, kept with the other buffers.  The running statistics are bit-equal on all ranks; the count
refusal does not apply (every rank has B >= 1).  The set of layers on batch statistics must be the same on every rank (the reference's
frozen set-up guarantees it); a rank that raises before a collective leaves the others to torch.distributed's timeout, as with any
collective.  The collective is not capturable in a graph.  World 1, or no initialised process group: the calls and bits of BatchNorm2d.
"""
import ctypes

import numpy as np
import torch
from torch import nn

from . import hip, sync_bn
from .registry import NECKS

C3S1, C3S2, C1, D2 = 0, 1, 2, 3  # include/shasta_hip.h SHASTA_NECK_*


def build_norm_layer(cfg, num_features):
    """det3d/models/utils/norm.py:67-108 for the types the neck configs use: dict(type="BN" | "BN1d" | "GN", eps=1e-5, requires_grad=True, ...)."""
    if not (isinstance(cfg, dict) and "type" in cfg):
        raise AssertionError("norm_cfg must be a dict with a 'type' key")
    kw = dict(cfg)
    kind = kw.pop("type")
    requires_grad = kw.pop("requires_grad", True)
    kw.setdefault("eps", 1e-5)
    if kind == "BN":
        layer = nn.BatchNorm2d(num_features, **kw)
    elif kind == "BN1d":
        layer = nn.BatchNorm1d(num_features, **kw)
    elif kind == "GN":
        if "num_groups" not in kw:
            raise AssertionError("GN needs num_groups")
        layer = nn.GroupNorm(num_channels=num_features, **kw)
    else:
        raise KeyError("Unrecognized norm type {}".format(kind))
    for p in layer.parameters():
        p.requires_grad = requires_grad
    return layer


@NECKS.register_module
class RPN(nn.Module):
    def __init__(self, layer_nums, ds_layer_strides, ds_num_filters, us_layer_strides, us_num_filters, num_input_features,
                 norm_cfg=None, name="rpn", logger=None, batch_statistics=False, **kwargs):
        super().__init__()
        self.batch_statistics = bool(batch_statistics)  # serve train() mode with batch-statistics BatchNorm2d (csrc/bn_maps.hip)
        self._layer_strides = ds_layer_strides
        self._num_filters = ds_num_filters
        self._layer_nums = layer_nums
        self._upsample_strides = us_layer_strides
        self._num_upsample_filters = us_num_filters
        self._num_input_features = num_input_features
        self._norm_cfg = dict(type="BN", eps=1e-3, momentum=0.01) if norm_cfg is None else norm_cfg

        assert len(self._layer_strides) == len(self._layer_nums)
        assert len(self._num_filters) == len(self._layer_nums)
        assert len(self._num_upsample_filters) == len(self._upsample_strides)
        self._upsample_start_idx = len(self._layer_nums) - len(self._upsample_strides)
        # every deblock must bring its block back to the same resolution
        ratios = [self._upsample_strides[i] / np.prod(self._layer_strides[: i + self._upsample_start_idx + 1])
                  for i in range(len(self._upsample_strides))]
        for r in ratios:
            assert r == ratios[0]

        in_filters = [self._num_input_features, *self._num_filters[:-1]]
        blocks, deblocks = [], []
        for i, layer_num in enumerate(self._layer_nums):
            blocks.append(self._make_layer(in_filters[i], self._num_filters[i], layer_num, stride=self._layer_strides[i]))
            k = i - self._upsample_start_idx
            if k >= 0:
                stride, planes = self._upsample_strides[k], self._num_upsample_filters[k]
                if stride > 1:
                    conv = nn.ConvTranspose2d(self._num_filters[i], planes, stride, stride=stride, bias=False)
                else:  # us stride <= 1 is a strided Conv2d in the reference (stride 1: a 1x1 convolution)
                    stride = int(np.round(1 / stride))
                    conv = nn.Conv2d(self._num_filters[i], planes, stride, stride=stride, bias=False)
                deblocks.append(nn.Sequential(conv, build_norm_layer(self._norm_cfg, planes), nn.ReLU()))
        self.blocks = nn.ModuleList(blocks)
        self.deblocks = nn.ModuleList(deblocks)
        if logger is not None:
            logger.info("Finish RPN Initialization")

        # HIP-side state (not parameters, not in state_dict)
        self._packed = None      # one byte tensor per layer
        self._packed_key = None  # one (pointer, version) key per layer
        self._stale = set()      # layers whose running statistics the kernels wrote: weights packed, alpha / beta' out of date
        self._bufs = None        # the two ping-pong buffers
        self._train_bufs = None  # train() mode: mean_m2, stat, the statistics workspace
        self._rank_stats = None  # train() mode with a SyncBatchNorm over several ranks: the record and gather buffers (sync_bn.RankStats)
        self._plan_now = None    # the chain of kernel layers and the module identities it was built from: see `_plan`
        self._plan_ids = None

    def _make_layer(self, inplanes, planes, num_blocks, stride=1):
        layers = [nn.ZeroPad2d(1), nn.Conv2d(inplanes, planes, 3, stride=stride, bias=False),
                  build_norm_layer(self._norm_cfg, planes), nn.ReLU()]
        for _ in range(num_blocks):
            layers += [nn.Conv2d(planes, planes, 3, padding=1, bias=False), build_norm_layer(self._norm_cfg, planes), nn.ReLU()]
        return nn.Sequential(*layers)

    @property
    def downsample_factor(self):
        factor = np.prod(self._layer_strides)
        if len(self._upsample_strides) > 0:
            factor /= self._upsample_strides[-1]
        return factor

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight, gain=1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    # ---- the reference's forward, restated ------------------------------------------------------------------
    def forward_layers(self, x):
        ups = []
        for i, block in enumerate(self.blocks):
            x = block(x)
            if i - self._upsample_start_idx >= 0:
                ups.append(self.deblocks[i - self._upsample_start_idx](x))
        if len(ups) > 0:
            x = torch.cat(ups, dim=1)
        return x

    # ---- kernel path ----------------------------------------------------------------------------------------
    @property
    def _plan(self):
        """The plan follows the modules: it is rebuilt - and the packed layers are dropped with it - when the identity of any module
        under `blocks` / `deblocks` differs from the one it was built from (`sync_bn.convert_syncbn_model` swaps new BatchNorm modules
        in, which share the old ones' tensors; the old objects' `training` flag no longer follows `train()` / `eval()`)."""
        ids = tuple(id(m) for seq in (*self.blocks, *self.deblocks) for m in seq)
        if ids != self._plan_ids:
            self._plan_now, self._plan_ids = self._make_plan(), ids
            self._packed = self._packed_key = None
            self._stale = set()
        return self._plan_now

    def _make_plan(self):
        """The chain of kernel layers: [(kind, conv, bn, role)], role = "block" or the deblock's index; None when a layer is outside what
        shasta_neck_layer_f32 serves (the shapes are checked per call, they depend on H and W)."""
        if len(self.deblocks) == 0:
            return None  # (the reference then returns the last block's map; not a configuration any shipped config uses)
        plan = []

        def bn_ok(bn):
            return isinstance(bn, (nn.BatchNorm2d, sync_bn.SyncBatchNorm)) and bn.affine and bn.track_running_stats

        for i, block in enumerate(self.blocks):
            mods = list(block)
            first, rest = mods[1:4], mods[4:]
            stride = first[0].stride[0]
            if stride not in (1, 2) or not bn_ok(first[1]):
                return None
            plan.append((C3S1 if stride == 1 else C3S2, first[0], first[1], "block"))
            for j in range(0, len(rest), 3):
                if not bn_ok(rest[j + 1]):
                    return None
                plan.append((C3S1, rest[j], rest[j + 1], "block"))
            k = i - self._upsample_start_idx
            if k >= 0:
                conv, bn = self.deblocks[k][0], self.deblocks[k][1]
                if not bn_ok(bn):
                    return None
                if isinstance(conv, nn.ConvTranspose2d) and conv.stride[0] == 2:
                    plan.append((D2, conv, bn, k))
                elif isinstance(conv, nn.Conv2d) and conv.kernel_size[0] == 1:
                    plan.append((C1, conv, bn, k))
                else:
                    return None
        return plan

    def _apply(self, fn, *a, **k):  # .to() / .cuda() / .float(): parameter storage moves -> drop the packed layers
        self.invalidate_weights_cache()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self.invalidate_weights_cache()
        return super().load_state_dict(*a, **k)

    def invalidate_weights_cache(self):
        """Forget the packed layers; the next kernel-path forward re-packs them.  They follow in-place writes, optimizer steps and
        load_state_dict by themselves (pointer + version checks); call this after a write that bumps no version counter."""
        self._packed_key = None
        self._stale = set()

    @staticmethod
    def _tensors(conv, bn):
        return [conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var]

    def _ensure_packed(self, dev, batch=()):
        """Every layer packed for its tensors as they are (pointer + version key per layer).  A layer in `batch` (it runs on batch
        statistics in this forward) reads the weight section only, so alpha / beta' marked stale by an earlier train() forward do not
        make it re-pack; every other layer is re-packed when stale."""
        if self._packed is None or self._packed_key is None:
            self._packed, self._packed_key, self._stale = [None] * len(self._plan_now), [None] * len(self._plan_now), set()
        lib = hip.load()
        packed = self._packed
        for i, (kind, conv, bn, _) in enumerate(self._plan_now):
            key = tuple((t.data_ptr(), t._version) for t in self._tensors(conv, bn)) + (str(dev),)
            if packed[i] is not None and self._packed_key[i] == key and (i in batch or i not in self._stale):
                continue
            ts = [t.detach().contiguous() for t in self._tensors(conv, bn)]
            cin, cout = conv.in_channels, conv.out_channels
            if kind == C1:  # the reference's 1x1 deblock is a Conv2d, (Cout, Cin, 1, 1); the C1 kind takes ConvTranspose2d's (Cin, Cout, 1, 1)
                ts[0] = ts[0].reshape(cout, cin).t().contiguous()
            nbytes = lib.shasta_neck_layer_packed_bytes(kind, cin, cout)
            if nbytes == 0:
                raise hip.ShastaHipError("RPN: layer %d -> %d channels is not served by shasta_neck_layer_f32" % (cin, cout))
            buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            hip.check(lib.shasta_neck_layer_pack_f32(*[hip.ptr(t) for t in ts], float(bn.eps), kind, cin, cout, hip.ptr(buf), nbytes,
                                                     hip.stream_ptr()), "shasta_neck_layer_pack_f32")
            packed[i], self._packed_key[i] = buf, key
            self._stale.discard(i)

    def _shapes(self, H, W):
        """Per layer of the plan: (H, W) of its input and of its output; None when a layer is not served at this map size."""
        lib = hip.load()
        shapes, out_hw = [], None
        for kind, conv, _, role in self._plan:
            h, w = H, W  # (a deblock reads its block's last map)
            if not lib.shasta_neck_layer_supported(kind, conv.in_channels, conv.out_channels, h, w):
                return None
            oh, ow = (h // 2, w // 2) if kind == C3S2 else (2 * h, 2 * w) if kind == D2 else (h, w)
            shapes.append((h, w, oh, ow))
            if role == "block":
                H, W = oh, ow
            else:
                if out_hw is not None and out_hw != (oh, ow):
                    raise ValueError("RPN: the deblocks' maps differ in size (%s vs %s): H and W must be multiples of the total "
                                     "downsampling stride" % (out_hw, (oh, ow)))
                out_hw = (oh, ow)
        return shapes

    def _batch_layers(self, B, shapes):
        """Indices of the plan's layers that run on batch statistics in this forward: torch's rule per BatchNorm module.  torch's
        refusals for them are made here, before any launch."""
        if not (self.training and self.batch_statistics):
            return frozenset()
        lib = hip.load()
        batch = []
        for i, ((_, conv, bn, _), s) in enumerate(zip(self._plan_now, shapes)):
            if not bn.training:
                continue
            if bn.momentum is None:
                raise hip.ShastaHipError("RPN: BatchNorm2d(momentum=None) (cumulative averaging of the running statistics) is not served "
                                         "in train() mode")
            if B * s[2] * s[3] < 2 and sync_bn.synced_world(bn) == 1:  # (several ranks: B >= 1 each, at least 2 values in total)
                raise ValueError("Expected more than 1 value per channel when training, got input size %s"
                                 % (torch.Size([B, conv.out_channels, s[2], s[3]]),))
            if not lib.shasta_bn_maps_supported(conv.out_channels):
                raise hip.ShastaHipError("RPN: batch statistics over maps of %d channels are not served" % conv.out_channels)
            batch.append(i)
        return frozenset(batch)

    def _ensure_train_bufs(self, B, shapes, batch, dev):
        lib = hip.load()
        cmax = max(self._plan_now[i][1].out_channels for i in batch)
        need = max(lib.shasta_bn_maps_workspace_bytes(B, self._plan_now[i][1].out_channels, shapes[i][2] * shapes[i][3]) for i in batch)
        tb = self._train_bufs
        if tb is None or tb[0].device != dev or tb[0].numel() < 2 * cmax or tb[2].numel() < need:
            self._train_bufs = None
            tb = self._train_bufs = (torch.empty(2 * cmax, dtype=torch.float32, device=dev), torch.empty(2 * cmax, dtype=torch.float32, device=dev),
                                     torch.empty(need, dtype=torch.uint8, device=dev))
        return tb

    def _ensure_rank_stats(self, width, world, dev):
        rs = self._rank_stats
        if rs is None or rs.width < width or rs.world < world or rs.device != dev:
            self._rank_stats = None
            rs = self._rank_stats = sync_bn.RankStats(width, world, dev)
        return rs

    def _kernel_path(self, x):
        if (self.training and not self.batch_statistics) or self._plan is None or x.dim() != 4 or x.dtype != torch.float32:
            return False
        params = [t for _, conv, bn, _ in self._plan_now for t in self._tensors(conv, bn)]
        if any(t.dtype != torch.float32 for t in params):
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in params)):
            return False
        return True

    def forward(self, x):
        if not self._kernel_path(x):
            return self.forward_layers(x)
        if not x.is_cuda:
            raise hip.ShastaHipError("RPN: expected a device tensor (the HIP path has no CPU fallback; forward_layers is the nn form)")
        B, cin, H, W = x.shape
        if cin != self._num_input_features:
            raise ValueError("RPN: expected %d input channels, got %d" % (self._num_input_features, cin))
        shapes = self._shapes(H, W)
        if shapes is None:
            return self.forward_layers(x)
        lib = hip.load()
        dev = x.device
        batch = self._batch_layers(B, shapes)
        self._ensure_packed(dev, batch)
        x = x.contiguous()
        need = max([B * conv.out_channels * s[2] * s[3] for (_, conv, _, role), s in zip(self._plan_now, shapes) if role == "block"])
        if self._bufs is None or self._bufs[0].numel() < need or self._bufs[0].device != dev:
            self._bufs = None
            self._bufs = [torch.empty(need, dtype=torch.float32, device=dev) for _ in range(2)]
        ctot = sum(self._num_upsample_filters)
        offs = np.concatenate([[0], np.cumsum(self._num_upsample_filters)]).tolist()
        oh, ow = next(s[2:] for (_, _, _, role), s in zip(self._plan_now, shapes) if role != "block")
        out = torch.empty(B, ctot, oh, ow, dtype=torch.float32, device=dev)
        stream = hip.stream_ptr()
        if batch:
            mm, stat, ws = self._ensure_train_bufs(B, shapes, batch, dev)
            worlds = {i: sync_bn.synced_world(self._plan_now[i][2]) for i in batch}  # > 1: statistics shared with other ranks
            if max(worlds.values()) > 1:
                ranks = self._ensure_rank_stats(max(self._plan_now[i][1].out_channels for i in batch if worlds[i] > 1), max(worlds.values()), dev)
        cur, nxt = x, 0
        for i, ((kind, conv, bn, role), pk, s) in enumerate(zip(self._plan_now, self._packed, shapes)):
            if role == "block":
                dst, total, off = self._bufs[nxt], conv.out_channels, 0
            else:
                dst, total, off = out, ctot, int(offs[role])
            args = (hip.ptr(cur), B, conv.in_channels, s[0], s[1], hip.ptr(pk), pk.numel(), kind, conv.out_channels, hip.ptr(dst), total, off,
                    stream)
            if i in batch:  # raw convolution into the destination, batch statistics of it, finalize, apply in place
                C, plane = conv.out_channels, s[2] * s[3]
                hip.check(lib.shasta_neck_layer_raw_f32(*args), "shasta_neck_layer_raw_f32")
                world = worlds[i]
                local = ranks.local(C, world) if world > 1 else mm  # (several ranks: the front of the local record)
                hip.check(lib.shasta_bn_maps_stats_f32(hip.ptr(dst), B, C, plane, total, off, hip.ptr(local), hip.ptr(ws), ws.numel(), stream),
                          "shasta_bn_maps_stats_f32")
                self._stale.add(i)  # (before the launch that writes the running statistics)
                if world > 1:  # one all-gather of the record, the merged finalize on the device
                    ranks.finalize(bn, C, B * plane, stat, stream)
                else:
                    hip.check(lib.shasta_bn_maps_finalize_f32(hip.ptr(mm), C, float(B * plane), float(bn.eps), float(bn.momentum), hip.ptr(stat),
                                                              hip.ptr(bn.running_mean), hip.ptr(bn.running_var),
                                                              ctypes.c_void_p(bn.num_batches_tracked.data_ptr()), stream),
                              "shasta_bn_maps_finalize_f32")
                hip.check(lib.shasta_bn_maps_apply_f32(hip.ptr(dst), B, C, plane, total, off, hip.ptr(stat), hip.ptr(bn.weight.detach()),
                                                       hip.ptr(bn.bias.detach()), 1, stream), "shasta_bn_maps_apply_f32")
            else:
                hip.check(lib.shasta_neck_layer_f32(*args), "shasta_neck_layer_f32")
            if role == "block":
                cur, nxt = dst, nxt ^ 1
        return out
