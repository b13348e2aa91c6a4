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
import numpy as np
import torch
from torch import nn

from . import frozen, hip, sync_bn
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
class RPN(frozen.FrozenStage):
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

        # HIP-side state (not parameters, not in state_dict); `_cache` (frozen.py) holds the packed layers, slot = index in the plan
        self._packed = None      # this forward's packed layers: one byte tensor per layer, in plan order
        self._bufs = None        # the two ping-pong buffers
        self._train_bufs = frozen.BatchStatistics(self._cache, "shasta_bn_maps_finalize_f32")  # train() mode: mean_m2, stat, workspace
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
            self._packed = None
            self._cache.clear()
        return self._plan_now

    def _make_plan(self):
        """The chain of kernel layers: [(kind, conv, bn, role)], role = "block" or the deblock's index; None when a layer is outside what
        shasta_neck_layer_f32 serves (the shapes are checked per call, they depend on H and W)."""
        if len(self.deblocks) == 0:
            return None  # (the reference then returns the last block's map; not a configuration any shipped config uses)
        plan = []

        def bn_ok(bn):
            return frozen.servable_norm(bn, (nn.BatchNorm2d, sync_bn.SyncBatchNorm))

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

    @staticmethod
    def _tensors(conv, bn):
        return [conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var]

    def _ensure_packed(self, dev, batch=()):
        """Every layer packed for its tensors as they are.  A layer in `batch` (it runs on batch statistics in this forward) reads the
        weight section only, so alpha / beta' marked stale by an earlier train() forward do not make it re-pack."""
        self._packed = [self._cache.get(i, self._tensors(conv, bn), dev, lambda: self._pack(kind, conv, bn, dev), reads_statistics=i not in batch)
                        for i, (kind, conv, bn, _) in enumerate(self._plan_now)]

    def _pack(self, kind, conv, bn, dev):
        lib = hip.load()
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
        return buf

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
            frozen.refuse_cumulative_average("RPN", "BatchNorm2d", bn)
            frozen.refuse_single_value(bn, (B, conv.out_channels, s[2], s[3]))
            if not lib.shasta_bn_maps_supported(conv.out_channels):
                raise hip.ShastaHipError("RPN: batch statistics over maps of %d channels are not served" % conv.out_channels)
            batch.append(i)
        return frozenset(batch)

    def _kernel_path(self, x):
        if (self.training and not self.batch_statistics) or self._plan is None or x.dim() != 4 or x.dtype != torch.float32:
            return False
        params = [t for _, conv, bn, _ in self._plan_now for t in self._tensors(conv, bn)]
        return frozen.all_fp32(params) and not frozen.wants_autograd(x, params)

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
            ws_bytes = max(lib.shasta_bn_maps_workspace_bytes(B, self._plan_now[i][1].out_channels, shapes[i][2] * shapes[i][3]) for i in batch)
            self._train_bufs.reserve([self._plan_now[i][2] for i in batch], ws_bytes, dev)
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
                stat = self._train_bufs.layer(i, bn, C, B * plane, lambda mm, ws: hip.check(lib.shasta_bn_maps_stats_f32(
                    hip.ptr(dst), B, C, plane, total, off, hip.ptr(mm), hip.ptr(ws), ws.numel(), stream), "shasta_bn_maps_stats_f32"), stream)
                hip.check(lib.shasta_bn_maps_apply_f32(hip.ptr(dst), B, C, plane, total, off, hip.ptr(stat), hip.ptr(bn.weight.detach()),
                                                       hip.ptr(bn.bias.detach()), 1, stream), "shasta_bn_maps_apply_f32")
            else:
                hip.check(lib.shasta_neck_layer_f32(*args), "shasta_neck_layer_f32")
            if role == "block":
                cur, nxt = dst, nxt ^ 1
        return out
