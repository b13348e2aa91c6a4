"""`SpMiddleResNetFHD`: the sparse 3-D ResNet backbone between the reader and the neck, on csrc/sparse_conv.hip: the eval-mode forward,
and (opt-in, `batch_statistics=True`) the train()-mode forward with batch-statistics BatchNorm1d on csrc/bn_rows.hip.

Mirror of det3d/models/backbones/scn.py:52-211 (`SparseBasicBlock`, `SpMiddleResNetFHD`): same constructor keywords, same sub-module
names and order, so the `backbone.*` entries of a reference checkpoint load as they are.  spconv (CUDA only) is not imported:
`SubMConv3d` and `SparseConv3d` here are parameter holders - `weight` in the spconv 2.x layout (Cout, kD, kH, kW, Cin), optional `bias`,
kernel, stride, padding, `indice_key` - and `load_state_dict` applies the reference's rule for spconv 1.x checkpoints
(det3d/torchie/trainer/checkpoint.py:77-91).  Their default init is a plain uniform(+-1/sqrt(fan_in)); spconv's own cannot be reproduced
without spconv, so no RNG parity with the reference is claimed (the backbone is loaded from a CenterPoint checkpoint and frozen).

`forward(voxel_features, coors, batch_size, input_shape)` returns `(ret, multi_scale_voxel_features)` as the reference does: `ret` is the
dense (B, C * D, H, W) map, the dict holds `conv1` .. `conv4` as `SparseLevel` objects (`features`, `indices`, `spatial_shape`,
`batch_size`, `dense()`).  conv1's rows are in the input's order, the strided levels are sorted by linear index ((b D + z) H + y) W + x.
The four neighbour tables of the twenty submanifold convolutions (`res0` .. `res3`) are built once per level; every strided convolution
has its own.  One host synchronisation per strided level (four per forward): the row count is read back to size the next level.

There is no nn form to fall back on: a CPU tensor, a norm other than BatchNorm1d and autograd (grad mode on with a parameter or the
input requiring grad) raise `ShastaHipError`, and so does `train()` mode unless the module was built with `batch_statistics=True`.

TRAIN() MODE (`batch_statistics=True`, or the attribute set later): the forward of the reference's training step, which freezes the
backbone but leaves it in train() mode (tools/nusc_shasta/train.py:184-193).  Each (convolution, BatchNorm1d) pair follows torch's
rule: where `bn.training` is true the layer is the raw convolution into a scratch, the batch statistics of its rows (float64 sums, fixed
tree: the same bits on every run), a finalize that updates `running_mean`, `running_var` and `num_batches_tracked` of the module in place
(momentum, unbiased variance), and the apply with ReLU and the block's residual; where it is false the layer is the eval one with the
running statistics, so a backbone in train() whose BatchNorm modules are all in eval() gives the eval forward's bits.  A module in
eval() is not affected by the switch.  A level with fewer than 2 rows raises ValueError as torch does; `momentum=None` raises
`ShastaHipError`.  Levels, row orders and host synchronisations are the eval forward's.  There is no backward: the parameters stay
frozen (`requires_grad_(False)`) or the call runs under `torch.no_grad()`.

SYNCHRONISED STATISTICS: after `sync_bn.convert_syncbn_model(model)` (the reference's training run, tools/nusc_shasta/train.py:155-156)
every norm is a `sync_bn.SyncBatchNorm`.  With more than one rank in its process group, a layer on batch statistics normalises with the
statistics of ALL ranks' rows: stats kernel into the local record, one all-gather, `shasta_bn_sync_finalize_f32` (csrc/bn_sync.hip, the
merge on the device, no host read), apply - `sync_bn.RankStats`.  The running statistics are bit-equal on all ranks.  The "more than 1
value" refusal becomes a refusal of an empty local input, made before the first collective (a non-empty cloud has at least one row at
every level, and two ranks then have at least two).  The set of layers on batch statistics must be the same on every rank (the
reference's frozen set-up guarantees it); a rank that raises before a collective leaves the others to torch.distributed's timeout, as
with any collective.  World 1, or no initialised process group: the calls and the bits of the plain BatchNorm1d.

Registration: the class is NOT put into BACKBONES at import (a string config `type="SpMiddleResNetFHD"` stays a KeyError until the
user decides).  Either pass the class itself, `backbone=dict(type=shasta_amd.backbone.SpMiddleResNetFHD, num_input_features=5,
ds_factor=8)`, or call `shasta_amd.backbone.register()` once and keep the reference's string configs.
"""
import math

import numpy as np
import torch
from torch import nn

from . import frozen, hip, sync_bn
from .neck import build_norm_layer
from .registry import BACKBONES


def _triple(v):
    return tuple(int(a) for a in v) if isinstance(v, (list, tuple)) else (int(v),) * 3


class _SparseConv(nn.Module):
    """Parameter holder of one spconv convolution (spconv 2.x weight layout)."""
    subm = False

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, indice_key=None):
        super().__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.kernel_size, self.stride, self.padding = _triple(kernel_size), _triple(stride), _triple(padding)
        self.indice_key = indice_key
        self.weight = nn.Parameter(torch.empty(self.out_channels, *self.kernel_size, self.in_channels))
        self.bias = nn.Parameter(torch.empty(self.out_channels)) if bias else None
        bound = 1.0 / math.sqrt(self.in_channels * int(np.prod(self.kernel_size)))
        nn.init.uniform_(self.weight, -bound, bound)
        if self.bias is not None:
            nn.init.uniform_(self.bias, -bound, bound)

    @property
    def geometry(self):
        """(kernel, stride, padding) as the kernels take them; spconv ignores stride and padding of a submanifold convolution."""
        if self.subm:
            return self.kernel_size, (1, 1, 1), tuple(k // 2 for k in self.kernel_size)
        return self.kernel_size, self.stride, self.padding

    def _load_from_state_dict(self, state_dict, prefix, *a, **k):
        """spconv 1.x checkpoints keep (kD, kH, kW, Cin, Cout) weights: a 5-D weight of another shape is tried as transpose(-1, -2), then
        as permute(4, 0, 1, 2, 3) - the reference's rule (det3d/torchie/trainer/checkpoint.py:77-91)."""
        t = state_dict.get(prefix + "weight")
        if t is not None and t.dim() == 5 and t.shape != self.weight.shape:
            if t.transpose(-1, -2).shape == self.weight.shape:
                state_dict[prefix + "weight"] = t.transpose(-1, -2).contiguous()
            elif t.permute(4, 0, 1, 2, 3).shape == self.weight.shape:
                state_dict[prefix + "weight"] = t.permute(4, 0, 1, 2, 3).contiguous()
        return super()._load_from_state_dict(state_dict, prefix, *a, **k)

    def extra_repr(self):
        return "%d, %d, kernel_size=%s, stride=%s, padding=%s, bias=%s, indice_key=%s" % (
            self.in_channels, self.out_channels, self.kernel_size, self.stride, self.padding, self.bias is not None, self.indice_key)

    def forward(self, *a, **k):
        raise hip.ShastaHipError("%s holds parameters only: the convolution runs inside SpMiddleResNetFHD.forward" % type(self).__name__)


class SubMConv3d(_SparseConv):
    subm = True


class SparseConv3d(_SparseConv):
    pass


def conv3x3(in_planes, out_planes, stride=1, indice_key=None, bias=True):
    return SubMConv3d(in_planes, out_planes, 3, stride=stride, padding=1, bias=bias, indice_key=indice_key)


class SparseBasicBlock(nn.Module):
    """scn.py:52-95: conv1-BN-ReLU, conv2-BN, + identity, ReLU."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, norm_cfg=None, downsample=None, indice_key=None):
        super().__init__()
        if norm_cfg is None:
            norm_cfg = dict(type="BN1d", eps=1e-3, momentum=0.01)
        bias = norm_cfg is not None
        self.conv1 = conv3x3(inplanes, planes, stride, indice_key=indice_key, bias=bias)
        self.bn1 = build_norm_layer(norm_cfg, planes)
        self.relu = nn.ReLU()
        self.conv2 = conv3x3(planes, planes, indice_key=indice_key, bias=bias)
        self.bn2 = build_norm_layer(norm_cfg, planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, *a, **k):
        raise hip.ShastaHipError("SparseBasicBlock holds parameters only: it runs inside SpMiddleResNetFHD.forward")


class SparseLevel:
    """What the reference's callers read of a SparseConvTensor: one level of the backbone."""

    def __init__(self, features, indices, spatial_shape, batch_size):
        self.features, self.indices = features, indices
        self.spatial_shape, self.batch_size = list(spatial_shape), int(batch_size)

    def dense(self):
        """(B, C, D, H, W) with exact zeros at inactive sites."""
        D, H, W = self.spatial_shape
        return _dense(self.features, self.indices, self.batch_size, (D, H, W)).view(self.batch_size, -1, D, H, W)


def _dense(features, coords, B, grid):
    n, C = features.shape
    D, H, W = grid
    out = torch.empty(B, C * D, H, W, dtype=torch.float32, device=features.device)
    hip.check(hip.load().shasta_spconv_dense_f32(hip.ptr(features), hip.ptr(coords), n, B, C, D, H, W, hip.ptr(out), hip.stream_ptr()),
              "shasta_spconv_dense_f32")
    return out


class _Level:
    """Rows of one level, their index workspace, and the submanifold neighbour table shared by the level's `indice_key`."""

    def __init__(self, coords, B, grid, index):
        self.coords, self.B, self.grid, self.index = coords, B, grid, index
        self.n = int(coords.shape[0])
        self._subm = None

    def neighbors(self, out_coords, geometry):
        """(n_out, K) table of a convolution that reads this level and writes the rows `out_coords`."""
        k, s, p = geometry
        n_out = int(out_coords.shape[0])
        nbr = torch.empty(n_out, int(np.prod(k)), dtype=torch.int32, device=out_coords.device)
        hip.check(hip.load().shasta_spconv_neighbors(hip.ptr(out_coords), n_out, self.B, *self.grid, *k, *s, *p, hip.ptr(self.index),
                                                     self.index.numel(), self.n, hip.ptr(nbr), hip.stream_ptr()), "shasta_spconv_neighbors")
        return nbr

    def subm_neighbors(self, geometry):
        if self._subm is None:
            self._subm = self.neighbors(self.coords, geometry)
        return self._subm


class SpMiddleResNetFHD(frozen.FrozenStage):
    def __init__(self, num_input_features=128, norm_cfg=None, name="SpMiddleResNetFHD", batch_statistics=False, **kwargs):
        super().__init__()
        self.name = name
        self.batch_statistics = bool(batch_statistics)  # serve train() mode with batch-statistics BatchNorm1d (csrc/bn_rows.hip)
        self.dcn = None
        self.zero_init_residual = False
        if norm_cfg is None:
            norm_cfg = dict(type="BN1d", eps=1e-3, momentum=0.01)

        def bn(c):
            return build_norm_layer(norm_cfg, c)

        def block(c, key):
            return SparseBasicBlock(c, c, norm_cfg=norm_cfg, indice_key=key)

        self.conv_input = nn.Sequential(SubMConv3d(num_input_features, 16, 3, bias=False, indice_key="res0"), bn(16), nn.ReLU(inplace=True))
        self.conv1 = nn.Sequential(block(16, "res0"), block(16, "res0"))
        self.conv2 = nn.Sequential(SparseConv3d(16, 32, 3, 2, padding=1, bias=False), bn(32), nn.ReLU(inplace=True),
                                   block(32, "res1"), block(32, "res1"))
        self.conv3 = nn.Sequential(SparseConv3d(32, 64, 3, 2, padding=1, bias=False), bn(64), nn.ReLU(inplace=True),
                                   block(64, "res2"), block(64, "res2"))
        self.conv4 = nn.Sequential(SparseConv3d(64, 128, 3, 2, padding=[0, 1, 1], bias=False), bn(128), nn.ReLU(inplace=True),
                                   block(128, "res3"), block(128, "res3"))
        self.extra_conv = nn.Sequential(SparseConv3d(128, 128, (3, 1, 1), (2, 1, 1), bias=False), bn(128), nn.ReLU())

        # HIP-side state (not parameters, not in state_dict); the packed layers are in `_cache` (frozen.py): slot i is the eval pack of
        # pair i (BatchNorm folded with the running statistics), slot (i, "raw") its raw pack (conv + bias) for batch statistics
        self._stats = frozen.BatchStatistics(self._cache, "shasta_bn_rows_finalize_f32")
        self._run = None  # this forward's layers: see `_ensure_packed`

    # ---- packed layers --------------------------------------------------------------------------------------
    def _pairs(self):
        """Every (conv, norm) of the forward, in order."""
        out = [(self.conv_input[0], self.conv_input[1])]
        for seq in (self.conv1, self.conv2, self.conv3, self.conv4, self.extra_conv):
            mods = list(seq)
            if isinstance(mods[0], _SparseConv):
                out.append((mods[0], mods[1]))
            for m in mods:
                if isinstance(m, SparseBasicBlock):
                    out += [(m.conv1, m.bn1), (m.conv2, m.bn2)]
        return out

    @staticmethod
    def _tensors(conv, bn):
        ts = [conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var]
        return ts + [conv.bias] if conv.bias is not None else ts

    def _check_servable(self, voxel_features, coors):
        if self.training and not self.batch_statistics:
            raise hip.ShastaHipError("SpMiddleResNetFHD: train() mode (batch-statistics BatchNorm) is not served by default: call eval() - "
                                     "the reference loads this backbone frozen - or build the module with batch_statistics=True")
        if not (voxel_features.is_cuda and coors.is_cuda):
            raise hip.ShastaHipError("SpMiddleResNetFHD: expected device tensors (the HIP path has no CPU fallback)")
        if voxel_features.dtype != torch.float32:
            raise hip.ShastaHipError("SpMiddleResNetFHD: fp32 voxel features only, got %s" % voxel_features.dtype)
        params = []
        for conv, bn in self._pairs():
            if not frozen.servable_norm(bn, (nn.BatchNorm1d, sync_bn.SyncBatchNorm)):
                raise hip.ShastaHipError("SpMiddleResNetFHD: only BatchNorm1d (or its sync_bn.SyncBatchNorm conversion) with affine parameters "
                                         "and running statistics is served, got %s" % type(bn).__name__)
            if self.training and bn.training:
                frozen.refuse_cumulative_average("SpMiddleResNetFHD", "BatchNorm1d", bn)
            params += self._tensors(conv, bn)
        if not frozen.all_fp32(params):
            raise hip.ShastaHipError("SpMiddleResNetFHD: fp32 parameters only")
        if frozen.wants_autograd(voxel_features, params):
            raise hip.ShastaHipError("SpMiddleResNetFHD: autograd is not served (no backward): run under torch.no_grad() or freeze the "
                                     "parameters with requires_grad_(False)")

    def _ensure_packed(self, dev):
        """id(conv) -> (eval slot, packed layer, bn): every layer packed for its tensors as they are.  torch's rule per BatchNorm module:
        a layer whose `bn` is in training mode runs on batch statistics in this forward - the raw pack, and `bn` - else the eval pack, None."""
        train, run = self.training and self.batch_statistics, {}
        for i, (conv, bn) in enumerate(self._pairs()):
            raw = train and bn.training
            pk = self._cache.get((i, "raw") if raw else i, self._tensors(conv, bn), dev, lambda: self._pack(conv, bn, dev, raw),
                                 reads_statistics=not raw)
            run[id(conv)] = (i, pk, bn if raw else None)
        return run

    def _pack(self, conv, bn, dev, raw):
        lib = hip.load()
        k, s, p = conv.geometry
        cin, cout, K = conv.in_channels, conv.out_channels, int(np.prod(k))
        nbytes = lib.shasta_spconv_layer_packed_bytes(cin, cout, K) if lib.shasta_spconv_supported(cin, cout, *k, *s, *p) else 0
        if nbytes == 0:
            raise hip.ShastaHipError("SpMiddleResNetFHD: a %d -> %d convolution with kernel %s, stride %s, padding %s is not served by "
                                     "shasta_spconv_layer_f32" % (cin, cout, k, s, p))
        if any(t.device != dev for t in self._tensors(conv, bn)):
            raise hip.ShastaHipError("SpMiddleResNetFHD: parameters and input are on different devices")
        w, g, b, mean, var = [t.detach().contiguous() for t in self._tensors(conv, bn)[:5]]
        bias = None if conv.bias is None else conv.bias.detach().contiguous()
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        if raw:
            if not lib.shasta_bn_rows_supported(cout):
                raise hip.ShastaHipError("SpMiddleResNetFHD: batch statistics over rows of %d channels are not served" % cout)
            hip.check(lib.shasta_spconv_layer_pack_raw_f32(hip.ptr(w), hip.ptr(bias), cin, cout, K, hip.ptr(buf), nbytes, hip.stream_ptr()),
                      "shasta_spconv_layer_pack_raw_f32")
        else:
            hip.check(lib.shasta_spconv_layer_pack_f32(hip.ptr(w), hip.ptr(bias), hip.ptr(g), hip.ptr(b), hip.ptr(mean), hip.ptr(var),
                                                       float(bn.eps), cin, cout, K, hip.ptr(buf), nbytes, hip.stream_ptr()),
                      "shasta_spconv_layer_pack_f32")
        return buf

    # ---- forward --------------------------------------------------------------------------------------------
    @staticmethod
    def _index_buffer(B, grid, rows, dev):
        nbytes = hip.load().shasta_spconv_index_workspace_bytes(B, *grid, rows)
        if nbytes == 0:
            raise hip.ShastaHipError("SpMiddleResNetFHD: a grid of %d x %s cells is not served (2^31 cells at most)" % (B, list(grid)))
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def _layer(self, x, n_in, nbr, conv, residual=None, relu=True):
        """One layer into a new (n_out, C) tensor.  Where its BatchNorm1d is in training mode: the raw convolution, the batch statistics of
        its rows, finalize (updates the module's running statistics in place), apply in place with the residual and the ReLU."""
        lib, s = hip.load(), hip.stream_ptr()
        n_out, K = nbr.shape
        C = conv.out_channels
        slot, pk, bn = self._run[id(conv)]
        self._check_rows(conv, n_out)
        y = torch.empty(n_out, C, dtype=torch.float32, device=nbr.device)
        args = (hip.ptr(x), n_in, conv.in_channels, hip.ptr(nbr), n_out, K, hip.ptr(pk), pk.numel(), C)
        if bn is None:
            hip.check(lib.shasta_spconv_layer_f32(*args, hip.ptr(residual), 1 if relu else 0, hip.ptr(y), s), "shasta_spconv_layer_f32")
            return y
        hip.check(lib.shasta_spconv_layer_f32(*args, None, 0, hip.ptr(y), s), "shasta_spconv_layer_f32")
        stat = self._stats.layer(slot, bn, C, n_out, lambda mm, ws: hip.check(lib.shasta_bn_rows_stats_f32(
            hip.ptr(y), n_out, C, hip.ptr(mm), hip.ptr(ws), ws.numel(), s), "shasta_bn_rows_stats_f32"), s)
        hip.check(lib.shasta_bn_rows_apply_f32(hip.ptr(y), n_out, C, hip.ptr(stat), hip.ptr(bn.weight.detach()), hip.ptr(bn.bias.detach()),
                                               hip.ptr(residual), 1 if relu else 0, hip.ptr(y), s), "shasta_bn_rows_apply_f32")
        return y

    def _check_rows(self, conv, n_out):
        """torch.nn.functional.batch_norm's check for a layer on batch statistics, before any launch of that layer."""
        bn = self._run[id(conv)][2]
        if bn is not None:
            frozen.refuse_single_value(bn, (n_out, conv.out_channels))

    def _blocks(self, x, lvl, mods):
        for m in mods:
            if not isinstance(m, SparseBasicBlock):
                continue
            self._check_rows(m.conv1, lvl.n)
            nbr = lvl.subm_neighbors(m.conv1.geometry)
            h = self._layer(x, lvl.n, nbr, m.conv1)
            x = self._layer(h, lvl.n, nbr, m.conv2, residual=x)
        return x

    def _down(self, x, lvl, conv):
        """A strided convolution: the output level (sorted rows, its index), and its features."""
        lib = hip.load()
        k, s, p = conv.geometry
        grid = tuple((i + 2 * pp - kk) // ss + 1 for i, kk, ss, pp in zip(lvl.grid, k, s, p))
        if min(grid) < 1:
            raise hip.ShastaHipError("SpMiddleResNetFHD: grid %s is too small for kernel %s, stride %s, padding %s" % (list(lvl.grid), k, s, p))
        reach = int(np.prod([-(-kk // ss) for kk, ss in zip(k, s)]))  # output sites one input row can activate
        cap = int(min(lvl.n * reach, lvl.B * int(np.prod(grid))))
        dev = x.device
        index = self._index_buffer(lvl.B, grid, cap, dev)
        coords = torch.empty(cap, 4, dtype=torch.int32, device=dev)
        count = torch.zeros(1, dtype=torch.int32, device=dev)
        hip.check(lib.shasta_spconv_out_coords(hip.ptr(lvl.coords), lvl.n, lvl.B, *lvl.grid, *k, *s, *p, hip.ptr(coords), cap, hip.ptr(count),
                                               hip.ptr(index), index.numel(), hip.stream_ptr()), "shasta_spconv_out_coords")
        n_out = int(count.item())  # the one host synchronisation of this level
        if n_out > cap:
            raise hip.ShastaHipError("SpMiddleResNetFHD: %d output sites from %d rows: the input coordinates are not unique" % (n_out, lvl.n))
        self._check_rows(conv, n_out)
        out_lvl = _Level(coords[:n_out], lvl.B, grid, index)
        y = self._layer(x, lvl.n, lvl.neighbors(out_lvl.coords, (k, s, p)), conv)
        return out_lvl, y

    def forward(self, voxel_features, coors, batch_size, input_shape):
        self._check_servable(voxel_features, coors)
        if voxel_features.dim() != 2 or voxel_features.shape[1] != self.conv_input[0].in_channels:
            raise ValueError("SpMiddleResNetFHD: expected (V, %d) voxel features, got %s"
                             % (self.conv_input[0].in_channels, tuple(voxel_features.shape)))
        if coors.dim() != 2 or coors.shape[1] != 4 or coors.shape[0] != voxel_features.shape[0]:
            raise ValueError("SpMiddleResNetFHD: expected (V, 4) coordinates (batch, z, y, x), got %s" % (tuple(coors.shape),))
        lib = hip.load()
        dev = voxel_features.device
        B = int(batch_size)
        grid = tuple(int(v) for v in (np.array(input_shape[::-1]) + [1, 0, 0]))  # sparse_shape, scn.py:181
        self._run = self._ensure_packed(dev)
        x = voxel_features.contiguous()
        coords = coors.int().contiguous()
        batch = [bn for _, _, bn in self._run.values() if bn is not None]  # the layers on batch statistics in this forward
        if batch:
            # (before the first collective; a non-empty cloud has at least 1 row at every level)
            if x.shape[0] == 0 and any(sync_bn.synced_world(bn) > 1 for bn in batch):
                raise ValueError("SpMiddleResNetFHD: an empty local input cannot take part in synchronised batch statistics")
            self._stats.reserve(batch, lib.shasta_bn_rows_workspace_bytes(max(bn.num_features for bn in batch)), dev)
        return self._forward(x, coords, B, grid)

    def _forward(self, x, coords, B, grid):
        lib = hip.load()
        dev = x.device
        V = int(x.shape[0])

        index = self._index_buffer(B, grid, V, dev)
        hip.check(lib.shasta_spconv_index_rows(hip.ptr(coords), V, B, *grid, hip.ptr(index), index.numel(), hip.stream_ptr()),
                  "shasta_spconv_index_rows")
        lvl = _Level(coords, B, grid, index)
        conv0 = self.conv_input[0]
        self._check_rows(conv0, V)
        x = self._layer(x, V, lvl.subm_neighbors(conv0.geometry), conv0)
        x = self._blocks(x, lvl, self.conv1)
        levels = {"conv1": SparseLevel(x, lvl.coords, lvl.grid, B)}
        for name in ("conv2", "conv3", "conv4"):
            seq = getattr(self, name)
            lvl, x = self._down(x, lvl, seq[0])
            x = self._blocks(x, lvl, seq)
            levels[name] = SparseLevel(x, lvl.coords, lvl.grid, B)
        lvl, x = self._down(x, lvl, self.extra_conv[0])
        ret = _dense(x, lvl.coords, B, lvl.grid)  # (B, C, D, H, W).view(B, C * D, H, W)
        return ret, levels


def register():
    """Put `SpMiddleResNetFHD` into BACKBONES under its name, for the reference's string configs.  Idempotent; refuses to displace a
    different class somebody registered under that name."""
    have = BACKBONES.get(SpMiddleResNetFHD.__name__)
    if have is SpMiddleResNetFHD:
        return SpMiddleResNetFHD
    if have is not None:
        raise KeyError("%s is already registered in %s as %r" % (SpMiddleResNetFHD.__name__, BACKBONES.name, have))
    return BACKBONES.register_module(SpMiddleResNetFHD)
