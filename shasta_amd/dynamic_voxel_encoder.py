"""DynamicVoxelEncoder (det3d/models/readers/dynamic_voxel_encoder.py:8-17,71-102): voxeliser and reader in one, on the device.

The reference range-filters every cloud, takes integer coordinates, `unique(dim=0)` of them and a `scatter_mean` of ALL points of
each voxel - no cap on the points of a voxel, no `max_voxel_num`.  Here the whole list of clouds is one call of
`shasta_dynvox_mean_f32` (csrc/dynvox.hip), whose rows equal the reference's on the CPU index for index and bit for bit: both range
faces inclusive (a point on an upper face gets coordinate == extent and its voxel is kept), coordinates by a true fp32 division,
voxels of a cloud sorted by (z, y, x), clouds in batch order, means from an in-order fp32 sum.

Deviations, both deliberate:
  * `coors_batch` is int32, the type the backbone's kernels consume; the reference's int64 carries nothing more (values below 2^31).
  * `virtual=True` (the hard-coded 22-channel painted-point variant, dynamic_voxel_encoder.py:19-68) is out of scope: the constructor
    raises NotImplementedError.
There is no CPU path: CPU tensors raise ShastaHipError."""
import ctypes as C

import numpy as np
import torch
from torch import nn

from . import hip
from .registry import READERS

MAX_CLOUDS = 32  # csrc/dynvox.hip DV_MAX_CLOUDS


def dynamic_voxelize(clouds, pc_range, voxel_size, shape, sync=True):
    """clouds: list of (P_i, ndim) fp32 device tensors (1 to 32 of them).  pc_range (6,), voxel_size (3,), shape (3,) = (gx, gy, gz).
    Returns (voxels (V, ndim) fp32, coors (V, 4) int32 rows (cloud, z, y, x), num_points (V,) int32, prefix (n + 1,) int32 device
    tensor: voxels before each cloud, the last word is V) - one host read, of V.  sync=False: nothing is read back, the first three
    keep one row per point (rows >= V are not written)."""
    if isinstance(clouds, tuple):  # (points (sum P, ndim), offsets): the clouds already back to back, as points_to_voxel_batch_device takes them
        points, offsets = clouds
        offsets = [int(o) for o in offsets]
        clouds = [points]
    else:
        offsets = None
    if not len(clouds):
        raise ValueError("dynamic_voxelize: an empty list of clouds")
    if not all(torch.is_tensor(c) and c.is_cuda for c in clouds):
        raise hip.ShastaHipError("DynamicVoxelEncoder needs device tensors; there is no CPU path")
    lib = hip.load()
    ndim = int(clouds[0].shape[1])
    if offsets is None:
        offsets = [0]
        for c in clouds:
            if c.dim() != 2 or c.shape[1] != ndim:
                raise ValueError("dynamic_voxelize: every cloud must be (P, %d)" % ndim)
            offsets.append(offsets[-1] + int(c.shape[0]))
    n = len(offsets) - 1
    points = (torch.cat([c.float() for c in clouds], dim=0) if len(clouds) > 1 else clouds[0].float()).contiguous()
    P, dev = offsets[-1] - offsets[0], points.device
    if offsets[-1] > points.shape[0]:
        raise ValueError("dynamic_voxelize: offsets beyond the points")
    rg = np.ascontiguousarray(pc_range, np.float32)
    vs = np.ascontiguousarray(voxel_size, np.float32)
    gx, gy, gz = (int(s) for s in shape)
    off = (C.c_int * (n + 1))(*offsets)
    wsb = lib.shasta_dynvox_workspace_bytes(off, n, gx, gy, gz)
    if wsb == 0:
        raise hip.ShastaHipError("dynamic voxelisation does not serve %d clouds on a %d x %d x %d grid (1 to %d clouds, fewer than "
                                 "2^31 cells in all)" % (n, gx, gy, gz, MAX_CLOUDS))
    cap = max(P, 1)
    voxels = torch.empty(cap, ndim, device=dev)
    coors = torch.empty(cap, 4, dtype=torch.int32, device=dev)
    num = torch.empty(cap, dtype=torch.int32, device=dev)
    prefix = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ws = torch.empty((wsb + 3) // 4, dtype=torch.int32, device=dev)
    hip.check(lib.shasta_dynvox_mean_f32(hip.ptr(points), off, n, ndim, rg.ctypes.data_as(C.c_void_p), vs.ctypes.data_as(C.c_void_p),
                                         gx, gy, gz, hip.ptr(voxels), hip.ptr(coors), hip.ptr(num), cap, hip.ptr(prefix), hip.ptr(ws),
                                         wsb, hip.stream_ptr()), "shasta_dynvox_mean_f32")
    if not sync:
        return voxels, coors, num, prefix
    V = int(prefix[n].item())
    return voxels[:V], coors[:V], num[:V], prefix


@READERS.register_module
class DynamicVoxelEncoder(nn.Module):
    def __init__(self, pc_range, voxel_size, virtual=False):
        super().__init__()
        if virtual:
            raise NotImplementedError("DynamicVoxelEncoder(virtual=True), the painted-point variant, is out of scope (DESIGN.md 8)")
        self.pc_range = torch.tensor(pc_range, dtype=torch.float32)
        self.voxel_size = torch.tensor(voxel_size, dtype=torch.float32)
        self.shape = torch.round((self.pc_range[3:] - self.pc_range[:3]) / self.voxel_size)
        self.shape_np = self.shape.numpy().astype(np.int32)
        self.virtual = virtual

    @torch.no_grad()
    def forward(self, points):
        """points: list of (P_i, ndim) fp32 device tensors -> (voxels_batch (V, ndim) fp32, coors_batch (V, 4) int32 rows
        (batch, z, y, x), shape_np).  One call of the kernel chain for the whole list and one host read (of V; the reference's
        `unique` synchronises too).  coors_batch is int32 where the reference has int64: the backbone's kernels read int32."""
        voxels, coors, _, _ = dynamic_voxelize(list(points), self.pc_range.numpy(), self.voxel_size.numpy(), self.shape_np)
        return voxels, coors, self.shape_np
