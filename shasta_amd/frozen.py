"""What the frozen detector stages share on the host: `SpMiddleResNetFHD` (backbone.py), `RPN` (neck.py), `CenterHead` (head.py).  No kernels
and no library calls of its own but the finalize of a layer on batch statistics.

THE CACHE RULE (`PackedLayers`): a layer's packed buffer is valid while the tensors it was packed from keep their storage pointers and version
counters and the device is the same; `.to()`, `load_state_dict` and `invalidate_weights_cache()` drop everything.  The kernels of a train()
forward write the running statistics through raw pointers, which bumps no version counter: the slot is marked stale BEFORE that launch, and the
next request that reads the statistics re-packs it.  A request that does not read them (the raw convolution of a layer on batch statistics)
is served from a stale entry."""
import ctypes

import torch
from torch import nn

from . import hip, sync_bn


class PackedLayers:
    """slot -> (key, what `pack()` returned), one entry per slot of the caller's choice."""

    def __init__(self):
        self._entries, self._stale = {}, set()

    def get(self, slot, tensors, dev, pack, reads_statistics=True):
        key = tuple((t.data_ptr(), t._version) for t in tensors) + (str(dev),)
        entry = self._entries.get(slot)
        if entry is None or entry[0] != key or (reads_statistics and slot in self._stale):
            entry = self._entries[slot] = (key, pack())
            self._stale.discard(slot)
        return entry[1]

    def mark_stale(self, slot):
        self._stale.add(slot)

    def clear(self):
        self._entries, self._stale = {}, set()


class FrozenStage(nn.Module):
    """Base of the three stages: the packed layers (`self._cache`) and the calls that drop them."""

    def __init__(self):
        super().__init__()
        self._cache = PackedLayers()  # HIP-side state (not parameters, not in state_dict)

    def _apply(self, fn, *a, **k):  # .to() / .cuda() / .float(): parameter storage moves -> drop the packed layers
        self.invalidate_weights_cache()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self.invalidate_weights_cache()
        return super().load_state_dict(*a, **k)

    def invalidate_weights_cache(self):
        """Forget the packed layers; the next kernel-path forward re-packs them.  They follow in-place writes, optimizer steps and
        load_state_dict by themselves (pointer + version checks); call this after a write that bumps no version counter."""
        self._cache.clear()


# ---- what the kernel paths serve: each stage decides whether a failed check raises or takes its nn form ---------------------------------
def servable_norm(bn, kinds):
    return isinstance(bn, kinds) and bn.affine and bn.track_running_stats


def all_fp32(tensors):
    return all(t.dtype == torch.float32 for t in tensors)


def wants_autograd(x, params):
    return torch.is_grad_enabled() and (x.requires_grad or any(t.requires_grad for t in params))


def refuse_cumulative_average(who, kind, bn):
    if bn.momentum is None:
        raise hip.ShastaHipError("%s: %s(momentum=None) (cumulative averaging of the running statistics) is not served in train() mode"
                                 % (who, kind))


def refuse_single_value(bn, size):
    """torch.nn.functional.batch_norm's check of a (N, C, *) input.  Several ranks: each has a value, at least 2 in total."""
    size = torch.Size(size)
    if size.numel() // size[1] < 2 and sync_bn.synced_world(bn) == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (size,))


class BatchStatistics:
    """The step of a layer whose BatchNorm is in training mode, between its raw convolution and its apply call.  Owns `mean_m2`, `stat`,
    the statistics workspace (`buffers`, in that order) and the `sync_bn.RankStats`; kept on the module and grown on demand, so the pointers
    are stable from the second identical forward on (graph capture).  `finalize`: `shasta_bn_rows_finalize_f32` or `shasta_bn_maps_finalize_f32`."""

    def __init__(self, cache, finalize):
        self._cache, self._finalize = cache, finalize
        self.buffers, self.ranks = (), None

    def __iter__(self):
        return iter(self.buffers)

    def reserve(self, bns, workspace_bytes, dev):
        """Before the first launch of a forward: room for the layers whose BatchNorm modules are `bns`."""
        width, b = max(bn.num_features for bn in bns), self.buffers
        if not b or b[0].device != dev or b[0].numel() < 2 * width or b[2].numel() < workspace_bytes:
            self.buffers = ()
            self.buffers = (torch.empty(2 * width, dtype=torch.float32, device=dev), torch.empty(2 * width, dtype=torch.float32, device=dev),
                            torch.empty(workspace_bytes, dtype=torch.uint8, device=dev))
        synced = [(sync_bn.synced_world(bn), bn.num_features) for bn in bns if sync_bn.synced_world(bn) > 1]
        if synced:  # statistics shared with other ranks: the record and gather buffers
            world, width, rs = max(w for w, _ in synced), max(c for _, c in synced), self.ranks
            if rs is None or rs.width < width or rs.world < world or rs.device != dev:
                self.ranks = None
                self.ranks = sync_bn.RankStats(width, world, dev)

    def layer(self, slot, bn, C, count, stats, stream):
        """`stats(mean_m2, workspace)` launches the stats kernel; then the slot's pack is marked stale and the finalize updates the module's
        running statistics in place (several ranks: one all-gather of the local record, the merged finalize).  Returns `stat` for apply."""
        mm, stat, ws = self.buffers
        world = sync_bn.synced_world(bn)
        stats(self.ranks.local(C, world) if world > 1 else mm, ws)
        self._cache.mark_stale(slot)  # (before the launch that writes the running statistics)
        if world > 1:
            self.ranks.finalize(bn, C, count, stat, stream)
        else:
            hip.check(getattr(hip.load(), self._finalize)(hip.ptr(mm), C, float(count), float(bn.eps), float(bn.momentum), hip.ptr(stat),
                                                          hip.ptr(bn.running_mean), hip.ptr(bn.running_var),
                                                          ctypes.c_void_p(bn.num_batches_tracked.data_ptr()), stream), self._finalize)
        return stat
