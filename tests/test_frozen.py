"""shasta_amd/frozen.py: the packed-layer cache of the frozen stages on the CPU (a counting `pack`, small tensors), and its rule on the
modules on the GPU - an eval forward of the backbone after a train() forward that raised half-way, and per-layer re-packing of the head."""
import copy

import numpy as np
import pytest
import torch

from tests import backbone_helpers as BH
from tests import backbone_train_helpers as BT
from tests import head_helpers as HH

# Two voxels in neighbouring cells at the far end of x in the 41 x 18 x 26 grid: a 3 / stride 2 / padding 1 convolution has 13 output
# sites along x, and the last one (12) is the only one that reads x = 24 or x = 25; z = y = 0 are read by site 0 alone.
TWO_VOXELS = np.array([[0, 0, 0, 24], [0, 0, 0, 25]], dtype=np.int32)
TWO_FEATS = torch.tensor([[1.0] * 5, [-1.0] * 5])
MOMENTUM = 0.5  # (moves the running statistics far enough in one step of two rows for a stale pack to miss the bar ten times over)


# ---- CPU: the cache class -----------------------------------------------------------------------------------------------
class _Counting:
    def __init__(self):
        self.count = {}

    def pack(self, slot):
        def pack():
            self.count[slot] = self.count.get(slot, 0) + 1
            return (slot, self.count[slot])
        return pack


def _get_all(cache, packs, tensors, dev="cpu", **kw):
    return [cache.get(slot, ts, dev, packs.pack(slot), **kw) for slot, ts in tensors.items()]


def test_cache_packs_once_and_follows_its_tensors():
    from shasta_amd.frozen import PackedLayers
    cache, packs = PackedLayers(), _Counting()
    tensors = {0: [torch.zeros(3), torch.ones(2)], ("raw", 1): [torch.zeros(4)], "shared": [torch.zeros(1), torch.zeros(1)]}
    assert _get_all(cache, packs, tensors) == [(0, 1), (("raw", 1), 1), ("shared", 1)]
    assert _get_all(cache, packs, tensors) == [(0, 1), (("raw", 1), 1), ("shared", 1)]  # nothing changed: the cached objects
    assert packs.count == {0: 1, ("raw", 1): 1, "shared": 1}
    tensors[0][1].add_(1.0)  # a version bump of one slot's tensor: that slot only
    _get_all(cache, packs, tensors)
    assert packs.count == {0: 2, ("raw", 1): 1, "shared": 1}
    tensors["shared"][0] = torch.zeros(1)  # another storage (version 0 again)
    _get_all(cache, packs, tensors)
    _get_all(cache, packs, tensors)
    assert packs.count == {0: 2, ("raw", 1): 1, "shared": 2}
    _get_all(cache, packs, tensors, dev="cuda:0")  # another device string: everything
    assert packs.count == {0: 3, ("raw", 1): 2, "shared": 3}
    _get_all(cache, packs, tensors, dev="cuda:0")
    cache.clear()
    assert _get_all(cache, packs, tensors, dev="cuda:0") == [(0, 4), (("raw", 1), 3), ("shared", 4)]


def test_cache_stale_slots_repack_for_readers_of_the_statistics_only():
    from shasta_amd.frozen import PackedLayers
    cache, packs = PackedLayers(), _Counting()
    tensors = {0: [torch.zeros(3)], 1: [torch.zeros(3)]}
    _get_all(cache, packs, tensors)
    cache.mark_stale(0)
    assert _get_all(cache, packs, tensors, reads_statistics=False) == [(0, 1), (1, 1)]  # served from the stale entry
    assert _get_all(cache, packs, tensors, reads_statistics=False) == [(0, 1), (1, 1)]  # ... which stays stale
    assert _get_all(cache, packs, tensors) == [(0, 2), (1, 1)]
    assert _get_all(cache, packs, tensors) == [(0, 2), (1, 1)]  # re-packed once
    cache.mark_stale(1)
    tensors[1][0].add_(1.0)  # stale and written: one pack, also for a request that does not read the statistics
    assert _get_all(cache, packs, tensors, reads_statistics=False) == [(0, 2), (1, 2)]
    assert _get_all(cache, packs, tensors) == [(0, 2), (1, 2)]  # (a pack takes the statistics as they are: no longer stale)
    cache.mark_stale(0)
    cache.clear()  # forgets the marks with the entries
    assert _get_all(cache, packs, tensors) == [(0, 3), (1, 3)] and _get_all(cache, packs, tensors) == [(0, 3), (1, 3)]
    cache.mark_stale(5)  # a slot nobody packed yet
    assert cache.get(5, tensors[0], "cpu", packs.pack(5)) == (5, 1) and cache.get(5, tensors[0], "cpu", packs.pack(5)) == (5, 1)


def test_one_api_on_the_three_stages():
    from shasta_amd import CenterHead
    from shasta_amd.backbone import SpMiddleResNetFHD
    from shasta_amd.frozen import FrozenStage
    from shasta_amd.neck import RPN
    for cls in (SpMiddleResNetFHD, RPN, CenterHead):
        assert issubclass(cls, FrozenStage)
        for name in ("_apply", "load_state_dict", "invalidate_weights_cache"):
            assert name not in vars(cls) and getattr(cls, name) is getattr(FrozenStage, name)


def test_two_voxels_become_one_row_at_the_first_strided_level():
    """The restatement alone: conv_input and conv1's four layers see 2 rows, conv2's strided convolution and everything after it 1."""
    from tests import test_backbone_train_kernels as TT
    m = TT._module(3)
    _, levels, stats = BT.reference_forward_train(m, TWO_FEATS, TWO_VOXELS, 1, TT.CASES["41x18x26"][0], torch.float64)
    assert [int(s[2]) for s in stats] == [2] * 5 + [1] * 16
    assert BH.mask_coords(levels["conv2"][1]).tolist() == [[0, 0, 0, 12]]


# ---- GPU: the backbone after a train() forward that raised half-way -----------------------------------------------------------
@pytest.mark.gpu
def test_backbone_eval_after_a_train_forward_that_raised():
    """Eval packs cached, then a train() forward that updates the running statistics of five layers and raises at the sixth (one row), then
    eval again: the result is the float64 restatement of the module as it now is, at the bar of
    test_eval_packs_follow_the_running_statistics - which the packs of the first eval forward would miss."""
    from tests import test_backbone_train_kernels as TT
    dev = TT._dev()
    c = TT._case("41x18x26")
    m = TT._module(TT.CASES["41x18x26"][2], norm_cfg=dict(type="BN1d", eps=1e-3, momentum=MOMENTUM))
    m.load_state_dict(c["m"].state_dict())
    m = m.to(dev)
    old64, _ = BH.reference_forward(copy.deepcopy(m).cpu().eval(), c["feats"], c["coords"], c["B"], c["shape"], torch.float64)
    atol = 2e-5 * max(1.0, float(old64.abs().max()))
    got_old = TT._run(m.eval(), c, dev)[0].cpu().double()  # caches the eval packs of the old statistics
    np.testing.assert_allclose(got_old.numpy(), old64.numpy(), rtol=1e-4, atol=atol)
    with torch.no_grad(), pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        m.train()(TWO_FEATS.to(dev), torch.from_numpy(TWO_VOXELS).to(dev), 1, c["shape"])
    assert [int(bn.num_batches_tracked) for bn in TT._bns(m)] == [1] * 5 + [0] * 16
    new64, _ = BH.reference_forward(copy.deepcopy(m).cpu().eval(), c["feats"], c["coords"], c["B"], c["shape"], torch.float64)
    stale = float((new64 - old64).abs().max())
    print("eval result moved by %.3e with the statistics of five layers (bar %.3e)" % (stale, atol))
    assert stale > 50 * atol  # a stale pack is off by far more than the bar
    got_new = TT._run(m.eval(), c, dev)[0].cpu().double()
    print("max |got - float64| = %.3e" % float((got_new - new64).abs().max()))
    np.testing.assert_allclose(got_new.numpy(), new64.numpy(), rtol=1e-4, atol=2e-5 * max(1.0, float(new64.abs().max())))


# ---- GPU: the head re-packs the layer that was written ------------------------------------------------------------------------
@pytest.mark.gpu
def test_head_follows_writes_layer_by_layer():
    """The two-task shape of test_forward_on_the_kernels_against_forward_layers_float64 and its end-to-end bar (forward_layers in float64,
    rtol = atol = 1e-4): after each write the kernel path gives the module as it now is, and not what it gave before."""
    dev = torch.device("cuda", 0)
    head = HH.make_head(24, HH.TWO_TASKS, 40 + 24).to(dev)
    x = torch.relu(torch.randn(3, 24, 5, 33, generator=torch.Generator().manual_seed(41)))

    def forward(what):
        with torch.no_grad():
            out = head(x.to(dev))
        ref = copy.deepcopy(head).cpu().double().forward_layers(x.double())
        for d, r in zip(out, ref):
            for n in d:
                np.testing.assert_allclose(d[n].cpu().double().numpy(), r[n].detach().numpy(), rtol=1e-4, atol=1e-4, err_msg=what)
        return torch.cat([d[n].reshape(-1) for d in out for n in d]).cpu().numpy(), head._packed

    prev, (shared, tasks) = forward("first forward")
    assert head._packed is not None, "the kernel path was not taken"
    writes = [("running_var of a first convolution's BatchNorm", lambda: head.tasks[1].reg[1].running_var.mul_(2.0), (True, True, False)),
              ("bias of a final convolution", lambda: head.tasks[0].hm[3].bias.add_(1.0), (True, False, True)),
              ("weight of the shared convolution", lambda: head.shared_conv[0].weight.mul_(1.1), (False, True, True))]
    for what, write, kept in writes:
        with torch.no_grad():
            write()
        out, (shared2, tasks2) = forward("after an in-place write: " + what)
        assert not np.allclose(out, prev, rtol=1e-4, atol=1e-4), what
        assert (shared2 is shared, tasks2[0] is tasks[0], tasks2[1] is tasks[1]) == kept, what  # only the written layer was re-packed
        prev, shared, tasks = out, shared2, tasks2
    with torch.no_grad():
        head.tasks[1].dim[1].bias.data.add_(0.5)  # (.data: no version bump - the documented case for invalidate_weights_cache)
    head.invalidate_weights_cache()
    out, _ = forward("after a .data write and invalidate_weights_cache()")
    assert not np.allclose(out, prev, rtol=1e-4, atol=1e-4)
