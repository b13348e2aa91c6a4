"""GPU: the frozen backbone and neck in train() mode after `sync_bn.convert_syncbn_model`, batch statistics shared over ranks
(csrc/bn_sync.hip through `sync_bn.RankStats`).  Rank r holds sample r of a batch; the truth is ONE process over the whole batch in
float64.  ONE spawn of two processes that share GPU 0 and exchange over gloo serves every two-rank check here (the pattern of
tests/test_multi_gpu.py's one-GPU tests: everything of the multi-rank path except RCCL itself); the RCCL variants run the same checks
on 2 / 4 / 8 real GPUs and skip on a smaller box."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import backbone_helpers as BH
from tests import backbone_train_helpers as BT
from tests import sync_bn_helpers as SH
from tests.neck_train_helpers import build_train_fixture_neck, layers64_train, train_fixture

pytestmark = pytest.mark.gpu
LEVELS = ("conv1", "conv2", "conv3", "conv4")
# case 41x18x26 of tests/test_backbone_train_kernels.py: input_shape (x, y, z), seed, blobs, rows per blob; B = the number of ranks
SHAPE, SEED, BLOBS, PER = [26, 18, 40], 32, 2, 60
FROZEN = 2  # the BatchNorm (state_dict order) that the mixed-mode check puts in eval()


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda", 0)


def _bns(m):
    return [b for b in m.modules() if isinstance(b, torch.nn.modules.batchnorm._BatchNorm)]


def _state(m):
    return [(b.running_mean.cpu().numpy().copy(), b.running_var.cpu().numpy().copy(), int(b.num_batches_tracked)) for b in _bns(m)]


def _backbone_module():
    from shasta_amd.backbone import SpMiddleResNetFHD
    m = SpMiddleResNetFHD(num_input_features=5, ds_factor=8, batch_statistics=True).train()
    BT.randomize_train(m, torch.Generator().manual_seed(SEED))
    return m


def _backbone_input(B):
    grid = (SHAPE[2] + 1, SHAPE[1], SHAPE[0])
    coords = BH.clustered_voxels(np.random.RandomState(SEED), B, grid, blobs=BLOBS, per_blob=PER)
    feats = torch.randn(len(coords), 5, generator=torch.Generator().manual_seed(SEED + 1))
    return coords, feats


def _neck_input(world):
    """Rank r feeds image r % 2 of the fixture; the whole batch is the fixture's two images world / 2 times over."""
    x = torch.from_numpy(train_fixture()["x"])
    return torch.cat([x] * (world // 2))


def _refuse_layers(m):
    def refuse(x):
        raise AssertionError("forward_layers was called: the kernel path was not taken")
    m.forward_layers = refuse


# ---- what every rank does ---------------------------------------------------------------------------------------------
def _rank_body(rank, world, dev):
    from shasta_amd import sync_bn
    from shasta_amd.sync_bn import convert_syncbn_model
    out = {}
    with torch.no_grad():
        # backbone: converted, train(), the rows of cloud `rank` as a batch of one
        coords, feats = _backbone_input(world)
        m = convert_syncbn_model(_backbone_module()).to(dev).train()
        assert all(type(b) is sync_bn.SyncBatchNorm for _, b in m._pairs()) and len(m._pairs()) == 21
        sel = coords[:, 0] == rank
        c = coords[sel].copy()
        c[:, 0] = 0
        ret, levels = m(feats[torch.from_numpy(sel)].to(dev), torch.from_numpy(c).to(dev), 1, SHAPE)
        out["backbone"] = dict(ret=ret.cpu().numpy(), state=_state(m),
                               levels={k: (levels[k].indices.cpu().numpy(), levels[k].dense().cpu().numpy(), levels[k].spatial_shape)
                                       for k in LEVELS})
        with pytest.raises(ValueError, match="empty local input"):  # refused before the first collective: the other rank is not waiting
            m(feats[:0].to(dev), torch.from_numpy(c[:0]).to(dev), 1, SHAPE)

        # neck: converted AFTER construction and after an eval forward built the plan and the packs from the old modules
        x = _neck_input(world)[rank:rank + 1].to(dev)
        n = build_train_fixture_neck(batch_statistics=True).to(dev)
        n.eval()(x)
        old = _bns(n)
        convert_syncbn_model(n)
        n.train()
        _refuse_layers(n)
        assert all(type(b) is sync_bn.SyncBatchNorm2d for b in _bns(n)) and all(o.training is False for o in old)  # (the orphans stay in eval())
        y = n(x)
        assert {id(bn) for _, _, bn, _ in n._plan} == {id(b) for b in _bns(n)}  # the plan follows the new modules
        out["neck"] = dict(y=y.cpu().numpy(), state=_state(n))
        # eval(): the module's mode decides, and the result is the eval kernels' on the updated statistics
        n.eval()
        y_eval = n(x)
        plain = build_train_fixture_neck().to(dev)
        plain.load_state_dict(n.state_dict())
        out["neck_eval_equal"] = bool(torch.equal(y_eval, plain.eval()(x))) and not bool(torch.equal(y_eval, y))
        out["neck_eval_state"] = _state(n)

        # neck, one BatchNorm in eval() on every rank: that layer stays on its running statistics
        k = convert_syncbn_model(build_train_fixture_neck(batch_statistics=True)).to(dev).train()
        _bns(k)[FROZEN].eval()
        _refuse_layers(k)
        before = _state(k)
        y = k(x)
        out["mixed"] = dict(y=y.cpu().numpy(), before=before, state=_state(k))
    return out


_RANKS = {}


def _ranks(world, backend):
    """One spawn per (world, backend) for the whole file; after a failure nothing more is started: the later tests fail with it."""
    key = (world, backend)
    if key not in _RANKS:
        try:
            _RANKS[key] = SH.run_workers(_rank_body, world, backend)
        except BaseException as e:  # noqa: BLE001
            _RANKS[key] = e
    if isinstance(_RANKS[key], BaseException):
        raise AssertionError("the ranks failed: %s" % _RANKS[key])
    return _RANKS[key]


# ---- the truth: one process over the whole batch ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _backbone_truth(B):
    m = _backbone_module()
    coords, feats = _backbone_input(B)
    r64, l64, s64 = BT.reference_forward_train(m, feats, coords, B, SHAPE, torch.float64)
    r32, l32, _ = BT.reference_forward_train(m, feats, coords, B, SHAPE, torch.float32)
    bars = {k: float((l32[k][0].double() - l64[k][0]).abs().max()) for k in LEVELS}  # as _restatement_errors does
    bars["ret"] = float((r32.double() - r64).abs().max())
    return dict(m=m, r64=r64, l64=l64, s64=s64, bars=bars)


def _check_backbone(res, world):
    """Active sets exact; values within 4 x the fp32 restatement's own error against float64; running statistics of all 21 layers within
    rtol 1e-5 of the whole batch's; num_batches_tracked 1 everywhere; running statistics bit-equal between the ranks."""
    t = _backbone_truth(world)
    assert len(t["s64"]) == 21 and all(s is not None for s in t["s64"])
    errs = {}
    for r in range(world):
        got = res[r]["backbone"]
        for k in LEVELS:
            idx, dense, shape = got["levels"][k]
            x64, mask = t["l64"][k][0][r:r + 1], t["l64"][k][1][r:r + 1]
            assert shape == list(x64.shape[2:]) and (idx[:, 0] == 0).all()
            lin = ((idx[:, 1].astype(np.int64) * shape[1]) + idx[:, 2]) * shape[2] + idx[:, 3]
            assert np.array_equal(idx[np.argsort(lin)], BH.mask_coords(mask)), (r, k)
            dense = torch.from_numpy(dense)
            assert dense.shape == x64.shape and bool((dense[mask.expand_as(x64) == 0] == 0).all())
            errs[k] = max(errs.get(k, 0.0), float((dense.double() - x64).abs().max()))
        ret = torch.from_numpy(got["ret"])
        assert ret.shape == t["r64"][r:r + 1].shape
        errs["ret"] = max(errs.get("ret", 0.0), float((ret.double() - t["r64"][r:r + 1]).abs().max()))
        assert float(ret.abs().max()) > 0
    for k in LEVELS + ("ret",):
        print("backbone, %d ranks, %s: max|got - f64| = %.3e, fp32 restatement %.3e, ratio %.2f" % (world, k, errs[k], t["bars"][k], errs[k] / t["bars"][k]))
    for k in LEVELS + ("ret",):
        assert errs[k] <= 4 * t["bars"][k], (k, errs[k], t["bars"][k])
    want = BT.expected_running(t["m"], t["s64"])
    worst = 0.0
    for i, (w, st) in enumerate(zip(want, res[0]["backbone"]["state"])):
        for got, ref in ((st[0], w[0].numpy()), (st[1], w[1].numpy())):
            worst = max(worst, float(np.abs((got - ref) / ref).max()))
            np.testing.assert_allclose(got.astype(np.float64), ref, rtol=1e-5, atol=0, err_msg="pair %d" % i)
        assert st[2] == 1
    print("backbone, %d ranks: running statistics, worst relative error %.3e" % (world, worst))
    _bit_equal_states([res[r]["backbone"]["state"] for r in range(world)])


def _bit_equal_states(states):
    for other in states[1:]:
        assert len(other) == len(states[0])
        for a, b in zip(states[0], other):
            assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32)) and a[2] == b[2]


@functools.lru_cache(maxsize=None)
def _neck_truth(world, frozen=None):
    """float64 forward_layers of the unconverted fixture module over the whole batch (for two ranks and nothing frozen: the golden
    itself), the running statistics after it, and the fp32 reference's own error."""
    fx = train_fixture()
    if world == 2 and frozen is None:
        names = [k[:-len(".running_mean")] for k in fx["keys"] if k.endswith(".running_mean")]
        want = [(fx["after"][n + ".running_mean"], fx["after"][n + ".running_var"], int(fx["after"][n + ".num_batches_tracked"])) for n in names]
        return dict(y64=fx["y64"], want=want, ref_err=float(np.abs(fx["y32"] - fx["y64"]).max()))
    m = build_train_fixture_neck()
    if frozen is not None:
        _bns(m)[frozen].eval()
    x = _neck_input(world)
    (y64,), s64 = layers64_train(m, [x])
    with torch.no_grad():
        ref_err = float((copy.deepcopy(m).forward_layers(x).double() - y64).abs().max())
    return dict(y64=y64.numpy(), want=[(a.numpy(), b.numpy(), c) for a, b, c in s64], ref_err=ref_err)


def _check_neck(res, world, key="neck", frozen=None):
    """Bars of tests/test_neck_train.py: the output within 4 x the fp32 reference's own max error against float64, running statistics
    within rtol 1e-5, num_batches_tracked equal; and the running statistics bit-equal between the ranks."""
    t = _neck_truth(world, frozen)
    assert t["ref_err"] > 0
    errs = [float(np.abs(res[r][key]["y"] - t["y64"][r:r + 1]).max()) for r in range(world)]
    print("%s, %d ranks: max|got - y64| per rank %s, reference max|y32 - y64| = %.3e, ratio %.2f"
          % (key, world, ["%.3e" % e for e in errs], t["ref_err"], max(errs) / t["ref_err"]))
    assert res[0][key]["y"].shape == t["y64"][:1].shape and max(errs) <= 4 * t["ref_err"]
    assert len(t["want"]) == 7 and min(float(np.abs(w[0]).min()) for w in t["want"]) > 0.2  # the relative bar means something
    for i, (w, st) in enumerate(zip(t["want"], res[0][key]["state"])):
        if i == frozen:
            continue
        np.testing.assert_allclose(st[0].astype(np.float64), w[0], rtol=1e-5, atol=0, err_msg="BatchNorm %d" % i)
        np.testing.assert_allclose(st[1].astype(np.float64), w[1], rtol=1e-5, atol=0, err_msg="BatchNorm %d" % i)
        assert st[2] == w[2] == 1
    _bit_equal_states([res[r][key]["state"] for r in range(world)])


# ---- two processes on one GPU over gloo -------------------------------------------------------------------------------
def test_two_ranks_backbone_equals_one_process_over_both_clouds():
    """On the parent commit the converted backbone raises ("only BatchNorm1d ... got SyncBatchNorm").

    Measured on an MI355X: see DESIGN.md section 4."""
    _check_backbone(_ranks(2, "gloo"), 2)


def test_two_ranks_neck_equals_one_process_over_both_images():
    """The neck converted after construction (the stale-plan path).  On the parent commit the plan keeps the orphaned BatchNorm2d
    objects: in eval() there (as here, after the eval forward) they put every layer on its running statistics, in train() they
    normalise with per-rank statistics.  The gap of per-rank statistics, from the float64 restatement on the CPU: image 0 alone through
    the train() neck differs from its rows of the whole-batch result by 1.07 (range 5.8), against a bar of 2.2e-5 - asserted below."""
    fx = train_fixture()
    t = _neck_truth(2)
    (alone,), _ = layers64_train(build_train_fixture_neck(), [torch.from_numpy(fx["x"][:1])])
    gap = float(np.abs(alone.numpy() - fx["y64"][:1]).max())
    print("per-rank statistics are off by %.3e (bar %.3e, range %.3e)" % (gap, 4 * t["ref_err"], float(np.abs(fx["y64"]).max())))
    assert gap > 1000 * 4 * t["ref_err"]
    res = _ranks(2, "gloo")
    _check_neck(res, 2)
    for r in range(2):
        assert res[r]["neck_eval_equal"]  # after eval(): the eval kernels' result on the updated statistics, bit for bit
        for a, b in zip(res[r]["neck"]["state"], res[r]["neck_eval_state"]):  # and an eval() forward moves no statistics
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 1


def test_two_ranks_neck_with_one_layer_on_running_statistics():
    res = _ranks(2, "gloo")
    _check_neck(res, 2, "mixed", frozen=FROZEN)
    for r in range(2):
        before, after = res[r]["mixed"]["before"], res[r]["mixed"]["state"]
        assert np.array_equal(before[FROZEN][0], after[FROZEN][0]) and np.array_equal(before[FROZEN][1], after[FROZEN][1])
        assert after[FROZEN][2] == 0 and [s[2] for s in after] == [0 if i == FROZEN else 1 for i in range(7)]
    full = _neck_truth(2)
    assert float(np.abs(_neck_truth(2, FROZEN)["y64"] - full["y64"]).max()) > 1e-3  # (not what the all-train module gives)


# ---- one process: the bits of the unconverted modules -----------------------------------------------------------------
def test_world_one_gives_the_bits_of_the_unconverted_modules():
    """No process group (and so world 1): a converted backbone and a converted neck make the calls of the plain modules."""
    from shasta_amd import sync_bn
    from shasta_amd.sync_bn import convert_syncbn_model
    dev = _dev()
    assert not torch.distributed.is_initialized()
    coords, feats = _backbone_input(2)
    fd, cd = feats.to(dev), torch.from_numpy(coords).to(dev)
    plain, conv = _backbone_module().to(dev), convert_syncbn_model(_backbone_module()).to(dev).train()
    assert all(type(b) is sync_bn.SyncBatchNorm and sync_bn.synced_world(b) == 1 for _, b in conv._pairs())
    with torch.no_grad():
        (r1, l1), (r2, l2) = plain(fd, cd, 2, SHAPE), conv(fd, cd, 2, SHAPE)
    assert torch.equal(r1, r2) and float(r1.abs().max()) > 0 and all(torch.equal(l1[k].features, l2[k].features) for k in LEVELS)
    for a, b in zip(_state(plain), _state(conv)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 1
    x = torch.from_numpy(train_fixture()["x"]).to(dev)
    plain, conv = build_train_fixture_neck(batch_statistics=True).to(dev), build_train_fixture_neck(batch_statistics=True).to(dev)
    assert conv._plan is not None  # (built from the old modules)
    convert_syncbn_model(conv)
    _refuse_layers(conv)
    with torch.no_grad():
        y1, y2 = plain(x), conv(x)
    assert torch.equal(y1, y2) and float(y1.abs().max()) > 0
    for a, b in zip(_state(plain), _state(conv)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == 1


# ---- RCCL on real GPUs ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 4, 8])
def test_rccl_backbone_and_neck_equal_one_process(world):
    if torch.cuda.device_count() < world:
        pytest.skip("needs %d GPUs, this box has %d" % (world, torch.cuda.device_count()))
    res = _ranks(world, "nccl")
    _check_backbone(res, world)
    _check_neck(res, world)
