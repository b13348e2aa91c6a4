"""The registered `RPN` neck in train() mode with `batch_statistics=True`: the training step's forward of the frozen neck on the
kernels of csrc/neck.hip (raw convolution) and csrc/bn_maps.hip (batch-statistics BatchNorm2d), against the reference's train-mode
fixture tests/golden/neck_train_golden.npz and the float64 restatement of tests/neck_train_helpers.py.

CPU part (not marked gpu): the keyword, the default path, the state_dict keys, the binding table.  GPU part: `forward_layers` is patched
to raise in every test but the default-path one, so a pass means the kernels computed the result."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests.neck_helpers import SHIPPED, fixture, layers64
from tests.neck_train_helpers import bns, build_train_fixture_neck, layers64_train, randomize_bn_train, train_fixture

gpu = pytest.mark.gpu
NEW_SYMBOLS = ("shasta_neck_layer_raw_f32", "shasta_bn_maps_supported", "shasta_bn_maps_workspace_bytes", "shasta_bn_maps_stats_f32",
               "shasta_bn_maps_finalize_f32", "shasta_bn_maps_apply_f32")


# ---- CPU ----------------------------------------------------------------------------------------------------------
def test_keyword_is_stored_and_can_be_set_later():
    from shasta_amd import builder
    fx = fixture()
    assert builder.build_neck(dict(type="RPN", **fx["cfg"])).batch_statistics is False
    m = builder.build_neck(dict(type="RPN", batch_statistics=True, **fx["cfg"]))
    assert m.batch_statistics is True
    m.batch_statistics = False
    assert m.batch_statistics is False
    assert builder.build_neck(dict(type="RPN", batch_statistics=1, **fx["cfg"])).batch_statistics is True


def test_default_module_in_train_mode_is_forward_layers_on_the_cpu():
    fx = train_fixture()
    m = build_train_fixture_neck()
    assert m.training and m.batch_statistics is False
    x = torch.from_numpy(fx["x"])
    with torch.no_grad():
        got = copy.deepcopy(m)(x)
        want = copy.deepcopy(m).forward_layers(x)
    assert torch.equal(got, want)
    # and forward_layers in train() mode is the reference's train-mode forward, within the reference's own fp32 error
    ref_err = float(np.abs(fx["y32"] - fx["y64"]).max())
    assert ref_err > 0 and float(np.abs(got.numpy() - fx["y64"]).max()) <= 4 * ref_err


def test_state_dict_keys_do_not_depend_on_the_switch():
    fx = train_fixture()
    a, b = build_train_fixture_neck(), build_train_fixture_neck(batch_statistics=True)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys()) == fx["keys"]
    assert len(bns(b)) == 7 and sorted(fx["after"]) == sorted(k for k in fx["keys"] if "running" in k or "num_batches" in k)


def test_binding_table_lists_the_new_entry_points():
    from shasta_amd import hip
    lib = hip.load()
    for name in NEW_SYMBOLS:
        assert name in hip.SYMBOLS and hasattr(lib, name), name
    assert hip.SYMBOLS["shasta_neck_layer_raw_f32"] == hip.SYMBOLS["shasta_neck_layer_f32"]
    assert lib.shasta_abi_version() == 16
    assert lib.shasta_bn_maps_supported(128) == 1 and lib.shasta_bn_maps_supported(48) == 0
    assert lib.shasta_bn_maps_workspace_bytes(1, 128, 180 * 180) >= 2 * 128 * 8


def test_cpu_tensor_with_the_switch_on_raises_as_the_eval_path_does():
    from shasta_amd import hip
    fx = train_fixture()
    m = build_train_fixture_neck(batch_statistics=True)
    with torch.no_grad(), pytest.raises(hip.ShastaHipError, match="device tensor"):
        m(torch.from_numpy(fx["x"]))
    assert all(int(bn.num_batches_tracked) == 0 for bn in bns(m))


# ---- GPU ----------------------------------------------------------------------------------------------------------
def _dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda", 0)


def _no_layers(monkeypatch, m):
    """From here on the nn form of `m` raises (set on the instance AFTER every copy the references need was taken)."""
    def refuse(x):
        raise AssertionError("forward_layers was called: the kernel path was not taken")
    monkeypatch.setattr(m, "forward_layers", refuse)
    return m


def _state(m):
    return [(bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)) for bn in bns(m)]


def _check_running(m, want, what, skip=()):
    """Running statistics against float64, rtol 1e-5 (the references keep the running means away from zero)."""
    worst = 0.0
    for i, (bn, w) in enumerate(zip(bns(m), want)):
        if i in skip:
            continue
        for got, ref in ((bn.running_mean, w[0]), (bn.running_var, w[1])):
            got, ref = got.cpu().double().numpy(), np.asarray(ref, np.float64)
            worst = max(worst, float(np.abs((got - ref) / ref).max()))
            np.testing.assert_allclose(got, ref, rtol=1e-5, atol=0, err_msg="%s, BatchNorm2d %d" % (what, i))
        assert int(bn.num_batches_tracked) == int(w[2]), (what, i)
    return worst


@gpu
def test_default_module_in_train_mode_is_forward_layers_on_the_device():
    fx, dev = train_fixture(), _dev()
    m = build_train_fixture_neck().to(dev)
    calls = []
    inner = m.forward_layers
    m.forward_layers = lambda t: (calls.append(1), inner(t))[1]
    with torch.no_grad():
        got = m(torch.from_numpy(fx["x"]).to(dev))
    assert len(calls) == 1 and got.shape == fx["y64"].shape and all(int(bn.num_batches_tracked) == 1 for bn in bns(m))


@gpu
def test_fixture_neck_vs_reference(monkeypatch):
    """The fixture's neck in train() on the kernels against the reference's float64 train-mode output.  Bar: 4 x the reference's own
    max|y32 - y64|, the project's bar for another fp32 summation order; running statistics within rtol 1e-5 of the reference's float64
    ones, num_batches_tracked equal.

    Measured on an MI355X: see DESIGN.md section 4."""
    fx, dev = train_fixture(), _dev()
    m = _no_layers(monkeypatch, build_train_fixture_neck(batch_statistics=True).to(dev))
    assert m.training and all(bn.training for bn in bns(m))
    with torch.no_grad():
        got = m(torch.from_numpy(fx["x"]).to(dev)).cpu().numpy()
    ref_err = float(np.abs(fx["y32"] - fx["y64"]).max())
    err = float(np.abs(got - fx["y64"]).max())
    print("fixture neck, train(): kernel max|got - y64| = %.3e, reference max|y32 - y64| = %.3e, ratio %.2f, range %.3e"
          % (err, ref_err, err / ref_err, float(np.abs(fx["y64"]).max())))
    assert got.shape == fx["y64"].shape and ref_err > 0
    assert err <= 4 * ref_err
    names = [k[:-len(".running_mean")] for k in fx["keys"] if k.endswith(".running_mean")]
    want = [(fx["after"][n + ".running_mean"], fx["after"][n + ".running_var"], fx["after"][n + ".num_batches_tracked"]) for n in names]
    assert len(want) == 7 and min(float(np.abs(w[0]).min()) for w in want) > 0.2  # the relative bar means something
    print("fixture neck, train(): running statistics, worst relative error %.3e" % _check_running(m, want, "fixture"))


SHIPPED_MAPS = ((8, 8), (12, 20))


@functools.lru_cache(maxsize=None)
def _shipped():
    """Shipped channels, train(), B = 2, two small maps fed one after the other: the template module (left unchanged: every test runs a
    deep copy), the inputs, the float64 restatement (outputs, running statistics after the second forward) and the bar - 4 x the error of
    fp32 forward_layers in train mode on the CPU against the restatement, pooled over both maps."""
    from shasta_amd import builder
    torch.manual_seed(71)
    m = builder.build_neck(dict(type="RPN", batch_statistics=True, **SHIPPED)).train()
    g = torch.Generator().manual_seed(72)
    randomize_bn_train(m, g)
    xs = [torch.randn(2, 256, h, w, generator=g) + 0.2 for h, w in SHIPPED_MAPS]
    y64, s64 = layers64_train(m, xs)
    m32 = copy.deepcopy(m)
    with torch.no_grad():
        ref_err = max(float((m32.forward_layers(x).double() - y).abs().max()) for x, y in zip(xs, y64))
    return dict(m=m, xs=xs, y64=y64, s64=s64, ref_err=ref_err)


@gpu
def test_shipped_channels_two_forwards_vs_float64(monkeypatch):
    """Bar: 4 x the error of fp32 forward_layers in train mode on the CPU against the float64 restatement, pooled over both maps.

    Measured on an MI355X: kernels 4.92e-5 / 6.69e-5 on the two maps, fp32 forward_layers 1.83e-5: ratio 3.67.  The distance to the CPU's
    error is the convolution's summation order (a sequential fp32 chain over Cin x 9 products per output, as in eval mode), which batch
    statistics over 32 .. 480 values per channel amplify: an fp32 emulation of that chain with torch's own BatchNorm gives 4.3e-5 /
    6.9e-5."""
    dev = _dev()
    c = _shipped()
    assert min(float(s[0].abs().min()) for s in c["s64"]) > 0.2 and all(s[2] == 2 for s in c["s64"]) and len(c["s64"]) == 14
    m = _no_layers(monkeypatch, copy.deepcopy(c["m"]).to(dev))
    errs = []
    with torch.no_grad():
        for x, y in zip(c["xs"], c["y64"]):
            got = m(x.to(dev)).cpu()
            assert got.shape == y.shape and got.shape[1] == 512
            errs.append(float((got.double() - y).abs().max()))
    print("shipped-channel neck, train(): kernel max err %.3e (per map %s), fp32 forward_layers max err %.3e, ratio %.2f, range %.3e"
          % (max(errs), ["%.3e" % e for e in errs], c["ref_err"], max(errs) / c["ref_err"], max(float(y.abs().max()) for y in c["y64"])))
    assert max(errs) <= 4 * c["ref_err"]
    print("shipped-channel neck, train(): running statistics after two forwards, worst relative error %.3e"
          % _check_running(m, c["s64"], "two forwards"))


@gpu
def test_mixed_modes_follow_torchs_rule_per_layer(monkeypatch):
    """Two BatchNorm2d modules in eval() inside a train() module: those layers use their running statistics and leave them unchanged,
    the others run on batch statistics and update."""
    dev = _dev()
    c = _shipped()
    tmpl = copy.deepcopy(c["m"])
    frozen = (0, 13)  # the first block layer and the last deblock: bns() order
    assert bns(tmpl)[0] is tmpl.blocks[0][2] and bns(tmpl)[13] is tmpl.deblocks[1][1]
    for i in frozen:
        bns(tmpl)[i].eval()
    assert tmpl.training
    x = c["xs"][0]
    (y64,), s64 = layers64_train(tmpl, [x])
    m = copy.deepcopy(tmpl).to(dev)
    before = _state(m)
    _no_layers(monkeypatch, m)
    with torch.no_grad():
        got = m(x.to(dev)).cpu().double()
    err = float((got - y64).abs().max())
    print("mixed modes: kernel max err %.3e, bar %.3e" % (err, 4 * c["ref_err"]))
    assert err <= 4 * c["ref_err"]
    assert float((y64 - c["y64"][0]).abs().max()) > 1e-3  # (not what the all-train module gives)
    after = _state(m)
    for i in frozen:
        assert torch.equal(after[i][0], before[i][0]) and torch.equal(after[i][1], before[i][1]) and after[i][2] == 0
    assert [s[2] for s in s64] == [0 if i in frozen else 1 for i in range(14)]
    _check_running(m, s64, "mixed modes", skip=frozen)


@gpu
def test_back_to_eval_after_a_training_forward(monkeypatch):
    """The kernels write the running statistics through raw pointers (no version bump): an eval forward after a train() forward folds
    the UPDATED statistics, also when eval packs of the old ones were cached.  Bar: the eval tests' (rtol 1e-4, atol 2e-5 max(1, range))."""
    fx, dev = train_fixture(), _dev()
    m = build_train_fixture_neck(batch_statistics=True, norm_cfg=dict(type="BN", eps=1e-3, momentum=0.5)).to(dev)
    x = torch.from_numpy(fx["x"]).to(dev)
    old64 = layers64(m, x)
    atol = 2e-5 * max(1.0, float(old64.abs().max()))
    _no_layers(monkeypatch, m)
    with torch.no_grad():
        got_old = m.eval()(x).cpu().double()  # caches the eval packs of the old statistics
        np.testing.assert_allclose(got_old.numpy(), old64.numpy(), rtol=1e-4, atol=atol)
        m.train()(x)
    assert all(int(bn.num_batches_tracked) == 1 for bn in bns(m))
    ref = build_train_fixture_neck()
    ref.load_state_dict(m.state_dict())
    new64 = layers64(ref, x)  # float64 eval of the state the kernels left
    stale = float((new64 - old64).abs().max())
    print("eval result moved by %.3e with the statistics (bar %.3e)" % (stale, atol))
    assert stale > 50 * atol  # a stale pack is off by far more than the bar
    with torch.no_grad():
        got_new = m.eval()(x).cpu().double()
        np.testing.assert_allclose(got_new.numpy(), new64.numpy(), rtol=1e-4, atol=2e-5 * max(1.0, float(new64.abs().max())))
        # and train() again does not need the eval packs: the statistics move on, the output (batch statistics only) keeps its bits
        y1 = m.train()(x).clone()
        y2 = m(x)
    assert torch.equal(y1, y2) and all(int(bn.num_batches_tracked) == 3 for bn in bns(m))


@gpu
def test_same_bits_on_a_second_identical_call(monkeypatch):
    fx, dev = train_fixture(), _dev()
    m = _no_layers(monkeypatch, build_train_fixture_neck(batch_statistics=True).to(dev))
    x = torch.from_numpy(fx["x"]).to(dev)
    start = _state(m)
    with torch.no_grad():
        y1 = m(x).clone()
        s1 = _state(m)
        for bn, s in zip(bns(m), start):  # restore the running statistics
            bn.running_mean.copy_(s[0])
            bn.running_var.copy_(s[1])
            bn.num_batches_tracked.fill_(s[2])
        y2 = m(x)
    s2 = _state(m)
    assert torch.equal(y1, y2) and float(y1.abs().max()) > 0
    for a, b, s in zip(s1, s2, start):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] == 1 and not torch.equal(a[0], s[0])


@gpu
def test_what_the_train_mode_refuses(monkeypatch):
    from shasta_amd import hip
    fx, dev = train_fixture(), _dev()
    m = _no_layers(monkeypatch, build_train_fixture_neck(batch_statistics=True).to(dev))
    with torch.no_grad():
        # 2 x 2 in: the stride-2 block's maps are 1 x 1, at B = 1 one value per channel
        with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
            m(torch.randn(1, 16, 2, 2, device=dev))
        assert all(int(bn.num_batches_tracked) == 0 for bn in bns(m))
        assert m(torch.randn(2, 16, 2, 2, device=dev)).shape == (2, 64, 2, 2)  # B = 2: two values, served
        cum = _no_layers(monkeypatch, build_train_fixture_neck(batch_statistics=True, norm_cfg=dict(type="BN", eps=1e-3, momentum=None)).to(dev))
        with pytest.raises(hip.ShastaHipError, match="momentum"):
            cum(torch.from_numpy(fx["x"]).to(dev))
        assert all(int(bn.num_batches_tracked) == 0 for bn in bns(cum))
        assert cum.eval()(torch.from_numpy(fx["x"]).to(dev)).shape == fx["y64"].shape  # eval() does not care
        with pytest.raises(hip.ShastaHipError, match="device tensor"):
            m(torch.from_numpy(fx["x"]))


@gpu
def test_graph_capture_and_replay(monkeypatch):
    """One small forward captured after a warm-up (a linear chain of launches): two replays advance num_batches_tracked by 2, the output
    equals the eager one; no buffer of the module is reallocated by the capture."""
    fx, dev = train_fixture(), _dev()
    m = _no_layers(monkeypatch, build_train_fixture_neck(batch_statistics=True).to(dev))
    x = torch.from_numpy(fx["x"]).to(dev)
    with torch.no_grad():
        eager = m(x).clone()
        static = x.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(static)  # warm-up: packed layers, ping-pong buffers, statistics buffers exist from here on
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        ptrs = [b.data_ptr() for b in m._bufs] + [b.data_ptr() for b in m._train_bufs] + [b.data_ptr() for b in m._packed]
        nbt = [int(bn.num_batches_tracked) for bn in bns(m)]
        assert nbt == [2] * 7
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = m(static)
        assert [b.data_ptr() for b in m._bufs] + [b.data_ptr() for b in m._train_bufs] + [b.data_ptr() for b in m._packed] == ptrs
        base = [int(bn.num_batches_tracked) for bn in bns(m)]
        graph.replay()
        graph.replay()
        torch.cuda.synchronize()
    assert [int(bn.num_batches_tracked) for bn in bns(m)] == [b + 2 for b in base]
    assert torch.equal(y, eager)


@gpu
def test_bevmap_with_both_switches_in_train_mode(monkeypatch):
    """BEVMap built as in tests/test_bevmap.py with batch_statistics=True on the backbone and on the neck, in train(): the map equals the
    neck's float64 restatement applied to the module's own backbone output, within 4 x the error of the neck's fp32 forward_layers on
    that input; neck.forward_layers is never called."""
    import shasta_amd
    from shasta_amd.backbone import SpMiddleResNetFHD
    from tests import backbone_train_helpers as BT
    from tests.test_bevmap import RANGE, VOXEL, _clouds
    dev = _dev()
    torch.manual_seed(61)
    m = shasta_amd.build_bev(dict(type="BEVMap", reader=dict(type="DynamicVoxelEncoder", pc_range=RANGE, voxel_size=VOXEL),
                                  backbone=dict(type=SpMiddleResNetFHD, num_input_features=5, ds_factor=8, batch_statistics=True),
                                  neck=dict(type="RPN", batch_statistics=True, **SHIPPED))).train()
    assert m.backbone.batch_statistics is True and m.neck.batch_statistics is True and m.neck.training
    BT.randomize_train(m.backbone, torch.Generator().manual_seed(62))
    randomize_bn_train(m.neck, torch.Generator().manual_seed(63))
    m = m.to(dev)
    neck0 = copy.deepcopy(m.neck).cpu()
    _no_layers(monkeypatch, m.neck)
    clouds = [c.to(dev) for c in _clouds(2)]
    with torch.no_grad():
        got = m(dict(points=clouds)).cpu()
        v, c, shape = m.reader(clouds)
        x = m.backbone(v, c, 2, shape)[0].cpu()  # batch statistics only: the bits of the forward above
    assert got.shape == (2, 512, 24, 24) and x.shape == (2, 256, 24, 24) and float(x.abs().max()) > 0
    (y64,), s64 = layers64_train(neck0, [x])
    with torch.no_grad():
        ref_err = float((copy.deepcopy(neck0).forward_layers(x).double() - y64).abs().max())
    err = float((got.double() - y64).abs().max())
    print("BEVMap, train(): neck max err %.3e, fp32 forward_layers max err %.3e, ratio %.2f, range %.3e"
          % (err, ref_err, err / ref_err, float(y64.abs().max())))
    assert ref_err > 0 and err <= 4 * ref_err
    _check_running(m.neck, s64, "BEVMap")
    assert all(int(bn.num_batches_tracked) == 1 for bn in bns(m.neck))
