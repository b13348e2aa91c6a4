"""CPU: the registered `RPN` neck (shasta_amd/neck.py) against the reference fixture tests/golden/neck_golden.npz - module creation
order, state_dict keys, the nn form of the forward - and the size / support queries of the neck's C ABI."""
import numpy as np
import pytest
import torch

from tests.neck_helpers import C1, C3S1, C3S2, D2, build_fixture_neck, fixture


def test_registry_builds_the_fixture_config_with_the_reference_tensors():
    """builder.build_neck under the fixture's seed: the reference's key list in the reference's order, every tensor bit for bit as the
    reference first constructs it (module creation order = RNG order)."""
    import shasta_amd
    assert shasta_amd.NECKS.get("RPN") is shasta_amd.RPN
    fx = fixture()
    m = build_fixture_neck(load_used=False)
    sd = m.state_dict()
    assert list(sd.keys()) == fx["keys"]
    assert len(fx["keys"]) == 42 and sum(v.numel() for v in sd.values()) == 88711
    assert fx["keys"][0] == "blocks.0.1.weight"  # the ZeroPad2d sits at index 0 of each block
    assert "deblocks.1.0.weight" in fx["keys"] and "deblocks.0.1.running_var" in fx["keys"]
    for k, v in sd.items():
        assert v.numpy().dtype == fx["init"][k].dtype and np.array_equal(v.numpy(), fx["init"][k]), k
    bn = m.blocks[0][2]
    assert isinstance(bn, torch.nn.BatchNorm2d) and bn.eps == 1e-3 and bn.momentum == 0.01  # the default norm
    assert m.downsample_factor == 1.0  # prod(ds strides) / last us stride


def test_forward_layers_matches_the_reference_within_its_own_error():
    """Padding, stride handling, the deconvolution weight layout, the concat order and eps against the reference: within 4 x the
    reference's own fp32 error against its float64 run."""
    fx = fixture()
    m = build_fixture_neck()
    with torch.no_grad():
        got = m.forward_layers(torch.from_numpy(fx["x"])).numpy()
    assert got.shape == fx["y64"].shape == (2, 64, 10, 38)
    ref_err = float(np.abs(fx["y32"] - fx["y64"]).max())
    err = float(np.abs(got - fx["y64"]).max())
    print("forward_layers: max|got - y64| = %.3e, reference max|y32 - y64| = %.3e, range %.3e" % (err, ref_err, float(np.abs(fx["y64"]).max())))
    assert ref_err > 0 and err <= 4 * ref_err
    # train() mode and autograd stay on the nn layers, also on the CPU (batch statistics, like the reference's frozen neck)
    x = torch.from_numpy(fx["x"]).requires_grad_(True)
    assert m(x).requires_grad
    with torch.no_grad():
        assert torch.equal(m.train()(x), m.forward_layers(x))


def test_kernel_path_refuses_cpu_tensors():
    from shasta_amd import hip
    fx = fixture()
    m = build_fixture_neck()
    with torch.no_grad(), pytest.raises(hip.ShastaHipError):
        m(torch.from_numpy(fx["x"]))


def test_size_and_support_queries_need_no_gpu():
    from shasta_amd import hip
    lib = hip.load()
    for kind in (C3S1, C3S2, C1, D2):
        for cin, cout in ((8, 32), (16, 64), (256, 128), (128, 256), (40, 96)):
            nbytes = lib.shasta_neck_layer_packed_bytes(kind, cin, cout)
            taps = 9 if kind in (C3S1, C3S2) else 4 if kind == D2 else 1
            assert nbytes >= (cin * cout * taps + 2 * cout) * 4, (kind, cin, cout)  # every weight + alpha, beta'
            assert lib.shasta_neck_layer_supported(kind, cin, cout, 6, 34) == 1
            assert lib.shasta_neck_layer_supported(kind, cin, cout, 1, 1) == (0 if kind == C3S2 else 1)
        assert lib.shasta_neck_layer_supported(kind, 12, 32, 6, 34) == 0
        assert lib.shasta_neck_layer_supported(kind, 16, 48, 6, 34) == 0
        assert lib.shasta_neck_layer_packed_bytes(kind, 12, 32) == 0 and lib.shasta_neck_layer_packed_bytes(kind, 16, 48) == 0
        assert lib.shasta_neck_layer_supported(kind, 16, 32, 0, 34) == 0 and lib.shasta_neck_layer_supported(kind, 16, 32, 6, 0) == 0
    assert lib.shasta_neck_layer_supported(C3S2, 16, 32, 5, 34) == 0 and lib.shasta_neck_layer_supported(C3S2, 16, 32, 6, 33) == 0
    assert lib.shasta_neck_layer_supported(C3S1, 16, 32, 5, 33) == 1
    assert lib.shasta_neck_layer_supported(4, 16, 32, 6, 34) == 0 and lib.shasta_neck_layer_supported(-1, 16, 32, 6, 34) == 0
    # the shipped layers at the shipped map
    for kind, cin, cout, hw in ((C3S1, 256, 128, 180), (C3S1, 128, 128, 180), (C3S2, 128, 256, 180), (C3S1, 256, 256, 90), (C1, 128, 256, 180),
                                (D2, 256, 256, 90)):
        assert lib.shasta_neck_layer_supported(kind, cin, cout, hw, hw) == 1


def test_constructor_asserts_and_module_api():
    from shasta_amd import builder
    fx = fixture()
    for bad in (dict(ds_layer_strides=[1]), dict(ds_num_filters=[32]), dict(us_num_filters=[32]), dict(us_layer_strides=[1, 1])):
        with pytest.raises(AssertionError):  # list lengths / the deblocks' common resolution, as the reference asserts
            builder.build_neck(dict(type="RPN", **dict(fx["cfg"], **bad)))
    # fewer deblocks than blocks: they belong to the LAST blocks (upsample_start_idx)
    m = builder.build_neck(dict(type="RPN", layer_nums=[1, 1], ds_layer_strides=[2, 2], ds_num_filters=[8, 8], us_layer_strides=[4],
                                us_num_filters=[8], num_input_features=8))
    assert len(m.blocks) == 2 and len(m.deblocks) == 1 and m.downsample_factor == 1.0
    assert isinstance(m.deblocks[0][0], torch.nn.ConvTranspose2d)
    with torch.no_grad():
        assert m.eval().forward_layers(torch.zeros(1, 8, 8, 8)).shape == (1, 8, 8, 8)
    # us stride < 1: the reference's strided Conv2d deblock; GroupNorm: both only through forward_layers
    m = builder.build_neck(dict(type="RPN", layer_nums=[1], ds_layer_strides=[1], ds_num_filters=[8], us_layer_strides=[0.5],
                                us_num_filters=[8], num_input_features=8, norm_cfg=dict(type="GN", num_groups=2)))
    assert m.deblocks[0][0].stride == (2, 2) and isinstance(m.deblocks[0][1], torch.nn.GroupNorm) and m._plan is None
    with torch.no_grad():
        assert m.eval()(torch.zeros(1, 8, 8, 8)).shape == (1, 8, 4, 4)
    # init_weights: xavier uniform on every Conv2d (bound sqrt(6 / (fan_in + fan_out)))
    m = build_fixture_neck(load_used=False)
    m.init_weights()
    w = m.blocks[1][1].weight.detach()
    bound = float(np.sqrt(6.0 / (32 * 9 + 64 * 9)))
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.9 * bound
