"""CPU: the host side of the sparse backbone (shasta_amd/backbone.py) - state_dict contract, spconv 1.x weight layouts, registration,
size queries - and the dense restatement of tests/backbone_helpers.py against a brute-force per-site loop."""
import numpy as np
import pytest
import torch

from tests import backbone_helpers as BH


def _expected_keys():
    """The reference's `backbone.*` keys and shapes (det3d/models/backbones/scn.py:98-161), written out."""
    def bn(prefix, c):
        return [(prefix + ".weight", (c,)), (prefix + ".bias", (c,)), (prefix + ".running_mean", (c,)), (prefix + ".running_var", (c,)),
                (prefix + ".num_batches_tracked", ())]

    def block(prefix, c):
        return ([(prefix + ".conv1.weight", (c, 3, 3, 3, c)), (prefix + ".conv1.bias", (c,))] + bn(prefix + ".bn1", c)
                + [(prefix + ".conv2.weight", (c, 3, 3, 3, c)), (prefix + ".conv2.bias", (c,))] + bn(prefix + ".bn2", c))

    keys = [("conv_input.0.weight", (16, 3, 3, 3, 5))] + bn("conv_input.1", 16) + block("conv1.0", 16) + block("conv1.1", 16)
    for name, cin, c in (("conv2", 16, 32), ("conv3", 32, 64), ("conv4", 64, 128)):
        keys += [(name + ".0.weight", (c, 3, 3, 3, cin))] + bn(name + ".1", c) + block(name + ".3", c) + block(name + ".4", c)
    keys += [("extra_conv.0.weight", (128, 3, 1, 1, 128))] + bn("extra_conv.1", 128)
    return keys


def _backbone(**kw):
    from shasta_amd.backbone import SpMiddleResNetFHD
    return SpMiddleResNetFHD(num_input_features=5, ds_factor=8, **kw)


def test_state_dict_keys_and_shapes():
    m = _backbone()
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == _expected_keys()
    assert len(got) == 21 + 16 + 21 * 5  # 21 weights, 16 biases (the blocks' convolutions), 21 BatchNorms
    assert all(bn.eps == 1e-3 and bn.momentum == 0.01 for bn in m.modules() if isinstance(bn, torch.nn.BatchNorm1d))


def test_spconv_1x_weights_load_permuted():
    """checkpoint.py:77-91: (kD, kH, kW, Cin, Cout) -> permute(4, 0, 1, 2, 3); a weight that only needs transpose(-1, -2) takes that."""
    import shasta_amd
    m = _backbone()
    g = torch.Generator().manual_seed(3)
    sd2 = {k: torch.randn(v.shape, generator=g) if v.dtype.is_floating_point else v.clone() for k, v in m.state_dict().items()}
    sd1 = {k: v.permute(1, 2, 3, 4, 0).contiguous() if v.dim() == 5 else v for k, v in sd2.items()}
    assert sd1["conv2.0.weight"].shape == (3, 3, 3, 16, 32)
    m.load_state_dict(sd1)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd2[k]), k
    # ... and through the parent module's load_state_dict (keys `backbone.*`), as a whole-model checkpoint arrives
    cfg = dict(type="Shasta", reader=None, backbone=dict(type=shasta_amd.backbone.SpMiddleResNetFHD, num_input_features=5, ds_factor=8),
               neck=None, bev_extractor=dict(type="BEVFeatureExtractor", pc_start=[-54, -54], voxel_size=[0.075, 0.075], out_stride=8),
               max_obj=4, num_feats=3, num_point=1)
    whole = shasta_amd.build_simp_track(cfg)
    sd = whole.state_dict()
    sd.update({"backbone." + k: v for k, v in sd1.items()})
    whole.load_state_dict(sd)
    assert torch.equal(whole.backbone.conv4[0].weight, sd2["conv4.0.weight"])
    # transpose(-1, -2) is tried first
    from shasta_amd.backbone import SparseConv3d
    c = SparseConv3d(4, 8, 3)
    w = torch.randn(8, 3, 3, 4, 3, generator=g)  # (.., Cin, kW) with the last two axes swapped
    c.load_state_dict({"weight": w, "bias": torch.zeros(8)})
    assert torch.equal(c.weight, w.transpose(-1, -2))
    with pytest.raises(RuntimeError):  # a shape that fits neither way stays an error
        c.load_state_dict({"weight": torch.zeros(8, 3, 3, 3, 5), "bias": torch.zeros(8)})


@pytest.fixture
def registry_restored():
    import shasta_amd
    before = dict(shasta_amd.BACKBONES.module_dict)
    yield shasta_amd.BACKBONES
    shasta_amd.BACKBONES.module_dict.clear()
    shasta_amd.BACKBONES.module_dict.update(before)


def test_registration(registry_restored):
    import shasta_amd
    from shasta_amd.backbone import SpMiddleResNetFHD, register
    reg = registry_restored
    reg.module_dict.pop("SpMiddleResNetFHD", None)  # (another test of this process may have registered it)
    base = dict(type="Shasta", reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5), neck=None,
                bev_extractor=dict(type="BEVFeatureExtractor", pc_start=[-54, -54], voxel_size=[0.075, 0.075], out_stride=8),
                max_obj=4, num_feats=3, num_point=1)
    with pytest.raises(KeyError):
        shasta_amd.build_simp_track(dict(base, backbone=dict(type="SpMiddleResNetFHD", num_input_features=5, ds_factor=8)))
    m = shasta_amd.build_simp_track(dict(base, backbone=dict(type=SpMiddleResNetFHD, num_input_features=5, ds_factor=8)))
    assert isinstance(m.backbone, SpMiddleResNetFHD) and "backbone.conv_input.0.weight" in m.state_dict()
    assert [type(c).__name__ for c in m.children()][:2] == ["VoxelFeatureExtractorV3", "SpMiddleResNetFHD"]
    assert register() is SpMiddleResNetFHD and register() is SpMiddleResNetFHD  # idempotent
    m = shasta_amd.build_simp_track(dict(base, backbone=dict(type="SpMiddleResNetFHD", num_input_features=5, ds_factor=8)))
    assert isinstance(m.backbone, SpMiddleResNetFHD)

    class Other(torch.nn.Module):
        pass

    reg.module_dict["SpMiddleResNetFHD"] = Other
    with pytest.raises(KeyError):
        register()
    assert reg.get("SpMiddleResNetFHD") is Other


def test_fresh_import_does_not_register():
    """In a fresh interpreter: importing the package leaves BACKBONES without the class (tests/test_abi.py relies on the KeyError)."""
    import os
    import subprocess
    import sys
    code = "import shasta_amd, shasta_amd.backbone; assert shasta_amd.BACKBONES.get('SpMiddleResNetFHD') is None; print('ok')"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_size_queries_and_supported_do_not_need_a_gpu():
    from shasta_amd import hip
    lib = hip.load()
    sub, s2, p011, last = (sum(BH.GEOMETRIES[n], ()) for n in ("subm", "k3s2p1", "k3s2p011", "k311s211p0"))
    for cin, cout, geom in ((5, 16, sub), (16, 16, sub), (32, 32, sub), (64, 64, sub), (128, 128, sub), (16, 32, s2), (32, 64, s2),
                            (64, 128, p011), (128, 128, last)):
        assert lib.shasta_spconv_supported(cin, cout, *geom) == 1
    assert lib.shasta_spconv_supported(24, 32, *sub) == 0 and lib.shasta_spconv_supported(16, 48, *sub) == 0
    assert lib.shasta_spconv_supported(16, 32, 5, 3, 3, 1, 1, 1, 1, 1, 1) == 0   # kernel size 5
    assert lib.shasta_spconv_supported(16, 32, 3, 3, 3, 3, 1, 1, 1, 1, 1) == 0   # stride 3
    assert lib.shasta_spconv_supported(16, 32, 3, 3, 3, 1, 1, 1, 2, 1, 1) == 0   # padding 2
    # packed layer: [taps][Cin -> 8 at least][Cout] weights + alpha + beta'
    assert lib.shasta_spconv_layer_packed_bytes(5, 16, 27) == (27 * 8 * 16 + 32) * 4
    assert lib.shasta_spconv_layer_packed_bytes(128, 128, 3) == (3 * 128 * 128 + 256) * 4
    assert lib.shasta_spconv_layer_packed_bytes(24, 32, 27) == 0 and lib.shasta_spconv_layer_packed_bytes(16, 32, 25) == 0
    # index of a level: bitmap + prefix counts (4 bytes per 32 cells each, whole blocks of 1024 words), block sums, one int per row
    shipped = lib.shasta_spconv_index_workspace_bytes(2, 41, 1440, 1440, 200000)
    cells = 2 * 41 * 1440 * 1440
    assert 2 * cells // 8 + 4 * 200000 <= shipped <= 2 * cells // 8 + 4 * 200000 + (1 << 16)
    assert lib.shasta_spconv_index_workspace_bytes(1, 1, 1, 1, 0) > 0
    assert lib.shasta_spconv_index_workspace_bytes(64, 41, 1440, 1440, 1) == 0  # 2^31 cells or more: not served
    assert lib.shasta_spconv_index_workspace_bytes(1, 0, 4, 4, 1) == 0


def test_train_mode_and_cpu_tensors_raise():
    from shasta_amd import hip
    m = _backbone()
    x, c = torch.zeros(3, 5), torch.zeros(3, 4, dtype=torch.int32)
    with pytest.raises(hip.ShastaHipError, match="train"):
        m(x, c, 1, [8, 8, 4])
    m.eval()
    with torch.no_grad(), pytest.raises(hip.ShastaHipError, match="device"):
        m(x, c, 1, [8, 8, 4])
    with pytest.raises(hip.ShastaHipError, match="holds parameters only"):
        m.conv1[0](x)
    gn = _backbone(norm_cfg=dict(type="GN", num_groups=4)).eval()
    assert isinstance(gn.conv_input[1], torch.nn.GroupNorm)  # builds, like the reference; the forward refuses (GPU test)


@pytest.mark.parametrize("name", list(BH.GEOMETRIES))
def test_dense_restatement_equals_the_per_site_loop(name):
    """1 x 5 x 6 x 7 grid, 8 -> 16 channels: conv3d + max_pool3d mask bookkeeping against the literal sums of the specification."""
    geom = BH.GEOMETRIES[name]
    subm = name == "subm"
    B, grid = 1, (5, 6, 7)
    rng = np.random.RandomState(5)
    coords = BH.random_voxels(rng, B, grid, 40)
    g = torch.Generator().manual_seed(6)
    feats = torch.randn(len(coords), 8, generator=g, dtype=torch.float64)
    w = torch.randn(16, *geom[0], 8, generator=g, dtype=torch.float64)
    bias = torch.randn(16, generator=g, dtype=torch.float64) if subm else None
    x, mask = BH.to_dense(feats, coords, B, grid)
    y, mo = BH.dense_conv(x, mask, w, bias, geom, subm)
    outs, want = BH.brute_conv(feats, coords, B, grid, w, bias, geom, subm)
    assert np.array_equal(BH.mask_coords(mo), outs)
    assert tuple(y.shape[2:]) == (grid if subm else BH.out_grid(grid, geom))
    np.testing.assert_allclose(BH.rows_of(y, outs).numpy(), want.numpy(), rtol=1e-12, atol=1e-12)
    assert float((y * (1 - mo)).abs().max()) == 0.0  # exact zeros at inactive sites
