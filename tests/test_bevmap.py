"""BEVMap on the device: DynamicVoxelEncoder (csrc/dynvox.hip) -> SpMiddleResNetFHD (sparse_conv.hip) -> RPN (neck.hip), and
CloudMaps, which feeds pipeline.run_split from point clouds.  Shapes of test_from_points_to_affinity_matrices: 192 x 192 x 40 voxels
of 0.5625 m, the shipped neck channels, B = 2, clustered clouds of ~900 points."""
import functools

import numpy as np
import pytest
import torch

from tests import backbone_helpers as BH
from tests.neck_helpers import SHIPPED, randomize_bn

pytestmark = pytest.mark.gpu
RANGE, VOXEL = [-54, -54, -5, 54, 54, 3], [0.5625, 0.5625, 0.2]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda", 0)


def _build(reader):
    import shasta_amd
    from shasta_amd.backbone import SpMiddleResNetFHD
    torch.manual_seed(61)
    m = shasta_amd.build_bev(dict(type="BEVMap", reader=reader, backbone=dict(type=SpMiddleResNetFHD, num_input_features=5, ds_factor=8),
                                  neck=dict(type="RPN", **SHIPPED))).eval()
    BH.randomize(m.backbone, torch.Generator().manual_seed(62))
    randomize_bn(m.neck, torch.Generator().manual_seed(63))
    return m


def _clouds(n, seed=64):
    g = torch.Generator().manual_seed(seed)
    clouds = []
    for _ in range(n):  # a few clusters inside the range
        centres = (torch.rand(6, 3, generator=g) - 0.5) * torch.tensor([90.0, 90.0, 5.0]) + torch.tensor([0.0, 0.0, -1.0])
        pts = centres.repeat_interleave(150, 0) + torch.randn(900, 3, generator=g) * torch.tensor([2.0, 2.0, 0.5])
        pts[0] = torch.tensor([54.0, 1.0, -1.0])  # on the upper x face: coordinate 192, one past the backbone's grid
        clouds.append(torch.cat([pts, torch.rand(900, 2, generator=g)], 1))
    return clouds


@functools.lru_cache(maxsize=None)
def _dynamic():
    """Model, clouds, the reader's rows and the composed map; computed once, shared, left unchanged."""
    dev = _dev()
    m = _build(dict(type="DynamicVoxelEncoder", pc_range=RANGE, voxel_size=VOXEL)).to(dev)
    clouds = [c.to(dev) for c in _clouds(2)]
    with torch.no_grad():
        v, c, shape = m.reader(clouds)
        want = m.neck(m.backbone(v, c, 2, shape)[0])
    torch.cuda.synchronize()
    return m, clouds, v, c, shape, want


def test_bevmap_is_the_composition_of_its_stages():
    m, clouds, v, c, shape, want = _dynamic()
    assert shape.tolist() == [192, 192, 40] and c.dtype == torch.int32 and int((c[:, 3] == 192).sum()) == 2
    with torch.no_grad():
        got = m(dict(points=clouds))
        x, vf = m.extract_feat(dict(points=clouds))
    assert got.shape == (2, 512, 24, 24) and float(got.abs().max()) > 0 and not torch.equal(got[0], got[1])
    assert torch.equal(got, want) and torch.equal(x, want) and set(vf) == {"conv1", "conv2", "conv3", "conv4"}
    with torch.no_grad():
        assert [torch.equal(a[0], want) for a in m.extract_feats([dict(points=clouds)] * 2)] == [True, True]


def test_dynamic_rows_through_the_backbone_against_float64():
    """The reader's sorted rows - one per cloud on the upper x face, outside the backbone's grid and therefore inactive - give the
    backbone output of the float64 dense restatement, at test_backbone_kernels' bound.  Same voxels, z extent, weights and cluster
    recipe as the other tests here, but a quarter of the x and y extent (48 x 48 x 40): the dense float64 restatement of the
    192 x 192 grid alone takes 16 s on the host, and the grid's size plays no part in what is checked."""
    import copy
    m, _, _, _, _, _ = _dynamic()
    reader = type(m.reader)([-13.5, -13.5, -5, 13.5, 13.5, 3], VOXEL)
    clouds = []
    for c in _clouds(2, seed=65):
        c = c.clone()
        c[:, :2] *= 0.25
        clouds.append(c.to(_dev()))
    with torch.no_grad():
        v, c, shape = reader(clouds)
        got = m.backbone(v, c, 2, shape)[0].cpu().double()
    assert shape.tolist() == [48, 48, 40]
    vc, cc = v.cpu(), c.cpu()
    inside = (cc[:, 2] < 48) & (cc[:, 3] < 48)
    assert int((~inside).sum()) == 2 and int(inside.sum()) > 500
    ref, _ = BH.reference_forward(copy.deepcopy(m.backbone).cpu(), vc[inside], cc[inside].numpy(), 2, shape, torch.float64)
    scale = float(ref.abs().max())
    assert scale > 0 and got.shape == ref.shape
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-4, atol=2e-5 * max(1.0, scale))


def test_voxels_branch_equals_its_composition():
    from shasta_amd.voxel_generator import VoxelGenerator
    dev = _dev()
    m = _build(dict(type="VoxelFeatureExtractorV3", num_input_features=5)).to(dev)
    clouds = [c.to(dev) for c in _clouds(2)]
    vg = VoxelGenerator(VOXEL, RANGE, 10, max_voxels=4000)
    voxels, coors, num, _, nv = vg.generate_batch_device(clouds)
    nv = nv.cpu().tolist()
    vs = torch.cat([voxels[b, :nv[b]] for b in range(2)])
    ns = torch.cat([num[b, :nv[b]] for b in range(2)])
    cs = torch.cat([torch.cat([torch.full((nv[b], 1), b, dtype=torch.int32, device=dev), coors[b, :nv[b]]], 1) for b in range(2)])
    shape = [vg.grid_size.tolist()]
    with torch.no_grad():
        got = m(dict(voxels=vs, num_points=ns, coordinates=cs, points=[None] * 2, shape=shape))
        want = m.neck(m.backbone(m.reader(vs, ns), cs, 2, shape[0])[0])
    assert got.shape == (2, 512, 24, 24) and float(got.abs().max()) > 0 and torch.equal(got, want)


def test_freeze_leaves_the_bits():
    m, clouds, _, _, _, want = _dynamic()
    import copy
    f = copy.deepcopy(m)
    assert f.freeze() is f and not f.training and not any(p.requires_grad for p in f.parameters())
    assert any(isinstance(x, torch.nn.BatchNorm2d) for x in f.neck.modules())  # not swapped for another class
    got = f(dict(points=clouds))  # no no_grad needed: nothing requires a gradient
    assert torch.equal(got, want)


def test_cloud_maps_feed_run_split(tmp_path):
    """run_split from point clouds (CloudMaps) returns exactly what it returns given the same maps computed beforehand."""
    import shasta_amd
    from shasta_amd import pipeline, scenes
    from shasta_amd.backbone import SpMiddleResNetFHD
    from tests import dynvox_helpers as H
    dev = _dev()
    paths, sc = scenes.write_synthetic_split(str(tmp_path), n_scenes=1, frames_per_scene=3, seed=3)
    models = {"car": pipeline.build_class_model("car", dev, seed=5)}
    torch.manual_seed(71)
    bev = shasta_amd.build_bev(dict(type="BEVMap", reader=dict(type="DynamicVoxelEncoder", pc_range=H.SHIPPED_RANGE, voxel_size=H.SHIPPED_VOXEL),
                                    backbone=dict(type=SpMiddleResNetFHD, num_input_features=5, ds_factor=8), neck=dict(type="RPN", **SHIPPED)))
    BH.randomize(bev.backbone, torch.Generator().manual_seed(72))
    randomize_bn(bev.neck, torch.Generator().manual_seed(73))
    bev = bev.to(dev).freeze()
    tokens = [t for _, toks in sc for t in toks]
    store = {t: H.radial_cloud(20000, 100 + i) for i, t in enumerate(tokens)}
    calls = []

    def clouds(token):
        calls.append(token)
        return store[token]

    feeder = shasta_amd.CloudMaps(bev, clouds, max_clouds=3)
    with torch.no_grad():
        maps = {t: bev(dict(points=[torch.from_numpy(store[t]).to(dev)]))[0] for t in tokens}
    assert maps[tokens[0]].shape == (512, 180, 180) and not torch.equal(maps[tokens[0]], maps[tokens[1]])

    class Precomputed:
        def neck_batch(self, toks, device):
            return torch.stack([maps[t] for t in toks]).to(device)

    four = [tokens[0]] + tokens  # a run as _run_features forms it: 4 tokens, two groups of at most 3
    assert torch.equal(feeder.neck_batch(four, dev), Precomputed().neck_batch(four, dev)) and calls == four
    got = pipeline.run_split(models, paths, sc, feeder, dev, batch_pairs=3)
    want = pipeline.run_split(models, paths, sc, Precomputed(), dev, batch_pairs=3)
    assert len(got) == 3 and got[0].keys() == want[0].keys() == {"car"}
    assert got[0] == want[0] and got[1] == want[1] and got[2] == want[2]
    assert sum(len(v) for v in got[1]["results"].values()) > 0
