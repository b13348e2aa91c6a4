"""Dynamic voxelisation (csrc/dynvox.hip, shasta_amd/dynamic_voxel_encoder.py) and the BEV registry.

CPU part: the numpy restatement (tests/dynvox_helpers.py) equals the reference's DynamicVoxelEncoder bit for bit on the stored golden;
registries, refusals, size queries.  GPU part: the kernel chain through the C ABI equals the restatement bit for bit - voxels as
uint32, coordinates, counts, the per-cloud prefix; no tolerance anywhere."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from tests import dynvox_helpers as H

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dynvox_golden.npz")
E_WORKSPACE, E_UNSUPPORTED = -2, -5
SMALL_RANGE, SMALL_VOXEL = [-4.0, -3.0, -1.0, 4.0, 3.0, 1.0], [0.25, 0.2, 0.4]  # 32 x 30 x 5
THREAD_MAX = 32  # csrc/dynvox.hip DV_THREAD_MAX: lists up to here are summed by one thread per (voxel, channel), longer ones by a wavefront


@functools.lru_cache(maxsize=None)
def _golden():
    g = np.load(GOLDEN)
    out = {}
    for b in ("faces", "crowded", "batch"):
        off = g[b + "_offsets"]
        out[b] = dict(range=g[b + "_range"], voxel=g[b + "_voxel"], clouds=[g[b + "_points"][off[i]:off[i + 1]] for i in range(len(off) - 1)],
                      voxels=g[b + "_voxels"], coors=g[b + "_coors"], shape=g[b + "_shape"])
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- CPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["faces", "crowded", "batch"])
def test_restatement_equals_the_reference_golden(name):
    g = _golden()[name]
    v, c, n, prefix = H.voxelize_batch(g["clouds"], g["range"], g["voxel"])
    assert v.dtype == np.float32 and g["voxels"].dtype == np.float32 and g["coors"].dtype == np.int64
    assert np.array_equal(_bits(v), _bits(g["voxels"]))
    assert np.array_equal(c, g["coors"])
    shape = H.grid_shape(g["range"], g["voxel"])
    assert shape.dtype == np.int32 and g["shape"].dtype == np.int32 and np.array_equal(shape, g["shape"])
    assert prefix[-1] == len(v) and int(n.sum()) <= sum(len(x) for x in g["clouds"])


def test_golden_holds_the_cases_it_is_for():
    g = _golden()
    _, c, _, _ = H.voxelize_batch(g["faces"]["clouds"], g["faces"]["range"], g["faces"]["voxel"])
    gx, gy, gz = g["faces"]["shape"]
    assert (c[:, 1] == gz).any() and (c[:, 2] == gy).any() and (c[:, 3] == gx).any() and (c[:, 1:] == 0).any(0).all()  # every face
    assert H.voxelize_batch(g["crowded"]["clouds"], g["crowded"]["range"], g["crowded"]["voxel"])[2].max() >= 2000
    assert [len(x) for x in g["batch"]["clouds"]][1] == 0 and len(g["batch"]["clouds"]) == 3
    assert os.path.getsize(GOLDEN) < 1 << 20


def test_registries_and_build_bev():
    import shasta_amd
    from shasta_amd.backbone import SpMiddleResNetFHD
    from tests.neck_helpers import SHIPPED
    assert shasta_amd.READERS.get("DynamicVoxelEncoder") is shasta_amd.DynamicVoxelEncoder
    assert shasta_amd.BEV.get("BEVMap") is shasta_amd.BEVMap and shasta_amd.BEV.get("SingleStageBEV") is shasta_amd.SingleStageBEV
    assert shasta_amd.BACKBONES.get("SpMiddleResNetFHD") is None  # still passed as a class
    reader = dict(type="DynamicVoxelEncoder", pc_range=H.SHIPPED_RANGE, voxel_size=H.SHIPPED_VOXEL)
    backbone = dict(type=SpMiddleResNetFHD, num_input_features=5, ds_factor=8)
    neck = dict(type="RPN", **SHIPPED)
    m = shasta_amd.build_bev(dict(type="BEVMap", reader=reader, backbone=backbone, neck=neck, pretrained=None), train_cfg=dict(a=1),
                             test_cfg=dict(x=2))
    assert type(m) is shasta_amd.BEVMap and isinstance(m, shasta_amd.SingleStageBEV) and isinstance(m, shasta_amd.BaseBEV)
    assert m.train_cfg == dict(a=1) and m.test_cfg == dict(x=2) and m.with_reader and m.with_neck
    assert [type(c).__name__ for c in m.children()] == ["DynamicVoxelEncoder", "SpMiddleResNetFHD", "RPN"]
    s = shasta_amd.build_simp_track(dict(type="Shasta", reader=dict(type="VoxelFeatureExtractorV3", num_input_features=5), backbone=backbone,
                                         neck=neck, max_obj=8, num_feats=7, num_point=5,
                                         bev_extractor=dict(type="BEVFeatureExtractor", pc_start=[-54, -54], voxel_size=[0.075, 0.075], out_stride=8)))
    want = [k for k in s.state_dict() if k.startswith(("backbone.", "neck."))]
    assert list(m.state_dict().keys()) == want and len(want) > 100
    assert all(m.state_dict()[k].shape == s.state_dict()[k].shape for k in want)
    with pytest.raises(KeyError):
        shasta_amd.build_bev(dict(type="NoSuchBEV", reader=None, backbone=None, neck=None))
    f = m.freeze()
    assert f is m and not m.training and not any(p.requires_grad for p in m.parameters())


def test_checkpoint_loading_bare_and_wrapped(tmp_path, capsys):
    import shasta_amd
    from tests.neck_helpers import SHIPPED
    cfg = dict(type="BEVMap", reader=None, backbone=None, neck=dict(type="RPN", **SHIPPED))
    src = shasta_amd.build_bev(cfg)
    with torch.no_grad():
        for p in src.parameters():
            p.add_(0.25)
    for name, obj in (("bare.pth", src.state_dict()), ("wrapped.pth", {"state_dict": {"module." + k: v for k, v in src.state_dict().items()}})):
        torch.save(obj, str(tmp_path / name))
        m = shasta_amd.build_bev(dict(cfg, pretrained=str(tmp_path / name)))
        assert "init weight from " + str(tmp_path / name) in capsys.readouterr().out
        assert all(torch.equal(v, src.state_dict()[k]) for k, v in m.state_dict().items())
    shasta_amd.build_bev(dict(cfg, pretrained=str(tmp_path / "absent.pth")))
    assert "no pretrained model at " + str(tmp_path / "absent.pth") in capsys.readouterr().out


def test_reader_constructor_and_refusals():
    import shasta_amd
    from shasta_amd import hip
    r = shasta_amd.DynamicVoxelEncoder(H.SHIPPED_RANGE, H.SHIPPED_VOXEL)
    assert r.shape_np.dtype == np.int32 and r.shape_np.tolist() == [1440, 1440, 40]
    assert r.pc_range.dtype == torch.float32 and r.voxel_size.dtype == torch.float32 and r.virtual is False
    assert r.shape.tolist() == [1440.0, 1440.0, 40.0] and len(list(r.parameters())) == 0
    with pytest.raises(NotImplementedError):
        shasta_amd.DynamicVoxelEncoder(H.SHIPPED_RANGE, H.SHIPPED_VOXEL, virtual=True)
    with pytest.raises(hip.ShastaHipError):
        r([torch.zeros(4, 5)])


def _offsets(sizes):
    return (C.c_int * (len(sizes) + 1))(*np.cumsum([0] + list(sizes)).tolist())


def test_size_query_needs_no_gpu():
    from shasta_amd import hip
    lib = hip.load()
    q = lib.shasta_dynvox_workspace_bytes
    # 16 clouds x 3e5 points at the shipped grid: two bitmap-sized arrays of 16 x 41 x 1441 x 1441 bits rounded up to scan blocks
    # (2 x 170 262 528 bytes), their block sums, six per-point int arrays and the small lists
    assert q(_offsets([300000] * 16), 16, 1440, 1440, 40) == 456521472
    assert q(_offsets([0]), 1, 3, 2, 1) == 18688
    assert 25 * 41 * 1441 * 1441 < 2 ** 31 <= 26 * 41 * 1441 * 1441
    assert q(_offsets([10] * 25), 25, 1440, 1440, 40) > 0
    assert q(_offsets([10] * 26), 26, 1440, 1440, 40) == 0  # num_clouds x cells >= 2^31
    assert q(_offsets([10] * 33), 33, 8, 8, 8) == 0 and q(_offsets([10]), 0, 8, 8, 8) == 0 and q(_offsets([10]), 1, 0, 8, 8) == 0
    assert q((C.c_int * 3)(0, 10, 5), 2, 8, 8, 8) == 0  # decreasing offsets


# ---- GPU: the kernel chain through the C ABI ------------------------------------------------------------------------------
def _dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda", 0)


SENTINEL = -12345


def _call(clouds, rg, vs, capacity=None, ws_bytes=None, ndim=None, shape=None, with_num=True):
    """(status, voxels, coors, num_points, prefix) as numpy: all `capacity` rows, untouched ones hold SENTINEL."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    sizes = [len(c) for c in clouds]
    nd = ndim if ndim is not None else clouds[0].shape[1]
    pts = torch.from_numpy(np.ascontiguousarray(np.concatenate(clouds), np.float32)).to(dev) if sum(sizes) else torch.zeros(1, nd, device=dev)
    cap = max(sum(sizes), 1) if capacity is None else capacity
    gx, gy, gz = (H.grid_shape(rg, vs) if shape is None else shape)
    off = _offsets(sizes)
    need = lib.shasta_dynvox_workspace_bytes(off, len(clouds), int(gx), int(gy), int(gz))
    wsb = need if ws_bytes is None else ws_bytes
    ws = torch.full((max(need, wsb, 4) // 4 + 1,), 0x5a5a5a5a, dtype=torch.int32, device=dev)  # stale workspace contents must not matter
    voxels = torch.full((max(cap, 1), nd), float(SENTINEL), device=dev)
    coors = torch.full((max(cap, 1), 4), SENTINEL, dtype=torch.int32, device=dev)
    num = torch.full((max(cap, 1),), SENTINEL, dtype=torch.int32, device=dev)
    prefix = torch.full((len(clouds) + 1,), SENTINEL, dtype=torch.int32, device=dev)
    r, v = np.asarray(rg, np.float32), np.asarray(vs, np.float32)
    rc = lib.shasta_dynvox_mean_f32(hip.ptr(pts), off, len(clouds), nd, r.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), int(gx),
                                    int(gy), int(gz), hip.ptr(voxels), hip.ptr(coors), hip.ptr(num) if with_num else None, cap, hip.ptr(prefix),
                                    hip.ptr(ws), wsb, hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, voxels.cpu().numpy(), coors.cpu().numpy(), num.cpu().numpy(), prefix.cpu().numpy()


def _check(clouds, rg, vs):
    """Runs the kernel chain and compares everything with the restatement, bit for bit.  Returns the restatement."""
    clouds = [np.ascontiguousarray(c, np.float32) for c in clouds]
    rc, voxels, coors, num, prefix = _call(clouds, rg, vs)
    assert rc == 0
    rv, rcoors, rn, rprefix = H.voxelize_batch(clouds, rg, vs)
    V = len(rv)
    assert np.array_equal(prefix, rprefix)
    assert np.array_equal(coors[:V], rcoors.astype(np.int32))
    assert np.array_equal(num[:V], rn)
    assert np.array_equal(_bits(voxels[:V]), _bits(rv))
    assert (coors[V:] == SENTINEL).all() and (num[V:] == SENTINEL).all() and (voxels[V:] == SENTINEL).all()  # rows >= V are not written
    return rv, rcoors, rn


def _in_cell(rng, rg, vs, cell, n, ndim=5):
    """n points strictly inside cell (x, y, z) of the grid."""
    lo, v = np.asarray(rg[:3], np.float64), np.asarray(vs, np.float64)
    p = lo + (np.asarray(cell) + 0.1 + 0.8 * rng.rand(n, 3)) * v
    return np.concatenate([p, rng.rand(n, ndim - 3) * 100 - 50], 1).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("rg,vs", [(SMALL_RANGE, SMALL_VOXEL), ([0.0, 0.0, 0.0, 8.0, 6.0, 2.0], [0.25, 0.2, 0.4])])
def test_faces(rg, vs):
    rng = np.random.RandomState(1)
    lo, hi = np.asarray(rg[:3], np.float32), np.asarray(rg[3:], np.float32)
    inside = (lo + (hi - lo) * rng.rand(40, 3)).astype(np.float32)
    pts = []
    for j in range(3):
        for face, out in ((lo[j], -np.inf), (hi[j], np.inf)):
            for val in (face, np.nextafter(face, np.float32(out)), np.nextafter(face, np.float32(-out))):  # on, one step outside, one inside
                p = inside[len(pts) % 40].copy()
                p[j] = val
                pts.append(p)
        for val in (np.nan, np.inf, -np.inf, -0.0, 0.0):
            p = inside[len(pts) % 40].copy()
            p[j] = val
            pts.append(p)
    pts.append(hi.copy())
    pts.append(lo.copy())
    pts = np.concatenate([np.asarray(pts, np.float32), inside])
    pts = np.concatenate([pts, rng.rand(len(pts), 2).astype(np.float32)], 1)
    _, c, n = _check([pts], rg, vs)
    g = H.grid_shape(rg, vs)
    assert (c[:, 3] == g[0]).any() and (c[:, 2] == g[1]).any() and (c[:, 1] == g[2]).any()  # coordinates equal to the extent are emitted
    dropped = len(pts) - int(n.sum())
    assert dropped >= 6 + 9  # one step outside each face; NaN and the infinities on each axis


@pytest.mark.gpu
def test_division_is_a_true_division():
    rng = np.random.RandomState(2)
    vs = np.float32(0.075)
    x = (rng.rand(2000000) * 108).astype(np.float32)
    differ = x[(x / vs).astype(np.int64) != (x * (np.float32(1) / vs)).astype(np.int64)]
    assert len(differ) >= 8
    pts = np.zeros((len(differ), 4), np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2], pts[:, 3] = differ, differ[::-1], 0.3, rng.rand(len(differ))
    _check([pts], [0.0, 0.0, 0.0, 108.0, 108.0, 8.0], [0.075, 0.075, 0.2])


@functools.lru_cache(maxsize=None)
def _crowded():
    rng = np.random.RandomState(3)
    crowd = _in_cell(rng, SMALL_RANGE, SMALL_VOXEL, (11, 7, 2), 30000)
    lo, hi = np.asarray(SMALL_RANGE[:3]), np.asarray(SMALL_RANGE[3:])
    rest = np.concatenate([lo + (hi - lo) * rng.rand(500, 3), rng.rand(500, 2)], 1).astype(np.float32)
    pts = np.concatenate([crowd, rest])[rng.permutation(30500)]
    pts.setflags(write=False)
    return pts


@pytest.mark.gpu
def test_crowded_voxel_is_summed_in_point_order():
    pts = _crowded()
    rv, rc, rn = H.voxelize_batch([pts], SMALL_RANGE, SMALL_VOXEL)[:3]
    row = int(np.argmax(rn))
    assert rn[row] >= 30000 and rc[row].tolist() == [0, 2, 7, 11]
    q = ((pts[:, :3] - np.asarray(SMALL_RANGE[:3], np.float32)) / np.asarray(SMALL_VOXEL, np.float32)).astype(np.int64)
    members = torch.from_numpy(pts[(q == [11, 7, 2]).all(1)])
    tree = (members.sum(0) / np.float32(len(members))).numpy()
    assert not np.array_equal(_bits(tree), _bits(rv[row]))  # a reordered sum shows in the bits: the case can tell the two apart
    _check([pts], SMALL_RANGE, SMALL_VOXEL)


@pytest.mark.gpu
@pytest.mark.parametrize("total", ["many", "few"])
def test_segment_seams(total):
    """List lengths around the wavefront (64), around DV_THREAD_MAX = 32 (thread-per-channel selection | wavefront radix sort) and around
    the 8-point fetch groups of the wavefront's sum; `few`: fewer than 256 points in all, so the radix sort takes a single pass."""
    rng = np.random.RandomState(4)
    counts = [1, 2, 31, THREAD_MAX, THREAD_MAX + 1, 40, 41, 63, 64, 65, 127, 128, 129, 255, 256, 257] if total == "many" else [1, THREAD_MAX, THREAD_MAX + 1, 64, 65]
    parts = [_in_cell(rng, SMALL_RANGE, SMALL_VOXEL, (3 + 2 * (i % 12), 1 + 3 * (i // 12), i % 5), n) for i, n in enumerate(counts)]
    pts = np.concatenate(parts)
    pts = pts[rng.permutation(len(pts))]
    assert (len(pts) < 256) == (total == "few")
    _, _, n = _check([pts], SMALL_RANGE, SMALL_VOXEL)
    assert sorted(n.tolist()) == sorted(counts)


@pytest.mark.gpu
def test_index_seams():
    """Occupied cells on both sides of bitmap-word (32) and scan-block (32 x 1024 cells) boundaries, and of the boundary between two
    clouds' cell spaces: grid 63 x 63 x 15 -> 64 x 64 x 16 = 65 536 cells per cloud."""
    rg, vs = [0.0, 0.0, 0.0, 63.0, 63.0, 15.0], [1.0, 1.0, 1.0]
    lins = [0, 31, 32, 33, 63, 64, 1023, 1024, 32767, 32768, 32769, 65503, 65504, 65535]
    clouds = []
    for b in range(2):
        pts = []
        for lin in lins[b:]:
            x, y, z = lin % 64, (lin // 64) % 64, lin // 4096
            p = [c + 0.5 if c < g else float(g) for c, g in zip((x, y, z), (63, 63, 15))]
            pts += [p + [float(lin), 1.0], p + [2.0, float(b)]]
        clouds.append(np.asarray(pts, np.float32))
    _, c, n = _check(clouds, rg, vs)
    assert len(c) == len(lins) + len(lins) - 1 and (n == 2).all()
    assert c[len(lins) - 1].tolist() == [0, 15, 63, 63] and c[len(lins)].tolist() == [1, 0, 0, 31]


@pytest.mark.gpu
def test_batch_is_the_clouds_concatenated():
    rng = np.random.RandomState(5)
    lo, hi = np.asarray(SMALL_RANGE[:3]), np.asarray(SMALL_RANGE[3:])
    a = np.concatenate([lo + (hi - lo) * rng.rand(333, 3), rng.rand(333, 2)], 1).astype(np.float32)
    a = np.concatenate([a, a[:70] + np.float32(0.01)])  # some shared voxels
    out = a[:77].copy()
    out[:, 0] += 100.0  # wholly out of range
    clouds = [a, np.zeros((0, 5), np.float32), out]
    assert [len(c) % 64 for c in clouds] == [19, 0, 13]
    rv, rc, rn = _check(clouds, SMALL_RANGE, SMALL_VOXEL)
    rc1, v1, c1, n1, p1 = _call([a], SMALL_RANGE, SMALL_VOXEL)
    assert rc1 == 0 and p1.tolist() == [0, len(rv)]
    assert np.array_equal(_bits(v1[:len(rv)]), _bits(rv)) and np.array_equal(c1[:len(rv)], rc.astype(np.int32))
    # the populated cloud last: its rows carry cloud index 2
    rv2, rc2, _ = _check([out, np.zeros((0, 5), np.float32), a], SMALL_RANGE, SMALL_VOXEL)
    assert np.array_equal(_bits(rv2), _bits(rv)) and (rc2[:, 0] == 2).all() and np.array_equal(rc2[:, 1:], rc[:, 1:])


@pytest.mark.gpu
@pytest.mark.parametrize("ndim", [3, 4, 5, 32])
def test_ndim(ndim):
    rng = np.random.RandomState(6 + ndim)
    pts = np.concatenate([_in_cell(rng, SMALL_RANGE, SMALL_VOXEL, (5, 5, 1), 70, ndim), _in_cell(rng, SMALL_RANGE, SMALL_VOXEL, (6, 5, 1), 9, ndim),
                          _in_cell(rng, SMALL_RANGE, SMALL_VOXEL, (31, 29, 4), 3, ndim)])
    _check([pts[rng.permutation(len(pts))]], SMALL_RANGE, SMALL_VOXEL)


@pytest.mark.gpu
def test_shipped_grid_radial_cloud():
    pts = H.radial_cloud(100000, 7)
    _, c, n = _check([pts], H.SHIPPED_RANGE, H.SHIPPED_VOXEL)
    assert len(c) > 50000 and n.max() > 1


@pytest.mark.gpu
@pytest.mark.parametrize("P", [0, 1])
def test_tiny_grid(P):
    rg, vs = [0.0, 0.0, 0.0, 3.0, 2.0, 1.0], [1.0, 1.0, 1.0]
    assert H.grid_shape(rg, vs).tolist() == [3, 2, 1]
    pts = np.asarray([[3.0, 2.0, 1.0, 9.0]], np.float32)[:P]
    rv, rc, _ = _check([pts], rg, vs)
    assert len(rv) == P and (P == 0 or rc[0].tolist() == [0, 1, 2, 3])


@pytest.mark.gpu
def test_two_calls_give_equal_bytes():
    pts = _crowded()
    a, b = _call([pts], SMALL_RANGE, SMALL_VOXEL), _call([pts], SMALL_RANGE, SMALL_VOXEL)
    assert a[0] == 0 and b[0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert x.tobytes() == y.tobytes()


@pytest.mark.gpu
def test_refusals_and_capacity():
    rng = np.random.RandomState(8)
    pts = np.concatenate([_in_cell(rng, SMALL_RANGE, SMALL_VOXEL, (i, i, i % 5), 3) for i in range(20)])

    def untouched(res):
        return all((a == SENTINEL).all() for a in res[1:])

    from shasta_amd import hip
    need = hip.load().shasta_dynvox_workspace_bytes(_offsets([len(pts)]), 1, 32, 30, 5)
    short = _call([pts], SMALL_RANGE, SMALL_VOXEL, ws_bytes=need - 1)
    assert short[0] == E_WORKSPACE and untouched(short)
    narrow = _call([pts[:, :2]], SMALL_RANGE, SMALL_VOXEL, ndim=2)
    assert narrow[0] == E_UNSUPPORTED and untouched(narrow)
    many = _call([pts[:1]] * 26, H.SHIPPED_RANGE, H.SHIPPED_VOXEL)  # 26 x 41 x 1441 x 1441 cells >= 2^31
    assert many[0] == E_UNSUPPORTED and untouched(many)
    # capacity < V is no refusal: the first `capacity` rows are written, the prefix still reports the full V
    rv, rc, rn, rprefix = H.voxelize_batch([pts], SMALL_RANGE, SMALL_VOXEL)
    assert len(rv) == 20
    rc_, v, c, n, prefix = _call([pts], SMALL_RANGE, SMALL_VOXEL, capacity=7)
    assert rc_ == 0 and prefix.tolist() == [0, 20] and len(v) == 7
    assert np.array_equal(_bits(v), _bits(rv[:7])) and np.array_equal(c, rc[:7].astype(np.int32)) and np.array_equal(n, rn[:7])
    # num_points may be NULL
    rc_, v, c, n, prefix = _call([pts], SMALL_RANGE, SMALL_VOXEL, with_num=False)
    assert rc_ == 0 and (n == SENTINEL).all() and np.array_equal(_bits(v[:20]), _bits(rv))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["faces", "crowded", "batch"])
def test_reader_equals_the_reference_golden(name):
    import shasta_amd
    g = _golden()[name]
    dev = _dev()
    reader = shasta_amd.build_from_cfg(dict(type="DynamicVoxelEncoder", pc_range=g["range"].tolist(), voxel_size=g["voxel"].tolist()),
                                       shasta_amd.READERS)
    voxels, coors, shape = reader([torch.from_numpy(c).to(dev) for c in g["clouds"]])
    assert voxels.dtype == torch.float32 and coors.dtype == torch.int32 and voxels.is_cuda and coors.is_cuda
    assert shape.dtype == np.int32 and np.array_equal(shape, g["shape"])
    assert np.array_equal(_bits(voxels.cpu().numpy()), _bits(g["voxels"]))
    assert np.array_equal(coors.cpu().numpy().astype(np.int64), g["coors"])
