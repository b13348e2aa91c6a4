"""CPU: the host side of the sparse backbone's train() mode (csrc/bn_rows.hip, shasta_amd/backbone.py `batch_statistics`): symbols,
size queries, refusals that come before any launch, the opt-in switch, and the batch-statistics dense restatement of
tests/backbone_train_helpers.py in float32 against float64."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import backbone_helpers as BH
from tests import backbone_train_helpers as BT
from tests.backbone_helpers import E_ARG, E_UNSUPPORTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("shasta_spconv_layer_pack_raw_f32", "shasta_bn_rows_supported", "shasta_bn_rows_workspace_bytes", "shasta_bn_rows_stats_f32",
       "shasta_bn_rows_finalize_f32", "shasta_bn_rows_apply_f32")


def _backbone(**kw):
    from shasta_amd.backbone import SpMiddleResNetFHD
    return SpMiddleResNetFHD(num_input_features=5, ds_factor=8, **kw)


def test_header_exports_and_binding_agree_on_the_new_symbols():
    from shasta_amd import hip
    lib = hip.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "shasta_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(shasta_[a-z0-9_]+)\s*\(", header))
    out = subprocess.run(["nm", "-D", "--defined-only", hip.lib_path()], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NEW:
        assert name in declared and name in exported and name in hip.SYMBOLS and hasattr(lib, name), name
        decl = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(hip.SYMBOLS[name][1]) == len(decl.split(",")), name  # one ctypes argument per declared parameter
    from shasta_amd import build
    assert "bn_rows.hip" in build.SOURCES


def test_size_queries_and_supported_do_not_need_a_gpu():
    from shasta_amd import hip
    lib = hip.load()
    for c in range(0, 260):
        assert lib.shasta_bn_rows_supported(c) == (1 if c in (16, 32, 64, 128) else 0)
        assert (lib.shasta_bn_rows_workspace_bytes(c) > 0) == (c in (16, 32, 64, 128))
    assert lib.shasta_bn_rows_supported(-16) == 0
    # float64 sum and sum of squares per channel and slice
    assert lib.shasta_bn_rows_workspace_bytes(128) == 8 * lib.shasta_bn_rows_workspace_bytes(16)
    assert lib.shasta_bn_rows_workspace_bytes(16) % (2 * 16 * 8) == 0
    # the raw pack is the eval pack's layout: its byte count is the one size query of both


def test_refusals_come_before_any_launch():
    """No GPU here: a call that reached a launch (or read one of these pointers on the host) would fail differently.  The buffers are
    host memory that no refused call may touch."""
    from shasta_amd import hip
    lib = hip.load()
    buf = (C.c_float * 1024)(*([-7.0] * 1024))
    p = C.cast(buf, C.c_void_p)
    ws = lib.shasta_bn_rows_workspace_bytes(128)
    for c in (0, 8, 24, 48, 96, 256):
        assert lib.shasta_bn_rows_stats_f32(p, 10, c, p, p, ws, None) == E_UNSUPPORTED
        assert b"16, 32, 64 or 128" in lib.shasta_last_error()
        assert lib.shasta_bn_rows_finalize_f32(p, c, 10.0, 1e-3, 0.01, p, p, p, None, None) == E_UNSUPPORTED
        assert lib.shasta_bn_rows_apply_f32(p, 10, c, p, p, p, None, 1, p, None) == E_UNSUPPORTED
    for c in (16, 32, 64, 128):
        assert lib.shasta_bn_rows_stats_f32(p, 0, c, p, p, ws, None) == E_ARG           # n = 0
        assert lib.shasta_bn_rows_stats_f32(p, -3, c, p, p, ws, None) == E_ARG
        assert lib.shasta_bn_rows_stats_f32(None, 10, c, p, p, ws, None) == E_ARG
        assert lib.shasta_bn_rows_stats_f32(p, 10, c, p, p, lib.shasta_bn_rows_workspace_bytes(c) - 1, None) == BH.E_WORKSPACE
        assert lib.shasta_bn_rows_finalize_f32(p, c, 0.0, 1e-3, 0.01, p, None, None, None, None) == E_ARG
        assert lib.shasta_bn_rows_apply_f32(p, 0, c, p, p, p, None, 1, p, None) == E_ARG
        assert lib.shasta_bn_rows_apply_f32(p, 10, c, p, p, p, None, 1, None, None) == E_ARG
    # raw pack: same served set and the same byte count as the eval pack
    for cin, cout, K in ((5, 16, 27), (16, 32, 27), (128, 128, 3)):
        need = lib.shasta_spconv_layer_packed_bytes(cin, cout, K)
        assert need > 0
        assert lib.shasta_spconv_layer_pack_raw_f32(p, None, cin, cout, K, p, need - 1, None) == BH.E_WORKSPACE
        assert lib.shasta_spconv_layer_pack_raw_f32(None, None, cin, cout, K, p, need, None) == E_ARG
    assert lib.shasta_spconv_layer_pack_raw_f32(p, None, 24, 32, 27, p, 1 << 20, None) == E_UNSUPPORTED
    assert lib.shasta_spconv_layer_pack_raw_f32(p, None, 16, 48, 27, p, 1 << 20, None) == E_UNSUPPORTED
    assert lib.shasta_spconv_layer_pack_raw_f32(p, None, 16, 32, 25, p, 1 << 20, None) == E_UNSUPPORTED
    assert all(v == -7.0 for v in buf)


def test_the_switch_is_opt_in():
    from shasta_amd import hip
    x, c = torch.zeros(3, 5), torch.zeros(3, 4, dtype=torch.int32)
    m = _backbone()
    assert m.batch_statistics is False and m.training
    with pytest.raises(hip.ShastaHipError, match="train") as e:
        m(x, c, 1, [8, 8, 4])
    assert "batch_statistics" in str(e.value)  # the refusal names the switch
    for on in (_backbone(batch_statistics=True), _backbone()):
        on.batch_statistics = True  # a plain attribute: also settable after construction
        with torch.no_grad(), pytest.raises(hip.ShastaHipError, match="device"):
            on(x, c, 1, [8, 8, 4])
    assert "batch_statistics" not in m.state_dict() and list(_backbone(batch_statistics=True).state_dict()) == list(m.state_dict())
    cum = _backbone(batch_statistics=True, norm_cfg=dict(type="BN1d", eps=1e-3, momentum=None))
    assert cum.conv_input[1].momentum is None  # builds; the forward refuses it (GPU test)


def test_train_restatement_float32_agrees_with_float64():
    """The helper itself: float32 against float64 on a small case, per layer statistics included; and with every BatchNorm in eval() it
    is backbone_helpers.reference_forward exactly."""
    shape, B = [14, 10, 40], 2
    grid = (41, 10, 14)
    m = _backbone().train()
    BT.randomize_train(m, torch.Generator().manual_seed(21))
    coords = BH.clustered_voxels(np.random.RandomState(21), B, grid, blobs=2, per_blob=60)
    feats = torch.randn(len(coords), 5, generator=torch.Generator().manual_seed(22))
    r64, l64, s64 = BT.reference_forward_train(m, feats, coords, B, shape, torch.float64)
    r32, l32, s32 = BT.reference_forward_train(m, feats, coords, B, shape, torch.float32)
    assert len(s64) == len(m._pairs()) == 21 and all(s is not None for s in s64)  # 1 + 4 + 3 x 5 + 1 BatchNorm1d modules
    assert sum(isinstance(mod, torch.nn.BatchNorm1d) for mod in m.modules()) == 21
    assert r32.dtype == torch.float32 and r64.shape == (B, 128 * 2, 2, 2)
    scale = float(r64.abs().max())
    err = float((r32.double() - r64).abs().max())
    print("range %.3g, max |f32 - f64| %.3e" % (scale, err))
    assert 0.1 <= scale <= 100 and 0 < err <= 1e-4 * scale
    for k in l64:
        assert torch.equal(l64[k][1], l32[k][1].double())
        assert float((l64[k][0] * (1 - l64[k][1])).abs().max()) == 0.0
    for (mean64, m264, n64), (mean32, m232, n32), (conv, bn) in zip(s64, s32, m._pairs()):
        assert n64 == n32 >= 2 and mean64.shape == (conv.out_channels,)
        np.testing.assert_allclose(mean32.double().numpy(), mean64.numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(m232.double().numpy(), m264.numpy(), rtol=1e-4)
    # the statistics are the batch's: a normalised layer has mean beta and variance gamma^2 var / (var + eps) over its active sites
    x, mask = BH.to_dense(feats.double(), coords, B, grid)
    y, _ = BH.dense_conv(x, mask, m.conv_input[0].weight.detach(), None, BH.SUBM, True)
    bn = m.conv_input[1]
    out, (mean, m2, n) = BT.dense_bn_train(y, mask, bn.weight.detach(), bn.bias.detach(), bn.eps)
    rows = BH.rows_of(out, coords)
    assert n == len(coords)
    np.testing.assert_allclose(rows.mean(0).numpy(), bn.bias.detach().double().numpy(), atol=1e-12)
    var = m2 / n
    np.testing.assert_allclose(rows.var(0, unbiased=False).numpy(), (bn.weight.detach().double() ** 2 * var / (var + bn.eps)).numpy(), rtol=1e-10)
    np.testing.assert_allclose(BH.rows_of(y, coords).mean(0).numpy(), mean.numpy(), atol=1e-12)
    # expected running statistics: torch's own BatchNorm1d on the rows of the first layer
    tbn = torch.nn.BatchNorm1d(16, eps=bn.eps, momentum=bn.momentum).double().train()
    tbn.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in bn.state_dict().items()})
    want_rows = tbn(BH.rows_of(y, coords))
    np.testing.assert_allclose(rows.numpy(), want_rows.detach().numpy(), rtol=1e-10, atol=1e-12)
    rm, rv = BT.expected_running(m, s64)[0]
    np.testing.assert_allclose(rm.numpy(), tbn.running_mean.numpy(), rtol=1e-12)
    np.testing.assert_allclose(rv.numpy(), tbn.running_var.numpy(), rtol=1e-12)
    # per-layer rule: every BatchNorm in eval() -> the eval restatement, bit for bit, and no statistics
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm1d):
            mod.eval()
    re64, _, se = BT.reference_forward_train(m, feats, coords, B, shape, torch.float64)
    assert all(s is None for s in se) and torch.equal(re64, BH.reference_forward(m, feats, coords, B, shape, torch.float64)[0])
    assert float((re64 - r64).abs().max()) > 1e-3
