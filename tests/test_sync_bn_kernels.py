"""GPU: `shasta_bn_sync_finalize_f32` (csrc/bn_sync.hip) through the C ABI - the merge of per-rank (mean, M2, count) records and the
finalize - against the plain finalize calls (R = 1: the same bits), the float64 restatement of tests/sync_bn_helpers.py on the same
records, and float64 statistics of real data that went through the stats kernels part by part.

Seams: C = 16 (one partial workgroup), 128 (one full workgroup), 256 (two); R = 1 (identity), 2, 3, 8 and 64 (the most served); counts
0 (skipped, also first and last), 1 and 2^31 + 5 (beyond int32 and beyond fp32's integers)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import sync_bn_helpers as SH
from tests.sync_bn_helpers import EPS

pytestmark = pytest.mark.gpu
SENTINEL = -7.0
E_ARG, E_ALIGN, E_UNSUPPORTED = -1, -4, -5  # include/shasta_hip.h
MOM = 0.1
BIG = 2 ** 31 + 5


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a device"
    return torch.device("cuda", 0)


def _i64(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _sync(lib, hip, records, R, C, running=None, nbt=None, merged=True, mom=MOM):
    """One call on a device copy of `records` (uint8 numpy); returns (rc, stat, mean_m2, n_total) with sentinel tails checked."""
    dev = _dev()
    rec = torch.from_numpy(np.ascontiguousarray(records)).to(dev)
    stat = torch.full((2 * C + 4,), SENTINEL, device=dev)
    mm = torch.full((2 * C + 4,), SENTINEL, device=dev) if merged else None
    nt = torch.full((2,), -3, dtype=torch.int64, device=dev)
    rm, rv = running if running is not None else (None, None)
    rc = lib.shasta_bn_sync_finalize_f32(hip.ptr(rec), R, C, EPS, mom, hip.ptr(stat), hip.ptr(mm), _i64(nt), hip.ptr(rm), hip.ptr(rv), _i64(nbt),
                                         hip.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(rec.cpu(), torch.from_numpy(np.ascontiguousarray(records)))  # the call reads the records only
    stat, nt = stat.cpu(), nt.cpu()
    assert bool((stat[2 * C:] == SENTINEL).all()) and int(nt[1]) == -3
    if mm is not None:
        mm = mm.cpu()
        assert bool((mm[2 * C:] == SENTINEL).all())
        mm = mm[:2 * C]
    return rc, stat[:2 * C], mm, int(nt[0])


def _running(C, g, dev):
    """Running statistics with the means kept away from zero, each with a sentinel tail."""
    rm0, rv0 = 0.2 + torch.rand(C, generator=g), 0.5 + torch.rand(C, generator=g)
    tail = torch.full((4,), SENTINEL)
    return rm0, rv0, torch.cat([rm0, tail]).to(dev), torch.cat([rv0, tail]).to(dev)


# ---- 1. R = 1: the bits of the plain finalize ---------------------------------------------------------------------------
@pytest.mark.parametrize("C,kind", [(16, "rows"), (128, "rows"), (256, "maps")])
def test_one_record_gives_the_bits_of_the_plain_finalize(C, kind):
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    assert lib.shasta_bn_sync_record_bytes(C) == 8 * C + 8
    plain = lib.shasta_bn_rows_finalize_f32 if kind == "rows" else lib.shasta_bn_maps_finalize_f32
    g = torch.Generator().manual_seed(C)
    for n in (1, 37, 2 ** 24 + 3):
        mm = torch.cat([torch.randn(C, generator=g), 5.0 + 50.0 * torch.rand(C, generator=g)])
        rm0, rv0, rm_a, rv_a = _running(C, g, dev)
        rm_b, rv_b = rm_a.clone(), rv_a.clone()
        nbt_a, nbt_b = torch.tensor(5, dtype=torch.int64, device=dev), torch.tensor(5, dtype=torch.int64, device=dev)
        mmd = mm.to(dev)
        want = torch.full((2 * C,), SENTINEL, device=dev)
        rc = plain(hip.ptr(mmd), C, float(n), EPS, MOM, hip.ptr(want), hip.ptr(rm_a), hip.ptr(rv_a), _i64(nbt_a), hip.stream_ptr())
        assert rc == 0, lib.shasta_last_error()
        records = SH.pack_records([(mm[:C].numpy(), mm[C:].numpy(), n)], C)
        rc, stat, merged, total = _sync(lib, hip, records, 1, C, (rm_b, rv_b), nbt_b)
        assert rc == 0, lib.shasta_last_error()
        assert torch.equal(stat, want.cpu()) and torch.equal(merged, mm) and total == n
        assert torch.equal(rm_a, rm_b) and torch.equal(rv_a, rv_b) and int(nbt_a) == int(nbt_b) == 6
        assert not torch.equal(rm_b[:C].cpu(), rm0) and bool((rm_b[C:] == SENTINEL).all()) and bool((rv_b[C:] == SENTINEL).all())
        # NULL running pointers and no merged output: stat (and the total) only, the same bits
        before = (rm_b.clone(), rv_b.clone())
        rc, stat2, merged2, _ = _sync(lib, hip, records, 1, C, None, None, merged=False)
        assert rc == 0 and merged2 is None and torch.equal(stat2, stat)
        assert torch.equal(rm_b, before[0]) and torch.equal(rv_b, before[1]) and int(nbt_b) == 6


# ---- 2. synthetic records against the float64 restatement ---------------------------------------------------------------
def _counts(R):
    base = {1: [1000], 2: [1, BIG], 3: [0, 1, BIG], 8: [7, 0, 1, BIG, 300, 0, 64, 12]}
    if R in base:
        return base[R]
    g = np.random.RandomState(R)
    c = g.randint(2, 5000, R).tolist()
    c[0], c[5], c[17], c[40], c[R - 1] = 0, 1, BIG, 0, 0
    return c


def _synthetic(R, C, seed):
    """Records whose rank means differ (offsets of the size of the spread), channel 3 cancelling (|mean| = 1e4 x the spread); an empty
    record holds NaN (it must not be read into the result), a record of one value has M2 = 0."""
    g = np.random.RandomState(seed)
    base = 0.5 + g.rand(C)
    records = []
    for n in _counts(R):
        mean = base + 0.3 * g.randn(C)
        var = 0.5 + g.rand(C)
        mean[3] = 1e3 + 0.01 * g.randn()
        var[3] = 0.01
        if n == 0:
            mean[:], var[:] = np.nan, np.nan
        records.append((mean.astype(np.float32), (var * max(n - 1, 0)).astype(np.float32), n))
    return records


@pytest.mark.parametrize("R", [1, 2, 3, 8, 64])
@pytest.mark.parametrize("C", [16, 128, 256])
def test_synthetic_records_vs_float64(C, R):
    """Bars: merged mean within 2^-23 max_r |mean_r| (the final fp32 rounding plus R float64 steps), merged M2 rtol 2^-23 (all its terms are
    non-negative), inverse std rtol 2^-22 and running statistics rtol 1e-6 (the bars of test_finalize_vs_float64), the total exact."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    records = _synthetic(R, C, 100 * C + R)
    buf = SH.pack_records(records, C)
    read = SH.unpack_records(buf, C)
    mean64, m264, N = SH.merge64(read)
    assert N == sum(_counts(R)) and (R == 1 or N > 2 ** 31) and np.isfinite(mean64).all() and (m264 >= 0).all()
    live = [r for r in read if r[2] > 0]
    if R > 1:
        assert float(np.abs(live[0][0] - live[-1][0])[:3].min()) > 0  # the rank means differ
    g = torch.Generator().manual_seed(C + R)
    rm0, rv0, rm, rv = _running(C, g, dev)
    nbt = torch.tensor(5, dtype=torch.int64, device=dev)
    rc, stat, merged, total = _sync(lib, hip, buf, R, C, (rm, rv), nbt)
    assert rc == 0, lib.shasta_last_error()
    assert total == N and int(nbt) == 6
    got_mean, got_m2 = merged[:C].double().numpy(), merged[C:].double().numpy()
    bar_mean = 2.0 ** -23 * np.max([np.abs(r[0]) for r in live], axis=0)
    e_mean = np.abs(got_mean - mean64)
    print("C %d R %d: N %d, mean err / bar %.3f, M2 rel err %.3e (cancelling channel: mean err %.3e, M2 rel err %.3e)"
          % (C, R, N, float((e_mean / bar_mean).max()), float((np.abs(got_m2 - m264) / m264.clip(1e-300)).max()), float(e_mean[3]),
             float(abs(got_m2[3] - m264[3]) / max(m264[3], 1e-300))))
    assert bool((e_mean <= bar_mean).all())
    np.testing.assert_allclose(got_m2, m264, rtol=2.0 ** -23, atol=0)
    assert torch.equal(stat[:C], merged[:C])
    want_mean, inv, want_rm, want_rv = SH.finalize64(mean64, m264, N, MOM, rm0.numpy(), rv0.numpy())
    np.testing.assert_allclose(stat[C:].double().numpy(), inv, rtol=2.0 ** -22, atol=0)
    assert float(np.abs(want_rm).min()) > 0.05  # the relative bar means something
    np.testing.assert_allclose(rm[:C].cpu().double().numpy(), want_rm, rtol=1e-6, atol=0)
    np.testing.assert_allclose(rv[:C].cpu().double().numpy(), want_rv, rtol=1e-6, atol=0)
    assert bool((rm[C:] == SENTINEL).all()) and bool((rv[C:] == SENTINEL).all())


# ---- 3. real data through the stats kernels, part by part ---------------------------------------------------------------
def _host_fp32_merge(parts):
    """The fp32 host restatement: per-part fp32 mean / M2, merged as sync_bn._SyncBNFn merges them."""
    st = []
    for p in parts:
        v = torch.from_numpy(p)
        v = v if v.dim() == 2 else v.permute(1, 0, 2).reshape(v.shape[1], -1).t()
        mean = v.mean(0)
        st.append((mean, (v - mean).square().sum(0), float(v.shape[0])))
    ns = torch.tensor([s[2] for s in st]).view(-1, 1)
    means, m2s = torch.stack([s[0] for s in st]), torch.stack([s[1] for s in st])
    n = ns.sum()
    mean = (means * ns).sum(0) / n
    m2 = (m2s + ns * (means - mean).square()).sum(0)
    return mean.double().numpy(), m2.double().numpy()


@pytest.mark.parametrize("kind", ["rows", "maps"])
def test_real_data_in_three_ragged_parts_vs_float64(kind):
    """(1000, 64) rows and (2, 32, 10 x 38) maps cut into three ragged parts, each through the existing stats kernel into its record, then
    the merge; against float64 statistics of the whole tensor.  Bar: 4 x the error of the fp32 host restatement (per-part fp32 mean / M2
    merged as sync_bn._SyncBNFn merges them) against the same float64, pooled per quantity over the channels - the project's rule in its
    whole-module tests.  No cancelling channel here: per-part fp32 means enter M2 through n_r d^2, which the analytic bars of the stats
    tests do not cover; test_synthetic_records_vs_float64 covers that channel on equal inputs.

    Measured on an MI355X: see DESIGN.md section 4."""
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    g = torch.Generator().manual_seed(11)
    if kind == "rows":
        C, sizes = 64, [313, 1, 686]
        whole = (torch.randn(1000, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)).numpy()
    else:
        C, sizes = 32, [380, 93, 287]
        whole = (torch.randn(2, C, 380, generator=g) * (0.5 + torch.rand(C, generator=g))[None, :, None]
                 + torch.randn(C, generator=g)[None, :, None]).numpy()
    parts = SH.ragged_split(whole, sizes)
    R = len(parts)
    rb = lib.shasta_bn_sync_record_bytes(C)
    gathered = torch.zeros(R * rb, dtype=torch.uint8, device=dev)
    for r, p in enumerate(parts):
        rec = gathered[r * rb:(r + 1) * rb]
        pd = torch.from_numpy(p).to(dev)
        if kind == "rows":
            ws = torch.empty(lib.shasta_bn_rows_workspace_bytes(C), dtype=torch.uint8, device=dev)
            rc = lib.shasta_bn_rows_stats_f32(hip.ptr(pd), p.shape[0], C, hip.ptr(rec[:8 * C].view(torch.float32)), hip.ptr(ws), ws.numel(),
                                              hip.stream_ptr())
        else:
            ws = torch.empty(lib.shasta_bn_maps_workspace_bytes(1, C, p.shape[2]), dtype=torch.uint8, device=dev)
            rc = lib.shasta_bn_maps_stats_f32(hip.ptr(pd), 1, C, p.shape[2], C, 0, hip.ptr(rec[:8 * C].view(torch.float32)), hip.ptr(ws),
                                              ws.numel(), hip.stream_ptr())
        assert rc == 0, lib.shasta_last_error()
        rec[8 * C:].view(torch.int64).fill_(sizes[r])  # the count, with no host read
    rc, stat, merged, total = _sync(lib, hip, gathered.cpu().numpy(), R, C)
    assert rc == 0, lib.shasta_last_error()
    mean64, m264, n = SH.part_stats64(whole)
    assert total == n == sum(sizes)
    ref_mean, ref_m2 = _host_fp32_merge(parts)
    for name, got, want, ref in (("mean", merged[:C].double().numpy(), mean64, ref_mean), ("M2", merged[C:].double().numpy(), m264, ref_m2)):
        err, ref_err = float(np.abs(got - want).max()), float(np.abs(ref - want).max())
        print("%s %s: kernel max|got - f64| = %.3e, fp32 host restatement %.3e, ratio %.2f" % (kind, name, err, ref_err, err / ref_err))
        assert ref_err > 0 and err <= 4 * ref_err, (name, err, ref_err)
    assert torch.equal(stat[:C], merged[:C])  # (the inverse std from the merged M2: test_synthetic_records_vs_float64's bar)


# ---- 4. refusals and the invalid-count rule -----------------------------------------------------------------------------
def test_refusals_come_before_any_launch_and_invalid_counts_give_nan():
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    C, R = 32, 3
    assert [lib.shasta_bn_sync_record_bytes(c) for c in (0, 8, 16, 24, 1024, 1040, 2048)] == [0, 0, 136, 0, 8200, 0, 0]
    records = torch.from_numpy(SH.pack_records(_synthetic(R, C, 5), C)).to(dev)
    wide = torch.zeros(65 * (8 * 2048 + 8), dtype=torch.uint8, device=dev)  # (large enough for every refused shape, should one launch)
    stat = torch.full((2 * 2048,), SENTINEL, device=dev)
    mm = torch.full((2 * 2048,), SENTINEL, device=dev)
    g = torch.Generator().manual_seed(1)
    rm = torch.rand(2048, generator=g).to(dev)
    rv = torch.rand(2048, generator=g).to(dev)
    rm0, rv0 = rm.clone(), rv.clone()
    nbt = torch.tensor(5, dtype=torch.int64, device=dev)
    nt = torch.tensor(-3, dtype=torch.int64, device=dev)
    s = hip.stream_ptr()

    def call(rec=wide, r=R, c=C, st=stat):
        return lib.shasta_bn_sync_finalize_f32(None if rec is None else hip.ptr(rec), r, c, EPS, MOM, None if st is None else hip.ptr(st), hip.ptr(mm),
                                               _i64(nt), hip.ptr(rm), hip.ptr(rv), _i64(nbt), s)

    assert call(c=24) == E_UNSUPPORTED and call(c=2048) == E_UNSUPPORTED and call(c=0) == E_UNSUPPORTED and call(c=8) == E_UNSUPPORTED
    assert call(r=0) == E_UNSUPPORTED and call(r=65) == E_UNSUPPORTED and call(r=-1) == E_UNSUPPORTED
    assert call(rec=None) == E_ARG and call(st=None) == E_ARG
    assert call(rec=wide[4:]) == E_ALIGN
    torch.cuda.synchronize()
    assert bool((stat == SENTINEL).all()) and bool((mm == SENTINEL).all()) and torch.equal(rm, rm0) and torch.equal(rv, rv0)
    assert int(nbt) == 5 and int(nt) == -3
    # invalid counts: all zero, and one negative - NaN stat, nothing else moves
    for counts in ([0, 0, 0], [5, -1, 7]):
        bad = SH.pack_records([(r[0], r[1], n) for r, n in zip(_synthetic(R, C, 5), counts)], C)
        nbt_b = torch.tensor(5, dtype=torch.int64, device=dev)
        rm_b, rv_b = rm0[:C + 4].clone(), rv0[:C + 4].clone()
        rc, st, _, total = _sync(lib, hip, bad, R, C, (rm_b, rv_b), nbt_b)
        assert rc == 0 and bool(torch.isnan(st).all()) and total == 0
        assert torch.equal(rm_b, rm0[:C + 4]) and torch.equal(rv_b, rv0[:C + 4]) and int(nbt_b) == 5
    assert call(rec=records) == 0  # and the good call serves
    torch.cuda.synchronize()
    assert bool(torch.isfinite(stat[:2 * C]).all()) and bool((stat[2 * C:] == SENTINEL).all()) and int(nbt) == 6 and int(nt) > 0


# ---- 5. determinism -----------------------------------------------------------------------------------------------------
def test_same_bits_on_two_runs_and_from_two_buffers():
    from shasta_amd import hip
    lib, dev = hip.load(), _dev()
    C, R = 256, 8
    buf = SH.pack_records(_synthetic(R, C, 9), C)
    g = torch.Generator().manual_seed(2)
    rm0, rv0, _, _ = _running(C, g, dev)
    outs = []
    for _ in range(2):  # (_sync copies the records into a fresh device buffer every time)
        rm, rv = rm0.to(dev), rv0.to(dev)
        rc, stat, merged, total = _sync(lib, hip, buf, R, C, (rm, rv), None)
        assert rc == 0
        outs.append((stat, merged, total, rm.cpu(), rv.cpu()))
    # and twice on ONE device buffer
    rec = torch.from_numpy(buf).to(dev)
    for _ in range(2):
        stat = torch.empty(2 * C, device=dev)
        rm, rv = rm0.to(dev), rv0.to(dev)
        assert lib.shasta_bn_sync_finalize_f32(hip.ptr(rec), R, C, EPS, MOM, hip.ptr(stat), None, None, hip.ptr(rm), hip.ptr(rv), None,
                                               hip.stream_ptr()) == 0
        outs.append((stat.cpu(), outs[0][1], outs[0][2], rm.cpu(), rv.cpu()))
    for o in outs[1:]:
        assert all(torch.equal(a, b) if torch.is_tensor(a) else a == b for a, b in zip(o, outs[0]))
    assert not torch.equal(outs[0][3], rm0)
