"""The batched Hungarian solver of csrc/lsap.hip (association.linear_assignment_device) against scipy.optimize.linear_sum_assignment:
the same row and column indices for every problem - no mask, no tolerance.  The tracker's matrices carry 1e18 for invalid pairs
(a float64 ulp is 128 there), so equal total cost would not pin anything: the optimum returned depends on the order of the additions
and on the tie rule, and the device has to reproduce both."""
import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

SHAPES = [(1, 1), (1, 5), (5, 1), (7, 12), (63, 64), (64, 65), (65, 64), (90, 130), (130, 90)]  # both sides of a wavefront, both orientations
FAMILIES = ["tracker", "tracker_quantised", "integers", "uniform"]


def _tracker_cost(rng, n, m, quantise):
    """pub_tracker.py:94-104 on synthetic centres: detections uniform in a 30 m square, the first min(n, m) tracks are detections plus
    N(0, 0.7 m) noise, permuted, the rest uniform; 3 classes, gate 2 m, float32 distances, + 1e18 for invalid pairs, clipped."""
    dets = rng.uniform(0, 30, (n, 2))
    k = min(n, m)
    trk = np.concatenate([dets[:k] + rng.normal(0, 0.7, (k, 2)), rng.uniform(0, 30, (m - k, 2))])
    perm = rng.permutation(m)
    trk = trk[perm]
    dc = rng.integers(0, 3, n)
    tc = np.concatenate([dc[:k], rng.integers(0, 3, m - k)])[perm]
    if quantise:
        dets, trk = np.round(dets * 2) / 2, np.round(trk * 2) / 2
    dets, trk = dets.astype(np.float32), trk.astype(np.float32)
    dist = np.sqrt(((trk.reshape(1, -1, 2) - dets.reshape(-1, 1, 2)) ** 2).sum(axis=2))
    invalid = ((dist > np.float32(2.0)) + (dc.reshape(n, 1) != tc.reshape(1, m))) > 0
    dist = dist + invalid * 1e18
    assert dist.dtype == np.float64
    dist[dist > 1e18] = 1e18
    return dist


def _cost(family, rng, n, m):
    if family == "tracker":
        return _tracker_cost(rng, n, m, False)
    if family == "tracker_quantised":
        return _tracker_cost(rng, n, m, True)
    if family == "integers":
        return rng.integers(0, 4, (n, m)).astype(np.float64)
    return rng.uniform(0, 1, (n, m))


def _padded(mats):
    Nmax, Mmax = max(c.shape[0] for c in mats), max(c.shape[1] for c in mats)
    batch = np.full((len(mats), Nmax, Mmax), np.nan)  # NaN in the padding: a solver that read it would report status 1
    for p, c in enumerate(mats):
        batch[p, :c.shape[0], :c.shape[1]] = c
    return batch, [c.shape[0] for c in mats], [c.shape[1] for c in mats]


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_batch_equals_scipy_index_for_index(family):
    from shasta_amd.association import linear_assignment_device
    valid = 0
    for seed in range(4):
        rng = np.random.default_rng(100 * FAMILIES.index(family) + seed)
        mats = [_cost(family, rng, n, m) for n, m in SHAPES]
        batch, n, m = _padded(mats)
        got = linear_assignment_device(batch, n, m)  # all shapes of the family: one launch
        assert len(got) == len(mats)
        for c, (r, q) in zip(mats, got):
            wr, wq = linear_sum_assignment(c)
            assert np.array_equal(r, wr) and np.array_equal(q, wq), (family, seed, c.shape)
            valid += int((c[wr, wq] < 1e16).sum())
    assert valid > 100  # (tracker families: neither all pairs valid nor none)


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_the_tracker_capacity_512_by_768(family):
    import torch
    from shasta_amd.association import linear_assignment_device
    c = _cost(family, np.random.default_rng(7 + FAMILIES.index(family)), 512, 768)
    wr, wq = linear_sum_assignment(c)
    r, q = linear_assignment_device(torch.from_numpy(c).cuda())  # a device tensor, single matrix
    assert np.array_equal(r, wr) and np.array_equal(q, wq)


@pytest.mark.gpu
def test_status_words_and_empty_problems():
    import torch
    from shasta_amd import hip
    from shasta_amd.association import linear_assignment_device
    lib = hip.load()
    rng = np.random.default_rng(5)
    good = rng.uniform(0, 1, (6, 9))
    nan = good.copy()
    nan[3, 4] = np.nan
    neg = good.copy()
    neg[0, 0] = -np.inf
    blocked = good.copy()
    blocked[2, :] = np.inf  # a row of forbidden pairs: infeasible
    one_inf = good.copy()
    one_inf[2, 5] = np.inf  # a single forbidden pair is fine
    batch, n, m = _padded([good, nan, blocked, neg, one_inf, good])
    n[5] = 0  # an empty problem
    dev = torch.device("cuda")
    cost = torch.from_numpy(batch).to(dev)
    col = torch.full((6, 6), 7, dtype=torch.int32, device=dev)
    status = torch.full((6,), 7, dtype=torch.int32, device=dev)
    nn, mm = torch.tensor(n, dtype=torch.int32, device=dev), torch.tensor(m, dtype=torch.int32, device=dev)
    hip.check(lib.shasta_lsap_f64(hip.ptr(cost), hip.ptr(nn), hip.ptr(mm), 6, 6, 9, hip.ptr(col), hip.ptr(status), hip.stream_ptr()), "lsap")
    assert status.cpu().tolist() == [0, 1, 2, 1, 0, 0]  # per problem: the neighbours of a refused one are solved
    col = col.cpu().numpy()
    for p, c in ((0, good), (4, one_inf)):
        wr, wq = linear_sum_assignment(c)
        assert np.array_equal(col[p], wq)
    assert (col[[1, 2, 3, 5]] == -1).all()
    # the Python surface raises where scipy raises, and returns scipy's empty result
    for bad in (nan, neg, blocked):
        with pytest.raises(ValueError):
            linear_sum_assignment(bad)
        with pytest.raises(ValueError):
            linear_assignment_device(bad)
    for shape in ((0, 4), (4, 0)):
        r, q = linear_assignment_device(np.zeros(shape))
        assert r.shape == q.shape == (0,) and r.dtype == q.dtype == np.int64
    res = linear_assignment_device(batch[[0, 5]], [6, 0], [9, 9])
    assert len(res[1][0]) == 0 and np.array_equal(res[0][1], linear_sum_assignment(good)[1])
    # beyond the capacity: an error with a message, not a wrong answer
    with pytest.raises(hip.ShastaHipError, match="1024"):
        linear_assignment_device(np.zeros((2, 1025)))


@pytest.mark.gpu
def test_the_trackers_form_clips_while_reading_and_flags_pairs_beyond_the_gate():
    """shasta_lsap_clip_f64 on the unclipped `dist + invalid * 1e18` of pub_tracker.py:102: the pairs scipy returns for the clipped
    matrix (:104-105), the "cost > 1e16" bit of every pair (:122), and the matrix itself untouched."""
    import torch
    from shasta_amd import hip
    lib = hip.load()
    rng = np.random.default_rng(9)
    mats = []
    for n, m in SHAPES:
        c = _tracker_cost(rng, n, m, False)
        c[rng.uniform(size=n) < 0.3] = 1e18  # detections without any track inside their gate: paired all the same
        c[c >= 1e18] += rng.uniform(0, 5e4, c.shape)[c >= 1e18]  # as before the clip: 1e18 + a distance of up to some 10 km
        mats.append(c)
    assert sum(int((c > 1e18).sum()) for c in mats) > 1000
    batch, n, m = _padded(mats)
    dev = torch.device("cuda")
    cost = torch.from_numpy(batch).to(dev)
    P, Nmax, Mmax = batch.shape
    col = torch.full((P, Nmax), 7, dtype=torch.int32, device=dev)
    over = torch.full((P, Nmax), 7, dtype=torch.int32, device=dev)
    status = torch.full((P,), 7, dtype=torch.int32, device=dev)
    nn, mm = torch.tensor(n, dtype=torch.int32, device=dev), torch.tensor(m, dtype=torch.int32, device=dev)
    hip.check(lib.shasta_lsap_clip_f64(hip.ptr(cost), hip.ptr(nn), hip.ptr(mm), P, Nmax, Mmax, 1e18, 1e16, hip.ptr(col), hip.ptr(over),
                                       hip.ptr(status), hip.stream_ptr()), "lsap_clip")
    assert status.cpu().tolist() == [0] * P
    assert np.array_equal(cost.cpu().numpy(), batch, equal_nan=True)
    col, over = col.cpu().numpy(), over.cpu().numpy()
    flagged = 0
    for p, c in enumerate(mats):
        clipped = np.minimum(c, 1e18)
        wr, wq = linear_sum_assignment(clipped)
        want_col = np.full(Nmax, -1)
        want_col[wr] = wq
        want_over = np.zeros(Nmax, int)
        want_over[wr] = clipped[wr, wq] > 1e16
        assert np.array_equal(col[p], want_col) and np.array_equal(over[p], want_over), c.shape
        flagged += int(want_over.sum())
    assert flagged > 20
