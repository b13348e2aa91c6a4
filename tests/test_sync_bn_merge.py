"""CPU: the truth the synchronised-statistics tests compare against, validated by itself - the float64 restatement of the sequential
merge of csrc/bn_sync.hip (tests/sync_bn_helpers.py) over ragged per-rank parts equals the float64 statistics of the whole batch."""
import numpy as np
import pytest

from tests import sync_bn_helpers as SH

# per R: part sizes with parts of 0, 1 and many rows
SIZES = {1: [211], 2: [1, 210], 3: [0, 1, 210], 8: [40, 0, 1, 97, 0, 3, 69, 1]}


def _rows(n, C, seed):
    g = np.random.RandomState(seed)
    y = g.randn(n, C) * (0.5 + g.rand(C)) + g.randn(C)
    y[:, 3] = 1e3 + 0.1 * g.randn(n)  # |mean| = 1e4 x std
    return y


@pytest.mark.parametrize("R", sorted(SIZES))
@pytest.mark.parametrize("kind", ["rows", "maps"])
def test_merge_over_ragged_parts_equals_the_whole_batch(R, kind):
    sizes, C = SIZES[R], 8
    n = sum(sizes)
    y = _rows(n, C, 10 * R + len(kind))
    assert abs(abs(y[:, 3].mean()) / y[:, 3].std() / 1e4 - 1) < 0.3
    whole = y if kind == "rows" else np.ascontiguousarray(y.T.reshape(C, 1, n).transpose(1, 0, 2))  # (1, C, n) maps of the same values
    parts = SH.ragged_split(whole, sizes)
    assert [p.shape[0] if kind == "rows" else p.shape[2] for p in parts] == sizes
    mean, m2, N = SH.merge64([SH.part_stats64(p) for p in parts])
    want_mean, want_m2, want_n = SH.part_stats64(whole)
    assert N == want_n == n
    np.testing.assert_allclose(mean, want_mean, rtol=1e-12, atol=0)
    np.testing.assert_allclose(m2, want_m2, rtol=1e-12, atol=0)


def test_one_record_is_the_identity_bit_for_bit():
    g = np.random.RandomState(3)
    mean, m2 = g.randn(16), 5.0 + g.rand(16)
    for records in ([(mean, m2, 37)], [(g.randn(16), g.rand(16), 0), (mean, m2, 37), (np.full(16, np.nan), np.full(16, np.nan), 0)]):
        got_mean, got_m2, N = SH.merge64(records)
        assert N == 37 and np.array_equal(got_mean.view(np.int64), mean.view(np.int64)) and np.array_equal(got_m2.view(np.int64), m2.view(np.int64))


def test_records_round_trip_through_their_bytes():
    g = np.random.RandomState(4)
    C = 16
    records = [(g.randn(C).astype(np.float32), g.rand(C).astype(np.float32), n) for n in (0, 1, 2 ** 31 + 5)]
    buf = SH.pack_records(records, C)
    assert buf.dtype == np.uint8 and buf.size == 3 * (8 * C + 8)
    for (a, b, n), (a2, b2, n2) in zip(records, SH.unpack_records(buf, C)):
        assert np.array_equal(a, a2) and np.array_equal(b, b2) and n == n2
