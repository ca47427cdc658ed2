"""tests/rows_ref.py (the numpy reference of the engineered-row GPU tests) pinned to the oracle on small
random cases, and its packed-format helpers to the rules of include/hga.h.  No GPU."""
import numpy as np
import pytest

import oracle
import rows_ref

THR = [33.333333333333336, 50.0, 60.0, 66.66666666666667, 75.0, 80.0, 100.0, 100.01]


def random_rows(seed, F, n=400, k=9):
    rng = np.random.default_rng(seed)
    keys = rng.choice(1 << (2 * k), n, replace=False).astype(np.uint64)
    counts = rng.integers(0, 51, (n, F)).astype(np.uint32)
    counts[rng.random((n, F)) < 0.4] = 0
    empty = ~counts.any(axis=1)
    counts[empty, rng.integers(0, F, int(empty.sum()))] = 1
    return keys, counts


@pytest.mark.parametrize("F", [1, 2, 3, 5])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_queries_equal_oracle(F, seed):
    keys, counts = random_rows(seed * 10 + F, F)
    dumps = [rows_ref.dump(keys, counts, f) for f in range(F)]
    ok, oc = oracle.merge(dumps)
    rk, rc = rows_ref.merge(rows_ref.from_dumps(dumps), 1, saturate=False)
    assert np.array_equal(rk, ok) and np.array_equal(rc, oc)
    sk, sc = rows_ref.merge([(keys, counts)], 1)
    assert np.array_equal(sk, ok) and np.array_equal(sc, oc) and sc.dtype == np.uint32
    for thr in (oracle.THRESHOLDS, THR, [100.01]):
        assert np.array_equal(rows_ref.spec_hist(oc, thr), oracle.specificity(oc, thr))
    tot = oc.sum(axis=1)
    for lower, upper in ((5, 60), (int(tot[0]), int(tot[0])), (-5, 2 ** 63 - 1), (9, 3), (1, 1)):
        want, nd = oracle.select(ok, oc, lower, upper)
        got, flags, gd = rows_ref.select(keys, counts, lower, upper)
        assert np.array_equal(got, want) and gd == nd == int(flags.sum())


def test_merge_drop_and_saturation():
    a = (np.array([7, 3, 9], np.uint64), np.array([[1, 0], [2, 2], [1 << 31, 1]], np.uint32))
    b = (np.array([9, 3, 8], np.uint64), np.array([[1 << 31, 1], [0, 1], [1, 1]], np.uint32))
    c = (np.array([9], np.uint64), np.array([[1 << 31, 0]], np.uint32))
    k, v = rows_ref.merge([a, b, c], 2)
    assert k.tolist() == [3, 9] and v.tolist() == [[2, 3], [rows_ref.U32_MAX, 2]]
    k, v = rows_ref.merge([a, b, c], 1, saturate=False)
    assert k.tolist() == [3, 7, 8, 9] and v[3].tolist() == [3 << 31, 2]


def test_spec_hist_raises_above_last_threshold():
    with pytest.raises(ValueError):
        rows_ref.spec_hist(np.array([[3, 0], [1, 1]], np.uint32), [50.0, 90.0])
    assert rows_ref.spec_hist(np.array([[3, 0], [1, 1]], np.uint32), [50.0, 100.01]).tolist() == [[1, 2, 1], [1, 3, 1]]


def test_pack_bits_table():
    for (k, F), bits in {(16, 1): 32, (5, 1): 32, (19, 3): 8, (13, 8): 4, (19, 7): 0, (31, 1): 0, (29, 2): 0,
                         (11, 9): 0}.items():
        assert rows_ref.pack_bits(k, F) == bits, (k, F)
    for k in range(1, 33):      # the rule of hga.h in full: (64 - 2k) / n_files, 0 below 4 or past 8 files
        for F in range(1, 12):
            cb = (64 - 2 * k) // F
            assert rows_ref.pack_bits(k, F) == (0 if cb < 4 or F > 8 else min(cb, 32))


def test_pieces_split_greedily():
    k, F = 13, 8   # 4 bits per count
    keys = np.array([5, 6, 7], np.uint64)
    counts = np.zeros((3, F), np.uint32)
    counts[0, 0], counts[1, 1], counts[1, 7], counts[2, 3] = 15, 16, 31, 1000
    assert rows_ref.pieces_per_row(counts, k, F).tolist() == [1, 3, 67]
    p = rows_ref.pieces(keys, counts, k, F)
    assert len(p) == 71
    pk, pc = rows_ref.unpack(p, k, F)
    assert pk.tolist() == [5] + [6] * 3 + [7] * 67
    assert pc[1:4, 1].tolist() == [15, 1, 0] and pc[1:4, 7].tolist() == [15, 15, 1]
    assert pc[4:, 3].tolist() == [15] * 66 + [10]
    mk, mc = rows_ref.merge([(pk, pc)], 1)
    assert np.array_equal(mk, keys) and np.array_equal(mc, counts)
    # one file, k <= 16: a piece holds a whole u32, nothing splits
    big = np.array([[rows_ref.U32_MAX]], np.uint32)
    assert rows_ref.pieces(np.array([9], np.uint64), big, 16, 1).tolist() == [9 | (rows_ref.U32_MAX << 32)]
