"""The row queries of the count step (rows, dump, spec_hist, select; csrc/count.hip) on rows the test
engineers itself with hga_count_add_rows, bit-exact against tests/rows_ref.py.

Rows counted from reads only ever reach two or three files and totals of a few thousand.  Here every
count of every row is chosen: 1 to 64 files, row counts around the four-row groups of kc_spec_hist and
the 4096-row chunks of kc_select, totals on both sides of the histogram's tiers (1024: LDS / dense
global, 65536: dense / overflow list), more than 1024 bins (the read-back past SPEC_CHUNK), an error
followed by a clean call, and select bounds at and around existing totals.  Row totals stay below 2^31
(the reference program's totals are int).  Every tier a test names is asserted on the reference
first."""
import functools
import math

import numpy as np
import pytest

import oracle
import rows_ref
from test_count_gpu import assert_same, random_streams, run_gpu
from test_dist import make_streams

pytestmark = pytest.mark.gpu

TL, TD = 1024, 65536              # kc_spec_hist: LDS totals, dense global totals (csrc/count.hip)
CHUNK = 4096                      # kc_select: rows per chunk
EVERYTHING = (1, 2 ** 31 - 1)
T3 = (50.0, 75.0, 100.01)
T8 = (33.333333333333336, 50.0, 60.0, 66.66666666666667, 75.0, 80.0, 100.0, 100.01)
T9 = tuple(sorted(T8 + (90.0,)))
T16 = tuple(sorted(T8 + (10.0, 20.0, 25.0, 30.0, 40.0, 70.0, 90.0, 200.0)))
T17 = tuple(sorted(T16 + (95.0,)))


def hga_error():
    import hga
    return hga.HgaError


def random_keys(rng, k, n):
    """n distinct canonical-code-sized values below 4^k, in random order."""
    lim = (1 << (2 * k)) - 1
    keys = np.zeros(0, np.uint64)
    while len(keys) < n:
        keys = np.unique(np.concatenate([keys, rng.integers(0, lim, 2 * n + 8, dtype=np.uint64, endpoint=True)]))
    return rng.permutation(keys)[:n]


def random_counts(rng, n, F):
    """Each row nonzero in a random subset of the files; every seventh row in exactly one file of index
    >= 2 (F >= 3).  Counts of 1-9 mostly, some up to 2000, a few up to 200 000."""
    c = rng.integers(1, 10, (n, F))
    mid, big = rng.random((n, F)), rng.random((n, F))
    c = np.where(mid < 0.25, rng.integers(10, 2001, (n, F)), c)
    c = np.where(big < 0.05, rng.integers(2001, 200_001, (n, F)), c)
    c[rng.random((n, F)) >= min(0.6, 2.5 / F)] = 0
    empty = ~c.any(axis=1)
    c[empty, rng.integers(0, F, int(empty.sum()))] = 7
    if F >= 3:
        lone = np.arange(0, n, 7)
        f = rng.integers(2, F, len(lone))
        v = c[lone, f]
        c[lone] = 0
        c[lone, f] = np.where(v > 0, v, 3)
    return c.astype(np.uint32)


def load_rows(ctx, k, keys, counts, rng=None):
    """count_begin, one count_add_rows per file (its nonzero rows, in any order), count_run(1)."""
    F = counts.shape[1]
    ctx.count_begin(k, F)
    for f in range(F):
        at = np.flatnonzero(counts[:, f])
        if rng is not None:
            at = rng.permutation(at)
        ctx.count_add_rows(f, keys[at], counts[at, f])
    ctx.count_run(1)


def check_rows(ctx, rk, rc):
    keys, counts = ctx.rows()
    assert np.array_equal(keys, rk)
    assert np.array_equal(counts, rc)
    assert ctx.count_stats().distinct_rows == len(rk)
    for f in range(rc.shape[1]):
        dk, dc = ctx.dump(f)
        wk, wc = rows_ref.dump(rk, rc, f)
        assert np.array_equal(dk, wk) and np.array_equal(dc, wc), f


def check_hist(ctx, rc, thr):
    assert np.array_equal(ctx.spec_hist(list(thr)), rows_ref.spec_hist(rc, thr))


def check_select(ctx, rk, rc, lower, upper):
    keys, flags, nd = ctx.select(lower, upper)
    wk, wf, wd = rows_ref.select(rk, rc, lower, upper)
    assert np.array_equal(keys, wk)
    assert np.array_equal(flags, wf)
    assert nd == wd
    return wk, wf, wd


def check_all(ctx, rk, rc, thr=oracle.THRESHOLDS, bounds=(EVERYTHING,)):
    check_rows(ctx, rk, rc)
    check_hist(ctx, rc, thr)
    return [check_select(ctx, rk, rc, lo, hi) for lo, hi in bounds]


# ---- 1. file counts and row-count edges ------------------------------------------------------------
FILES = (1, 2, 3, 4, 5, 8, 9, 16, 33, 64)
EDGES = (1, 2, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1)
SHAPES = sorted({(19, F, CHUNK + 1) for F in FILES} | {(32, F, CHUNK + 1) for F in (1, 3, 9)} |
                {(k, F, n) for k in (19, 32) for F in (1, 3) for n in EDGES})


@pytest.mark.parametrize("k,F,n", SHAPES)
def test_files_and_row_count_edges(gpu_ctx, k, F, n):
    """F files (kc_spec_hist's loop past file 3, kc_select's loop past file 1) and row counts that end
    inside, at and after a four-row group and a 4096-row chunk; at k = 32 the discriminative flag is a
    word of its own instead of key bit 63."""
    rng = np.random.default_rng(1000 * k + 10 * F + n % 10)
    keys, counts = random_keys(rng, k, n), random_counts(rng, n, F)
    rk, rc = rows_ref.merge([(keys, counts)], 1)
    assert len(rk) == n and int(rc.astype(np.uint64).sum(axis=1).max()) < 2 ** 31
    tot = np.sort(rc.astype(np.uint64).sum(axis=1))
    mid = (int(tot[len(tot) // 4]), int(tot[3 * len(tot) // 4]))
    load_rows(gpu_ctx, k, keys, counts, rng)
    (sk, sf, sd), _ = check_all(gpu_ctx, rk, rc, bounds=(EVERYTHING, mid))
    assert len(sk) == n
    if F >= 3:   # rows present in one file only, and that file is not one of the first two
        lone = ((rc > 0).sum(axis=1) == 1) & (rc[:, 2:] > 0).any(axis=1)
        assert 10 * int(lone.sum()) >= n and sf[lone].all() and sd >= int(lone.sum())


@pytest.mark.parametrize("F", [0, 65])
def test_file_count_out_of_range(gpu_ctx, F):
    with pytest.raises(hga_error(), match="hga status 1"):   # HGA_ERR_INVALID
        gpu_ctx.count_begin(19, F)
    gpu_ctx.count_begin(19, 64)


@pytest.mark.parametrize("k,F", [(19, 14), (13, 15)])
def test_file_count_limit_with_reads(gpu_ctx, k, F):
    """Reads are counted with one counter per file in every slot of kc_count's LDS table: the most files
    it holds (14 with u64 remainders, 15 with u32 ones) still count exactly, one more is refused by
    count_run (HGA_ERR_INVALID) unless no file has reads (test_files_and_row_count_edges, F >= 16)."""
    streams = make_streams(n_reads=150, n_files=F + 1)
    ref = oracle.count_pipeline(streams[:F], k, 2, 9)
    assert_same(run_gpu(gpu_ctx, streams[:F], k, 2, 9), ref)
    assert len(ref["keys"]) > 1000 and ref["counts"][:, F - 1].any()
    gpu_ctx.count_begin(k, F + 1)
    gpu_ctx.count_add(F, streams[F])
    with pytest.raises(hga_error(), match="hga status 1: too many files with reads"):
        gpu_ctx.count_run(2)
    gpu_ctx.count_begin(k, F + 1)   # the same session shape from dump rows alone
    gpu_ctx.count_add_rows(F, *ref["dumps"][F - 1])
    gpu_ctx.count_run(2)
    keys, counts = gpu_ctx.rows()
    assert np.array_equal(keys, ref["dumps"][F - 1][0]) and np.array_equal(counts[:, F], ref["dumps"][F - 1][1])
    assert not counts[:, :F].any()


# ---- 2. histogram tiers ----------------------------------------------------------------------------
def split3(rng, total):
    """Three counts summing to `total`: in one, two or three files."""
    c = [0, 0, 0]
    files = rng.permutation(3)
    ways = min(int(rng.integers(1, 4)), total)
    cuts = sorted(int(x) for x in rng.integers(1, total, ways - 1)) if total > 1 else []
    for f, a, b in zip(files, [0] + cuts, cuts + [total]):
        c[f] += b - a
    return c


EDGE_TOTALS = (1, TL - 1, TL, TL + 1, TD - 1, TD, TD + 1, 2 ** 31 - 1)
ON_THRESHOLD = [(32768, 32768, 0), (0, 32768, 32768), (49152, 16384, 0), (16384, 0, 49152), (2 << 20, 1 << 20, 0),
                (1 << 19, 2 << 20, 1 << 19), (1, 1, 0), (3, 1, 0), (0, 2, 1), (2, 1, 0), (512, 512, 0), (768, 256, 0),
                (256, 511, 256), (1 << 30, 1 << 29, 1 << 29), (3 << 28, 1 << 28, 0), (40000, 10000, 0)]


@functools.lru_cache(maxsize=None)
def tier_rows(n=6000, on_threshold=True):
    """k = 19, F = 3: totals log-uniform from 1 to 2^22, several rows at every total of EDGE_TOTALS, and
    rows whose ratio lies on a threshold (or one double below it) at small and large totals."""
    rng = np.random.default_rng(42)
    rows = [split3(rng, t) for t in EDGE_TOTALS for _ in range(6)]
    rows += [[t, 0, 0] for t in EDGE_TOTALS] + [[0, 0, t] for t in EDGE_TOTALS]
    if on_threshold:
        rows += [list(r) for r in ON_THRESHOLD for _ in range(3)]
    while len(rows) < n:
        rows.append(split3(rng, max(1, int(2.0 ** rng.uniform(0, 22)))))
    counts = np.array(rows, np.uint32)
    keys = random_keys(rng, 19, len(counts))
    rk, rc = rows_ref.merge([(keys, counts)], 1)
    rk.setflags(write=False)
    rc.setflags(write=False)
    return keys, counts, rk, rc


def assert_all_tiers(rc):
    tot = set(rc.astype(np.uint64).sum(axis=1).tolist())
    assert set(EDGE_TOTALS) <= tot
    assert min(tot) < TL <= max(t for t in tot if t < TD) and max(tot) >= TD


@pytest.mark.parametrize("thr,fp64", [(T3, False), (T8, False), (T9, False), (T16, False), (T3, True), (T8, True)],
                         ids=["3", "8", "9", "16", "3-fp64", "8-fp64"])
def test_histogram_tiers(gpu_ctx, monkeypatch, thr, fp64):
    """Totals in LDS (< 1024), in the dense global histogram (< 65536) and in the overflow list, with
    the u16 boundary table (at most 8 thresholds) and with spec_index in doubles (more, or
    HGA_SPEC_FP64); ratios that land exactly on a threshold (1/2, 3/4), or on the last double below it
    (2/3 against 66.66666666666667), at totals of 2 to 2^31."""
    keys, counts, rk, rc = tier_rows()
    assert_all_tiers(rc)
    ref = rows_ref.spec_hist(rc, thr)
    for row, exact in (((32768, 32768, 0), True), ((49152, 16384, 0), True), ((2 << 20, 1 << 20, 0), False)):
        x = (float(max(row)) / float(sum(row))) * 100   # on a threshold, or (2/3) the last double below it
        assert row in ON_THRESHOLD and (x in T8 if exact else math.nextafter(x, 100.0) in T8)
    if fp64:
        monkeypatch.setenv("HGA_SPEC_FP64", "1")
    else:
        monkeypatch.delenv("HGA_SPEC_FP64", raising=False)
    load_rows(gpu_ctx, 19, keys, counts)
    assert np.array_equal(gpu_ctx.spec_hist(list(thr)), ref)
    assert int(ref[:, 2].sum()) == len(rk)


def test_histogram_tiers_other_queries(gpu_ctx):
    keys, counts, rk, rc = tier_rows()
    load_rows(gpu_ctx, 19, keys, counts)
    check_all(gpu_ctx, rk, rc, thr=T8, bounds=(EVERYTHING, (TL, TD), (TD, 2 ** 31 - 1), (TL - 1, TL - 1)))


def test_seventeen_thresholds_are_invalid(gpu_ctx):
    keys, counts, rk, rc = tier_rows()
    load_rows(gpu_ctx, 19, keys, counts)
    with pytest.raises(hga_error(), match="hga status 1"):
        gpu_ctx.spec_hist(list(T17))
    check_hist(gpu_ctx, rc, T16)


# ---- 3. more than 1024 bins ------------------------------------------------------------------------
def test_more_than_1024_bins(gpu_ctx):
    """3000 rows with 3000 distinct totals around 1024: the compacted triples no longer fit the first
    read-back chunk (SPEC_CHUNK = 1024), so the host fetches the whole list."""
    rng = np.random.default_rng(3)
    counts = np.array([split3(rng, t) for t in range(1, 3001)], np.uint32)
    keys = random_keys(rng, 19, len(counts))
    rk, rc = rows_ref.merge([(keys, counts)], 1)
    load_rows(gpu_ctx, 19, keys, counts)
    for thr in (T8, T16):
        ref = rows_ref.spec_hist(rc, thr)
        assert len(ref) > 1024 and ref[:, 1].min() < TL < ref[:, 1].max()
        assert np.array_equal(gpu_ctx.spec_hist(list(thr)), ref)
    check_all(gpu_ctx, rk, rc, thr=oracle.THRESHOLDS, bounds=((1000, 1100),))


# ---- 4. error, then recovery -----------------------------------------------------------------------
def test_error_then_recovery(gpu_ctx):
    """A threshold list that ends at 90.0 fails on the first single-file row (specificity 100); the next
    calls on the same rows must find no bin of the failed one: with 100.01 appended, with a shorter
    list (bins at threshold indices it does not scan), and with the long one again."""
    keys, counts, rk, rc = tier_rows()
    assert_all_tiers(rc)
    assert ((rc > 0).sum(axis=1) == 1).any()
    short = tuple(t for t in T9 if t <= 90.0)
    with pytest.raises(ValueError):
        rows_ref.spec_hist(rc, short)
    load_rows(gpu_ctx, 19, keys, counts)
    with pytest.raises(hga_error(), match="above the last threshold"):
        gpu_ctx.spec_hist(list(short))
    check_hist(gpu_ctx, rc, short + (100.01,))
    with pytest.raises(hga_error(), match="above the last threshold"):
        gpu_ctx.spec_hist(list(short))
    check_hist(gpu_ctx, rc, (100.01,))
    check_hist(gpu_ctx, rc, (50.0, 100.01))
    check_hist(gpu_ctx, rc, short + (100.01,))
    check_rows(gpu_ctx, rk, rc)


# ---- 5. select bounds ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def select_rows(n):
    rng = np.random.default_rng(n)
    counts = np.array([split3(rng, int(t)) for t in rng.integers(1, 400, n)], np.uint32)
    keys = random_keys(rng, 19, n)
    rk, rc = rows_ref.merge([(keys, counts)], 1)
    return keys, counts, rk, rc


def test_select_bounds(gpu_ctx):
    keys, counts, rk, rc = select_rows(5000)
    tot = rc.astype(np.int64).sum(axis=1)
    common = int(np.bincount(tot).argmax())
    lo_t, hi_t = int(np.sort(tot)[1000]), int(np.sort(tot)[4000])
    load_rows(gpu_ctx, 19, keys, counts)
    n_of = {}
    for lower, upper in ((common, common), (hi_t, lo_t), (-5, lo_t), (hi_t, 2 ** 63 - 1), (-5, 2 ** 63 - 1),
                         (int(tot.min()), int(tot.max())), (int(tot.max()) + 1, 2 ** 40), (-9, 0), (lo_t, hi_t),
                         (2 ** 63 - 1, 2 ** 63 - 1), (-2 ** 63, -1)):
        wk, _, wd = check_select(gpu_ctx, rk, rc, lower, upper)
        n_of[(lower, upper)] = (len(wk), wd)
    assert n_of[(common, common)][0] == int((tot == common).sum()) > 1
    assert n_of[(hi_t, lo_t)] == (0, 0) and hi_t > lo_t
    assert n_of[(-5, 2 ** 63 - 1)][0] == len(rk) and n_of[(int(tot.max()) + 1, 2 ** 40)] == (0, 0)
    assert n_of[(lo_t, hi_t)][0] == int(((tot >= lo_t) & (tot <= hi_t)).sum())


def test_select_msd_sort_three_files(gpu_ctx):
    """40 000 rows: past 2^15 the export is ordered by the MSD pass and segment sorts, here with the
    count loop over a third file."""
    keys, counts, rk, rc = select_rows(40_000)
    load_rows(gpu_ctx, 19, keys, counts)
    wk, _, wd = check_select(gpu_ctx, rk, rc, 2, 2 ** 31 - 1)
    assert len(wk) >= 1 << 15 and wd > 0
    check_select(gpu_ctx, rk, rc, 100, 200)
    check_rows(gpu_ctx, rk, rc)
    check_hist(gpu_ctx, rc, T8)


# ---- 6. reads and rows together, three files -------------------------------------------------------
def test_reads_and_rows_three_files(gpu_ctx):
    """File 0 from reads, file 1 from reads and dump rows on overlapping keys, file 2 from dump rows
    only: the reads get the per-file drop (min 2), the dump rows are summed in as they are."""
    k, min_c = 19, 2
    rng = np.random.default_rng(6)
    streams = random_streams(66, 2, 300, 100)
    read_dumps = [oracle.count_stream(s, k, min_c) for s in streams]
    all1 = oracle.count_stream(streams[1], k, 1)[0]   # file 1's k-mers, the dropped singletons included
    k1 = np.unique(np.concatenate([all1[::5], random_keys(rng, k, 300)]))
    k2 = np.unique(np.concatenate([read_dumps[0][0][::9], all1[::11], random_keys(rng, k, 500)]))
    rows1 = (k1, rng.integers(1, 6, len(k1)).astype(np.uint32))
    rows2 = (k2, rng.integers(1, 3000, len(k2)).astype(np.uint32))
    assert len(np.intersect1d(k1, read_dumps[1][0])) > 50 and len(np.setdiff1d(k1, read_dumps[1][0])) >= 300
    gpu_ctx.count_begin(k, 3)
    gpu_ctx.count_add(0, streams[0])
    gpu_ctx.count_add(1, streams[1])
    gpu_ctx.count_add_rows(1, rows1[0][::-1], rows1[1][::-1])
    gpu_ctx.count_add_rows(2, *rows2)
    gpu_ctx.count_run(min_c)
    src = rows_ref.from_dumps([read_dumps[0], read_dumps[1], (np.zeros(0, np.uint64), np.zeros(0, np.uint32))])
    src += [rows_ref.from_dumps([(np.zeros(0, np.uint64), np.zeros(0, np.uint32)), rows1, rows2])[f] for f in (1, 2)]
    rk, rc = rows_ref.merge(src, 1)
    lone2 = ((rc > 0).sum(axis=1) == 1) & (rc[:, 2] > 0)
    assert lone2.sum() > 100 and (rc[:, 1] == 1).any()   # a dump row of 1 survives next to the dropped reads
    check_all(gpu_ctx, rk, rc, bounds=(EVERYTHING, (2, 9)))
