"""The small launches and host waits around the count step's big kernels (DESIGN.md §4 "count tail"):
the spill blocks inside the one re-bin launch, the layout scan that reads the fine histograms transposed
and writes the per-file bucket runs, the pipeline counters from run to run, the specificity histogram's
bins and counters left clear from call to call, and the export sort enqueued before the select's
synchronisation with its go / no-go word.  Everything against the oracle."""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

THR7 = oracle.THRESHOLDS
THR9 = [50.0, 60.0] + list(oracle.THRESHOLDS)   # more than 8: kc_spec_hist's double path
ALL = (1, 10 ** 9)


def rand_seq(n, seed, alphabet="ACGT"):
    rng = random.Random(seed)
    return "".join(rng.choice(alphabet) for _ in range(n)).encode()


def reads_of(g, n, length, seed):
    rng = random.Random(seed)
    return b"\n".join(g[s:s + length] for s in (rng.randrange(0, len(g) - length) for _ in range(n)))


def mutate(g, every, seed):
    rng = random.Random(seed)
    b = bytearray(g)
    for i in range(0, len(b), every):
        b[i] = ord(rng.choice("ACGT"))
    return bytes(b)


def load(ctx, streams, k):
    ctx.count_begin(k, len(streams))
    for f, s in enumerate(streams):
        ctx.count_add(f, s)


def windows(streams, k):
    return sum(oracle.count_instances(s, k) for s in streams)


def check_rows(ctx, streams, k, ref):
    keys, counts = ctx.rows()
    assert np.array_equal(keys, ref[0]) and np.array_equal(counts, ref[1])
    assert ctx.count_stats().instances == windows(streams, k)


def check_select(ctx, ref, lower, upper):
    """One selection: ascending, the oracle's keys, count of discriminative keys and flags."""
    keys, counts = ref
    sel, flags, nd = ctx.select(lower, upper)
    o_sel, o_nd = oracle.select(keys, counts, lower, upper)
    assert np.all(sel[1:] > sel[:-1])
    assert np.array_equal(sel, o_sel) and nd == o_nd
    nz = (counts > 0).sum(1)
    assert np.array_equal(flags.astype(bool), nz[np.searchsorted(keys, sel)] == 1)
    return len(sel)


def cu_count():
    """Compute units of the device, from the HIP runtime the library has loaded (63 is
    hipDeviceAttributeMultiprocessorCount)."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    v = C.c_int(0)
    assert C.CDLL(path).hipDeviceGetAttribute(C.byref(v), 63, int(os.environ.get("HGA_DEVICE", "0"))) == 0
    assert 1 <= v.value <= 4096
    return v.value


# ---- 1. spill blocks and listed buckets through the merged re-bin launch --------------------------------
def test_spills_and_listed_buckets(gpu_ctx):
    """Two files of ACGTACGT..., sized from the CU count so that a bin1 workgroup's super-tile is three
    8192-base tiles (more than two tiles' worth, rounded up to whole tiles): the sequence has two canonical
    19-mers, so a workgroup puts at least 12288 elements into one level-1 region, more than one 8192-element
    block: every workgroup's run spills, and the spill blocks are re-binned by the workgroups appended to
    the first-block grid.  Each file's run in the two occupied fine buckets is millions long (>= 65536: the
    buckets are listed for the generic kc_count), and every total is >= 65536 (the histogram's overflow
    list).  count_stats() does not expose the spill or listed figures; the sizes above guarantee both."""
    cus = cu_count()
    per_file = cus * (2 * 8192 + 1000)   # total / (2 super-tiles per CU) = 17384 bases -> 3 tiles (9 MB at 256 CUs)
    streams = [(b"ACGT" * (per_file // 4 + 1))[:per_file], (b"CGTA" * (per_file // 4 + 1))[:per_file]]
    ref = oracle.count_files_mt(streams, 19, 2, 16)
    assert 1 <= len(ref[0]) <= 4 and int(ref[1].min()) >= 65536
    for _ in range(2):
        load(gpu_ctx, streams, 19)
        gpu_ctx.count_run(2)
        check_rows(gpu_ctx, streams, 19, ref)
        assert gpu_ctx.count_stats().max_split == 1   # a handful of distinct keys never splits a bucket
        assert np.array_equal(gpu_ctx.spec_hist(THR7), oracle.specificity(ref[1], THR7))
        assert check_select(gpu_ctx, ref, *ALL) == len(ref[0])


@pytest.mark.parametrize("three_launch", [False, True], ids=["scan", "transpose_scan_fs"])
def test_layout_paths(gpu_ctx, hga_mod, monkeypatch, three_launch):
    """The layout as one transposed-read scan, and (HGA_LAYOUT_T, the path of inputs with more than 1024 bin1
    workgroups) as transpose + scan + kc_fs, on three files of uneven sizes, the last one shorter than k: a
    file's first workgroup then falls anywhere in a scan tile, and the last file's runs are all empty."""
    if three_launch:
        monkeypatch.setenv("HGA_LAYOUT_T", "1")
    g = hga_mod.gen_genome(700_000, 61)
    streams = [hga_mod.gen_art(g, 30_000, 150, 62).seq, reads_of(mutate(g, 30, 63), 7_001, 131, 64), b"ACGTAC"]
    ref = oracle.count_files_mt(streams, 19, 1, 16)
    load(gpu_ctx, streams, 19)
    gpu_ctx.count_run(1)
    check_rows(gpu_ctx, streams, 19, ref)
    check_select(gpu_ctx, ref, 2, 50)


# ---- 2. the pipeline counters from run to run -------------------------------------------------------
def test_counters_across_runs(gpu_ctx, hga_mod):
    g = hga_mod.gen_genome(200_000, 5)
    big = [hga_mod.gen_art(g, 12_000, 150, 6).seq, hga_mod.gen_art(mutate(g, 40, 7), 12_000, 150, 8).seq]
    small = [reads_of(g, 900, 120, 9), reads_of(g, 700, 120, 10)]
    load(gpu_ctx, big, 19)
    gpu_ctx.count_run(2)
    gpu_ctx.count_run(1)   # the first run is never queried: its counters must not leak into this one
    ref1 = oracle.count_files_mt(big, 19, 1, 16)
    assert np.array_equal(gpu_ctx.spec_hist(THR7), oracle.specificity(ref1[1], THR7))   # settles the run
    check_rows(gpu_ctx, big, 19, ref1)
    check_select(gpu_ctx, ref1, 3, 30)
    load(gpu_ctx, small, 19)
    gpu_ctx.count_run(2)
    ref2 = oracle.count_files_mt(small, 19, 2, 16)
    check_rows(gpu_ctx, small, 19, ref2)
    assert np.array_equal(gpu_ctx.spec_hist(THR7), oracle.specificity(ref2[1], THR7))
    gpu_ctx.count_run(2)
    check_rows(gpu_ctx, small, 19, ref2)
    check_select(gpu_ctx, ref2, *ALL)


# ---- 3. the specificity histogram called again and again, on a pending and on a settled count ------------
@functools.lru_cache(maxsize=None)
def hist_input(kind):
    g = rand_seq(60_000, 31)
    if kind == "ge1024":     # a 60-base motif 2000 times over: 60 19-mers with totals in [1024, 65536)
        a = g + b"\n" + rand_seq(60, 32) * 2000
    else:                    # a homopolymer block: one 19-mer with a total >= 65536
        a = g + b"\n" + b"A" * 100_000
    streams = (reads_of(g, 6_000, 150, 33) + b"\n" + a, reads_of(mutate(g, 35, 34), 6_000, 150, 35))
    ref = oracle.count_files_mt(list(streams), 19, 2, 16)
    tot = ref[1].sum(1)
    assert (tot.max() >= 65536) if kind == "ge65536" else (1024 <= tot.max() < 65536)
    return streams, ref


@pytest.mark.parametrize("kind", ["ge1024", "ge65536"])
@pytest.mark.parametrize("thr", [THR7, THR9], ids=["thr7", "thr9"])
def test_spec_hist_repeated(gpu_ctx, kind, thr):
    streams, ref = hist_input(kind)
    want = oracle.specificity(ref[1], thr)
    load(gpu_ctx, list(streams), 19)
    gpu_ctx.count_run(2)
    first = gpu_ctx.spec_hist(thr)     # on the pending count: rows from its device cursor
    again = gpu_ctx.spec_hist(thr)     # on the settled count: bins and counters were left clear
    third = gpu_ctx.spec_hist(thr)
    assert np.array_equal(first, want)
    assert np.array_equal(again, first) and np.array_equal(third, first)
    check_rows(gpu_ctx, list(streams), 19, ref)


# ---- 4. every branch of the select behind the speculative enqueue, k = 15 -------------------------------
MARKER = b"\n".join([b"ACGTTGCAAGGCTAC"] * 700)   # one 15-mer far above every other total


@functools.lru_cache(maxsize=None)
def select_input(kind):
    if kind == "one_digit":   # 100 000 reads of 15 bases, AAAAAA + 9 random: every key in the 12-bit digit 0,
        rng = random.Random(41)   # ~83 K distinct > the 32 K a segment may hold: the device says no
        reads = [b"AAAAAA" + "".join(rng.choice("ACGT") for _ in range(9)).encode() for _ in range(100_000)]
        reads[:60] = [b"AAAAAACGTACGTAC"] * 60   # one key far above every other total (bounds that keep one)
        streams = (b"\n".join(reads[:50_000]), b"\n".join(reads[50_000:]))
        min_count = 1
    elif kind == "bucketed":  # 300 kb at 20x: ~70 keys in each of the 4096 digits
        g = rand_seq(300_000, 42)
        streams = (reads_of(g, 20_000, 150, 43) + b"\n" + MARKER, reads_of(mutate(g, 50, 44), 20_000, 150, 45))
        min_count = 2
    else:                     # fewer than 2^15 rows: no MSD path
        g = rand_seq(20_000, 46)
        streams = (reads_of(g, 1_500, 150, 47) + b"\n" + MARKER, reads_of(mutate(g, 50, 48), 1_500, 150, 49))
        min_count = 2
    return streams, min_count, oracle.count_files_mt(list(streams), 15, min_count, 16)


@pytest.mark.parametrize("kind", ["one_digit", "bucketed", "small"])
def test_select_branches(gpu_ctx, kind):
    streams, min_count, ref = select_input(kind)
    rows = len(ref[0])
    assert (rows < 1 << 15) if kind == "small" else (rows >= 1 << 15)
    tot = ref[1].sum(1, dtype=np.int64)
    top = int(tot.max())
    assert int((tot == top).sum()) == 1
    bounds = [ALL, (2, 40) if kind != "one_digit" else (1, 2), (top, top), (top + 1, top + 10)]
    want_n = [rows, None, 1, 0]
    load(gpu_ctx, list(streams), 15)
    gpu_ctx.count_run(min_count)
    for _ in range(2):
        for (lo, hi), wn in zip(bounds, want_n):
            n = check_select(gpu_ctx, ref, lo, hi)
            assert wn is None or n == wn
    if kind == "one_digit":   # the digit's kept keys pass a segment's capacity with every key kept
        assert int((ref[0] >> np.uint64(18) == 0).sum()) == rows > 32768
