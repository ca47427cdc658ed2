"""Every size-selected path of count_run (csrc/count.hip) at inputs of a few tens of KB, bit-exact against
the oracle: rows, counts, per-file dumps, specificity histogram, selection, n_discr and instances.

count_run picks its kernels from (k, fb, F), and fb (the fine-bucket bits) from the input's size, so the
small inputs of the other count tests only ever reach fb 0-2.  Here the test hooks HGA_FB_MIN / HGA_FB_MAX
(and HGA_COUNT_LEGACY, HGA_CS_LAZY, HGA_SPLIT3_FORCE, HGA_LAYOUT_T) put small inputs on the paths of large
ones.  `fb_of` and `expected_path` restate count_run's rules; every test asserts a witness that the path it
names ran (stats.buckets, stats.max_split, launch counts), so a rule that changes in count_run without
changing here fails the witness instead of silently testing another kernel."""
import functools
import random

import numpy as np
import pytest

import oracle
from test_count_gpu import assert_same, random_streams
from test_count_tail_gpu import cu_count

pytestmark = pytest.mark.gpu

# constants of csrc/count.hip / csrc/sort.hip that the rules below use
MAX_FB, MAX_FB1, PB_PACKED, PB_GENERIC = 12, 6, 65536, 16384
TILE, MAX_SF3, LAYOUT_W_MAX = 8192, 4096, 1024
HOOKS = ("HGA_FB_MIN", "HGA_FB_MAX", "HGA_COUNT_LEGACY", "HGA_CS_LAZY", "HGA_SPLIT3_FORCE", "HGA_SPLIT3_TARGET",
         "HGA_LAYOUT_T", "HGA_B1_SOLE", "HGA_ROW_CAP")
ALPHABET = "ACGTACGTACGTNacgt"
ALL = (1, 10 ** 9)
# the one 32-mer whose mixed 64-bit key is all ones (canonical form of its reverse complement ONES_RC)
ONES = b"CGCGTAGAGATATAATAAAAAAAAAAAAAAAA"
ONES_RC = b"TTTTTTTTTTTTTTTTATTATATCTCTACGCG"
ONES_CODE = 0x66c88cc300000000


# ---- count_run's rules, restated -------------------------------------------------------------------------
def fb_of(total, k, F, fb_min=0, fb_max=MAX_FB, legacy=False):
    """count_run's fine-bucket bits: one more while a bucket's share of the bytes is above ~64 K (packed
    counts) or 16 K windows, between the hooks' bounds, never more than the key has; k = 32 never runs
    with fb = 0 (the remainder would be the whole 64-bit key, and one key equals the empty marker)."""
    nbits = 2 * k
    packed = F <= 2 and nbits - min(MAX_FB, nbits) <= 31 and not legacy
    per_bucket = PB_PACKED if packed else PB_GENERIC
    fb = 0
    while fb < min(fb_max, MAX_FB) and fb < nbits and ((total >> fb) > per_bucket or fb < fb_min):
        fb += 1
    if nbits == 64 and fb == 0:
        fb = 1
    return fb


def fb3_forced(want, F, rbits):
    """count_run's third-level bits under HGA_SPLIT3_FORCE."""
    fb3 = 0
    while fb3 < want and fb3 < 8 and (2 << fb3) * F <= MAX_SF3 and rbits - fb3 > 1:
        fb3 += 1
    return fb3


def expected_path(k, F, fb, legacy=False):
    """The kernels count_run launches for (k, fb, F): its HGA_BIN1 / HGA_REBIN dispatch and the `packed &&
    e32` choice of the count kernel, as 'bin1<E1,K,FB>-rebin<E1,E>-count...'."""
    nbits = 2 * k
    e1_32 = nbits - min(fb, MAX_FB1) <= 32
    e32 = nbits - fb <= 31
    packed = F <= 2 and nbits - min(MAX_FB, nbits) <= 31 and not legacy
    if e1_32 and k == 19 and fb == MAX_FB:
        b1 = "u32,19,12"
    elif e1_32 and k in (19, 17, 15):
        b1 = f"u32,{k},0"
    elif e1_32:
        b1 = "u32,0,0"
    elif k == 21:
        b1 = "u64,21,0"
    else:
        b1 = "u64,0,0"
    count = "count_s" if packed and e32 else "count<u32>" if e32 else "count<u64>"
    return f"bin1<{b1}>-rebin<{'u32' if e1_32 else 'u64'},{'u32' if e32 else 'u64'}>-{count}"


def test_expected_path_table():
    """The rows of the dispatch table as count_run's comments and DESIGN.md §4 give them."""
    assert expected_path(19, 2, 12) == "bin1<u32,19,12>-rebin<u32,u32>-count_s"
    assert expected_path(19, 2, 7) == "bin1<u32,19,0>-rebin<u32,u32>-count_s"
    assert expected_path(19, 2, 6) == "bin1<u32,19,0>-rebin<u32,u64>-count<u64>"
    assert expected_path(19, 2, 2) == "bin1<u64,0,0>-rebin<u64,u64>-count<u64>"
    assert expected_path(17, 2, 2) == "bin1<u32,17,0>-rebin<u32,u64>-count<u64>"
    assert expected_path(15, 2, 0) == "bin1<u32,15,0>-rebin<u32,u32>-count_s"
    assert expected_path(16, 2, 1) == "bin1<u32,0,0>-rebin<u32,u32>-count_s"
    assert expected_path(20, 2, 9) == "bin1<u64,0,0>-rebin<u64,u32>-count_s"
    assert expected_path(21, 2, 11) == "bin1<u64,21,0>-rebin<u64,u32>-count_s"
    assert expected_path(21, 2, 10) == "bin1<u64,21,0>-rebin<u64,u64>-count<u64>"
    assert expected_path(19, 3, 12) == "bin1<u32,19,12>-rebin<u32,u32>-count<u32>"
    assert expected_path(19, 2, 12, legacy=True) == "bin1<u32,19,12>-rebin<u32,u32>-count<u32>"
    assert expected_path(22, 2, 12) == "bin1<u64,0,0>-rebin<u64,u64>-count<u64>"
    assert fb_of(35_000 * 2, 19, 2) == 1 and fb_of(35_000 * 2, 19, 2, fb_min=12) == 12
    assert fb_of(100, 32, 2) == 1 and fb_of(100, 3, 1, fb_min=12) == 6


# ---- running one case ------------------------------------------------------------------------------------
def set_hooks(mp, hooks):
    for name in HOOKS:
        mp.delenv(name, raising=False)
    for name, v in hooks.items():
        mp.setenv("HGA_" + name, str(v))


def load(ctx, streams, k):
    ctx.count_begin(k, len(streams))
    for f, s in enumerate(streams):
        ctx.count_add(f, s)


def run_loaded(ctx, F, min_count, lower, upper):
    """count_run on the loaded input with every output fetched, and the launch counts of the run."""
    ctx.profile(True)
    try:
        ctx.profile_reset()
        ctx.count_run(min_count)
        st = ctx.count_stats()
        launches = {n: ctx.profile_get(n)[1] for n in ("kc_bin1", "kc_layout", "kc_rebin", "kc_split3", "kc_count")}
    finally:
        ctx.profile(False)
    keys, counts = ctx.rows()
    hist = ctx.spec_hist(oracle.THRESHOLDS) if len(keys) else np.zeros((0, 3), np.int64)
    sel, flags, nd = ctx.select(lower, upper)
    dumps = [ctx.dump(f) for f in range(F)]
    return {"keys": keys, "counts": counts, "hist": hist, "selected": sel, "flags": flags, "n_discr": nd,
            "dumps": dumps, "stats": st, "launches": launches}


def check(r, o, streams, k, F, hooks, transposed=False):
    """Bit-exact outputs, then the witnesses of the path: bucket count from fb_of (times the forced third
    level), one kc_split3 launch iff a third level ran, one (scan) or two (transpose + kc_fs) kc_layout."""
    assert_same(r, o)
    assert len(r["dumps"]) == len(o["dumps"]) == F
    assert r["stats"].instances == sum(oracle.count_instances(s, k) for s in streams)
    nz = (o["counts"] > 0).sum(1)
    assert np.array_equal(r["flags"].astype(bool), nz[np.searchsorted(o["keys"], o["selected"])] == 1)
    fb = fb_of(sum(len(s) for s in streams), k, F, int(hooks.get("FB_MIN", 0)), int(hooks.get("FB_MAX", MAX_FB)),
               "COUNT_LEGACY" in hooks)
    fb3 = fb3_forced(int(hooks["SPLIT3_FORCE"]), F, 2 * k - fb) if "SPLIT3_FORCE" in hooks else 0
    assert r["stats"].buckets == 1 << (fb + fb3)
    assert r["launches"]["kc_split3"] == (1 if fb3 else 0)
    assert r["launches"]["kc_layout"] == (2 if transposed or "LAYOUT_T" in hooks else 1)
    assert r["launches"]["kc_bin1"] == r["launches"]["kc_rebin"] == r["launches"]["kc_count"] == 1
    return fb


def run_case(ctx, mp, streams, k, hooks, min_count=2, sel=(2, 6), o=None, transposed=False):
    F = len(streams)
    set_hooks(mp, hooks)
    load(ctx, streams, k)
    r = run_loaded(ctx, F, min_count, *sel)
    if o is None:
        o = oracle.count_pipeline(streams, k, sel[0], sel[1], min_count=min_count)
    fb = check(r, o, streams, k, F, hooks, transposed)
    return r, o, fb


@functools.lru_cache(maxsize=None)
def std_case(k, F, min_count=2, sel=(2, 6)):
    """The standard input (about 35 KB per file) and its oracle result, computed once per (k, F, min)."""
    streams = random_streams(1000 + k, F, 400, 120, ALPHABET)
    return streams, oracle.count_pipeline(streams, k, sel[0], sel[1], min_count=min_count)


def rand_seq(n, seed):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(n)).encode()


# ---- 1. dispatch matrix (HGA_FB_MIN) ---------------------------------------------------------------------
MATRIX = [(19, fb) for fb in (5, 6, 7, 11, 12)] + [(17, fb) for fb in (1, 2, 3, 12)] + [(15, 12)] + \
         [(16, fb) for fb in (0, 1, 12)] + [(18, fb) for fb in (3, 4, 7)] + [(20, fb) for fb in (8, 9)] + \
         [(21, fb) for fb in (10, 11, 12)] + [(k, 12) for k in (22, 27, 31, 32)]


def test_matrix_covers_every_instance():
    """The matrix (with the headline's F = 3 / legacy legs for the generic u32 kernel) reaches every kc_bin1
    instance, every kc_rebin pair and every count kernel at fb >= 6."""
    paths = [expected_path(k, 2, fb) for k, fb in MATRIX if fb >= 6] + [expected_path(19, 3, 12)]
    for b1 in ("u32,19,12", "u32,19,0", "u32,17,0", "u32,15,0", "u32,0,0", "u64,21,0", "u64,0,0"):
        assert any(f"bin1<{b1}>" in p for p in paths), b1
    for pair in ("u32,u32", "u32,u64", "u64,u32", "u64,u64"):
        assert any(f"rebin<{pair}>" in p for p in paths), pair
    for cnt in ("count_s", "count<u32>", "count<u64>"):
        assert any(p.endswith(cnt) for p in paths), cnt


@pytest.mark.parametrize("k,fb_min", MATRIX, ids=[f"k{k}-fb{fb}-{expected_path(k, 2, fb)}" for k, fb in MATRIX])
def test_dispatch_matrix(gpu_ctx, monkeypatch, k, fb_min):
    streams, o = std_case(k, 2)
    # (70 KB of input have fb = 1 by themselves: fb = 0 takes HGA_FB_MAX)
    _, _, fb = run_case(gpu_ctx, monkeypatch, streams, k, {"FB_MIN": fb_min} if fb_min else {"FB_MAX": 0}, o=o)
    assert fb == fb_min


HEADLINE = [("F1", 1, 2, {}), ("F3", 3, 2, {}), ("min1", 2, 1, {}), ("min3", 2, 3, {}),
            ("inline", 2, 2, {"CS_LAZY": 0}), ("lazy", 2, 2, {"CS_LAZY": 1}), ("legacy", 2, 2, {"COUNT_LEGACY": 1})]


@pytest.mark.parametrize("F,min_count,extra", [h[1:] for h in HEADLINE],
                         ids=[f"{h[0]}-{expected_path(19, h[1], 12, 'COUNT_LEGACY' in h[3])}" for h in HEADLINE])
def test_headline_variants(gpu_ctx, monkeypatch, F, min_count, extra):
    """kc_bin1<u32,19,12> (the benchmark's instance) with 1 and 3 files, min 1 and 3, either claim mode of
    kc_count_s and the generic u32 kernel."""
    streams, o = std_case(19, F, min_count)
    _, _, fb = run_case(gpu_ctx, monkeypatch, streams, 19, dict(extra, FB_MIN=12), min_count=min_count, o=o)
    assert fb == 12


# ---- 2. remainders of 0-2 bits ---------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2])
@pytest.mark.parametrize("k", [1, 2, 3, 5, 6, 7])
def test_tiny_remainders(gpu_ctx, monkeypatch, k, F):
    """fb = min(12, 2k): the remainder has 0 bits (k <= 6: the bucket is the whole key) or 2 (k = 7), as a
    small k on a large file has in production."""
    streams, o = std_case(k, F, 1, ALL)
    _, _, fb = run_case(gpu_ctx, monkeypatch, streams, k, {"FB_MIN": 12}, min_count=1, sel=ALL, o=o)
    assert fb == min(12, 2 * k) and 2 * k - fb == (2 if k == 7 else 0)
    assert expected_path(k, F, fb).endswith("rebin<u32,u32>-count_s")


# ---- 3. fb = 12 with the other switches ------------------------------------------------------------------
def test_fb12_split3_forced(gpu_ctx, monkeypatch):
    streams, o = std_case(19, 2)
    r, _, _ = run_case(gpu_ctx, monkeypatch, streams, 19, {"FB_MIN": 12, "SPLIT3_FORCE": 4}, o=o)
    assert r["stats"].buckets == 4096 << 4


def test_fb12_split3_forced_k32_three_files(gpu_ctx, monkeypatch):
    streams, o = std_case(32, 3)
    r, _, _ = run_case(gpu_ctx, monkeypatch, streams, 32, {"FB_MIN": 12, "SPLIT3_FORCE": 2}, o=o)
    assert r["stats"].buckets == 4096 << 2 and expected_path(32, 3, 12).endswith("count<u64>")


def test_fb12_transposed_layout(gpu_ctx, monkeypatch):
    """4096 buckets through kc_transpose, the scan and kc_fs (two launches named kc_layout)."""
    streams, o = std_case(19, 2)
    r, _, _ = run_case(gpu_ctx, monkeypatch, streams, 19, {"FB_MIN": 12, "LAYOUT_T": 1}, o=o)
    assert r["launches"]["kc_layout"] == 2 and r["stats"].buckets == 4096


def test_fb12_one_listed_bucket(gpu_ctx, monkeypatch):
    """70 000 instances of poly-A beside the random reads: that bucket's run in file 0 is >= 65536, so
    kc_count_s lists it for kc_count<u32> and counts the other 4095 itself.  (Counted in the packed 16 bits,
    70 000 would carry into file 1's half.)"""
    streams = list(std_case(19, 2)[0])
    streams[0] = streams[0] + b"\n" + b"A" * 70_018
    r, o, _ = run_case(gpu_ctx, monkeypatch, streams, 19, {"FB_MIN": 12}, min_count=1, sel=ALL)
    assert o["keys"][0] == 0 and o["counts"][0, 0] >= 70_000
    assert expected_path(19, 2, 12).endswith("count_s") and r["stats"].buckets == 4096


def test_fb12_empty_middle_file(gpu_ctx, monkeypatch):
    streams = list(std_case(19, 3)[0])
    streams[1] = b""
    r, o, _ = run_case(gpu_ctx, monkeypatch, streams, 19, {"FB_MIN": 12})
    assert len(o["keys"]) > 100 and not o["counts"][:, 1].any()


def test_fb12_single_workgroup(gpu_ctx, monkeypatch):
    """One read of 5000 bases: one kc_bin1 workgroup, so the layout scan covers W * nb + 1 = 4097 entries,
    an exact multiple of its 4096-entry tile plus the final entry alone in the last tile."""
    streams = [rand_seq(5000, 5)]
    r, o, _ = run_case(gpu_ctx, monkeypatch, streams, 19, {"FB_MIN": 12}, min_count=1, sel=(1, 6))
    assert len(o["keys"]) > 4900 and r["stats"].buckets == 4096 and r["launches"]["kc_layout"] == 1


def test_rerun_across_layouts(gpu_ctx, monkeypatch):
    """One loaded input, count_run with 4096 buckets, with the size's own 2, with 4096 again: the buffers
    and the cached per-file table are reused across the layouts."""
    streams, o = std_case(19, 2)
    load(gpu_ctx, streams, 19)
    for hooks in ({"FB_MIN": 12}, {}, {"FB_MIN": 12}):
        set_hooks(monkeypatch, hooks)
        fb = check(run_loaded(gpu_ctx, 2, 2, 2, 6), o, streams, 19, 2, hooks)
        assert fb == (12 if hooks else 1)


# ---- 4. the 16-bit packed counts of kc_count_s -----------------------------------------------------------
# (without the hook these 65-140 KB inputs have fb <= 2 and run kc_count<u64>; both are checked)
PACKED16 = [
    ("65535-65535", [b"A" * (65535 + 18), b"T" * (65535 + 18)], [[65535, 65535]]),
    ("65535-65536-listed", [b"A" * (65535 + 18), b"T" * (65536 + 18)], [[65535, 65536]]),
    ("F1-70000", [b"A" * 70_018], [[70_000]]),
    ("empty-70000-listed", [b"", b"A" * 70_018], [[0, 70_000]]),
]


@pytest.mark.parametrize("fb_min", [12, 0], ids=["fb12", "own-fb"])
@pytest.mark.parametrize("streams,rows", [p[1:] for p in PACKED16], ids=[p[0] for p in PACKED16])
def test_packed_16bit_counts(gpu_ctx, monkeypatch, streams, rows, fb_min):
    """One 19-mer 65 535 to 70 000 times per file: the largest count kc_count_s holds in 16 bits, the first
    it must hand to kc_count<u32> (F = 2 only: one file has the whole word)."""
    r, o, fb = run_case(gpu_ctx, monkeypatch, streams, 19, {"FB_MIN": fb_min} if fb_min else {}, min_count=1, sel=ALL)
    assert o["keys"].tolist() == [0] and o["counts"].tolist() == rows
    assert r["counts"].tolist() == rows
    assert expected_path(19, len(streams), fb).endswith("count_s" if fb_min else "count<u64>")


# ---- 5. sub-range splitting ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def split_case(k):
    streams = [rand_seq(60_000, 1), rand_seq(60_000, 2)] if k == 15 else [rand_seq(100_000, 3)]
    return streams, oracle.count_pipeline(streams, k, 1, 5, min_count=1)


@pytest.mark.parametrize("lazy", [0, 1], ids=["inline", "lazy"])
def test_count_s_subrange_split(gpu_ctx, monkeypatch, lazy):
    """~120 K distinct 15-mers in the single bucket of kc_count_s (8192 slots): the bucket is counted in
    sub-ranges, with new keys claimed inline or through the miss queue."""
    streams, o = split_case(15)
    assert len(o["keys"]) > 100_000
    r, _, fb = run_case(gpu_ctx, monkeypatch, streams, 15, {"FB_MAX": 0, "CS_LAZY": lazy}, min_count=1, sel=(1, 5), o=o)
    assert fb == 0 and expected_path(15, 2, 0).endswith("count_s")
    assert r["stats"].buckets == 1 and r["stats"].max_split > 1


def test_generic_subrange_split(gpu_ctx, monkeypatch):
    """The same for kc_count<u64>: ~100 K distinct 25-mers in one bucket."""
    streams, o = split_case(25)
    assert len(o["keys"]) > 90_000
    r, _, fb = run_case(gpu_ctx, monkeypatch, streams, 25, {"FB_MAX": 0}, min_count=1, sel=(1, 5), o=o)
    assert fb == 0 and expected_path(25, 1, 0).endswith("count<u64>")
    assert r["stats"].buckets == 1 and r["stats"].max_split > 1


# ---- 6. the large-input layout at a small size -----------------------------------------------------------
def test_clamped_super_tiles_and_three_launch_layout(gpu_ctx, monkeypatch):
    """HGA_FB_MAX=0 gives one level-1 region, so st_cap is 7680 bases and ~9 MB of reads are 'far larger
    inputs' for count_run: the super-tiles are clamped to one tile and there are more than 1024 kc_bin1
    workgroups, past what the one-launch layout scan takes.  Reads from a 2 kb genome keep the single
    bucket's distinct keys under one table (no sub-range split)."""
    cus = cu_count()
    total = max(9_000_000, 24_000 * cus)
    g = rand_seq(2000, 21)
    rng = random.Random(22)
    n = total // 2 // 151 + 1
    streams = [b"\n".join(g[s:s + 150] for s in (rng.randrange(0, len(g) - 150) for _ in range(n))) for _ in range(2)]
    total = sum(len(s) for s in streams)
    st_cap = TILE * 1 * 15 // 16
    assert total // (cus * 2) + 1 > st_cap + st_cap // 2            # count_run clamps st_pos to st_cap ...
    st_pos = max(TILE, -(-st_cap // TILE) * TILE)                   # ... rounded up to whole tiles
    assert sum(-(-len(s) // st_pos) for s in streams) > LAYOUT_W_MAX
    o = oracle.count_pipeline(streams, 15, 2, 10 ** 9)
    assert 1000 < len(o["keys"]) < 6000
    r, _, fb = run_case(gpu_ctx, monkeypatch, streams, 15, {"FB_MAX": 0}, sel=(2, 10 ** 9), o=o, transposed=True)
    assert fb == 0 and r["stats"].buckets == 1 and r["stats"].max_split == 1
    assert r["launches"]["kc_layout"] == 2


# ---- 7. the all-ones key ---------------------------------------------------------------------------------
def ones_streams(with_reads):
    streams = [ONES + b"\n" + ONES, ONES_RC]
    if with_reads:
        extra = random_streams(7, 2, 40, 120, ALPHABET)
        streams = [e + b"\n" + s for e, s in zip(extra, streams)]
    return streams


@pytest.mark.parametrize("with_reads", [False, True], ids=["alone", "in-8KB"])
@pytest.mark.parametrize("fb_min", [0, 1, 12])
def test_all_ones_key(gpu_ctx, monkeypatch, fb_min, with_reads):
    """The 32-mer whose mixed key is 0xFFFF...F.  With the whole 64-bit key as the remainder (fb = 0) it
    would equal kc_count<uint64_t>'s EMPTY and be dropped; count_run therefore gives k = 32 at least one
    bucket bit, which the bucket count witnesses (2 buckets for these <= 16 KB inputs without a hook)."""
    streams = ones_streams(with_reads)
    total = sum(len(s) for s in streams)
    assert total <= PB_GENERIC and (not with_reads or total > 6000)
    r, o, fb = run_case(gpu_ctx, monkeypatch, streams, 32, {"FB_MIN": fb_min} if fb_min else {}, min_count=1, sel=ALL)
    at = int(np.searchsorted(o["keys"], ONES_CODE))
    assert o["keys"][at] == ONES_CODE and o["counts"][at].tolist() == [2, 1]
    assert r["keys"][at] == ONES_CODE and r["counts"][at].tolist() == [2, 1]
    assert fb == max(fb_min, 1) and r["stats"].buckets == 1 << fb


def test_all_ones_key_fb_max_0(gpu_ctx, monkeypatch):
    """HGA_FB_MAX=0 asks for no bucket bits: k = 32 still gets one."""
    r, _, fb = run_case(gpu_ctx, monkeypatch, ones_streams(True), 32, {"FB_MAX": 0}, min_count=1, sel=ALL)
    assert fb == 1 and r["stats"].buckets == 2
    assert ONES_CODE in r["keys"].tolist()
