"""The SDK lookup in read batches (hga_lookup_begin / _add_reads / _finish) on the MI355X: every result array
and size equals oracle.construct_indices on the concatenated reads, however the reads are cut into batches;
the hit arrays keep their contents when they grow; the slots are as large as hga_lookup_batch_estimate says;
the state rules of include/hga.h; connections and spanning-tree tails on a batched result."""
import functools
import os
import random

import numpy as np
import pytest

import oracle
import treetails_ref as tt
from test_lookup_gpu import NAMES, random_case

pytestmark = pytest.mark.gpu
HGA_ERR_STATE = 4
STATE = f"hga status {HGA_ERR_STATE}:"


def csr(reads):
    return b"".join(reads), np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)


def split_reads(bases, offsets):
    o = [int(x) for x in offsets]
    return [bases[a:b] for a, b in zip(o[:-1], o[1:])]


def feed(ctx, batches, first_id):
    """One session over `batches` (lists of reads) on a ctx with the SDK set loaded."""
    ctx.lookup_begin(first_id)
    for b in batches:
        ctx.lookup_add_reads(*csr(b))
    ctx.lookup_finish()


def check(ctx, reads, k, sdk, first_id, want=None):
    """The nine arrays and the sizes against the oracle on the concatenated reads."""
    if want is None:
        want = oracle.construct_indices(*csr(reads), k, sdk, first_id)
    got = ctx.lookup_fetch()
    for n in NAMES:
        assert np.array_equal(got[n], want[n]), n
    s = ctx.lookup_sizes()
    assert s.n_reads == len(reads)
    assert s.hits == len(want["hit_kid"])
    assert s.firsts == len(want["first_kid"])
    assert s.reads_hit == int((np.diff(want["hit_ptr"]) > 0).sum())
    assert s.windows == sum(max(0, len(r) - k + 1) for r in reads)
    return want


def run(ctx, batches, k, sdk, first_id, want=None):
    ctx.lookup_load(k, sdk)
    feed(ctx, batches, first_id)
    return check(ctx, [r for b in batches for r in b], k, sdk, first_id, want)


def cut(reads, bounds):
    bounds = [0] + list(bounds) + [len(reads)]
    return [reads[a:b] for a, b in zip(bounds[:-1], bounds[1:])]


# ---- partitions of the inputs of test_lookup_random_vs_oracle

@functools.lru_cache(maxsize=None)
def partition_case(k):
    bases, offsets, sdk = random_case(k, 700, 200, k, "ACGTACGTACGTNa", 3000)
    reads = split_reads(bases, offsets)
    return reads, sdk, oracle.construct_indices(bases, offsets, k, sdk, 7)


def partition_batches(kind, reads):
    if kind == "one":
        return [reads]
    if kind == "single_reads_first":
        return [[r] for r in reads[:40]] + [reads[40:]]
    if kind == "random9":
        return cut(reads, sorted(random.Random(9).sample(range(1, len(reads)), 8)))
    assert kind == "large_then_small"   # the second slot use leaves the first batch's state beyond its end
    return [reads[:400], reads[400:690], reads[690:693], reads[693:]]


@pytest.mark.parametrize("kind", ["one", "single_reads_first", "random9", "large_then_small"])
@pytest.mark.parametrize("k", [1, 15, 19, 32])
def test_partitions(gpu_ctx, k, kind):
    reads, sdk, want = partition_case(k)
    batches = partition_batches(kind, reads)
    assert sum(len(b) for b in batches) == len(reads)
    run(gpu_ctx, batches, k, sdk, 7, want)
    assert gpu_ctx.lookup_batch_stats().batches == len(batches)


@pytest.mark.parametrize("k", [1, 15, 19, 32])
def test_partitions_with_empty_and_hitless_batches(gpu_ctx, k):
    """Batches of no reads, of empty reads only and of N-only reads (no hit), first, in the middle and last."""
    reads, sdk, _ = partition_case(k)
    body = cut(reads, [150, 300, 520])
    empty, blanks, hitless = [], [b"", b"", b""], [b"N" * 90, b"N" * 33, b"n" * 7]
    batches = [empty, blanks, hitless, body[0], hitless, empty, body[1], blanks, body[2], empty, body[3], blanks,
               hitless, empty]
    run(gpu_ctx, batches, k, sdk, 7)
    assert gpu_ctx.lookup_batch_stats().batches == len(batches)


# ---- the cases of test_lookup_edges

EDGES = [
    ([b"", b"", b"ACGT"], [0, 1, 5]),
    ([b"A" * 100, b"", b"T" * 50], [0]),
    ([b"AC", b"G", b"T"], [1, 2, 3]),
    ([b"NNNNNNNN", b"acgtacgt"], [0, 27]),
    ([b"ACGTACGT"], []),   # the empty SDK set
]


@pytest.mark.parametrize("how", ["one_read_per_batch", "cut_after_first"])
@pytest.mark.parametrize("case", range(len(EDGES)))
def test_edges(gpu_ctx, case, how):
    reads, sdk = EDGES[case]
    batches = [[r] for r in reads] if how == "one_read_per_batch" else [reads[:1], reads[1:]]
    run(gpu_ctx, batches, 4, np.array(sdk, np.uint64), 1)


# ---- reads whose every window hits: the per-read sort tiers see global read indices

def test_hit_dense_reads_across_batches(gpu_ctx):
    """The pattern of test_lookup_hit_dense_reads.  The read with > 16 384 hits (radix_sort_u64 over the whole
    s_key, read bits included) is in the third batch of four; the mid (> 512 hits) and big (> 2 048) segment
    sort tiers are in the second and the fourth.  A batch-local read index in s_key would sort the third
    batch's hits in front of the first's."""
    rng = random.Random(31840)
    k = 15

    def dense(L):
        unit = "".join(rng.choice("ACGT") for _ in range(max(L // 3, k + 1)))
        return (unit * 4)[:L].encode()

    batches = [[dense(300), b"ACGTN" * 10, dense(40)],
               [dense(90), dense(1500), b"", dense(700)],
               [dense(60), dense(25000), dense(45)],
               [dense(5000), b"ACGTN" * 10, dense(2600)]]
    reads = [r for b in batches for r in b]
    pool = set()
    for r in reads:
        pool.update(oracle.kmer_windows(r, k)[0].tolist())
    sdk = np.array(rng.sample(sorted(pool), len(pool)), np.uint64)
    want = run(gpu_ctx, batches, k, sdk, 3)
    per_read = np.diff(want["hit_ptr"])
    assert per_read[8] > 16384 and 512 < per_read[4] <= 2048 and per_read[10] > 2048 and per_read[12] > 2048


# ---- the hit arrays grow with their contents kept

def test_regrowth_keeps_earlier_hits(hga_mod):
    rng = random.Random(5)
    k = 15
    genome = "".join(rng.choice("ACGT") for _ in range(4000))
    sdk = np.unique(oracle.kmer_windows(genome.encode(), k)[0])
    batches = []
    for j in range(64):   # batch j: j + 1 reads of 100 bases, every window a hit
        batches.append([genome[s:s + 100].encode() for s in (rng.randrange(0, 3900) for _ in range(j + 1))])
    with hga_mod.Ctx(int(os.environ.get("HGA_DEVICE", "0"))) as ctx:   # fresh: its hit arrays start empty
        want = run(ctx, batches, k, sdk, 1)
        st = ctx.lookup_batch_stats()
    assert len(want["hit_kid"]) > 100_000
    assert st.batches == 64 and st.regrowths >= 2
    assert st.result_bytes >= 24 * len(want["hit_kid"])
    assert st.host_waits <= st.batches + 1


# ---- the slots are what the estimate says

def test_slot_memory_follows_the_batch_size(hga_mod):
    rng = random.Random(6)
    k = 19
    genome = "".join(rng.choice("ACGT") for _ in range(30_000))
    sdk = np.unique(oracle.kmer_windows(genome.encode(), k)[0])[::5]
    reads = [genome[s:s + 128].encode() for s in (rng.randrange(0, 29_800) for _ in range(32 * 32 - 10))]
    want = oracle.construct_indices(*csr(reads), k, sdk, 1)
    seen = {}
    for per in (32, 16):   # 32 batches of <= 4 096 bases, then the same reads as 64 batches of half the size
        batches = [reads[i:i + per] for i in range(0, len(reads), per)]
        assert len(batches) == 1024 // per and max(sum(map(len, b)) for b in batches) == 128 * per
        with hga_mod.Ctx(int(os.environ.get("HGA_DEVICE", "0"))) as ctx:
            run(ctx, batches, k, sdk, 1, want)
            st = ctx.lookup_batch_stats()
            assert st.slot_bytes == ctx.lookup_batch_estimate(128 * per, per)
            assert st.batches == len(batches) and st.reads == len(reads) and st.bases == 128 * len(reads)
            assert st.host_waits <= st.batches + 1
            seen[per] = st.slot_bytes
            one_shot = ctx.lookup_batch_estimate(128 * len(reads), len(reads))
        assert st.slot_bytes < one_shot
    assert seen[16] < seen[32]


# ---- state rules

def small_case():
    reads = [b"ACGTACGTAC", b"TTTTACGTAA", b"", b"GGGACGTACG"]
    return reads, np.array([27, 108, 6], np.uint64)   # k = 4


def test_state_rules(hga_mod):
    reads, sdk = small_case()
    with hga_mod.Ctx(int(os.environ.get("HGA_DEVICE", "0"))) as ctx:
        with pytest.raises(hga_mod.HgaError, match=STATE):
            ctx.lookup_begin(1)                       # no SDK set
        with pytest.raises(hga_mod.HgaError, match=STATE):
            ctx.lookup_batch_stats()                  # no session yet
        ctx.lookup_load(4, sdk)
        with pytest.raises(hga_mod.HgaError, match=STATE):
            ctx.lookup_add_reads(*csr(reads))         # no begin
        with pytest.raises(hga_mod.HgaError, match=STATE):
            ctx.lookup_finish()
        ctx.lookup_begin(5)
        ctx.lookup_add_reads(*csr(reads[:2]))
        for call in (ctx.lookup_run, ctx.lookup_fetch, ctx.lookup_sizes, lambda: ctx.lookup_load(4, sdk),
                     lambda: ctx.connections_run(min_score=1), lambda: ctx.hll_registers(4)):
            with pytest.raises(hga_mod.HgaError, match=STATE + ".*session is open"):
                call()
        # an invalid batch leaves the session as it was
        with pytest.raises(hga_mod.HgaError, match="hga status 1:"):
            ctx.lookup_add_reads(b"ACGT", np.array([0, 3, 2], np.uint64))
        ctx.lookup_add_reads(*csr(reads[2:]))
        ctx.lookup_finish()
        check(ctx, reads, 4, sdk, 5)
        with pytest.raises(hga_mod.HgaError, match=STATE):
            ctx.hll_registers(4)                      # no reads are resident after finish
        with pytest.raises(hga_mod.HgaError, match=STATE):
            ctx.lookup_run()
        with pytest.raises(hga_mod.HgaError, match=STATE):
            ctx.lookup_add_reads(*csr(reads))         # the session is closed
        check(ctx, reads, 4, sdk, 5)                  # and the result is still there


def test_begin_twice_restarts(gpu_ctx):
    reads, sdk = small_case()
    gpu_ctx.lookup_load(4, sdk)
    gpu_ctx.lookup_begin(1)
    gpu_ctx.lookup_add_reads(*csr([b"ACGTACGTACGTACGT"] * 50))
    gpu_ctx.lookup_begin(9)
    assert gpu_ctx.lookup_batch_stats().batches == 0
    gpu_ctx.lookup_add_reads(*csr(reads[:1]))
    gpu_ctx.lookup_add_reads(*csr(reads[1:]))
    gpu_ctx.lookup_finish()
    check(gpu_ctx, reads, 4, sdk, 9)


def test_set_reads_returns_to_one_shot(gpu_ctx, hga_mod):
    reads, sdk = small_case()
    gpu_ctx.lookup_load(4, sdk)
    gpu_ctx.lookup_begin(1)
    gpu_ctx.lookup_add_reads(*csr([b"ACGTACGTACGTACGT"] * 50))
    gpu_ctx.lookup_set_reads(*csr(reads), 2)
    with pytest.raises(hga_mod.HgaError, match=STATE):
        gpu_ctx.lookup_finish()
    gpu_ctx.lookup_run()
    check(gpu_ctx, reads, 4, sdk, 2)
    assert len(gpu_ctx.hll_registers(4)) == 1024      # the reads are resident again


def test_second_session_with_another_sdk_set(gpu_ctx):
    reads15, sdk15, want15 = partition_case(15)
    run(gpu_ctx, cut(reads15, [100, 450]), 15, sdk15, 7, want15)
    reads19, sdk19, want19 = partition_case(19)
    run(gpu_ctx, cut(reads19, [30, 31, 600]), 19, sdk19, 7, want19)


# ---- what follows a lookup works on a batched result

@pytest.fixture(scope="module")
def three_batch_ctx(hga_mod):
    rng = np.random.default_rng(3)
    k = 15
    gnm = bytes(rng.choice(list(b"ACGT"), 5000).tolist())
    starts = rng.integers(0, 5000 - 120, 400)
    lens = rng.integers(30, 120, 400)
    reads = [gnm[s:s + n] for s, n in zip(starts.tolist(), lens.tolist())]
    sdk = np.unique(oracle.kmer_windows(gnm, k)[0])[::3]
    ctx = hga_mod.Ctx(int(os.environ.get("HGA_DEVICE", "0")))
    idx = run(ctx, cut(reads, [120, 290]), k, sdk, 7)
    yield ctx, idx, lens
    ctx.close()


def test_connections_on_a_batched_result(three_batch_ctx):
    ctx, idx, _ = three_batch_ctx
    got = ctx.connections(min_score=1)
    exp = oracle.connections(idx, min_score=1, first_read_id=7)
    assert len(exp[0]) > 100
    for a, b, name in zip(got, exp, ("x", "y", "score", "is_good")):
        assert np.array_equal(a, b), name


def test_tree_tails_read_lengths_on_a_batched_result(three_batch_ctx):
    """read_length = NULL: hga_tree_tails takes the lengths from the session's cumulative host offsets."""
    ctx, _, lens = three_batch_ctx
    rng = np.random.default_rng(8)
    ids = 7 + rng.permutation(400)[:60]
    tree = [(int(ids[a]), int(ids[b])) for a, b in tt.random_tree(60, rng)]
    ov = rng.integers(0, 25, len(tree)).astype(np.int32)
    by_id = {7 + i: int(l) for i, l in enumerate(lens)}
    got = ctx.tree_tails([tree], ov, None, 150)
    want = tt.tree_tails([tree], ov.tolist(), by_id, 150)
    assert got[0][0].tolist() == want[0].left and got[1][0].tolist() == want[0].right
    assert tuple(map(int, got[2][0])) == want[0].ends
    assert len(tree) == 59 and (want[0].left or want[0].right)
