"""Counting in key-range passes (hga_count_set_passes / _estimate / _get_pass_stats) on the MI355X,
through the C ABI: for any pass count the rows, both dumps, the histogram, the export, the flags and
n_discr are the oracle's, bit for bit.  The shapes are the smallest at which the pass logic can still
go wrong: every key width / element type / compile-time-k variant of kc_bin1, 1-5 files, every
size-selected path inside a pass, several super-tiles and spill blocks, the budget choice, re-runs,
dump rows, a key range heavier than its pass's buffers, and a ctx with a communicator."""
import functools
import random

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

HGA_ERR_OOM, HGA_ERR_STATE = 3, 4


@pytest.fixture
def pctx(gpu_ctx):
    """The shared ctx; the pass setting is the default again afterwards."""
    yield gpu_ctx
    gpu_ctx.count_set_passes(0, 0)


def run_gpu(ctx, streams, k, lower, upper, min_count=2, thr=oracle.THRESHOLDS):
    ctx.count_begin(k, len(streams))
    for f, s in enumerate(streams):
        ctx.count_add(f, s)
    ctx.count_run(min_count)
    return fetch(ctx, len(streams), lower, upper, thr)


def fetch(ctx, n_files, lower, upper, thr=oracle.THRESHOLDS):
    keys, counts = ctx.rows()
    hist = ctx.spec_hist(thr) if len(keys) else np.zeros((0, 3), np.int64)
    sel, flags, nd = ctx.select(lower, upper)
    dumps = [ctx.dump(f) for f in range(n_files)]
    return {"keys": keys, "counts": counts, "hist": hist, "selected": sel, "flags": flags, "n_discr": nd,
            "dumps": dumps, "stats": ctx.count_stats(), "pass_stats": ctx.count_pass_stats()}


def assert_same(g, o):
    assert np.array_equal(g["keys"], o["keys"])
    assert np.array_equal(g["counts"], o["counts"])
    assert np.array_equal(g["hist"], o["hist"])
    assert np.array_equal(g["selected"], o["selected"])
    assert g["n_discr"] == o["n_discr"]
    if "dumps" in o:
        for (gk, gc), (ok, oc) in zip(g["dumps"], o["dumps"]):
            assert np.array_equal(gk, ok) and np.array_equal(gc, oc)
    # the discriminative flags: a selected row with exactly one file present
    nz = (o["counts"] > 0).sum(1)
    assert np.array_equal(g["flags"].astype(bool), nz[np.searchsorted(o["keys"], o["selected"])] == 1)


def assert_equal_runs(a, b):
    for name in ("keys", "counts", "hist", "selected", "flags"):
        assert np.array_equal(a[name], b[name]), name
    assert a["n_discr"] == b["n_discr"]
    for (ak, ac), (bk, bc) in zip(a["dumps"], b["dumps"]):
        assert np.array_equal(ak, bk) and np.array_equal(ac, bc)


def random_streams(seed, n_files, n_reads, rlen, alphabet="ACGT", dup=0.5):
    rng = random.Random(seed)
    out = []
    base = ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, rlen))) for _ in range(n_reads)]
    for f in range(n_files):
        rs = [r for r in base if rng.random() < 0.7] + \
             ["".join(rng.choice(alphabet) for _ in range(rng.randint(0, rlen))) for _ in range(n_reads // 3)]
        rs += rs[: int(len(rs) * dup)]
        rng.shuffle(rs)
        out.append("\n".join(rs).encode())
    return out


@functools.lru_cache(maxsize=None)
def small_case(k):
    """test_count_random_vs_oracle's shape, and its oracle (computed once per k)."""
    streams = random_streams(k, 2, 400, 120, "ACGTACGTACGTNacgt")
    return streams, oracle.count_pipeline(streams, k, 2, 6)


@functools.lru_cache(maxsize=None)
def c1_case():
    """BASELINE config 1's shape (500 kb pair at 30x, 26.4 M instances) and the multi-threaded oracle."""
    import hga
    ga = hga.gen_genome(500_000, 1)
    gb = hga.gen_haplotype(ga, 0.03, 0, 2)
    streams = [hga.gen_art(ga, 100_000, 150, 3).seq, hga.gen_art(gb, 100_000, 150, 4).seq]
    o = {"dumps": [oracle.count_stream(s, 19, 2, threads=8) for s in streams]}
    o["keys"], o["counts"] = oracle.merge(o["dumps"])
    o["hist"] = oracle.specificity(o["counts"], oracle.THRESHOLDS)
    o["selected"], o["n_discr"] = oracle.select(o["keys"], o["counts"], 10, 25)
    return streams, o


# 1. forced P over the key widths: clamping at tiny k, u32 and u64 level-1 elements, the compile-time-k
#    variants 15 / 17 / 19 / 21 and the runtime-k one, k = 32's all-ones key under pass bits
@pytest.mark.parametrize("P", [2, 4, 8])
@pytest.mark.parametrize("k", [1, 2, 5, 12, 15, 16, 17, 19, 21, 22, 31, 32])
def test_passes_forced_over_key_widths(pctx, k, P):
    streams, o = small_case(k)
    pctx.count_set_passes(P, 0)
    r = run_gpu(pctx, streams, k, 2, 6)
    assert_same(r, o)
    assert r["pass_stats"].passes <= P
    if k >= 12:
        assert r["pass_stats"].passes == P


# 2. files and the per-file drop (F >= 3: the generic kc_count)
@pytest.mark.parametrize("n_files", [1, 2, 3, 5])
@pytest.mark.parametrize("min_count", [1, 2, 3])
def test_passes_files_and_min(pctx, n_files, min_count):
    streams = random_streams(100 + n_files, n_files, 300, 100)
    o = oracle.count_pipeline(streams, 19, 2, 9, min_count=min_count)
    pctx.count_set_passes(4, 0)
    r = run_gpu(pctx, streams, 19, 2, 9, min_count=min_count)
    assert_same(r, o)
    assert r["pass_stats"].passes == 4


# 3. the size-selected paths inside a pass (HGA_B1_BRANCHFREE is a compile-time switch: not here)
@pytest.mark.parametrize("env", [{"HGA_FB_MIN": "12"}, {"HGA_SPLIT3_FORCE": "3"}, {"HGA_CS_LAZY": "0"}, {"HGA_CS_LAZY": "1"},
                                 {"HGA_COUNT_LEGACY": "1"}, {"HGA_LAYOUT_T": "1"},
                                 {"HGA_FB_MIN": "12", "HGA_SPLIT3_FORCE": "3", "HGA_CS_LAZY": "1"}],
                         ids=lambda e: "+".join(f"{k[4:]}={v}" for k, v in e.items()))
def test_passes_size_selected_paths(pctx, monkeypatch, env):
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    streams, o = small_case(19)
    pctx.count_set_passes(4, 0)
    r = run_gpu(pctx, streams, 19, 2, 6)
    assert_same(r, o)
    assert r["pass_stats"].passes == 4
    if "HGA_FB_MIN" in env:
        assert r["stats"].buckets >= 4096


# 4. several super-tiles per file and spill blocks
@pytest.mark.parametrize("P", [2, 8])
def test_passes_c1_scale_vs_oracle(pctx, P):
    streams, o = c1_case()
    pctx.count_set_passes(P, 0)
    r = run_gpu(pctx, streams, 19, 10, 25)
    assert_same(r, o)
    assert r["pass_stats"].passes == P
    assert r["stats"].instances == 2 * 100_000 * 132


# 5. conservation and the pass statistics
def test_passes_conservation_and_stats(pctx):
    streams, _ = c1_case()
    pctx.count_set_passes(8, 0)
    pctx.count_begin(19, 1)
    pctx.count_add(0, streams[0])
    pctx.count_run(1)
    st, ps = pctx.count_stats(), pctx.count_pass_stats()
    keys, counts = pctx.rows()
    assert st.instances == 100_000 * 132
    assert int(counts.astype(np.uint64).sum()) == st.instances
    assert np.all(keys[1:] > keys[:-1])
    assert ps.passes == 8
    assert ps.min_pass_instances <= st.instances / ps.passes <= ps.max_pass_instances
    assert ps.work_bytes == pctx.count_estimate(1, 8)


# 6. the budget picks P; the estimate is the run's request
def test_passes_budget_mode(pctx):
    streams, o = c1_case()
    pctx.count_begin(19, 2)
    for f, s in enumerate(streams):
        pctx.count_add(f, s)
    e1 = pctx.count_estimate(2, 1)
    pctx.count_set_passes(0, e1 // 3)
    pctx.count_run(2)
    r = fetch(pctx, 2, 10, 25)
    assert_same(r, o)
    ps = r["pass_stats"]
    print(f"one-pass estimate {e1}, budget {e1 // 3}: passes {ps.passes}, work_bytes {ps.work_bytes}")
    assert ps.passes >= 4
    assert ps.work_bytes <= e1 // 3
    assert pctx.count_estimate(2, ps.passes) == ps.work_bytes
    assert pctx.count_estimate(2, 0) == ps.work_bytes
    pctx.count_set_passes(1, 0)
    pctx.count_run(2)
    r1 = fetch(pctx, 2, 10, 25)
    assert r1["pass_stats"].passes == 1 and r1["pass_stats"].work_bytes == e1
    assert_equal_runs(r1, r)


# 7. re-runs on one ctx, and dump rows
def test_passes_rerun(pctx):
    streams, o = small_case(19)
    runs = []
    for P in (4, 4, 1, 4):
        pctx.count_set_passes(P, 0)
        if not runs:
            runs.append(run_gpu(pctx, streams, 19, 2, 6))
        else:
            pctx.count_run(2)
            runs.append(fetch(pctx, 2, 2, 6))
        assert runs[-1]["pass_stats"].passes == P
    assert_same(runs[0], o)
    for r in runs[1:]:
        assert_equal_runs(r, runs[0])


def test_passes_dump_rows(pctx):
    streams, _ = small_case(19)
    k0, c0 = oracle.count_stream(streams[0], 19, 2)
    got = []
    for P in (1, 4):
        pctx.count_set_passes(P, 0)
        pctx.count_begin(19, 2)
        pctx.count_add_rows(0, k0[::-1], c0[::-1])
        pctx.count_add(1, streams[1])
        pctx.count_run(2)
        got.append(fetch(pctx, 2, 2, 6))
        assert got[-1]["pass_stats"].passes == P
    assert_equal_runs(got[1], got[0])
    assert_same(got[1], oracle.count_pipeline(streams, 19, 2, 6))


# 8. a key range heavier than its pass's buffers: the oracle's result or HGA_ERR_OOM, nothing else
def heavy_case():
    import hga
    g = hga.gen_genome(400_000, 5)
    return [b"A" * 3_000_000 + b"\n" + g, b"C" * 1_000_000 + b"\n" + g[:200_000]]


def test_passes_heavy_range(pctx, hga_mod):
    """Poly-A and poly-C next to a genome (test_count_level1_overflow_retry's input) at P = 4: one pass
    holds most of the input.  At the base margin that is the heavy-range error (clipped writes, no
    fault), its text naming passes and budget; under a budget of the one-pass request every buffer
    holds the whole input and the result must be the oracle's."""
    streams = heavy_case()
    o = oracle.count_pipeline(streams, 21, 1, 10 ** 9, min_count=1)
    pctx.count_set_passes(4, 0)
    try:
        r = run_gpu(pctx, streams, 21, 1, 10 ** 9, min_count=1)
    except hga_mod.HgaError as e:
        msg = str(e)
        assert msg.startswith(f"hga status {HGA_ERR_OOM}:"), msg
        assert "passes = 4" in msg and "budget" in msg, msg
        print("heavy range at the base margin:", msg)
    else:
        print("heavy range at the base margin: counted")
        assert_same(r, o)
    # the ctx is usable afterwards, and with room for the worst case the count is exact
    pctx.count_set_passes(4, pctx.count_estimate(1, 1))
    pctx.count_run(1)
    r = fetch(pctx, 2, 1, 10 ** 9)
    assert_same(r, o)
    assert r["pass_stats"].passes == 4


# 9. not with a communicator
def test_passes_refused_with_communicator(hga_mod):
    streams, _ = small_case(19)
    with hga_mod.Ctx(0) as ctx:
        ctx.comm_init_host(0, 1, hga_mod.transport_of(lambda send, recv: None, 1))
        ctx.count_begin(19, 2)
        for f, s in enumerate(streams):
            ctx.count_add(f, s)
        ctx.count_set_passes(4, 0)
        with pytest.raises(hga_mod.HgaError) as ei:
            ctx.count_run(2)
        assert str(ei.value).startswith(f"hga status {HGA_ERR_STATE}:") and "communicator" in str(ei.value)
        ctx.count_set_passes(1, 0)   # one pass still runs there
        ctx.count_run(2)
        assert ctx.count_pass_stats().passes == 1
