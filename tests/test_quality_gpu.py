"""hga_connections_quality on the MI355X: plot_connection_quality's two histograms
(src/clustering/ReadClusteringEngine.cpp:19-34 over every row, :102-124 over the best row per candidate) of
explicit ordered lists and of the ctx's own connection results, against a dict restatement written here; the
error and state rules; and bin/categorization -d piping the five debug plots through HGA_PLOT_CMD."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import tailsets_ref as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hybrid-genome-assembler_amd", "bin")
GOLD = os.path.join(ROOT, "tests", "golden")
HGA_ERR_INVALID, HGA_ERR_STATE = 1, 4
DEVICE = int(os.environ.get("HGA_DEVICE", "0"))
V = 300   # reads of the small lookup: ReadIDs 1..V


def restatement(x, y, score, good, per_candidate):
    """(scores ascending, good counts, bad counts) as the reference's two loops count them."""
    rows = list(zip((int(v) for v in y), (int(v) for v in score), (bool(v) for v in good)))
    if per_candidate:   # :103-109: the entry starts at {0, false} and is replaced only on a strictly larger score
        best = {}
        for yy, s, g in rows:
            cur = best.setdefault(yy, (0, False))
            if s > cur[0]:
                best[yy] = (s, g)
        counted = list(best.values())
    else:
        counted = [(s, g) for _, s, g in rows]
    hist = {}
    for s, g in counted:
        hist.setdefault(s, [0, 0])[0 if g else 1] += 1
    scores = sorted(hist)
    return scores, [hist[s][0] for s in scores], [hist[s][1] for s in scores]


def check(ctx, x, y, score, good, vertex_class=None, first_id=1):
    x, y = np.asarray(x, np.uint32), np.asarray(y, np.uint32)
    score = np.asarray(score, np.uint64)
    flags = np.zeros(len(x), np.uint8) if good is None else np.asarray(good, np.uint8)
    if vertex_class is not None:
        vc = np.asarray(vertex_class, np.int32)
        flags = vc[x - first_id] == vc[y - first_id]
    for per_candidate in (False, True):
        s, g, b = ctx.connections_quality(x, y, score, good, per_candidate, vertex_class)
        assert s.dtype == g.dtype == b.dtype == np.uint64
        want = restatement(x, y, score, flags, per_candidate)
        assert (s.tolist(), g.tolist(), b.tolist()) == tuple(want), per_candidate
        assert all(gi + bi > 0 for gi, bi in zip(g.tolist(), b.tolist()))


def load_small(ctx, n_reads):
    rng = np.random.default_rng(3)
    gnm = bytes(rng.choice(list(b"ACGT"), 4000).tolist())
    starts = rng.integers(0, 4000 - 60, n_reads)
    lens = rng.integers(30, 60, n_reads)
    bases = b"".join(gnm[s:s + n] for s, n in zip(starts.tolist(), lens.tolist()))
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    codes, _ = oracle.kmer_windows(gnm, 15)
    ctx.lookup_load(15, np.unique(codes)[::5])
    ctx.lookup_set_reads(bases, offsets, 1)
    ctx.lookup_run()
    assert ctx.lookup_sizes().n_reads == n_reads


@pytest.fixture(scope="module")
def small_ctx(hga_mod):
    ctx = hga_mod.Ctx(DEVICE)
    load_small(ctx, V)
    yield ctx
    ctx.close()


def random_list(rng, n, n_scores, max_score=50):
    """n rows in result order with about n_scores distinct scores, ids in 1..V."""
    pool = np.sort(rng.choice(np.arange(1, max(max_score, n_scores) + 1), n_scores, replace=False))[::-1]
    score = np.sort(rng.choice(pool, n))[::-1].astype(np.uint64) if n else np.zeros(0, np.uint64)
    return (rng.integers(1, V + 1, n).astype(np.uint32), rng.integers(1, V + 1, n).astype(np.uint32), score,
            rng.integers(0, 2, n).astype(np.uint8))


def test_tile_constant(hga_mod):
    assert hga_mod.lib().hga_connections_quality_tile() == hga_mod.QUALITY_TILE


def test_sizes_around_the_tile(small_ctx, hga_mod):
    T = hga_mod.QUALITY_TILE
    rng = np.random.default_rng(11)
    for n in (0, 1, T - 1, T, T + 1, 3 * T + 5):
        check(small_ctx, *random_list(rng, n, 7))
    s, g, b = small_ctx.connections_quality(*random_list(rng, 0, 1))
    assert len(s) == len(g) == len(b) == 0


def test_one_run_over_tiles_and_all_distinct(small_ctx, hga_mod):
    T = hga_mod.QUALITY_TILE
    rng = np.random.default_rng(12)
    # one score in every row: one run over more than two tiles
    n = 2 * T + 77
    x, y, _, g = random_list(rng, n, 1)
    check(small_ctx, x, y, np.full(n, 1, np.uint64), g)
    # every score distinct: every run has length 1
    n = 2 * T + 3
    x, y, _, g = random_list(rng, n, 1)
    check(small_ctx, x, y, np.arange(n, 0, -1).astype(np.uint64) * 3, g)


def test_run_boundary_on_a_tile_edge(small_ctx, hga_mod):
    T = hga_mod.QUALITY_TILE
    rng = np.random.default_rng(13)
    n = 3 * T
    x, y, _, g = random_list(rng, n, 1)
    score = np.concatenate([np.full(T, 9), np.full(T, 5), np.full(T - 1, 2), [1]]).astype(np.uint64)
    check(small_ctx, x, y, score, g)
    # ... and one row to either side of it
    for cut in (T - 1, T + 1):
        check(small_ctx, x, y, np.concatenate([np.full(cut, 9), np.full(n - cut, 4)]).astype(np.uint64), g)


def test_wide_scores_null_flags_and_classes(small_ctx, hga_mod):
    rng = np.random.default_rng(14)
    n = 700
    x, y, _, g = random_list(rng, n, 1)
    score = np.sort(rng.choice(np.array([2 ** 63, 2 ** 63 - 1, 2 ** 40, 2 ** 40 - 1, 2 ** 32, 17, 1, 0], np.uint64), n))[::-1]
    check(small_ctx, x, y, score, g)
    check(small_ctx, x, y, score, None)                          # is_good NULL: all 0
    cls = rng.integers(-2, 3, V).astype(np.int32)
    check(small_ctx, x, y, score, g, vertex_class=cls)           # the classes override the stored flags
    check(small_ctx, x, y, score, None, vertex_class=cls)


def test_one_candidate_in_every_row(small_ctx, hga_mod):
    T = hga_mod.QUALITY_TILE
    rng = np.random.default_rng(15)
    n = 3 * T + 5
    x, _, score, g = random_list(rng, n, 9)
    check(small_ctx, x, np.full(n, 7, np.uint32), score, g)      # one word takes every offer
    s, gg, b = small_ctx.connections_quality(x, np.full(n, 7, np.uint32), score, g, True)
    assert s.tolist() == [int(score[0])] and int(gg[0] + b[0]) == 1


def test_same_candidate_and_score_the_earlier_position_wins(small_ctx):
    for flags in ((1, 0), (0, 1)):
        s, g, b = small_ctx.connections_quality([1, 2], [5, 5], [8, 8], flags, True)
        assert (s.tolist(), g.tolist(), b.tolist()) == ([8], [flags[0]], [1 - flags[0]])
    # across a wave and across workgroups
    n = 5000
    x = np.arange(n, dtype=np.uint32) % V + 1
    y = np.full(n, 9, np.uint32)
    y[1::2] = 10
    g = np.zeros(n, np.uint8)
    g[0] = 1
    check(small_ctx, x, y, np.full(n, 4, np.uint64), g)
    assert small_ctx.connections_quality(x, y, np.full(n, 4, np.uint64), g, True)[1].tolist() == [1]
    # a kept row of score 0 is bad whatever its flag (:105-108)
    s, g, b = small_ctx.connections_quality([1], [2], [0], [1], True)
    assert (s.tolist(), g.tolist(), b.tolist()) == ([0], [0], [1])


def raw(hga_mod, ctx, x, y, s, g, n, per_candidate=0, vc=None):
    p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))
    ps, pg, pb = (C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint64)())
    r = C.c_uint64(12345)
    st = hga_mod.lib().hga_connections_quality(ctx._h, p(x, C.c_uint32), p(y, C.c_uint32), p(s, C.c_uint64), p(g, C.c_uint8),
                                               n, per_candidate, p(vc, C.c_int32), C.byref(ps), C.byref(pg), C.byref(pb),
                                               C.byref(r))
    if st == 0:
        for q in (ps, pg, pb):
            hga_mod.lib().hga_free(q)
    return st, r.value


def test_one_read_lookup(hga_mod):
    """V = 1: the only legal rows are self pairs, which count like any row (the plots never look at x); any
    other id is outside the lookup's reads."""
    with hga_mod.Ctx(DEVICE) as ctx:
        load_small(ctx, 1)
        for per_candidate, want in ((False, ([3, 4], [0, 1], [2, 0])), (True, ([4], [1], [0]))):
            s, g, b = ctx.connections_quality([1, 1, 1], [1, 1, 1], [4, 3, 3], [1, 0, 0], per_candidate)
            assert (s.tolist(), g.tolist(), b.tolist()) == want
        one, two, sc = np.array([1], np.uint32), np.array([2], np.uint32), np.array([3], np.uint64)
        assert raw(hga_mod, ctx, one, two, sc, None, 1) == (HGA_ERR_INVALID, 12345)
        assert raw(hga_mod, ctx, two, one, sc, None, 1) == (HGA_ERR_INVALID, 12345)
        assert raw(hga_mod, ctx, one, one, sc, None, 1) == (0, 1)


def test_errors_and_state(hga_mod):
    rng = np.random.default_rng(16)
    x, y, s, g = random_list(rng, 500, 6)
    with hga_mod.Ctx(DEVICE) as ctx:
        assert raw(hga_mod, ctx, x, y, s, g, len(x))[0] == HGA_ERR_STATE          # before hga_lookup_run
        assert raw(hga_mod, ctx, None, None, None, None, 0)[0] == HGA_ERR_STATE
        load_small(ctx, V)
        assert raw(hga_mod, ctx, None, None, None, None, 0)[0] == HGA_ERR_STATE   # no connection result yet
        check(ctx, x, y, s, g)
        # an unsorted list
        bad = s.copy()
        bad[200], bad[201] = 1, 2
        assert bad[200] < bad[201]
        assert raw(hga_mod, ctx, x, y, bad, g, len(x)) == (HGA_ERR_INVALID, 12345)
        # an id outside the lookup's reads, on either side
        for ids in (0, V + 1, 2 ** 32 - 1):
            for side in (0, 1):
                b = [x.copy(), y.copy()]
                b[side][321] = ids
                assert raw(hga_mod, ctx, b[0], b[1], s, g, len(x)) == (HGA_ERR_INVALID, 12345)
        # every NULL mix but "all three NULL" and "none NULL"
        for mask in range(1, 7):
            a = [None if mask >> i & 1 else v for i, v in enumerate((x, y, s))]
            assert raw(hga_mod, ctx, a[0], a[1], a[2], g, len(x)) == (HGA_ERR_INVALID, 12345)
        assert raw(hga_mod, ctx, x, y, s, g, 2 ** 32 - 1)[0] == HGA_ERR_INVALID   # the forest's limit, before a row is read
        with pytest.raises(ValueError):
            ctx.connections_quality(x, y[:-1], s)
        with pytest.raises(ValueError):
            ctx.connections_quality(x, y, s, vertex_class=np.zeros(V + 1, np.int32))
        check(ctx, x, y, s, g)                                                    # the ctx is still usable
        # a connection result: the NULL form answers; hga_lookup_run ends its life
        n = ctx.connections_run(min_score=1)
        assert raw(hga_mod, ctx, None, None, None, None, 0)[0] == 0
        rows = ctx.connections_range(0, n)
        check(ctx, x, y, s, g)                                                    # an explicit call leaves it alone
        assert all(np.array_equal(a, b) for a, b in zip(rows, ctx.connections_range(0, n)))
        ctx.lookup_run()
        assert raw(hga_mod, ctx, None, None, None, None, 0)[0] == HGA_ERR_STATE


def quality_of_result(ctx, n, vertex_class=None, first_id=1):
    """Both modes on the ctx's result of n rows against the restatement over the fetched rows, twice."""
    x, y, s, g = ctx.connections_range(0, n)
    assert len(x) == n
    flags = g
    if vertex_class is not None:
        vc = np.asarray(vertex_class, np.int32)
        flags = vc[x - first_id] == vc[y - first_id]
    out = []
    for per_candidate in (False, True):
        want = restatement(x, y, s, flags, per_candidate)
        for _ in range(2):   # the scratch is reused
            got = ctx.connections_quality(per_candidate=per_candidate, vertex_class=vertex_class)
            assert tuple(a.tolist() for a in got) == tuple(want)
        out.append(want)
    assert all(np.array_equal(a, b) for a, b in zip((x, y, s, g), ctx.connections_range(0, n)))   # only read
    return out


def test_on_a_connection_result(gpu_ctx, hga_mod):
    g = np.load(os.path.join(GOLD, "lookup_golden.npz"))
    rec = hga_mod.load_records([os.path.join(GOLD, p) for p in ("reads_a.fq", "reads_b.fq", "reads_c.fa")], True)
    gpu_ctx.lookup_load(19, g["sdk_keys_id_order"])
    gpu_ctx.lookup_set_reads(rec["bases"], rec["offsets"], 1)
    gpu_ctx.lookup_run()
    n = gpu_ctx.connections_run(min_score=1, categories=rec["category"])
    assert n > hga_mod.QUALITY_TILE
    every, best = quality_of_result(gpu_ctx, n)
    assert sum(every[1]) > 0 and sum(every[2]) > 0 and sum(every[1]) + sum(every[2]) == n
    assert sum(best[1]) + sum(best[2]) == len(set(gpu_ctx.connections_range(0, n)[1].tolist()))
    # the classes of the categories give the stored flags again
    assert quality_of_result(gpu_ctx, n, vertex_class=np.asarray(rec["category"], np.int32)) == [every, best]


def test_on_a_merged_component_state(gpu_ctx, hga_mod):
    ref = tr.case_b(hga_mod)
    c = ref.c
    gpu_ctx.lookup_load(c.k, c.sdk)
    gpu_ctx.lookup_set_reads(c.bases, c.offsets, c.first_id)
    gpu_ctx.lookup_run()
    gpu_ctx.components_merge(c.steps[1].groups)
    pivots = np.array(sorted(set(c.steps[1].survivors) | set(c.rest)), np.uint32)
    n = gpu_ctx.components_connections(pivots, 1)
    assert n > 100
    n_reads = gpu_ctx.lookup_sizes().n_reads
    cls = (np.arange(n_reads) % 3).astype(np.int32)
    every, best = quality_of_result(gpu_ctx, n, vertex_class=cls, first_id=c.first_id)
    assert sum(every[1]) > 0 and sum(every[2]) > 0
    stored = quality_of_result(gpu_ctx, n)   # hga_components_connections stores is_good = 0
    assert sum(stored[0][1]) == 0 and sum(stored[0][2]) == n


def test_profile_labels(small_ctx):
    rng = np.random.default_rng(17)
    x, y, s, g = random_list(rng, 3000, 5)
    small_ctx.profile(True)
    try:
        small_ctx.profile_reset()
        small_ctx.connections_quality(x, y, s, g, True)
        assert [small_ctx.profile_get(k)[1] for k in ("cq_first", "cq_tile", "cq_scan", "cq_runs")] == [1, 1, 1, 1]
        small_ctx.profile_reset()
        small_ctx.connections_quality(x, y, s, g, False)
        assert [small_ctx.profile_get(k)[1] for k in ("cq_first", "cq_tile", "cq_scan", "cq_runs")] == [0, 1, 1, 1]
    finally:
        small_ctx.profile(False)


# ---------------------------------------------------------------- bin/categorization -d with HGA_PLOT_CMD
def kmer_str(code, k):
    return "".join("ACGT"[(int(code) >> (2 * (k - 1 - i))) & 3] for i in range(k))


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory, hga_mod):
    """test_cli_gpu.py's two-haplotype case, and the host engine's plots for it (tests/test_plots.py checks
    those against the restatement on the CPU)."""
    tmp = tmp_path_factory.mktemp("quality_cli")
    k = 15
    ga = hga_mod.gen_genome(40_000, 5)
    gb = hga_mod.gen_haplotype(ga, 0.02, 0, 6)
    paths = [str(tmp / "hapA.fa"), str(tmp / "hapB.fa")]
    hga_mod.write_nanosim_fasta(ga, "hapA", 180, 7, paths[0])
    hga_mod.write_nanosim_fasta(gb, "hapB", 180, 8, paths[1])
    ka, _ = oracle.kmer_windows(ga, k)
    kb, _ = oracle.kmer_windows(gb, k)
    sdk = np.setxor1d(np.unique(ka), np.unique(kb))
    (tmp / "sdk.txt").write_text("".join(kmer_str(c, k) + "\n" for c in sdk))
    rec = hga_mod.load_records(paths, True)
    idx = oracle.construct_indices(rec["bases"], rec["offsets"], k, sdk)
    cfg = hga_mod.cluster_config(5, -1, 0.15, 0, 8, 10, 1, 16)
    plots = []
    hga_mod.cluster_host(rec["bases"], rec["offsets"], np.asarray(rec["category"], np.int32), idx, int(rec["meta"][-1][4]),
                         cfg, True, start=rec["start"], end=rec["end"], plots=plots)
    assert [kind for kind, _ in plots] == ["connection_histogram", "component_coverage", "connection_histogram",
                                           "component_coverage"]
    return tmp, paths, plots


def run_cli(tmp, paths, name, plot_dir=None, gpus=1, **env_add):
    env = dict(os.environ, HGA_TIMING="1")
    for var in ("HGA_HOST_CONNECTIONS", "HGA_HOST_OVERLAPS", "HGA_DEVICE_SETS", "HGA_SETS_BYTES", "HGA_DEVICE_TAILS",
                "HGA_DEVICE_FOREST", "HGA_DEVICE_ENRICH", "HGA_PLOT_CMD", "HGA_PLOT_KIND", "HGA_PLOT_SEQ"):
        env.pop(var, None)
    env.update(env_add)
    if plot_dir is not None:
        os.makedirs(plot_dir)
        env["HGA_PLOT_CMD"] = f"cat > {plot_dir}/$HGA_PLOT_SEQ.$HGA_PLOT_KIND.txt"
    out = subprocess.run([os.path.join(BIN, "categorization"), *paths, "-k", str(tmp / "sdk.txt"), "-d", "-o",
                          str(tmp / name), "--sc_min_size", "5", "--core_enrichment", "8", "--tail_amplification", "10",
                          "--gpus", str(gpus)], capture_output=True, text=True, cwd=tmp, env=env, timeout=300)
    assert out.returncode == 0, out.stderr
    timing = dict(ln.split()[1:3] for ln in out.stderr.splitlines() if ln.startswith("hga-timing "))
    lines = [ln for ln in out.stdout.splitlines() if " took " not in ln]
    return lines, timing


@pytest.fixture(scope="module")
def cli_plain(cli_case):
    tmp, paths, _ = cli_case
    before = set(os.listdir(tmp))
    lines, timing = run_cli(tmp, paths, "plain")
    assert set(os.listdir(tmp)) - before == {"plain"}   # no plot file appears
    assert (timing["quality.device_calls"], timing["quality.host_calls"]) == ("0", "0")
    return lines


@pytest.mark.parametrize("name,gpus,env,calls", [
    ("default", 1, {}, ("1", "1")),
    ("device", 1, dict(HGA_DEVICE_FOREST="1", HGA_DEVICE_ENRICH="1", HGA_DEVICE_SETS="1"), ("2", "0")),
    ("two", 2, {}, ("0", "2"))])
def test_categorization_pipes_the_plots(cli_case, cli_plain, name, gpus, env, calls):
    """The files HGA_PLOT_CMD's command writes, named by HGA_PLOT_SEQ and HGA_PLOT_KIND, hold the host engine's
    wires byte for byte: by default (the first list stays on the device, the enrichment list is fetched), with
    both lists left on the device (two hga_connections_quality calls) and with two ranks (the gathered list is
    fetched); stdout is that of the run without HGA_PLOT_CMD."""
    tmp, paths, plots = cli_case
    plot_dir = tmp / f"plots_{name}"
    lines, timing = run_cli(tmp, paths, name, plot_dir=plot_dir, gpus=gpus, **env)
    want = {f"{i + 1}.{kind}.txt": wire for i, (kind, wire) in enumerate(plots)}
    assert sorted(os.listdir(plot_dir)) == sorted(want)
    for f, wire in want.items():
        assert open(plot_dir / f, newline="").read() == wire, f
    assert lines == cli_plain
    assert (timing["quality.device_calls"], timing["quality.host_calls"]) == calls
