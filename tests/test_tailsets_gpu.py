"""hga_components_overlaps and hga_components_set_scores on the MI355X against tests/tailsets_ref.py
(tests/pyref_cluster.py's Engine on the merge sequences of tests/components_ref.py), their error and
state rules, the KmerID-tiled path of the set scores, and bin/categorization under HGA_DEVICE_SETS=1
against its default run and its host run."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import overlap_ref
import tailsets_ref as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hybrid-genome-assembler_amd", "bin")
HGA_ERR_INVALID, HGA_ERR_STATE = 1, 4


def lookup(ctx, c):
    ctx.lookup_load(c.k, c.sdk)
    ctx.lookup_set_reads(c.bases, c.offsets, c.first_id)
    ctx.lookup_run()


def state_snapshot(ctx):
    sz = ctx.components_sizes()
    return ctx.components_index(), (sz.index_entries, sz.survivors, sz.survivor_kmers, sz.merges)


def same_state(a, b):
    return np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1], b[0][1]) and a[1] == b[1]


def both_orders(st):
    return np.concatenate([st.x, st.y]), np.concatenate([st.y, st.x])


@pytest.fixture
def no_sets_bytes(monkeypatch):
    monkeypatch.delenv("HGA_SETS_BYTES", raising=False)
    return monkeypatch


@pytest.mark.parametrize("make", [tr.case_a, tr.case_b], ids=["A", "B"])
def test_overlaps_follow_the_merges(make, gpu_ctx, hga_mod):
    ref = make(hga_mod)
    c = ref.c
    lookup(gpu_ctx, c)
    for st in ref.steps:
        if st.no:
            gpu_ctx.components_merge(c.steps[st.no].groups)
        before = state_snapshot(gpu_ctx)
        x, y = both_orders(st)
        ov, sh = gpu_ctx.components_overlaps(x, y)
        n = len(st.x)
        assert ov.dtype == np.int32 and sh.dtype == np.uint32
        assert np.array_equal(ov[:n], ov[n:]) and np.array_equal(sh[:n], sh[n:])   # symmetric
        bad = np.flatnonzero((ov[:n] != st.overlap) | (sh[:n] != st.shared))
        assert len(bad) == 0, (st.no, [(int(st.x[i]), int(st.y[i]), int(ov[i]), int(st.overlap[i])) for i in bad[:5]])
        if st.no == 0:   # before any merge: hga_read_overlaps on the same pairs
            rov, rsh = gpu_ctx.read_overlaps(x, y)
            assert np.array_equal(ov, rov) and np.array_equal(sh, rsh)
        # NULL outputs, one at a time
        L = hga_mod.lib()
        u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        only = np.zeros(n, np.int32)
        assert L.hga_components_overlaps(gpu_ctx._h, u32(st.x), u32(st.y), n, only.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0
        assert np.array_equal(only, st.overlap)
        assert same_state(state_snapshot(gpu_ctx), before)
    got = gpu_ctx.lookup_fetch()
    for name, want in c.idx.items():
        if name in got:
            assert np.array_equal(got[name], want), name
    # back to the lookup's state: the last step's pairs read as read-level overlaps again
    gpu_ctx.components_reset()
    x, y = both_orders(ref.steps[-1])
    ov, sh = gpu_ctx.components_overlaps(x, y)
    rov, rsh = gpu_ctx.read_overlaps(x, y)
    want_ov, want_sh = overlap_ref.read_overlaps(c.idx, x, y, c.first_id)
    assert np.array_equal(ov, rov) and np.array_equal(sh, rsh)
    assert np.array_equal(ov, want_ov) and np.array_equal(sh, want_sh)
    assert (ov[:len(ref.steps[-1].x)] != ref.steps[-1].overlap).sum() >= 100


@pytest.mark.parametrize("make", [tr.case_a, tr.case_b], ids=["A", "B"])
def test_set_scores_follow_the_merges(make, gpu_ctx, hga_mod, no_sets_bytes):
    ref = make(hga_mod)
    c = ref.c
    lookup(gpu_ctx, c)
    gpu_ctx.profile(True)
    try:
        for st in ref.steps:
            if st.no:
                gpu_ctx.components_merge(c.steps[st.no].groups)
            before = state_snapshot(gpu_ctx)
            no_sets_bytes.delenv("HGA_SETS_BYTES", raising=False)
            gpu_ctx.profile_reset()
            score, size = gpu_ctx.components_set_scores(st.sets, st.set_pairs)
            assert score.dtype == np.uint64 and size.dtype == np.uint64
            assert size.tolist() == st.set_size.tolist()
            assert score.tolist() == st.score.tolist()
            assert gpu_ctx.profile_get("cs_pairs")[1] == 1   # every row in one tile, every pair in one launch
            # n_pairs == 0 still returns the sizes
            none, size0 = gpu_ctx.components_set_scores(st.sets, np.zeros((0, 2), np.uint32))
            assert len(none) == 0 and size0.tolist() == st.set_size.tolist()
            # rows of 30 16-byte words: 3840 KmerIDs per tile
            tiles = -(-ref.K // 3840)
            no_sets_bytes.setenv("HGA_SETS_BYTES", str(16 * 30 * len(st.sets)))
            gpu_ctx.profile_reset()
            tscore, tsize = gpu_ctx.components_set_scores(st.sets, st.set_pairs)
            assert gpu_ctx.profile_get("cs_pairs")[1] == tiles
            assert tiles >= 3 or c.name == "B"
            assert tsize.tolist() == st.set_size.tolist() and tscore.tolist() == st.score.tolist()
            # one 16-byte word per row: 128 KmerIDs per tile
            no_sets_bytes.setenv("HGA_SETS_BYTES", "1")
            gpu_ctx.profile_reset()
            tscore, tsize = gpu_ctx.components_set_scores(st.sets, st.set_pairs)
            assert gpu_ctx.profile_get("cs_pairs")[1] == -(-ref.K // 128)
            assert tsize.tolist() == st.set_size.tolist() and tscore.tolist() == st.score.tolist()
            assert same_state(state_snapshot(gpu_ctx), before)
    finally:
        gpu_ctx.profile(False)
    got = gpu_ctx.lookup_fetch()
    for name, want in c.idx.items():
        if name in got:
            assert np.array_equal(got[name], want), name


def test_errors_and_state(gpu_ctx, hga_mod, no_sets_bytes):
    L = hga_mod.lib()
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    one, sp, out = np.array([1], np.uint32), np.array([0, 1], np.uint64), np.zeros(1, np.uint64)
    zero = np.zeros(1, np.uint32)
    with hga_mod.Ctx(int(os.environ.get("HGA_DEVICE", "0"))) as fresh:
        assert L.hga_components_overlaps(fresh._h, u32(one), u32(one), 1, None, None) == HGA_ERR_STATE
        assert L.hga_components_set_scores(fresh._h, u64(sp), u32(one), 1, u32(zero), u32(zero), 1, u64(out), None) == HGA_ERR_STATE
        with pytest.raises(hga_mod.HgaError, match=f"status {HGA_ERR_STATE}"):
            fresh.components_overlaps([1], [1])
    ref = tr.case_b(hga_mod)
    c = ref.c
    lookup(gpu_ctx, c)
    gpu_ctx.components_merge(c.steps[1].groups)
    merged = state_snapshot(gpu_ctx)
    first, last = c.first_id, c.first_id + c.n - 1
    a, b = c.rest[152], c.rest[153]
    # empty calls
    assert L.hga_components_overlaps(gpu_ctx._h, None, None, 0, None, None) == 0
    assert L.hga_components_set_scores(gpu_ctx._h, None, None, 0, None, None, 0, None, None) == 0
    ov, sh = gpu_ctx.components_overlaps([], [])
    assert len(ov) == 0 and len(sh) == 0
    score, size = gpu_ctx.components_set_scores([], np.zeros((0, 2), np.uint32))
    assert len(score) == 0 and len(size) == 0
    for x, y in (([first - 1], [a]), ([a], [last + 1]), ([a, b, last + 1], [a, b, a])):
        with pytest.raises(hga_mod.HgaError, match=f"status {HGA_ERR_INVALID}"):
            gpu_ctx.components_overlaps(x, y)
        assert same_state(state_snapshot(gpu_ctx), merged)
    bad_sets = [([[a], [first - 1]], [(0, 1)]), ([[a, last + 1]], [(0, 0)]),        # an id outside the reads
                ([[a], [b]], [(0, 2)]), ([[a], [b]], [(2, 0)]), ([], [(0, 0)])]   # a pair index >= n_sets
    for sets, pairs in bad_sets:
        with pytest.raises(hga_mod.HgaError, match=f"status {HGA_ERR_INVALID}"):
            gpu_ctx.components_set_scores(sets, pairs)
        assert same_state(state_snapshot(gpu_ctx), merged)
    ids, down = np.array([a, b, a], np.uint32), np.array([0, 2, 1, 3], np.uint64)   # a decreasing set_ptr
    assert L.hga_components_set_scores(gpu_ctx._h, u64(down), u32(ids), 3, u32(zero), u32(zero), 1, u64(out), None) == HGA_ERR_INVALID
    assert same_state(state_snapshot(gpu_ctx), merged)
    # and the calls still answer on the merged state
    st = ref.steps[1]
    ov, sh = gpu_ctx.components_overlaps(st.x, st.y)
    assert np.array_equal(ov, st.overlap) and np.array_equal(sh, st.shared)


def kmer_str(code, k):
    return "".join("ACGT"[(int(code) >> (2 * (k - 1 - i))) & 3] for i in range(k))


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory, hga_mod):
    """The 40 kb two-haplotype workload and arguments of test_components_gpu.py's cli_case."""
    import pyref_cluster as pc
    tmp = tmp_path_factory.mktemp("tailsets_cli")
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
    args = ["--sc_min_size", "3", "--sc_max_size", "40", "--sc_fraction", "0.3", "--core_enrichment", "4",
            "--tail_amplification", "6", "--spectral_dims", "4"]
    cfg = dict(sc_min=3, sc_max=40, sc_fraction=0.3, sc_score=0, enrich=4, tail=6, dims=4)
    rec = hga_mod.load_records(paths, True)
    idx = oracle.construct_indices(rec["bases"], rec["offsets"], k, sdk)
    eng = pc.Engine(idx, np.diff(rec["offsets"]), rec["category"], int(rec["meta"][-1][4]), True, cfg,
                    start=rec["start"], end=rec["end"])
    eng.run()

    def run(name, gpus=1, **env_add):
        env = dict(os.environ, HGA_TIMING="1")
        for var in ("HGA_HOST_CONNECTIONS", "HGA_HOST_OVERLAPS", "HGA_DEVICE_SETS", "HGA_SETS_BYTES"):
            env.pop(var, None)
        env.update(env_add)
        out = subprocess.run([os.path.join(BIN, "categorization"), *paths, "-k", str(tmp / "sdk.txt"), "-d", "-o",
                              str(tmp / name), *args, "--gpus", str(gpus)], capture_output=True, text=True, cwd=tmp,
                             env=env, timeout=300)
        assert out.returncode == 0, out.stderr
        timing = dict(ln.split()[1:3] for ln in out.stderr.splitlines() if ln.startswith("hga-timing "))
        lines = [ln for ln in out.stdout.splitlines() if " took " not in ln]
        files = {f: open(tmp / name / f).read() for f in sorted(os.listdir(tmp / name))}
        assert "Calculation of tail connections took" in out.stdout
        return lines, files, timing

    return run, eng.printed


def check_sets_timing(t):
    assert int(t["tails.overlap_edges_host"]) == 0 and int(t["tails.overlap_edges_device"]) > 0
    assert int(t["sets.device_calls"]) >= 1 and "tails.sets_device" in t
    assert "merge1.union" not in t and "merge1.device" in t
    assert int(t["conn.host_calls"]) == 0


def test_categorization_device_sets_equal_default_and_host(cli_case):
    run, printed = cli_case
    sets = run("sets", HGA_DEVICE_SETS="1")
    default = run("default")
    host = run("host", HGA_HOST_CONNECTIONS="1")
    for other in (default, host):
        assert sets[0] == other[0]
        assert sets[1] == other[1] and len(sets[1]) > 1
    assert [ln for ln in sets[0] if ln.startswith("#")] == printed
    check_sets_timing(sets[2])
    # the default path as it was: survivor edges on the host, host unions, no set-score call
    d = default[2]
    assert int(d["tails.overlap_edges_host"]) > 0 and "merge1.union" in d and "sets.device_calls" not in d
    assert int(sets[2]["tails.overlap_edges_device"]) == int(d["tails.overlap_edges_device"]) + int(d["tails.overlap_edges_host"])
    # the mode needs the device component state: under either host switch it is off
    for var in ("HGA_HOST_CONNECTIONS", "HGA_HOST_OVERLAPS"):
        off = run("off_" + var, HGA_DEVICE_SETS="1", **{var: "1"})
        assert off[0] == default[0] and off[1] == default[1]
        assert "sets.device_calls" not in off[2] and "merge1.union" in off[2]


def test_categorization_device_sets_tiled_and_two_ranks(cli_case):
    run, printed = cli_case
    one = run("one", HGA_DEVICE_SETS="1")
    tiled = run("tiled", HGA_DEVICE_SETS="1", HGA_SETS_BYTES="4096")
    two = run("two", gpus=2, HGA_DEVICE_SETS="1")
    for other in (tiled, two):
        assert one[0] == other[0]
        assert one[1] == other[1] and len(one[1]) > 1
        check_sets_timing(other[2])
    assert [ln for ln in one[0] if ln.startswith("#")] == printed
