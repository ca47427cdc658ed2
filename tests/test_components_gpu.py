"""hga_components_* on the MI355X: merge_components (ReadClusteringEngine.cpp:341-422) and get_connections
(:301-333) on merged components against tests/pyref_cluster.py's Engine on the two shared cases of
tests/components_ref.py, the lookup's own state left intact, the entry points' error and state rules, and
bin/categorization with the post-merge connections on the device against its host path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import components_ref as cr
import oracle
import overlap_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hybrid-genome-assembler_amd", "bin")
HGA_ERR_INVALID, HGA_ERR_STATE = 1, 4


def lookup(ctx, c):
    ctx.lookup_load(c.k, c.sdk)
    ctx.lookup_set_reads(c.bases, c.offsets, c.first_id)
    ctx.lookup_run()


def conns(ctx, pivots, min_score):
    n = ctx.components_connections(pivots, min_score)
    x, y, s, g = ctx.connections_range(0, n)
    assert len(x) == n and not g.any()
    return list(zip(x.tolist(), y.tolist(), s.tolist()))


def check_state(ctx, c, step_no, ids):
    st = c.steps[step_no]
    ptr, idx = ctx.components_index()
    want_ptr, want_idx = st.csr()
    assert np.array_equal(ptr, want_ptr)
    assert np.array_equal(idx, want_idx)
    for i in ids:
        got = ctx.components_kmers(i)
        assert got.dtype == np.uint32 and got.tolist() == st.kmers[i], i
    sv = c.all_survivors(step_no)
    sz = ctx.components_sizes()
    assert sz.index_entries == len(want_idx)
    assert sz.survivors == len(sv)
    assert sz.survivor_kmers == sum(len(st.kmers[i]) for i in sv)
    assert sz.merges == sum(len(g) >= 2 for s in c.steps[:step_no + 1] for g in s.groups)


def state_snapshot(ctx):
    sz = ctx.components_sizes()
    return ctx.components_index(), (sz.index_entries, sz.survivors, sz.survivor_kmers, sz.merges)


def same_state(a, b):
    return np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1], b[0][1]) and a[1] == b[1]


@pytest.mark.parametrize("make", [cr.case_a, cr.case_b], ids=["A", "B"])
def test_connections_before_any_merge(make, gpu_ctx, hga_mod):
    c = make(hga_mod)
    lookup(gpu_ctx, c)
    no_hit = c.first_id + int(np.flatnonzero(np.diff(c.idx["hit_ptr"]) == 0)[0])
    pivots = np.array(c.ids[::3] + [c.ids[-1], no_hit], np.uint32)
    for s in (1, 4):
        x, y, sc, _ = oracle.connections(c.idx, pivots=pivots, min_score=s, first_read_id=c.first_id)
        want = list(zip(x.tolist(), y.tolist(), sc.tolist()))
        assert len(want) > 1000
        assert conns(gpu_ctx, pivots, s) == want
        gx, gy, gs, _ = gpu_ctx.connections(pivots, 1, s)   # hga_connections_run(pivots, 1, s, NULL)
        assert list(zip(gx.tolist(), gy.tolist(), gs.tolist())) == want
    assert conns(gpu_ctx, [no_hit], 1) == []
    assert conns(gpu_ctx, pivots, 1 << 32) == []   # a min_score wider than 32 bits: nothing, as connections_run
    assert gpu_ctx.connections_run(pivots, 1, 1 << 32) == 0
    check_state(gpu_ctx, c, 0, c.ids[:5])


def test_case_a_merges(gpu_ctx, hga_mod):
    c = cr.case_a(hga_mod)
    lookup(gpu_ctx, c)
    for no in (1, 2, 3):
        st = c.steps[no]
        gpu_ctx.components_merge(st.groups)
        members = [m for g in st.groups for m in g[1:]]
        touched = {i for s in c.steps[:no + 1] for g in s.groups if len(g) >= 2 for i in g}
        untouched = [i for i in c.ids if i not in touched]
        check_state(gpu_ctx, c, no, c.all_survivors(no) + members[:5] + untouched[:5])
        want = st.connections(c.all_survivors(no), 4)
        assert conns(gpu_ctx, c.all_survivors(no), 4) == want
        if no < 3:
            assert len(want) > 50
        piv = members[:40]
        assert conns(gpu_ctx, piv, 6) == st.connections(piv, 6)
        if no == 3:   # 56 index entries are left: nothing reaches 4 any more
            assert conns(gpu_ctx, c.all_survivors(no) + piv, 1) == st.connections(c.all_survivors(no) + piv, 1)
    assert sum(len(l) for l in c.steps[3].kci) < 100


def test_case_b_merges(gpu_ctx, hga_mod):
    c = cr.case_b(hga_mod)
    lookup(gpu_ctx, c)
    sv = c.steps[1].survivors
    untouched = c.rest[152:157]
    # merge 1: groups of 1, 2, 3, 64, 65 and 0 members
    gpu_ctx.components_merge(c.steps[1].groups)
    members = c.steps[1].groups[4][1:6]
    check_state(gpu_ctx, c, 1, sv + members + untouched)
    piv = sv + members + untouched + [c.genome_read]
    want = c.steps[1].connections(piv, 1)
    scores = sorted({t[2] for t in want})
    assert len(want) > 2000 and len(scores) > 500 and scores[-1] > 2000
    assert conns(gpu_ctx, piv, 1) == want
    mid = scores[len(scores) // 2]   # a score that occurs: pairs at the bound stay, those below go
    want_mid = c.steps[1].connections(piv, mid)
    assert 0 < len(want_mid) < len(want) and want_mid[-1][2] == mid
    assert conns(gpu_ctx, piv, mid) == want_mid
    assert conns(gpu_ctx, piv, mid + 1) == c.steps[1].connections(piv, mid + 1)
    # merge 2: a survivor as a non-survivor member, a survivor surviving again with 150 fresh members
    gpu_ctx.components_merge(c.steps[2].groups)
    check_state(gpu_ctx, c, 2, c.all_survivors(2) + c.rest[:5] + untouched)
    piv = [sv[0], sv[2], c.rest[150], sv[3]] + untouched + [c.genome_read]
    want = c.steps[2].connections(piv, 1)
    assert len(want) > 50
    assert conns(gpu_ctx, piv, 1) == want
    # a pivot listed twice gives its pairs twice, as the reference's loop over component_ids would
    twice = conns(gpu_ctx, [sv[3], sv[3]], 1)
    once = c.steps[2].connections([sv[3]], 1)
    assert twice == sorted(once + once, key=lambda t: (-t[2], t[0], t[1])) and once


def test_lookup_state_stays_intact(gpu_ctx, hga_mod):
    c = cr.case_b(hga_mod)
    lookup(gpu_ctx, c)
    gpu_ctx.components_merge(c.steps[1].groups)
    gpu_ctx.components_merge(c.steps[2].groups)
    assert conns(gpu_ctx, c.steps[2].survivors, 1)
    got = gpu_ctx.lookup_fetch()
    for name, want in c.idx.items():
        if name in got:
            assert np.array_equal(got[name], want), name
    x, y, s, _ = oracle.connections(c.idx, min_score=1, first_read_id=c.first_id)
    gx, gy, gs, _ = gpu_ctx.connections(min_score=1)
    assert np.array_equal(gx, x) and np.array_equal(gy, y) and np.array_equal(gs, s)
    rng = np.random.default_rng(11)
    px, py = rng.integers(c.first_id, c.first_id + c.n, (2, 10)).astype(np.uint32)
    ov, sh = gpu_ctx.read_overlaps(px, py)
    want_ov, want_sh = overlap_ref.read_overlaps(c.idx, px, py, c.first_id)
    assert np.array_equal(ov, want_ov) and np.array_equal(sh, want_sh) and sh.any()
    check_state(gpu_ctx, c, 2, c.all_survivors(2))   # and the view is still the merged one


def test_errors_and_state(gpu_ctx, hga_mod):
    L = hga_mod.lib()
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    one, gp, n = np.array([1], np.uint32), np.array([0, 1], np.uint64), C.c_uint64()
    with hga_mod.Ctx(int(os.environ.get("HGA_DEVICE", "0"))) as fresh:
        sz = hga_mod.ComponentsSizes()
        assert L.hga_components_merge(fresh._h, u64(gp), u32(one), 1) == HGA_ERR_STATE
        assert L.hga_components_connections(fresh._h, u32(one), 1, 1, C.byref(n)) == HGA_ERR_STATE
        assert L.hga_components_get_sizes(fresh._h, C.byref(sz)) == HGA_ERR_STATE
        assert L.hga_components_fetch_index(fresh._h, None, None) == HGA_ERR_STATE
        assert L.hga_components_fetch_kmers(fresh._h, 1, None, C.byref(n)) == HGA_ERR_STATE
        assert L.hga_components_reset(fresh._h) == HGA_ERR_STATE
        with pytest.raises(hga_mod.HgaError, match=f"status {HGA_ERR_STATE}"):
            fresh.components_merge([[1, 2]])
    c = cr.case_b(hga_mod)
    lookup(gpu_ctx, c)
    first, last = c.first_id, c.first_id + c.n - 1
    pristine = state_snapshot(gpu_ctx)
    assert pristine[1] == (len(c.idx["kci_read"]), 0, 0, 0)
    # no-ops: empty calls, empty and one-member groups (a no-hit or unknown id is only checked for range there)
    assert L.hga_components_merge(gpu_ctx._h, None, None, 0) == 0
    assert L.hga_components_connections(gpu_ctx._h, None, 0, 1, C.byref(n)) == 0 and n.value == 0
    gpu_ctx.components_merge([])
    gpu_ctx.components_merge([[], [c.ids[3]], [], [c.no_hit]])
    assert conns(gpu_ctx, [], 1) == []
    assert same_state(state_snapshot(gpu_ctx), pristine)
    gpu_ctx.components_merge(c.steps[1].groups)
    merged = state_snapshot(gpu_ctx)
    assert not same_state(merged, pristine)
    a, b, d = c.rest[152], c.rest[153], c.rest[154]
    bad_calls = [[[a, b], [d, first - 1]], [[a, last + 1, b]], [[last + 1]],   # out of range
                 [[a, b, c.no_hit]], [[c.no_hit, a]],                            # no hits inside a group
                 [[a, b], [d, a]], [[a, b, a]], [[a], [b, a]]]                  # listed twice in one call
    for groups in bad_calls:
        with pytest.raises(hga_mod.HgaError, match=f"status {HGA_ERR_INVALID}"):
            gpu_ctx.components_merge(groups)
        assert same_state(state_snapshot(gpu_ctx), merged), groups
    for piv in ([first - 1], [a, last + 1]):
        with pytest.raises(hga_mod.HgaError, match=f"status {HGA_ERR_INVALID}"):
            gpu_ctx.components_connections(piv, 1)
    with pytest.raises(hga_mod.HgaError, match=f"status {HGA_ERR_INVALID}"):
        gpu_ctx.components_kmers(last + 1)
    assert len(gpu_ctx.components_kmers(c.no_hit)) == 0
    check_state(gpu_ctx, c, 1, c.steps[1].survivors)
    # NULL outputs of the fetches
    assert L.hga_components_fetch_index(gpu_ctx._h, None, None) == 0
    ptr = np.zeros(len(c.sdk) + 1, np.uint64)
    assert L.hga_components_fetch_index(gpu_ctx._h, u64(ptr), None) == 0
    assert np.array_equal(ptr, c.steps[1].csr()[0])
    # reset and a new lookup_run each return to the lookup's state
    gpu_ctx.components_reset()
    assert same_state(state_snapshot(gpu_ctx), pristine)
    gpu_ctx.components_merge(c.steps[1].groups)
    assert same_state(state_snapshot(gpu_ctx), merged)
    gpu_ctx.lookup_run()
    assert same_state(state_snapshot(gpu_ctx), pristine)
    check_state(gpu_ctx, c, 0, c.steps[1].survivors)


def kmer_str(code, k):
    return "".join("ACGT"[(int(code) >> (2 * (k - 1 - i))) & 3] for i in range(k))


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory, hga_mod):
    """The 40 kb two-haplotype workload and arguments of test_overlaps_gpu.py's cli_case: three merges
    (scaffold, spectral, enrichment), two amplify_component calls per scaffold component and the
    enrichment pass after the first of them."""
    import pyref_cluster as pc
    tmp = tmp_path_factory.mktemp("components_cli")
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

    def run(name, gpus=1, host_connections=False):
        env = dict(os.environ, HGA_TIMING="1")
        env.pop("HGA_HOST_CONNECTIONS", None)
        if host_connections:
            env["HGA_HOST_CONNECTIONS"] = "1"
        out = subprocess.run([os.path.join(BIN, "categorization"), *paths, "-k", str(tmp / "sdk.txt"), "-d", "-o",
                              str(tmp / name), *args, "--gpus", str(gpus)], capture_output=True, text=True, cwd=tmp,
                             env=env, timeout=300)
        assert out.returncode == 0, out.stderr
        timing = dict(ln.split()[1:3] for ln in out.stderr.splitlines() if ln.startswith("hga-timing "))
        lines = [ln for ln in out.stdout.splitlines() if " took " not in ln]
        files = {f: open(tmp / name / f).read() for f in sorted(os.listdir(tmp / name))}
        assert "Calculation of enrichment connections took" in out.stdout
        return lines, files, int(timing["conn.device_calls"]), int(timing["conn.host_calls"]), timing

    return run, eng.printed


def test_categorization_device_components_equal_host(cli_case):
    run, printed = cli_case
    dev = run("dev")
    host = run("host", host_connections=True)
    assert dev[0] == host[0]
    assert dev[1] == host[1] and len(dev[1]) > 1
    assert [ln for ln in dev[0] if ln.startswith("#")] == printed
    assert dev[2] > 2 and dev[3] == 0
    assert host[2] == 0 and host[3] == dev[2]
    assert "merge1.device" in dev[4] and "merge1.kci_update" not in dev[4]
    assert "merge1.kci_update" in host[4] and "merge1.device" not in host[4]


def test_categorization_device_components_two_ranks(cli_case):
    """--gpus 2: rank 0's ctx holds the gathered index (hga_lookup_gather), so its component state
    covers every read."""
    run, printed = cli_case
    one = run("one")
    two = run("two", gpus=2)
    assert one[0] == two[0]
    assert one[1] == two[1] and len(one[1]) > 1
    assert two[2] > 2 and two[2:4] == one[2:4]
