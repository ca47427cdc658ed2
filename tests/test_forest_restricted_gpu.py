"""hga_spanning_forest_restricted on the MI355X, bit-exact against tests/forest_restricted_ref.py's straight loop:
explicit edge lists with restricted ids (every case of forest_restricted_ref.cases, windows included), the
ctx's connection results (golden data, a merged component state with the survivors restricted), the error and
state rules, a plain call after a restricted one, and bin/categorization under HGA_DEVICE_ENRICH=1."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import forest_ref as fr
import forest_restricted_ref as rr
import overlap_ref
import tailsets_ref as tr
from test_forest_gpu import kmer_str, load_wide

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hybrid-genome-assembler_amd", "bin")
GOLD = os.path.join(ROOT, "tests", "golden")
HGA_ERR_INVALID, HGA_ERR_STATE = 1, 4
DEVICE = int(os.environ.get("HGA_DEVICE", "0"))
ALL = 2 ** 64 - 1


@pytest.fixture(scope="module")
def wide_ctx(hga_mod):
    ctx = hga_mod.Ctx(DEVICE)
    load_wide(ctx)
    yield ctx
    ctx.close()


def check(got, x, y, restricted, first=0, count=None):
    """got = (pos, x, y) of a restricted call on entries [first, first + count) of the list (x, y)."""
    n = len(x)
    a = min(first, n)
    b = n if count is None else min(n, a + count)
    want = [a + p for p in rr.kruskal_restricted(x[a:b], y[a:b], restricted)]
    pos, gx, gy = got
    assert pos.dtype == np.uint64 and gx.dtype == np.uint32 and gy.dtype == np.uint32
    assert pos.tolist() == want
    assert np.array_equal(gx, np.asarray(x, np.uint32)[want]) and np.array_equal(gy, np.asarray(y, np.uint32)[want])
    return want


@pytest.mark.parametrize("name", sorted(rr.cases()))
def test_explicit_edges(name, wide_ctx):
    c = rr.cases()[name]
    got = wide_ctx.spanning_forest(c.x, c.y, c.first, c.count, restricted=c.restricted)
    assert got[0].tolist() == rr.expected(name)[0]
    want = check(got, c.x, c.y, c.restricted, c.first, c.count)
    # union_find over the accepted connections alone, with the restricted set, repeats the full list's merges
    a, b = rr.window(c)
    rel = [p - a for p in want]
    for min_size in (2, 3):
        assert rr.replay(got[1], got[2], range(len(want)), c.restricted, min_size) == \
            rr.full(c.x[a:b], c.y[a:b], rel, c.restricted, min_size)


def test_no_restricted_id_is_the_plain_call(wide_ctx):
    """n_restricted == 0 launches nothing new; a restricted call launches sf_restrict once and the same rounds."""
    x, y = fr.shapes()["halving"]
    wide_ctx.profile(True)
    try:
        wide_ctx.profile_reset()
        plain = wide_ctx.spanning_forest(x, y)
        counts = {k: wide_ctx.profile_get(k)[1] for k in ("sf_init", "sf_restrict", "sf_min", "sf_hook", "sf_jump")}
        assert counts["sf_restrict"] == 0 and counts["sf_init"] == 1
        wide_ctx.profile_reset()
        none = wide_ctx.spanning_forest(x, y, restricted=[])
        assert {k: wide_ctx.profile_get(k)[1] for k in counts} == counts
        assert all(np.array_equal(a, b) for a, b in zip(plain, none))
        wide_ctx.profile_reset()
        c = rr.cases()["halving_ends"]
        check(wide_ctx.spanning_forest(c.x, c.y, restricted=c.restricted), c.x, c.y, c.restricted)
        assert wide_ctx.profile_get("sf_restrict")[1] == 1 and wide_ctx.profile_get("sf_init")[1] == 1
        rounds = rr.model("halving_ends")[1]
        assert rounds <= wide_ctx.profile_get("sf_min")[1] <= rounds + 1
        # every hub-leaf edge of round 0 offers to best[R]: still one round that hooks, and the one that ends
        c = rr.cases()["hubs"]
        wide_ctx.profile_reset()
        check(wide_ctx.spanning_forest(c.x, c.y, restricted=c.restricted), c.x, c.y, c.restricted)
        assert wide_ctx.profile_get("sf_min")[1] == rr.model("hubs")[1] + 1 == 2
    finally:
        wide_ctx.profile(False)


def test_a_plain_call_after_a_restricted_one(wide_ctx):
    """Nothing of the contracted start is left in comp: the same list, restricted and then plain."""
    for name in ("hubs", "random_3_some", "cliques_cross_last"):
        c = rr.cases()[name]
        restricted = check(wide_ctx.spanning_forest(c.x, c.y, restricted=c.restricted), c.x, c.y, c.restricted)
        pos, gx, gy = wide_ctx.spanning_forest(c.x, c.y)
        want = fr.kruskal(c.x, c.y)
        assert pos.tolist() == want != restricted
        assert np.array_equal(gx, c.x[want]) and np.array_equal(gy, c.y[want])
        check(wide_ctx.spanning_forest(c.x, c.y, restricted=c.restricted), c.x, c.y, c.restricted)


def restricted_forest_of_result(ctx, n, restricted):
    """The restricted call on the ctx's connection result of n rows (x == y == NULL) against the fetched rows."""
    rows = ctx.connections_range(0, n)
    assert len(rows[0]) == n
    x, y = rows[0], rows[1]
    by_rule = []
    whole = rr.kruskal_restricted(x, y, restricted, by_rule)
    assert check(ctx.spanning_forest(restricted=restricted), x, y, restricted) == whole
    for first, count in ((0, n // 2), (n // 3, n // 2), (n // 3, None), (n, 3)):
        check(ctx.spanning_forest(first=first, count=count, restricted=restricted), x, y, restricted, first, count)
    assert all(np.array_equal(a, b) for a, b in zip(rows, ctx.connections_range(0, n)))   # the result is only read
    return whole, by_rule, fr.kruskal(x, y)


def test_on_a_connection_result(gpu_ctx, hga_mod):
    g = np.load(os.path.join(GOLD, "lookup_golden.npz"))
    rec = hga_mod.load_records([os.path.join(GOLD, p) for p in ("reads_a.fq", "reads_b.fq", "reads_c.fa")], True)
    gpu_ctx.lookup_load(19, g["sdk_keys_id_order"])
    gpu_ctx.lookup_set_reads(rec["bases"], rec["offsets"], 1)
    gpu_ctx.lookup_run()
    n = gpu_ctx.connections_run(min_score=1)
    n_reads = len(rec["offsets"]) - 1
    restricted = np.arange(1, n_reads + 1, 3, dtype=np.uint32)   # every third read, with or without hits
    whole, by_rule, plain = restricted_forest_of_result(gpu_ctx, n, restricted)
    assert 0 < len(whole) < len(plain) and by_rule


def test_on_a_merged_component_state(gpu_ctx, hga_mod):
    ref = tr.case_b(hga_mod)
    c = ref.c
    gpu_ctx.lookup_load(c.k, c.sdk)
    gpu_ctx.lookup_set_reads(c.bases, c.offsets, c.first_id)
    gpu_ctx.lookup_run()
    gpu_ctx.components_merge(c.steps[1].groups)
    survivors = np.array(sorted(c.steps[1].survivors), np.uint32)
    n = gpu_ctx.components_connections(survivors, 1)   # the enrichment step's list: the cores are the pivots
    assert n > 100 and len(survivors) >= 2
    whole, by_rule, plain = restricted_forest_of_result(gpu_ctx, n, survivors)
    assert by_rule and 0 < len(whole) < len(plain)   # (the case's figures on the CPU: 792 rows, 195 against 198)
    # and on the list of every component, where cores also meet through third reads
    pivots = np.array(sorted(set(c.steps[1].survivors) | set(c.rest)), np.uint32)
    n = gpu_ctx.components_connections(pivots, 1)
    whole, by_rule, plain = restricted_forest_of_result(gpu_ctx, n, survivors)
    assert by_rule and 0 < len(whole) < len(plain) < n


def raw(hga_mod, ctx, x, y, n, first, count, restricted, n_restricted, want_edges=True):
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))
    m = C.c_uint64(12345)
    st = hga_mod.lib().hga_spanning_forest_restricted(ctx._h, p(x), p(y), n, first, count, p(restricted), n_restricted,
                                                      C.byref(m) if want_edges else None)
    return st, m.value


def test_errors_and_state(hga_mod):
    L = hga_mod.lib()
    fetch_state = lambda ctx: L.hga_spanning_forest_fetch(ctx._h, None, None, None)
    one, two = np.array([fr.FIRST_ID], np.uint32), np.array([fr.FIRST_ID + 1], np.uint32)
    last = fr.FIRST_ID + fr.N_READS - 1
    with hga_mod.Ctx(DEVICE) as ctx:
        # before hga_lookup_run
        assert raw(hga_mod, ctx, one, two, 1, 0, ALL, one, 1)[0] == HGA_ERR_STATE
        assert raw(hga_mod, ctx, None, None, 0, 0, ALL, one, 1)[0] == HGA_ERR_STATE
        assert fetch_state(ctx) == HGA_ERR_STATE
        with pytest.raises(hga_mod.HgaError, match=f"status {HGA_ERR_STATE}"):
            ctx.spanning_forest(one, two, restricted=one)
        load_wide(ctx)
        c = rr.cases()["doubled_repeats"]
        x, y, r = c.x, c.y, c.restricted
        good = rr.expected("doubled_repeats")[0]
        # no connection result yet; exactly one NULL; a null n_edges
        assert raw(hga_mod, ctx, None, None, 0, 0, ALL, r, len(r))[0] == HGA_ERR_STATE
        assert raw(hga_mod, ctx, x, None, len(x), 0, ALL, r, len(r))[0] == HGA_ERR_INVALID
        assert raw(hga_mod, ctx, x, y, len(x), 0, ALL, r, len(r), want_edges=False)[0] == HGA_ERR_INVALID
        assert fetch_state(ctx) == HGA_ERR_STATE
        # a good call; the first and the last ReadID are legal restricted ids
        assert raw(hga_mod, ctx, x, y, len(x), 0, ALL, r, len(r)) == (0, len(good))
        assert fetch_state(ctx) == 0
        ends = np.array([last, fr.FIRST_ID], np.uint32)
        assert raw(hga_mod, ctx, x, y, len(x), 0, ALL, ends, 2) == (0, len(fr.expected("doubled")))
        # a NULL list with a count: refused, and a failed call leaves no result
        assert raw(hga_mod, ctx, x, y, len(x), 0, ALL, None, 3) == (HGA_ERR_INVALID, 12345)
        assert fetch_state(ctx) == HGA_ERR_STATE
        # a restricted id outside the reads, anywhere in the list
        for bad in (fr.FIRST_ID - 1, last + 1, 0, 2 ** 32 - 1):
            for at in (0, 3, len(r) - 1):
                check(ctx.spanning_forest(x, y, restricted=r), x, y, r)
                assert fetch_state(ctx) == 0
                b = r.copy()
                b[at] = bad
                assert raw(hga_mod, ctx, x, y, len(x), 0, ALL, b, len(b)) == (HGA_ERR_INVALID, 12345)
                assert fetch_state(ctx) == HGA_ERR_STATE
                # ... unless it is past the count
                if at == len(r) - 1:
                    assert raw(hga_mod, ctx, x, y, len(x), 0, ALL, b, len(b) - 1) == (0, len(good))
        # an edge id outside the reads: as for the plain call, and no result is left
        check(ctx.spanning_forest(x, y, restricted=r), x, y, r)
        bx = x.copy()
        bx[7] = last + 1
        assert raw(hga_mod, ctx, bx, y, len(x), 0, ALL, r, len(r)) == (HGA_ERR_INVALID, 12345)
        assert fetch_state(ctx) == HGA_ERR_STATE
        assert raw(hga_mod, ctx, bx, y, len(x), 8, ALL, r, len(r))[0] == 0   # outside the range the call works on
        # no count: the plain call, whatever the pointer; an empty clipped range is HGA_OK with no edge
        plain = fr.expected("doubled")
        assert raw(hga_mod, ctx, x, y, len(x), 0, ALL, None, 0) == (0, len(plain))
        assert raw(hga_mod, ctx, x, y, len(x), 0, ALL, r, 0) == (0, len(plain))
        pos = np.zeros(len(plain), np.uint64)
        assert L.hga_spanning_forest_fetch(ctx._h, pos.ctypes.data_as(C.POINTER(C.c_uint64)), None, None) == 0
        assert pos.tolist() == plain
        for first, count in ((0, 0), (len(x), 5), (ALL, ALL)):
            assert raw(hga_mod, ctx, x, y, len(x), first, count, r, len(r)) == (0, 0)
            assert fetch_state(ctx) == 0
        # a failed plain call keeps the earlier result, as before
        check(ctx.spanning_forest(x, y, restricted=r), x, y, r)
        assert L.hga_spanning_forest(ctx._h, bx.ctypes.data_as(C.POINTER(C.c_uint32)),
                                     y.ctypes.data_as(C.POINTER(C.c_uint32)), len(x), 0, ALL,
                                     C.byref(C.c_uint64())) == HGA_ERR_INVALID
        pos = np.zeros(len(good), np.uint64)
        assert L.hga_spanning_forest_fetch(ctx._h, pos.ctypes.data_as(C.POINTER(C.c_uint64)), None, None) == 0
        assert pos.tolist() == good
        # hga_lookup_run ends the result's life
        ctx.lookup_run()
        assert fetch_state(ctx) == HGA_ERR_STATE
        assert raw(hga_mod, ctx, None, None, 0, 0, ALL, r, len(r))[0] == HGA_ERR_STATE
        check(ctx.spanning_forest(x, y, restricted=r), x, y, r)


@pytest.fixture(scope="module")
def cli(tmp_path_factory, hga_mod):
    """bin/categorization on overlap_ref.tails_case's files with default arguments (plus `extra`)."""
    tmp = tmp_path_factory.mktemp("enrich_cli")
    paths, k, sdk, rec, idx, c = overlap_ref.tails_case(hga_mod, tmp)
    (tmp / "sdk.txt").write_text("".join(kmer_str(code, k) + "\n" for code in sdk))
    done = {}

    def run(name, extra=(), gpus=1, **env_add):
        if name in done:
            return done[name]
        env = dict(os.environ, HGA_TIMING="1")
        for var in ("HGA_HOST_CONNECTIONS", "HGA_HOST_OVERLAPS", "HGA_DEVICE_SETS", "HGA_SETS_BYTES", "HGA_DEVICE_TAILS",
                    "HGA_DEVICE_FOREST", "HGA_DEVICE_ENRICH"):
            env.pop(var, None)
        env.update(env_add)
        out = subprocess.run([os.path.join(BIN, "categorization"), *paths, "-k", str(tmp / "sdk.txt"), "-d", "-o",
                              str(tmp / name), *extra, "--gpus", str(gpus)], capture_output=True, text=True, cwd=tmp,
                             env=env, timeout=300)
        assert out.returncode == 0, out.stderr
        timing = dict(ln.split()[1:3] for ln in out.stderr.splitlines() if ln.startswith("hga-timing "))
        took = [ln.split(" took ")[0] for ln in out.stdout.splitlines() if " took " in ln]
        lines = [ln for ln in out.stdout.splitlines() if " took " not in ln]
        files = {f: open(tmp / name / f).read() for f in sorted(os.listdir(tmp / name))}
        done[name] = (lines, files, timing, took)
        return done[name]

    return run


def keys(run, prefix):
    return [key for key in run[2] if key.startswith(prefix)]


def test_categorization_device_enrich(cli):
    default = cli("default")
    assert len(default[1]) > 1 and sum(ln.startswith("#") for ln in default[0]) > 3
    assert not keys(default, "enrich.") and not keys(default, "forest.")
    for name, env in (("enrich", {}), ("enrich_forest", dict(HGA_DEVICE_FOREST="1")),
                      ("enrich_sets", dict(HGA_DEVICE_SETS="1"))):
        got = cli(name, HGA_DEVICE_ENRICH="1", **env)
        assert got[0] == default[0] and got[1] == default[1]
        at = got[3].index("Calculation of enrichment connections")
        assert got[3] == default[3] and got[3][at + 1] == "Merging into core components"
        t = got[2]
        assert int(t["enrich.device_calls"]) == 1
        # (tests/test_forest_restricted.py checks on the CPU that this workload's list is longer than its forest)
        assert int(t["enrich.connections"]) > int(t["enrich.edges"]) >= 1
        assert bool(keys(got, "forest.")) == ("HGA_DEVICE_FOREST" in env)
        if "HGA_DEVICE_FOREST" in env:
            assert int(t["forest.device_calls"]) == 1
    assert cli("enrich")[2]["enrich.edges"] == cli("enrich_sets")[2]["enrich.edges"]


def test_categorization_enrich_capped_host_and_two_ranks(cli):
    default = cli("default")
    capped = cli("capped", extra=("--sc_max_size", "40"))
    capped_enrich = cli("capped_enrich", extra=("--sc_max_size", "40"), HGA_DEVICE_ENRICH="1")
    assert capped_enrich[0] == capped[0] and capped_enrich[1] == capped[1]
    assert not keys(capped, "enrich.") and not keys(capped_enrich, "forest.")
    host = cli("host_conn", HGA_DEVICE_ENRICH="1", HGA_HOST_CONNECTIONS="1")   # the switch needs the device state
    assert not keys(host, "enrich.") and host[0] == default[0] and host[1] == default[1]
    two = cli("two", gpus=2, HGA_DEVICE_ENRICH="1")
    assert two[0] == default[0] and two[1] == default[1]
    assert int(two[2]["enrich.device_calls"]) == 1 and not keys(two, "forest.")
    one = cli("enrich", HGA_DEVICE_ENRICH="1")[2]
    assert (two[2]["enrich.connections"], two[2]["enrich.edges"]) == (one["enrich.connections"], one["enrich.edges"])
