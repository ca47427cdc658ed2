"""hga_spanning_forest on the MI355X, bit-exact against tests/forest_ref.py's Kruskal loop: explicit edge lists
(every shape of forest_ref.shapes, windows of one list), the launch counts the pointer doubling and the
rounds promise, the ctx's connection results (golden data, a merged component state, a gathered two-rank
ctx), the error and state rules, and bin/categorization under HGA_DEVICE_FOREST=1."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import forest_ref as fr
import oracle
import overlap_ref
import pyref_cluster as pc
import tailsets_ref as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hybrid-genome-assembler_amd", "bin")
GOLD = os.path.join(ROOT, "tests", "golden")
HGA_ERR_INVALID, HGA_ERR_STATE = 1, 4
DEVICE = int(os.environ.get("HGA_DEVICE", "0"))


def load_wide(ctx):
    """fr.N_READS short reads from fr.FIRST_ID on: the vertex range of forest_ref's shapes."""
    rng = np.random.default_rng(2)
    gnm = bytes(rng.choice(list(b"ACGT"), 6000).tolist())
    starts = rng.integers(0, 6000 - 40, fr.N_READS)
    lens = rng.integers(20, 40, fr.N_READS)
    bases = b"".join(gnm[s:s + n] for s, n in zip(starts.tolist(), lens.tolist()))
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    codes, _ = oracle.kmer_windows(gnm, 15)
    ctx.lookup_load(15, np.unique(codes)[::7])
    ctx.lookup_set_reads(bases, offsets, fr.FIRST_ID)
    ctx.lookup_run()
    assert ctx.lookup_sizes().n_reads == fr.N_READS


@pytest.fixture(scope="module")
def wide_ctx(hga_mod):
    ctx = hga_mod.Ctx(DEVICE)
    load_wide(ctx)
    yield ctx
    ctx.close()


def check(got, x, y, first=0, count=None):
    """got = (pos, x, y) of a call on entries [first, first + count) of the list (x, y)."""
    n = len(x)
    a = min(first, n)
    b = n if count is None else min(n, a + count)
    want = [a + p for p in fr.kruskal(x[a:b], y[a:b])]
    pos, gx, gy = got
    assert pos.dtype == np.uint64 and gx.dtype == np.uint32 and gy.dtype == np.uint32
    assert pos.tolist() == want
    assert np.array_equal(gx, np.asarray(x, np.uint32)[want]) and np.array_equal(gy, np.asarray(y, np.uint32)[want])
    return want


@pytest.mark.parametrize("name", sorted(fr.shapes()))
def test_explicit_edges(name, wide_ctx):
    x, y = fr.shapes()[name]
    got = wide_ctx.spanning_forest(x, y)
    assert got[0].tolist() == fr.expected(name)
    want = check(got, x, y)
    for min_size in (1, 3):   # union_find over the accepted connections alone repeats the full list's merges
        assert fr.replay(got[1], got[2], range(len(want)), min_size) == fr.full(x, y, min_size)


def test_launch_counts_of_the_chains(wide_ctx):
    wide_ctx.profile(True)
    try:
        # the ascending chain hooks into one path of depth 4096 in its only round: 12 doublings flatten it,
        # and the round that finds nothing left launches one more
        x, y = fr.shapes()["chain"]
        assert fr.model("chain")[1:] == (1, 4096)
        wide_ctx.profile_reset()
        check(wide_ctx.spanning_forest(x, y), x, y)
        assert wide_ctx.profile_get("sf_jump")[1] <= 13
        assert wide_ctx.profile_get("sf_min")[1] == wide_ctx.profile_get("sf_hook")[1] == 2
        # the halving chain: a round joins neighbours pairwise only
        x, y = fr.shapes()["halving"]
        rounds = fr.model("halving")[1]
        assert rounds == 12
        wide_ctx.profile_reset()
        check(wide_ctx.spanning_forest(x, y), x, y)
        assert rounds <= wide_ctx.profile_get("sf_min")[1] <= rounds + 1
        assert wide_ctx.profile_get("sf_gather")[1] == 1
    finally:
        wide_ctx.profile(False)


def test_windows_of_one_list(wide_ctx):
    x, y = fr.shapes()["random_1"]
    n = len(x)
    for first, count in ((0, 0), (0, 1), (5, 2048), (2049, 7000), (0, 2049), (n - 100, 1000), (n, 5), (n + 9, 1),
                         (7, None)):
        want = check(wide_ctx.spanning_forest(x, y, first, count), x, y, first, count)
        assert want if first < n and count != 0 else want == []
    # the window's forest is the forest of the slice
    pos, gx, gy = wide_ctx.spanning_forest(x, y, 2049, 7000)
    alone = wide_ctx.spanning_forest(x[2049:9049], y[2049:9049])
    assert (alone[0] + 2049).tolist() == pos.tolist() and np.array_equal(alone[1], gx) and np.array_equal(alone[2], gy)


def forest_of_result(ctx, n, fractions=(0, 0.15, 0.3, 1.0)):
    """hga_spanning_forest on prefixes of the ctx's connection result of n rows against the fetched rows."""
    rows = ctx.connections_range(0, n)
    assert len(rows[0]) == n
    x, y = rows[0], rows[1]
    sizes = []
    for f in fractions:
        prefix = int(n * f)
        want = check(ctx.spanning_forest(first=0, count=prefix), x, y, 0, prefix)
        sizes.append(len(want))
        again = ctx.connections_range(0, n)   # the result is only read
        assert all(np.array_equal(a, b) for a, b in zip(rows, again))
    check(ctx.spanning_forest(), x, y)                    # to the end
    check(ctx.spanning_forest(first=n // 3, count=n // 2), x, y, n // 3, n // 2)
    return sizes


def test_on_a_connection_result(gpu_ctx, hga_mod):
    g = np.load(os.path.join(GOLD, "lookup_golden.npz"))
    rec = hga_mod.load_records([os.path.join(GOLD, p) for p in ("reads_a.fq", "reads_b.fq", "reads_c.fa")], True)
    gpu_ctx.lookup_load(19, g["sdk_keys_id_order"])
    gpu_ctx.lookup_set_reads(rec["bases"], rec["offsets"], 1)
    gpu_ctx.lookup_run()
    n = gpu_ctx.connections_run(min_score=1)
    sizes = forest_of_result(gpu_ctx, n)
    assert sizes[0] == 0 and 0 < sizes[1] <= sizes[2] <= sizes[3] < n


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
    sizes = forest_of_result(gpu_ctx, n)
    assert 0 < sizes[1] and sizes[3] < n


def _gathered_worker(rank, world, port, out_path):
    """tests/test_dist_gpu.py's sharded lookup and gathered connections, then the forest of the gathered list."""
    import torch.distributed as dist

    import hga
    import hga_dist
    from test_dist import lookup_case
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    ctx = hga.Ctx(0)
    try:
        hga_dist.attach(ctx)
        reads, sdk = lookup_case()
        a, b = len(reads) * rank // world, len(reads) * (rank + 1) // world
        mine = reads[a:b]
        ctx.lookup_load(13, sdk)
        ctx.lookup_set_reads(b"".join(mine), np.cumsum([0] + [len(r) for r in mine]).astype(np.uint64), 1 + a)
        ctx.lookup_run()
        ctx.lookup_gather()
        ctx.connections_run(pivots=np.arange(1 + a, 1 + b, dtype=np.uint32), min_score=2)
        n = ctx.connections_gather()
        ctx._conn_n = n
        sizes = forest_of_result(ctx, n)
        # explicit ids of the other rank's reads are vertices too
        other = np.arange(1, len(reads) + 1, dtype=np.uint32)
        check(ctx.spanning_forest(other[:-1], other[1:]), other[:-1], other[1:])
        open(out_path + f".{rank}.ok", "w").write(" ".join(map(str, [n] + sizes)))
    finally:
        ctx.close()
        dist.destroy_process_group()


def test_on_a_gathered_ctx(tmp_path):
    import torch.multiprocessing as mp
    from test_dist import _free_port
    out = str(tmp_path / "sf")
    mp.start_processes(_gathered_worker, args=(2, _free_port(), out), nprocs=2, start_method="spawn")
    seen = [open(out + f".{rank}.ok").read().split() for rank in range(2)]
    assert seen[0] == seen[1] and int(seen[0][0]) > 100 and 0 < int(seen[0][2]) < int(seen[0][0])


def raw(hga_mod, ctx, x, y, n, first, count, want_edges=True):
    p = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))
    m = C.c_uint64(12345)
    st = hga_mod.lib().hga_spanning_forest(ctx._h, p(x), p(y), n, first, count, C.byref(m) if want_edges else None)
    return st, m.value


def test_errors_and_state(hga_mod):
    L = hga_mod.lib()
    ALL = 2 ** 64 - 1
    one, two = np.array([fr.FIRST_ID], np.uint32), np.array([fr.FIRST_ID + 1], np.uint32)
    with hga_mod.Ctx(DEVICE) as ctx:
        # before hga_lookup_run
        assert raw(hga_mod, ctx, one, two, 1, 0, ALL)[0] == HGA_ERR_STATE
        assert raw(hga_mod, ctx, None, None, 0, 0, ALL)[0] == HGA_ERR_STATE
        assert L.hga_spanning_forest_fetch(ctx._h, None, None, None) == HGA_ERR_STATE
        with pytest.raises(hga_mod.HgaError, match=f"status {HGA_ERR_STATE}"):
            ctx.spanning_forest(one, two)
        load_wide(ctx)
        # no forest call yet; no connection result yet
        assert L.hga_spanning_forest_fetch(ctx._h, None, None, None) == HGA_ERR_STATE
        assert raw(hga_mod, ctx, None, None, 0, 0, ALL)[0] == HGA_ERR_STATE
        # exactly one NULL; a null n_edges
        assert raw(hga_mod, ctx, one, None, 1, 0, ALL)[0] == HGA_ERR_INVALID
        assert raw(hga_mod, ctx, None, two, 1, 0, ALL)[0] == HGA_ERR_INVALID
        assert raw(hga_mod, ctx, one, two, 1, 0, ALL, want_edges=False)[0] == HGA_ERR_INVALID
        with pytest.raises(ValueError):
            ctx.spanning_forest(one, None)
        assert L.hga_spanning_forest_fetch(ctx._h, None, None, None) == HGA_ERR_STATE   # none of them counted
        # a good call, then ids outside the reads: refused, and the earlier result stays
        x, y = fr.shapes()["doubled"]
        good = check(ctx.spanning_forest(x, y), x, y)
        last = fr.FIRST_ID + fr.N_READS - 1
        assert raw(hga_mod, ctx, np.array([last], np.uint32), np.array([fr.FIRST_ID], np.uint32), 1, 0, ALL) == (0, 1)
        check(ctx.spanning_forest(x, y), x, y)
        for bad in (fr.FIRST_ID - 1, last + 1, 0, 2 ** 32 - 1):
            for at in (0, 7, len(x) - 1):
                for side in (0, 1):
                    b = [x.copy(), y.copy()]
                    b[side][at] = bad
                    assert raw(hga_mod, ctx, b[0], b[1], len(x), 0, ALL) == (HGA_ERR_INVALID, 12345)
                    # ... unless the entry is outside the range the call works on
                    if at == 7:
                        assert raw(hga_mod, ctx, b[0], b[1], len(x), 8, ALL)[0] == 0
                        check(ctx.spanning_forest(x, y), x, y)
        pos = np.zeros(len(good), np.uint64)
        assert L.hga_spanning_forest_fetch(ctx._h, pos.ctypes.data_as(C.POINTER(C.c_uint64)), None, None) == 0
        assert pos.tolist() == good
        # x[i] == y[i] is legal; an empty clipped range is HGA_OK with no edge
        assert raw(hga_mod, ctx, one, one, 1, 0, ALL) == (0, 0)
        for first, count in ((0, 0), (len(x), 5), (len(x) + 100, ALL), (ALL, ALL)):
            assert raw(hga_mod, ctx, x, y, len(x), first, count) == (0, 0)
            assert L.hga_spanning_forest_fetch(ctx._h, None, None, None) == 0
        assert raw(hga_mod, ctx, None, None, 0, 0, 0)[0] == HGA_ERR_STATE   # still no connection result
        # more than 2^32 - 2 entries after clipping: refused before an entry is read; a window of them is fine
        assert raw(hga_mod, ctx, x, y, 2 ** 32, 0, ALL) == (HGA_ERR_INVALID, 12345)
        assert raw(hga_mod, ctx, x, y, 2 ** 32, 0, 2 ** 32 - 1) == (HGA_ERR_INVALID, 12345)
        assert raw(hga_mod, ctx, x, y, 2 ** 32, 0, len(x)) == (0, len(good))
        # each fetch output alone
        gx, gy = np.zeros(len(good), np.uint32), np.zeros(len(good), np.uint32)
        assert L.hga_spanning_forest_fetch(ctx._h, None, gx.ctypes.data_as(C.POINTER(C.c_uint32)), None) == 0
        assert L.hga_spanning_forest_fetch(ctx._h, None, None, gy.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
        assert np.array_equal(gx, x[good]) and np.array_equal(gy, y[good])
        # a connection result: the NULL form answers, and a later explicit call leaves the result alone
        n = ctx.connections_run(min_score=1)
        rows = ctx.connections_range(0, n)
        if n:
            check(ctx.spanning_forest(), rows[0], rows[1])
        check(ctx.spanning_forest(x, y), x, y)
        assert all(np.array_equal(a, b) for a, b in zip(rows, ctx.connections_range(0, n)))
        # hga_lookup_run ends the result's life, and the connection result's
        ctx.lookup_run()
        assert L.hga_spanning_forest_fetch(ctx._h, None, None, None) == HGA_ERR_STATE
        assert raw(hga_mod, ctx, None, None, 0, 0, ALL)[0] == HGA_ERR_STATE
        check(ctx.spanning_forest(x, y), x, y)


def kmer_str(code, k):
    return "".join("ACGT"[(int(code) >> (2 * (k - 1 - i))) & 3] for i in range(k))


@pytest.fixture(scope="module")
def cli(tmp_path_factory, hga_mod):
    """bin/categorization on overlap_ref.tails_case's files with default arguments (plus `extra`)."""
    tmp = tmp_path_factory.mktemp("forest_cli")
    paths, k, sdk, rec, idx, c = overlap_ref.tails_case(hga_mod, tmp)
    (tmp / "sdk.txt").write_text("".join(kmer_str(code, k) + "\n" for code in sdk))
    done = {}

    def run(name, extra=(), gpus=1, **env_add):
        if name in done:
            return done[name]
        env = dict(os.environ, HGA_TIMING="1")
        for var in ("HGA_HOST_CONNECTIONS", "HGA_HOST_OVERLAPS", "HGA_DEVICE_SETS", "HGA_SETS_BYTES", "HGA_DEVICE_TAILS",
                    "HGA_DEVICE_FOREST"):
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


def test_categorization_device_forest(cli):
    default = cli("default")
    assert len(default[1]) > 1 and sum(ln.startswith("#") for ln in default[0]) > 3
    assert not any(key.startswith("forest.") for key in default[2])
    for name, env in (("forest", {}), ("forest_sets", dict(HGA_DEVICE_SETS="1"))):
        got = cli(name, HGA_DEVICE_FOREST="1", **env)
        assert got[0] == default[0] and got[1] == default[1]
        at = got[3].index("Calculation of connections between reads")
        assert got[3] == default[3] and got[3][at + 1] == "Union-find"
        t = got[2]
        assert int(t["forest.device_calls"]) == 1
        # (tests/test_forest.py checks both on the CPU for this workload)
        assert int(t["forest.edges"]) > 1000 and int(t["forest.connections"]) > 2 * int(t["forest.edges"])


def test_categorization_forest_not_taken_and_two_ranks(cli):
    default = cli("default")
    capped = cli("capped", extra=("--sc_max_size", "40"))
    capped_forest = cli("capped_forest", extra=("--sc_max_size", "40"), HGA_DEVICE_FOREST="1")
    assert not any(key.startswith("forest.") for key in capped_forest[2])
    assert capped_forest[0] == capped[0] and capped_forest[1] == capped[1]
    host = cli("host_conn", HGA_DEVICE_FOREST="1", HGA_HOST_CONNECTIONS="1")   # the switch needs the device state
    assert not any(key.startswith("forest.") for key in host[2]) and host[0] == default[0] and host[1] == default[1]
    two = cli("two", gpus=2, HGA_DEVICE_FOREST="1")
    assert two[0] == default[0] and two[1] == default[1]
    assert int(two[2]["forest.device_calls"]) == 1
    assert two[2]["forest.edges"] == cli("forest", HGA_DEVICE_FOREST="1")[2]["forest.edges"]
