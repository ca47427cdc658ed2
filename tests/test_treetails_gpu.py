"""hga_tree_tails on the MI355X against tests/treetails_ref.py: every shape and arithmetic kind with explicit
overlaps and lengths, the pointer-jumping rounds, a forest and its permutation, overlap = NULL on merged
component states, the error and state rules, a gathered two-rank ctx, and bin/categorization under
HGA_DEVICE_TAILS=1 / 0."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import oracle
import tailsets_ref as tr
import treetails_ref as tt
from test_tailsets_gpu import cli_case, lookup, same_state, state_snapshot   # noqa: F401 (cli_case: a fixture)

pytestmark = pytest.mark.gpu
HGA_ERR_INVALID, HGA_ERR_STATE = 1, 4
AVG_TAIL = 20000


@pytest.fixture(scope="module")
def wide_ctx(hga_mod):
    """A ctx whose lookup holds tt.N_READS short reads from tt.FIRST_ID on: the id range of the forests."""
    rng = np.random.default_rng(2)
    gnm = bytes(rng.choice(list(b"ACGT"), 6000).tolist())
    starts = rng.integers(0, 6000 - 40, tt.N_READS)
    lens = rng.integers(20, 40, tt.N_READS)
    bases = b"".join(gnm[s:s + n] for s, n in zip(starts.tolist(), lens.tolist()))
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    codes, _ = oracle.kmer_windows(gnm, 15)
    ctx = hga_mod.Ctx(int(os.environ.get("HGA_DEVICE", "0")))
    ctx.lookup_load(15, np.unique(codes)[::7])
    ctx.lookup_set_reads(bases, offsets, tt.FIRST_ID)
    ctx.lookup_run()
    assert ctx.lookup_sizes().n_reads == tt.N_READS
    ctx.own_lengths = lens.astype(np.uint32)
    yield ctx
    ctx.close()


def compare(got, want):
    left, right, ends = got
    assert len(left) == len(right) == len(ends) == len(want)
    bad = [t for t, r in enumerate(want)
           if left[t].tolist() != r.left or right[t].tolist() != r.right or tuple(map(int, ends[t])) != r.ends]
    assert not bad, [(t, ends[t], want[t].ends, len(left[t]), len(want[t].left), len(right[t]), len(want[t].right))
                     for t in bad[:4]]


@pytest.mark.parametrize("kind", ["plain", "equal", "wrap", "negative"])
def test_shapes_in_one_call(kind, wide_ctx):
    f, w = tt.shapes_forest(), tt.weights("shapes", kind)
    for tail in (AVG_TAIL,) + tt.TAILS:
        got = wide_ctx.tree_tails(f.trees, w.overlap, w.length, tail)
        assert got[0][0].dtype == np.uint32
        compare(got, tt.expected("shapes", kind, tail))


def test_rounds_follow_the_largest_tree_not_the_depth(wide_ctx):
    f, w = tt.shapes_forest(), tt.weights("shapes", "plain")
    at = np.concatenate([[0], np.cumsum([len(t) for t in f.trees])])
    wide_ctx.profile(True)
    try:
        for t, tree in enumerate(f.trees):
            if len(tree) not in (1, 31, 32, 33, 1023, 1024, 1025, 3000):
                continue
            ov = w.overlap[at[t]:at[t + 1]]
            wide_ctx.profile_reset()
            got = wide_ctx.tree_tails([tree], ov, w.length, AVG_TAIL)
            compare(got, [tt.TreeRef(tree, ov.tolist(), w.by_id, AVG_TAIL)])
            assert wide_ctx.profile_get("tt_jump")[1] == math.ceil(math.log2(2 * len(tree))), len(tree)
            for name in ("tt_expand", "tt_link", "tt_pos", "tt_finish"):
                assert wide_ctx.profile_get(name)[1] == 1, name
            for name in ("tt_weigh", "tt_far_dist", "tt_far_id", "tt_scan_apply"):
                assert wide_ctx.profile_get(name)[1] == 3, name
        wide_ctx.profile_reset()
        wide_ctx.tree_tails(f.trees, w.overlap, w.length, AVG_TAIL)
        assert wide_ctx.profile_get("tt_jump")[1] == 14   # 2 * 4999 directed edges in the largest tree
        assert wide_ctx.profile_get("co_wave")[1] == 0    # explicit overlaps: none computed
    finally:
        wide_ctx.profile(False)


@pytest.mark.parametrize("kind", ["plain", "wrap"])
def test_forest_and_its_permutation(kind, wide_ctx):
    f, w = tt.random_forest(), tt.weights("forest", kind)
    want = tt.expected("forest", kind, AVG_TAIL)
    got = wide_ctx.tree_tails(f.trees, w.overlap, w.length, AVG_TAIL)
    compare(got, want)
    at = np.concatenate([[0], np.cumsum([len(t) for t in f.trees])])
    order = np.random.default_rng(4).permutation(len(f.trees))
    ov = np.concatenate([w.overlap[at[t]:at[t + 1]] for t in order])
    again = wide_ctx.tree_tails([f.trees[t] for t in order], ov, w.length, AVG_TAIL)
    for i, t in enumerate(order):
        assert again[0][i].tolist() == got[0][t].tolist() and again[1][i].tolist() == got[1][t].tolist()
        assert again[2][i] == got[2][t]


def test_null_read_length_is_the_ctx_own_reads(wide_ctx):
    f, w = tt.random_forest(), tt.weights("forest", "plain")
    trees = f.trees[:40]
    ov = w.overlap[:sum(len(t) for t in trees)] % 17
    by_id = {tt.FIRST_ID + i: int(l) for i, l in enumerate(wide_ctx.own_lengths)}
    compare(wide_ctx.tree_tails(trees, ov, None, 50), tt.tree_tails(trees, ov.tolist(), by_id, 50))


@pytest.mark.parametrize("make", [tr.case_a, tr.case_b], ids=["A", "B"])
def test_null_overlap_follows_the_merges(make, gpu_ctx, hga_mod):
    ref = make(hga_mod)
    c = ref.c
    lookup(gpu_ctx, c)
    lengths = np.diff(np.asarray(c.offsets, np.uint64)).astype(np.uint32)
    by_id = {c.first_id + i: int(l) for i, l in enumerate(lengths)}
    tail = 2 * int(lengths.mean())
    gpu_ctx.profile(True)
    try:
        for st in ref.steps:
            if st.no:
                gpu_ctx.components_merge(c.steps[st.no].groups)
            trees, host_ov = tt.merged_trees(ref, st.no)
            before = state_snapshot(gpu_ctx)
            x = [a for t in trees for a, _ in t]
            y = [b for t in trees for _, b in t]
            ov, _ = gpu_ctx.components_overlaps(x, y)
            assert ov.tolist() == host_ov
            want = tt.tree_tails(trees, ov.tolist(), by_id, tail)
            gpu_ctx.profile_reset()
            compare(gpu_ctx.tree_tails(trees, tail_length=tail), want)          # both NULL
            assert gpu_ctx.profile_get("co_wave")[1] == 1
            compare(gpu_ctx.tree_tails(trees, None, lengths, tail), want)       # the engine's call
            compare(gpu_ctx.tree_tails(trees, ov, lengths, tail), want)
            assert same_state(state_snapshot(gpu_ctx), before)
    finally:
        gpu_ctx.profile(False)
    got = gpu_ctx.lookup_fetch()
    for name, value in c.idx.items():
        if name in got:
            assert np.array_equal(got[name], value), name


SENT = 0xA5


def raw_call(hga_mod, ctx, tree_ptr, edges, n_trees, overlap=None, tail=7):
    """The C entry with sentinel-filled outputs: (status, whether every output byte is still the sentinel)."""
    tp = np.asarray(tree_ptr, np.uint64)
    xy = np.asarray(edges, np.uint32).reshape(-1, 2)
    ex, ey = np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1])
    ov = None if overlap is None else np.asarray(overlap, np.int32)
    n_out = len(ex) + n_trees + 1
    outs = [np.full(n_trees + 1, SENT, np.uint8).repeat(8), np.full(n_out * 4, SENT, np.uint8),
            np.full(n_trees + 1, SENT, np.uint8).repeat(8), np.full(n_out * 4, SENT, np.uint8),
            np.full(max(n_trees, 1) * C.sizeof(hga_mod.TreeEnds), SENT, np.uint8)]
    p = lambda a, ct: a.ctypes.data_as(C.POINTER(ct))
    st = hga_mod.lib().hga_tree_tails(ctx._h, p(tp, C.c_uint64), p(ex, C.c_uint32), p(ey, C.c_uint32), n_trees,
                                      None if ov is None else p(ov, C.c_int32), None, tail, p(outs[0], C.c_uint64),
                                      p(outs[1], C.c_uint32), p(outs[2], C.c_uint64), p(outs[3], C.c_uint32),
                                      p(outs[4], hga_mod.TreeEnds))
    return st, all((o == SENT).all() for o in outs)


def test_errors_leave_outputs_and_state(hga_mod, gpu_ctx):
    L = hga_mod.lib()
    with hga_mod.Ctx(int(os.environ.get("HGA_DEVICE", "0"))) as fresh:
        assert raw_call(hga_mod, fresh, [0, 1], [(1, 2)], 1, [0]) == (HGA_ERR_STATE, True)
        with pytest.raises(hga_mod.HgaError, match=f"status {HGA_ERR_STATE}"):
            fresh.tree_tails([[(1, 2)]], [0], None, 1)
    ref = tr.case_b(hga_mod)
    c = ref.c
    lookup(gpu_ctx, c)
    gpu_ctx.components_merge(c.steps[1].groups)
    merged = state_snapshot(gpu_ctx)
    first, last = c.first_id, c.first_id + c.n - 1
    a, b, d, e, g = (int(i) for i in c.rest[150:155])
    bad = {
        "decreasing tree_ptr": ([0, 2, 1], [(a, b), (b, d)], 2),
        "id below the reads": ([0, 1], [(first - 1, a)], 1),
        "id above the reads": ([0, 2], [(a, b), (b, last + 1)], 1),
        "id in two trees": ([0, 1, 2], [(a, b), (b, d)], 2),
        "self-loop": ([0, 2], [(a, b), (b, b)], 1),
        "repeated edge": ([0, 2], [(a, b), (a, b)], 1),
        "repeated edge, reversed": ([0, 3], [(a, b), (d, a), (b, a)], 1),
        "cycle": ([0, 3], [(a, b), (b, d), (d, a)], 1),
        "two parts": ([0, 2], [(a, b), (d, e)], 1),
        "triangle and an edge": ([0, 4], [(a, b), (b, d), (d, a), (e, g)], 1),   # E + 1 vertices, no tree
        "a bad tree after a good one": ([0, 1, 3], [(a, b), (d, e), (e, d)], 2),
    }
    for name, (tp, edges, nt) in bad.items():
        for ov in (None, [3] * len(edges)):
            assert raw_call(hga_mod, gpu_ctx, tp, edges, nt, ov) == (HGA_ERR_INVALID, True), name
        assert same_state(state_snapshot(gpu_ctx), merged), name
    with pytest.raises(hga_mod.HgaError, match=f"status {HGA_ERR_INVALID}"):
        gpu_ctx.tree_tails([[(a, b), (b, a)]], [1, 1], None, 1)
    # no trees; only empty trees
    assert L.hga_tree_tails(gpu_ctx._h, None, None, None, 0, None, None, 0, None, None, None, None, None) == 0
    assert gpu_ctx.tree_tails([]) == ([], [], [])
    left, right, ends = gpu_ctx.tree_tails([[], []], tail_length=5)
    assert [len(v) for v in left + right] == [0, 0, 0, 0] and ends == [(0, 0, 0, 0)] * 2
    # and the call still answers on the merged state
    trees, host_ov = tt.merged_trees(ref, 1)
    lengths = np.diff(np.asarray(c.offsets, np.uint64))
    by_id = {c.first_id + i: int(l) for i, l in enumerate(lengths)}
    compare(gpu_ctx.tree_tails(trees, tail_length=4000), tt.tree_tails(trees, host_ov, by_id, 4000))
    assert same_state(state_snapshot(gpu_ctx), merged)


def _gathered_worker(rank, world, port, out_path):
    """The set-up of tests/test_dist_gpu.py's sharded lookup (its case, its attach), then hga_tree_tails on
    the gathered index."""
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
        lengths = np.array([len(r) for r in reads], np.uint32)
        by_id = {1 + i: int(l) for i, l in enumerate(lengths)}
        ids = (1 + np.random.default_rng(8).permutation(len(reads))[:120]).tolist()   # ids of both ranks' reads
        trees = [[(ids[i], ids[i + 1]) for i in range(59)], [(ids[60], v) for v in ids[61:]]]
        own = [[(1 + a + i, 1 + a + i + 1) for i in range(20)]]
        own_by_id = {1 + a + i: len(r) for i, r in enumerate(mine)}
        before = ctx.tree_tails(own, tail_length=300)   # before the gather: this rank's own reads, NULL lengths
        x, y = [p for t in own for p, _ in t], [q for t in own for _, q in t]
        want = tt.tree_tails(own, ctx.components_overlaps(x, y)[0].tolist(), own_by_id, 300)
        assert [v.tolist() for v in before[0]] == [r.left for r in want] and before[2] == [r.ends for r in want]
        ctx.lookup_gather()
        try:
            ctx.tree_tails(trees, tail_length=300)
            raise AssertionError("NULL read_length on a gathered ctx was accepted")
        except hga.HgaError as err:
            assert "status 4" in str(err), str(err)
        x, y = [p for t in trees for p, _ in t], [q for t in trees for _, q in t]
        ov, _ = ctx.components_overlaps(x, y)
        got = ctx.tree_tails(trees, None, lengths, 300)
        want = tt.tree_tails(trees, ov.tolist(), by_id, 300)
        assert [v.tolist() for v in got[0]] == [r.left for r in want]
        assert [v.tolist() for v in got[1]] == [r.right for r in want]
        assert got[2] == [r.ends for r in want]
        open(out_path + f".{rank}.ok", "w").write(str(int((ov > 0).sum())))
    finally:
        ctx.close()
        dist.destroy_process_group()


def test_gathered_ctx_needs_read_lengths(tmp_path):
    import torch.multiprocessing as mp
    from test_dist import _free_port
    out = str(tmp_path / "tt")
    mp.start_processes(_gathered_worker, args=(2, _free_port(), out), nprocs=2, start_method="spawn")
    for rank in range(2):
        assert os.path.exists(out + f".{rank}.ok")


def test_categorization_device_tails(cli_case):
    run, printed = cli_case
    dev = run("tt_dev", HGA_DEVICE_SETS="1", HGA_DEVICE_TAILS="1")
    host = run("tt_host", HGA_DEVICE_SETS="1", HGA_DEVICE_TAILS="0")
    two = run("tt_two", gpus=2, HGA_DEVICE_SETS="1", HGA_DEVICE_TAILS="1")
    off = run("tt_off", HGA_DEVICE_TAILS="1")   # without HGA_DEVICE_SETS=1 nothing changes
    for other in (host, two, off):
        assert dev[0] == other[0]
        assert dev[1] == other[1] and len(dev[1]) > 1
    assert [ln for ln in dev[0] if ln.startswith("#")] == printed
    for t in (dev[2], two[2]):
        assert int(t["tails.tree_tails_calls"]) == 1 and "tails.tree_tails_device" in t
        assert int(t["tails.overlap_edges_host"]) == 0
        assert int(t["tails.overlap_edges_device"]) == int(host[2]["tails.overlap_edges_device"]) > 0
        assert float(t["tails.spanning_tree_tails"]) >= float(t["tails.tree_tails_device"])
    for t in (host[2], off[2]):
        assert "tails.tree_tails_calls" not in t and "tails.tree_tails_device" not in t
    assert int(host[2]["tails.overlap_edges_host"]) == 0 and int(off[2]["tails.overlap_edges_host"]) > 0
