"""hga_read_overlaps (approximate_read_overlap per spanning-tree edge, ReadClusteringEngine.cpp:491-513)
on the MI355X: the kernel bit-exact against the numpy distinct-list formula (tests/overlap_ref.py, pinned
to the restatement's multiset formulation by tests/test_overlaps.py), the entry point's error and state
rules, and bin/categorization with the tail stage's edge overlaps on the device against its host path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import overlap_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hybrid-genome-assembler_amd", "bin")
HGA_ERR_INVALID, HGA_ERR_STATE = 1, 4


def kmer_str(code, k):
    return "".join("ACGT"[(int(code) >> (2 * (k - 1 - i))) & 3] for i in range(k))


def lookup(ctx, bases, offsets, k, sdk, first_id=1):
    ctx.lookup_load(k, sdk)
    ctx.lookup_set_reads(bases, offsets, first_id)
    ctx.lookup_run()


def check(ctx, idx, x, y, first_id=1):
    x, y = np.asarray(x, np.uint32), np.asarray(y, np.uint32)
    ov, sh = ctx.read_overlaps(x, y)
    want_ov, want_sh = overlap_ref.read_overlaps(idx, x, y, first_id)
    assert ov.dtype == np.int32 and sh.dtype == np.uint32
    assert np.array_equal(sh, want_sh)
    assert np.array_equal(ov, want_ov)
    return want_ov, want_sh


def test_read_overlaps_against_numpy(gpu_ctx, hga_mod):
    first_id = 1000
    bases, offsets, k, sdk, idx = overlap_ref.nanosim_case(hga_mod, first_id)
    n = len(offsets) - 1
    lookup(gpu_ctx, bases, offsets, k, sdk, first_id)
    got = gpu_ctx.lookup_fetch()
    assert np.array_equal(got["first_kid"], idx["first_kid"]) and np.array_equal(got["first_pos"], idx["first_pos"])
    rng = np.random.default_rng(5)
    cx, cy, _, _ = oracle.connections(idx, min_score=1, first_read_id=first_id)
    assert len(cx) > 1000
    no_hits = first_id + np.flatnonzero(np.diff(idx["first_ptr"]) == 0).astype(np.uint32)
    assert len(no_hits) >= 2
    rx, ry = rng.integers(first_id, first_id + n, (2, 2000)).astype(np.uint32)
    same = rng.integers(first_id, first_id + n, 50).astype(np.uint32)
    other = rng.integers(first_id, first_id + n, len(no_hits)).astype(np.uint32)
    x = np.concatenate([cx, rx, same, cx[:20], cx[:20], no_hits, no_hits, no_hits[:1]])
    y = np.concatenate([cy, ry, same, cy[:20], cy[:20], other, no_hits[::-1], no_hits[:1]])
    x, y = np.concatenate([x, y]), np.concatenate([y, x])   # each pair reversed as well
    want_ov, want_sh = check(gpu_ctx, idx, x, y, first_id)
    assert (want_sh[:len(cx)] > 0).all() and (want_ov > 0).sum() > 1000 and (want_sh == 0).sum() > 100


def test_read_overlaps_length_edges(gpu_ctx, hga_mod):
    bases, offsets, k, sdk, idx, names = overlap_ref.length_edge_case(hga_mod)
    cnt = dict(zip(names, np.diff(idx["first_ptr"]).tolist()))
    assert [cnt[f"n{v}"] for v in (0, 1, 63, 64, 65, 127, 128, 129)] == [0, 1, 63, 64, 65, 127, 128, 129]
    assert min(cnt["whole"], cnt["front"], cnt["back"]) > 4096
    lookup(gpu_ctx, bases, offsets, k, sdk)
    n = len(names)
    x, y = np.divmod(np.arange(n * n), n)   # every ordered pair, x == y included
    want_ov, want_sh = check(gpu_ctx, idx, x + 1, y + 1)
    at = lambda a, b: names.index(a) * n + names.index(b)
    assert (want_ov[at("left_of_w1", "right_of_w1")], want_sh[at("left_of_w1", "right_of_w1")]) == (0, 1)
    assert (want_ov[at("n1", "whole")], want_sh[at("n1", "whole")]) == (0, 1)
    fp, fk = idx["first_ptr"], idx["first_kid"]
    lst = lambda a: fk[fp[names.index(a)]:fp[names.index(a) + 1]]
    assert np.intersect1d(lst("n64"), lst("ends_of_n64")).tolist() == [lst("n64")[0], lst("n64")[-1]]
    assert want_sh[at("n64", "ends_of_n64")] == 2 and want_ov[at("n64", "ends_of_n64")] > 0
    for v in (63, 64, 65, 127, 128, 129):
        assert want_sh[at(f"n{v}", "whole")] == v == want_sh[at(f"n{v}", f"n{v}")]
    assert want_sh[at("front", "back")] > 4096


def test_read_overlaps_errors_and_state(gpu_ctx, hga_mod):
    L = hga_mod.lib()
    one = np.array([1], np.uint32)
    with hga_mod.Ctx(int(os.environ.get("HGA_DEVICE", "0"))) as fresh:
        assert L.hga_read_overlaps(fresh._h, one.ctypes.data_as(C.POINTER(C.c_uint32)),
                                   one.ctypes.data_as(C.POINTER(C.c_uint32)), 1, None, None) == HGA_ERR_STATE
        with pytest.raises(hga_mod.HgaError, match=f"status {HGA_ERR_STATE}"):
            fresh.read_overlaps(one, one)
    first_id = 1000
    bases, offsets, k, sdk, idx = overlap_ref.nanosim_case(hga_mod, first_id)
    n = len(offsets) - 1
    lookup(gpu_ctx, bases, offsets, k, sdk, first_id)
    good = np.array([first_id, first_id + n - 1, first_id + 7], np.uint32)
    check(gpu_ctx, idx, good, good[::-1], first_id)
    for bad in (first_id - 1, first_id + n):
        for pos in range(3):
            b = good.copy()
            b[pos] = bad
            for x, y in ((b, good), (good, b)):
                with pytest.raises(hga_mod.HgaError, match=f"status {HGA_ERR_INVALID}"):
                    gpu_ctx.read_overlaps(x, y)
    ov, sh = gpu_ctx.read_overlaps(np.zeros(0, np.uint32), np.zeros(0, np.uint32))   # n = 0
    assert len(ov) == 0 and len(sh) == 0
    assert L.hga_read_overlaps(gpu_ctx._h, None, None, 0, None, None) == 0
    # either output may be NULL
    rng = np.random.default_rng(1)
    x, y = rng.integers(first_id, first_id + n, (2, 300)).astype(np.uint32)
    want_ov, want_sh = overlap_ref.read_overlaps(idx, x, y, first_id)
    px, py = x.ctypes.data_as(C.POINTER(C.c_uint32)), y.ctypes.data_as(C.POINTER(C.c_uint32))
    ov, sh = np.full(300, -7, np.int32), np.full(300, 9, np.uint32)
    assert L.hga_read_overlaps(gpu_ctx._h, px, py, 300, ov.ctypes.data_as(C.POINTER(C.c_int32)), None) == 0
    assert L.hga_read_overlaps(gpu_ctx._h, px, py, 300, None, sh.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
    assert L.hga_read_overlaps(gpu_ctx._h, px, py, 300, None, None) == 0
    assert np.array_equal(ov, want_ov) and np.array_equal(sh, want_sh)
    # another lookup on the same ctx: the answers follow it (reads in reverse order, ReadIDs from 1)
    lens = np.diff(offsets).astype(np.int64)
    rev = b"".join(bases[int(offsets[i]):int(offsets[i + 1])] for i in range(n - 1, -1, -1))
    roff = np.concatenate([[0], np.cumsum(lens[::-1])]).astype(np.uint64)
    lookup(gpu_ctx, rev, roff, k, sdk, 1)
    ridx = oracle.construct_indices(rev, roff, k, sdk, 1)
    x1, y1 = (first_id + n - x).astype(np.uint32), (first_id + n - y).astype(np.uint32)   # the same reads' new ids
    got_ov, got_sh = check(gpu_ctx, ridx, x1, y1, 1)
    assert np.array_equal(got_ov, want_ov) and np.array_equal(got_sh, want_sh)
    with pytest.raises(hga_mod.HgaError, match=f"status {HGA_ERR_INVALID}"):
        gpu_ctx.read_overlaps([first_id], [first_id])   # past the new lookup's n reads
    # a lookup without a single hit: all zeros
    lookup(gpu_ctx, b"A" * 300, np.array([0, 100, 300], np.uint64), k, sdk, 5)
    assert gpu_ctx.lookup_sizes().firsts == 0
    ov, sh = gpu_ctx.read_overlaps([5, 6, 5], [6, 6, 5])
    assert not ov.any() and not sh.any()


@pytest.fixture(scope="module")
def cli_case(tmp_path_factory, hga_mod):
    """The 40 kb two-haplotype workload of test_cli_gpu.py::test_categorization_clusters_and_export in its
    second configuration: it reaches "Calculation of tail connections" with 219 spanning-tree edges
    between never-merged components and 50 touching a merge survivor (counted on the host with
    cluster_host(batched_overlaps=True))."""
    import pyref_cluster as pc
    tmp = tmp_path_factory.mktemp("overlaps_cli")
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

    def run(name, gpus=1, host_overlaps=False):
        env = dict(os.environ, HGA_TIMING="1")
        env.pop("HGA_HOST_OVERLAPS", None)
        if host_overlaps:
            env["HGA_HOST_OVERLAPS"] = "1"
        out = subprocess.run([os.path.join(BIN, "categorization"), *paths, "-k", str(tmp / "sdk.txt"), "-d", "-o",
                              str(tmp / name), *args, "--gpus", str(gpus)], capture_output=True, text=True, cwd=tmp,
                             env=env, timeout=300)
        assert out.returncode == 0, out.stderr
        timing = dict(ln.split()[1:3] for ln in out.stderr.splitlines() if ln.startswith("hga-timing tails.overlap_edges"))
        lines = [ln for ln in out.stdout.splitlines() if " took " not in ln]
        files = {f: open(tmp / name / f).read() for f in sorted(os.listdir(tmp / name))}
        assert "Calculation of tail connections took" in out.stdout
        return lines, files, int(timing["tails.overlap_edges_device"]), int(timing["tails.overlap_edges_host"])

    return run, eng.printed


def test_categorization_device_overlaps_equal_host(cli_case):
    run, printed = cli_case
    dev = run("dev")
    host = run("host", host_overlaps=True)
    assert dev[0] == host[0]
    assert dev[1] == host[1] and len(dev[1]) > 1
    assert [ln for ln in dev[0] if ln.startswith("#")] == printed
    assert dev[2] > 0 and dev[3] > 0 and dev[2] + dev[3] == host[3]
    assert host[2] == 0


def test_categorization_device_overlaps_two_ranks(cli_case):
    """--gpus 2: rank 0's ctx holds the gathered index (hga_lookup_gather), so the engine's default
    hga_read_overlaps call answers for every read."""
    run, printed = cli_case
    one = run("one")
    two = run("two", gpus=2)
    assert one[0] == two[0]
    assert one[1] == two[1] and len(one[1]) > 1
    assert two[2] > 0 and two[2:] == one[2:]
