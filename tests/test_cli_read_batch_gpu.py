"""bin/categorization --read-batch SIZE: the lookup fed in read batches.  The index file, the debug line and
the exported clusters are what tests/test_cli_gpu.py compares the default run with (the golden index, which
is the oracle's, and the Python restatement of run_clustering + export_components), on one rank and on two;
HGA_TIMING=1 reports the batches; a zero or malformed SIZE is an argument error worded as --mem-budget's."""
import os
import subprocess

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "hybrid-genome-assembler_amd", "bin")
GOLD = os.path.join(ROOT, "tests", "golden")


def kmer_str(code, k):
    return "".join("ACGT"[(int(code) >> (2 * (k - 1 - i))) & 3] for i in range(k))


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [["--read-batch", "2K"], ["--gpus", "2", "--read-batch=2K"]], ids=["one_rank", "two_ranks"])
def test_categorization_golden_in_read_batches(tmp_path, extra):
    g = np.load(os.path.join(GOLD, "lookup_golden.npz"))
    paths = [os.path.join(GOLD, p) for p in ("reads_a.fq", "reads_b.fq", "reads_c.fa")]
    out = subprocess.run([os.path.join(BIN, "categorization"), *paths, "-k", os.path.join(GOLD, "sdk_19.txt"),
                          "-d", "--index-out", str(tmp_path / "idx.bin"), *extra], capture_output=True, text=True,
                         cwd=tmp_path, timeout=300, env=dict(os.environ, HGA_TIMING="1"))
    assert out.returncode == 0, out.stderr
    assert "reads_a.fq:\n- " in out.stdout and "Index construction took " in out.stdout
    cat = g["category"]
    disc = tot = 0
    for i in range(len(g["kci_ptr"]) - 1):
        cs = {int(cat[r - 1]) for r in g["kci_read"][g["kci_ptr"][i]:g["kci_ptr"][i + 1]]}
        disc += len(cs) == 1
        tot += len(cs) > 0
    assert f"{disc} out of {tot} kmers are discriminative \n" in out.stdout
    raw = open(tmp_path / "idx.bin", "rb").read()
    n, H, U, K, k = np.frombuffer(raw[:40], np.uint64)
    assert (n, H, U, K, k) == (len(g["hit_ptr"]) - 1, len(g["hit_kid"]), len(g["first_kid"]), len(g["kci_ptr"]) - 1, 19)
    off = 40
    for name, cnt, dt in [("hit_ptr", n + 1, np.uint64), ("sorted_kid", H, np.uint32), ("first_ptr", n + 1, np.uint64),
                          ("first_kid", U, np.uint32), ("first_pos", U, np.uint32), ("kci_ptr", K + 1, np.uint64),
                          ("kci_read", H, np.uint32)]:
        arr = np.frombuffer(raw[off:off + int(cnt) * np.dtype(dt).itemsize], dt)
        off += int(cnt) * np.dtype(dt).itemsize
        assert np.array_equal(arr, g[name]), name
    # rank 0's batches: its share of the bases in pieces of at most 2 KiB
    timing = dict(ln.split()[1:3] for ln in out.stderr.splitlines() if ln.startswith("hga-timing "))
    assert int(timing["lookup.batches"]) > 4 and int(timing["lookup.slot_bytes"]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [["--read-batch", "2K"], ["--gpus", "2", "--read-batch", "2K"]], ids=["one_rank", "two_ranks"])
def test_categorization_clusters_in_read_batches(tmp_path, hga_mod, extra):
    """The whole run against the Python restatement, as test_categorization_clusters_and_export."""
    import pyref_cluster as pc
    k = 15
    cfg = dict(sc_min=5, sc_max=-1, sc_fraction=0.15, sc_score=0, enrich=8, tail=10, dims=16)
    ga = hga_mod.gen_genome(40_000, 5)
    gb = hga_mod.gen_haplotype(ga, 0.02, 0, 6)
    paths = [str(tmp_path / "hapA.fa"), str(tmp_path / "hapB.fa")]
    hga_mod.write_nanosim_fasta(ga, "hapA", 180, 7, paths[0])
    hga_mod.write_nanosim_fasta(gb, "hapB", 180, 8, paths[1])
    ka, _ = oracle.kmer_windows(ga, k)
    kb, _ = oracle.kmer_windows(gb, k)
    sdk = np.setxor1d(np.unique(ka), np.unique(kb))
    (tmp_path / "sdk.txt").write_text("".join(kmer_str(c, k) + "\n" for c in sdk))
    out = subprocess.run([os.path.join(BIN, "categorization"), *paths, "-k", str(tmp_path / "sdk.txt"), "-d",
                          "-o", str(tmp_path / "clusters"), "--sc_min_size", "5", "--core_enrichment", "8",
                          "--tail_amplification", "10", *extra], capture_output=True, text=True, cwd=tmp_path, timeout=300)
    assert out.returncode == 0, out.stderr
    rec = hga_mod.load_records(paths, True)
    idx = oracle.construct_indices(rec["bases"], rec["offsets"], k, sdk)
    lengths = np.diff(rec["offsets"])
    eng = pc.Engine(idx, lengths, rec["category"], int(rec["meta"][-1][4]), True, cfg, start=rec["start"],
                    end=rec["end"])
    want = eng.run()
    assert f"Exported {len(want)} components\n" in out.stdout
    assert [ln for ln in out.stdout.splitlines() if ln.startswith("#")] == eng.printed
    files = sorted(os.listdir(tmp_path / "clusters"))
    assert files == sorted(f"#{c}.fa" for c in want) and len(files) > 1
    headers = [l.split("\n")[0] for p in paths for l in open(p).read().split(">")[1:]]
    for c in want:
        text = open(tmp_path / "clusters" / f"#{c}.fa").read()
        members = sorted(eng.comps[c]["reads"])
        exp = "".join(f">{headers[r - 1]}\n{rec['bases'][rec['offsets'][r - 1]:rec['offsets'][r]].decode()}\n"
                      for r in members)
        assert text == exp


@pytest.mark.parametrize("size", ["0", "0K", "2X", "2KB", "abc", "", "99999999999G"])
def test_read_batch_size_errors(tmp_path, size):
    """No GPU: the options are parsed before anything else happens."""
    out = subprocess.run([os.path.join(BIN, "categorization"), "reads.fa", "-k", "sdk.txt", f"--read-batch={size}"],
                         capture_output=True, text=True, cwd=tmp_path, timeout=60)
    assert out.returncode != 0
    assert f"the argument ('{size}') for option '--read-batch' is invalid" in out.stderr
