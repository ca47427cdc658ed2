"""Expected values of hga_read_overlaps: the distinct-list formula in numpy, and the workloads the
CPU and GPU overlap tests share."""
import numpy as np

import oracle


def read_overlaps(idx, x, y, first_id=1):
    """(overlap int32[n], shared uint32[n]) of the ReadID pairs (x[i], y[i]): S = the intersection of the
    two reads' first_kid slices; overlap = max over the two reads of max - min of first_pos over S, 0 if
    S is empty; shared = |S|."""
    fp, fk, fpos = idx["first_ptr"], idx["first_kid"], idx["first_pos"]
    ov, sh = np.zeros(len(x), np.int32), np.zeros(len(x), np.uint32)
    for i, (a, b) in enumerate(zip(x, y)):
        a, b = int(a) - first_id, int(b) - first_id
        a0, a1, b0, b1 = int(fp[a]), int(fp[a + 1]), int(fp[b]), int(fp[b + 1])
        s, ia, ib = np.intersect1d(fk[a0:a1], fk[b0:b1], assume_unique=True, return_indices=True)
        sh[i] = len(s)
        if len(s):
            pa, pb = fpos[a0:a1][ia].astype(np.int64), fpos[b0:b1][ib].astype(np.int64)
            ov[i] = max(pa.max() - pa.min(), pb.max() - pb.min())
    return ov, sh


def nanosim_case(hga_mod, first_id=1, k=17):
    """The 60 kb / 300 read / every 5th genome k-mer case of test_connect_gpu.py (k = 17 there), with
    two reads without hits appended if it has none: (bases, offsets, k, sdk, idx)."""
    gnm = hga_mod.gen_genome(60_000, 11)
    r = hga_mod.gen_nanosim(gnm, 300, 12)
    c, _ = oracle.kmer_windows(gnm, k)
    sdk = np.unique(c)[::5]
    bases, offsets = r.bases, np.asarray(r.offsets, np.uint64)
    idx = oracle.construct_indices(bases, offsets, k, sdk, first_id)
    if not (np.diff(idx["first_ptr"]) == 0).any():
        bases = bases + b"A" * 200
        offsets = np.concatenate([offsets, offsets[-1] + np.array([100, 200], np.uint64)])
        idx = oracle.construct_indices(bases, offsets, k, sdk, first_id)
    return bases, offsets, k, sdk, idx


def tails_case(hga_mod, tmp_path):
    """The workload of test_clustering.py::test_tails_and_spectral_stages_reached (500 kb, two haplotypes
    with identical stretches, more than 2 scaffold components): (fasta paths, k, sdk, rec, idx, cfg dict)."""
    L, GAP, PER, k = 500_000, 40_000, 150_000, 19
    ga = hga_mod.gen_genome(L, 11)
    gb = bytearray(hga_mod.gen_haplotype(ga, 0.021, 0, 12))
    for s0 in range(PER // 2, L, PER):
        gb[s0:s0 + GAP] = ga[s0:s0 + GAP]
    gb = bytes(gb)
    ra, rb = hga_mod.gen_art(ga, 30 * L // 150, 150, 13), hga_mod.gen_art(gb, 30 * L // 150, 150, 14)
    sdk = oracle.count_pipeline([ra.seq, rb.seq], k, 10, 25)["selected"]
    n = round(L / 7777 * 60)
    paths = [str(tmp_path / "a.fasta"), str(tmp_path / "b.fasta")]
    hga_mod.write_nanosim_fasta(ga, "A", n, 15, paths[0])
    hga_mod.write_nanosim_fasta(gb, "B", n, 16, paths[1])
    rec = hga_mod.load_records(paths, True)
    idx = oracle.construct_indices(rec["bases"], np.asarray(rec["offsets"], np.uint64), k, sdk)
    cfg = dict(sc_min=30, sc_max=-1, sc_fraction=0.15, sc_score=0, enrich=20, tail=40, dims=16)
    return paths, k, sdk, rec, idx, cfg


def length_edge_case(hga_mod):
    """Reads cut by hand from one 30 kb genome (k = 15, every 2nd genome k-mer an SDK) whose distinct-hit
    counts are 0, 1, 63, 64, 65, 127, 128, 129 and, three times, more than 4096; two reads that share
    exactly one KmerID; and a read that shares with the 64-hit read only the smallest and the largest
    KmerID of that read's list.  Returns (bases, offsets, k, sdk, idx, names): names[i] labels read i."""
    k = 15
    gnm = hga_mod.gen_genome(30_000, 21)
    c, _ = oracle.kmer_windows(gnm, k)
    sdk = np.unique(c)[::2]
    hit = np.isin(c, sdk)   # per window start

    def cut(start, want):   # the shortest read from window `start` with `want` distinct SDK k-mers
        w = start
        seen = set()
        while len(seen) < want:
            if hit[w]:
                seen.add(int(c[w]))
            w += 1
        return gnm[start:w - 1 + k] if want else b"A" * 100

    reads = {"whole": gnm, "front": gnm[:20_000], "back": gnm[5_000:]}
    for j, want in enumerate((0, 1, 63, 64, 65, 127, 128, 129)):
        reads[f"n{want}"] = cut(1000 + 2500 * j, want)
    # two reads whose only common window is one SDK window w1
    w1 = 26_000 + int(np.flatnonzero(hit[26_000:])[0])
    reads["left_of_w1"], reads["right_of_w1"] = gnm[w1 - 400:w1 + k], gnm[w1:w1 + 400]
    # the windows of n64's smallest and largest KmerID (KmerID = rank in the sorted SDK list), joined
    # around a stretch of genome that n64 does not touch
    s64 = 1000 + 2500 * 3
    w64 = slice(s64, s64 + len(reads["n64"]) - k + 1)
    own = np.unique(c[w64][hit[w64]])
    wa, wb = int(np.flatnonzero(c == own[0])[0]), int(np.flatnonzero(c == own[-1])[0])
    reads["ends_of_n64"] = gnm[wa:wa + k] + gnm[20_000:23_000] + gnm[wb:wb + k]
    names = list(reads)
    bases = b"".join(reads[n] for n in names)
    offsets = np.cumsum([0] + [len(reads[n]) for n in names]).astype(np.uint64)
    return bases, offsets, k, sdk, oracle.construct_indices(bases, offsets, k, sdk, 1), names
