"""Spanning-tree read overlaps (approximate_read_overlap, ReadClusteringEngine.cpp:491-507) in their
batched form: the distinct-list formula hga_read_overlaps computes against the restatement's multiset
formulation, and the engine's batching / eligibility rule through the host hook (no device)."""
import numpy as np

import oracle
import overlap_ref
import pyref_cluster as pc


def test_distinct_list_formula_equals_multiset_formulation(hga_mod):
    """k = 11 on the 60 kb genome: KmerIDs repeat inside reads, so the multiset intersection pairs
    duplicates while the distinct lists do not — the results agree all the same."""
    first_id = 1000
    bases, offsets, k, sdk, idx = overlap_ref.nanosim_case(hga_mod, first_id, k=11)
    n = len(offsets) - 1
    eng = pc.Engine(idx, np.diff(offsets), np.zeros(n, np.int32), 0, False, {}, first_id=first_id)
    rng = np.random.default_rng(7)
    cx, cy, _, _ = oracle.connections(idx, min_score=1, first_read_id=first_id)
    pick = rng.choice(len(cx), 150, replace=False)
    with_hits = np.array(sorted(eng.comps), np.uint32)
    x = np.concatenate([cx[pick], rng.choice(with_hits, 150)]).astype(np.uint32)
    y = np.concatenate([cy[pick], rng.choice(with_hits, 150)]).astype(np.uint32)
    repeated = np.diff(idx["hit_ptr"]) != np.diff(idx["first_ptr"])   # reads with a KmerID twice in sorted_kid
    assert repeated[np.concatenate([x, y]) - first_id].any()
    ov, sh = overlap_ref.read_overlaps(idx, x, y, first_id)
    assert (sh[:150] > 0).all() and (sh[150:] == 0).any()
    assert ov.tolist() == [eng.overlap(int(a), int(b)) for a, b in zip(x, y)]


def test_engine_with_batched_overlaps_equals_restatement(hga_mod, tmp_path):
    """The tail stage with its edge overlaps taken through the batched hook (edges between never-merged
    components from the distinct-list formula, edges touching a merge survivor from the host's
    approximate_read_overlap) returns what the plain host run and the restatement return."""
    _, k, sdk, rec, idx, c = overlap_ref.tails_case(hga_mod, tmp_path)
    offsets = np.asarray(rec["offsets"], np.uint64)
    lengths = np.diff(offsets)
    avg = int(lengths.sum() // len(lengths))
    cats = np.asarray(rec["category"], np.int32)
    cfg = hga_mod.cluster_config(c["sc_min"], c["sc_max"], c["sc_fraction"], c["sc_score"], c["enrich"], c["tail"], 1,
                                 c["dims"])
    plain_stats, stats = {}, {}
    plain = hga_mod.cluster_host(rec["bases"], offsets, cats, idx, avg, cfg, True, start=rec["start"], end=rec["end"],
                                 stats=plain_stats)
    got = hga_mod.cluster_host(rec["bases"], offsets, cats, idx, avg, cfg, True, start=rec["start"], end=rec["end"],
                               batched_overlaps=True, stats=stats)
    assert "Calculation of tail connections took" in got[2]
    assert plain_stats["overlap_edges_batched"] == 0 and plain_stats["overlap_edges_host"] > 0
    assert stats["overlap_edges_batched"] > 0 and stats["overlap_edges_host"] > 0
    assert stats["overlap_edges_batched"] + stats["overlap_edges_host"] == plain_stats["overlap_edges_host"]
    hashes = lambda log: [ln for ln in log.splitlines() if ln.startswith("#")]
    assert got[0].tolist() == plain[0].tolist()
    assert np.array_equal(got[1], plain[1])
    assert hashes(got[2]) == hashes(plain[2])
    eng = pc.Engine(idx, lengths, cats, avg, True, c, start=rec["start"], end=rec["end"])
    assert got[0].tolist() == eng.run()
    assert hashes(got[2]) == eng.printed
    owner = np.zeros(len(lengths), np.uint32)
    for cid in got[0].tolist():
        owner[np.asarray(eng.comps[cid]["reads"]) - 1] = cid
    assert np.array_equal(got[1], owner)
