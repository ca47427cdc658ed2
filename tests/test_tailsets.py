"""The tail stage without host KmerID lists, on the CPU: the two entry points in the header and the
binding, the engine's batching of that mode (every spanning-tree edge in one component-overlap call, one
set-score call over the tail ids still in the index) through the host hooks against the plain host run
and tests/pyref_cluster.py, and the non-vacuity of the cases the GPU tests share (tests/tailsets_ref.py)."""
import os
import re

import numpy as np

import overlap_ref
import pyref_cluster as pc
import tailsets_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_declared_and_bound(hga_mod):
    header = open(os.path.join(ROOT, "include", "hga.h")).read()
    for name in ("hga_components_overlaps", "hga_components_set_scores"):
        assert re.search(r"hga_status\s+%s\s*\(" % name, header), name
        assert name in hga_mod.HGA_SYMBOLS, name
    assert len(hga_mod.HGA_SYMBOLS["hga_components_overlaps"][1]) == 6
    assert len(hga_mod.HGA_SYMBOLS["hga_components_set_scores"][1]) == 9
    for meth in ("components_overlaps", "components_set_scores"):
        assert callable(getattr(hga_mod.Ctx, meth, None)), meth


def test_engine_with_device_sets_hooks_equals_plain_run_and_restatement(hga_mod, tmp_path):
    _, k, sdk, rec, idx, c = overlap_ref.tails_case(hga_mod, tmp_path)
    offsets = np.asarray(rec["offsets"], np.uint64)
    lengths = np.diff(offsets)
    avg = int(lengths.sum() // len(lengths))
    cats = np.asarray(rec["category"], np.int32)
    cfg = hga_mod.cluster_config(c["sc_min"], c["sc_max"], c["sc_fraction"], c["sc_score"], c["enrich"], c["tail"], 1,
                                 c["dims"])

    def run(**kw):
        stats = {}
        return hga_mod.cluster_host(rec["bases"], offsets, cats, idx, avg, cfg, True, start=rec["start"], end=rec["end"],
                                    stats=stats, **kw), stats

    plain, plain_stats = run()
    got, stats = run(device_sets=True)
    both, both_stats = run(device_sets=True, batched_overlaps=True)
    batched, batched_stats = run(batched_overlaps=True)
    assert "Calculation of tail connections took" in got[2] and "Spectral clustering took" in got[2]
    edges = plain_stats["overlap_edges_host"]
    assert plain_stats["overlap_edges_batched"] == 0 and edges > 0
    assert stats == {"overlap_edges_batched": edges, "overlap_edges_host": 0}
    assert both_stats == stats
    # the read-overlap hook alone keeps the edges that touch a merge survivor on the host, as before
    assert batched_stats["overlap_edges_host"] > 0 and batched_stats["overlap_edges_batched"] > 0
    assert batched_stats["overlap_edges_batched"] + batched_stats["overlap_edges_host"] == edges
    hashes = lambda log: [ln for ln in log.splitlines() if ln.startswith("#")]
    for other in (got, both, batched):
        assert other[0].tolist() == plain[0].tolist()
        assert np.array_equal(other[1], plain[1])
        assert hashes(other[2]) == hashes(plain[2])
    eng = pc.Engine(idx, lengths, cats, avg, True, c, start=rec["start"], end=rec["end"])
    assert got[0].tolist() == eng.run()
    assert hashes(got[2]) == eng.printed
    owner = np.zeros(len(lengths), np.uint32)
    for cid in got[0].tolist():
        owner[np.asarray(eng.comps[cid]["reads"]) - 1] = cid
    assert np.array_equal(got[1], owner)


def test_cases_are_not_hollow(hga_mod):
    a, b = tr.case_a(hga_mod), tr.case_b(hga_mod)   # each asserts its own conditions while it is built
    assert len(a.steps) == 4 and len(b.steps) == 3
    assert a.K == 11997 and b.K == 2000
    for case in (a, b):
        for st in case.steps:
            assert len(st.x) == len(st.overlap) == len(st.shared) > 300
            assert len(st.set_pairs) == len(st.score) == len(st.sets) * (len(st.sets) + 1) // 2
            # both orders of a pair are asked for on the device; the reference is symmetric by definition
            assert (st.x == st.y).sum() >= 3
    # case B: every KmerID in one union, and the genome-long read (more entries than KmerIDs) among the pairs
    assert max(st.largest_union for st in b.steps) == b.K
    assert all((st.y == b.c.genome_read).any() for st in b.steps[1:])
