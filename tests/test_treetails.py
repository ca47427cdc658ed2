"""hga_tree_tails on the CPU: the entry in the header and the binding, the stand-alone restatement
(tests/treetails_ref.py) against tests/pyref_cluster.py's Engine.tails, the engine's one-call batching of
HGA_DEVICE_TAILS=1 through the host hook against the plain run, and the non-vacuity of the forests the
GPU tests share."""
import os
import re

import numpy as np

import overlap_ref
import pyref_cluster as pc
import treetails_ref as tt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_declared_and_bound(hga_mod):
    header = open(os.path.join(ROOT, "include", "hga.h")).read()
    assert re.search(r"hga_status\s+hga_tree_tails\s*\(", header)
    assert re.search(r"}\s*hga_tree_ends\s*;", header)
    assert "hga_tree_tails" in hga_mod.HGA_SYMBOLS
    assert len(hga_mod.HGA_SYMBOLS["hga_tree_tails"][1]) == 13
    assert hasattr(hga_mod.lib(), "hga_tree_tails")
    assert callable(getattr(hga_mod.Ctx, "tree_tails", None))
    ends = hga_mod.TreeEnds
    assert [f[0] for f in ends._fields_] == ["right_id", "right_dist", "left_id", "left_dist"]
    assert ends.right_dist.offset == 8 and ends.left_id.offset == 16 and ends.left_dist.offset == 24
    # a null context is rejected, not dereferenced
    assert hga_mod.lib().hga_tree_tails(None, None, None, None, 0, None, None, 0, None, None, None, None, None) == 1


def test_restatement_and_hooked_engine_on_the_tails_case(hga_mod, tmp_path):
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
    sets, sets_stats = run(device_sets=True)
    got, stats = run(device_sets=True, device_tails=True)
    alone, alone_stats = run(device_tails=True)   # the hook without the sets mode: the default overlaps, one call
    assert "Calculation of tail connections took" in got[2] and "Spectral clustering took" in got[2]
    assert stats == sets_stats and stats["overlap_edges_host"] == 0 and stats["overlap_edges_batched"] > 0
    assert alone_stats == plain_stats
    hashes = lambda log: [ln for ln in log.splitlines() if ln.startswith("#")]
    for other in (got, sets, alone):
        assert other[0].tolist() == plain[0].tolist()
        assert np.array_equal(other[1], plain[1])
        assert hashes(other[2]) == hashes(plain[2])

    # the restatement against Engine.tails, on the trees and the merged state the run meets
    eng = pc.Engine(idx, lengths, cats, avg, True, c, start=rec["start"], end=rec["end"])
    seen, engine_tails = [], eng.tails

    def spy(tree):
        out = engine_tails(tree)
        ov = [eng.overlap(a, b) for a, b in tree]
        ref = tt.TreeRef(tree, ov, eng.lengths, eng.avg_len * 2)
        seen.append((tree, out, ref, ov))
        return out

    eng.tails = spy
    assert got[0].tolist() == eng.run()
    assert hashes(got[2]) == eng.printed
    assert len(seen) > 2 and sum(len(tree) for tree, *_ in seen) == stats["overlap_edges_batched"]
    for tree, (left, right), ref, _ in seen:
        assert ref.left == left and ref.right == right
        assert ref.ends[0] in right and ref.ends[2] in left and len(tree) >= 29
    # whole trees at once give the same
    many = tt.tree_tails([tree for tree, *_ in seen], [d for *_, ov in seen for d in ov], eng.lengths, eng.avg_len * 2)
    assert [(r.left, r.right) for r in many] == [(ref.left, ref.right) for _, _, ref, _ in seen]


def test_cases_are_not_hollow():
    tt.check_not_hollow()   # a tie decided by id, a wrapped distance, three passes from three vertices, ...
    shapes, forest = tt.shapes_forest(), tt.random_forest()
    sizes = [len(t) for t in shapes.trees]
    for n in (0, 1, 31, 32, 33, 64, 1023, 1024, 1025, 3000, 4999):
        assert n in sizes, n
    assert len(forest.trees) == 300 and 1 <= min(map(len, forest.trees)) and max(map(len, forest.trees)) <= 200
    for f in (shapes, forest):   # no id in two trees
        ids = [sorted({v for e in t for v in e}) for t in f.trees]
        assert sum(map(len, ids)) == len({v for t in ids for v in t}) == f.n_edges + sum(1 for t in f.trees if t)
