"""hga_spanning_forest_restricted on the CPU: the entry in the header, the binding and the library, the straight
loop with the restricted rule against the contracted Borůvka model on every case the GPU tests use, the replay
argument with a restricted set, and the engine's HGA_DEVICE_ENRICH=1 path through the host hook against the
plain run, on a workload whose enrichment step is shown not to be vacuous."""
import os
import re

import numpy as np
import pytest

import forest_ref as fr
import forest_restricted_ref as rr
import overlap_ref
import pyref_cluster as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_declared_and_bound(hga_mod):
    header = open(os.path.join(ROOT, "include", "hga.h")).read()
    assert re.search(r"hga_status\s+hga_spanning_forest_restricted\s*\(", header)
    for cite in (":456", ":478", ":788-789"):
        assert cite in header
    assert "capped or restricted call" not in header   # only the capped call is not answered
    assert len(hga_mod.HGA_SYMBOLS["hga_spanning_forest_restricted"][1]) == 9
    L = hga_mod.lib()
    assert hasattr(L, "hga_spanning_forest_restricted")
    # a null context is rejected, not dereferenced
    assert L.hga_spanning_forest_restricted(None, None, None, 0, 0, 0, None, 0, None) == 1
    assert "hgc_enrich_forest_calls" in hga_mod.CLUSTER_SYMBOLS


def test_cases_are_not_hollow():
    rr.check_not_hollow()


@pytest.mark.parametrize("name", sorted(rr.cases()))
def test_loop_equals_the_contracted_model_and_replays(name):
    c = rr.cases()[name]
    a, b = rr.window(c)
    want, _ = rr.expected(name)
    assert rr.model(name)[0] == want
    x, y = c.x[a:b], c.y[a:b]
    rel = [p - a for p in want]
    for min_size in (1, 2, 3):
        assert rr.replay(x, y, rel, c.restricted, min_size) == rr.full(x, y, rel, c.restricted, min_size)
    # what min_size 1 loses is exactly the one-member components of the ids with no accepted connection
    whole = pc.union_find(list(zip(x.tolist(), y.tolist(), [0] * len(x))), set(c.restricted.tolist()), 1, -1)
    got = rr.replay(x, y, rel, c.restricted, 1)
    seen = {int(v) for p in rel for v in (x[p], y[p])}
    assert [ct for ct in whole if ct not in got] == [([v], []) for v in sorted((set(x.tolist()) | set(y.tolist())) - seen)]
    assert [ct for ct in whole if ct in got] == got


def test_contraction_on_random_multigraphs():
    rng = np.random.default_rng(23)
    for _ in range(80):
        v, e = int(rng.integers(2, 40)), int(rng.integers(0, 120))
        xy = rng.integers(1, 1 + v, (e, 2))
        xy = np.concatenate([xy, xy[: e // 3, ::-1], xy[: e // 4]])   # both directions, repeats
        xy = xy[rng.permutation(len(xy))]
        x, y = xy[:, 0], xy[:, 1]
        for size in (0, 1, 2, v // 3, v):
            restricted = rng.choice(np.arange(1, 1 + v), size, replace=False)
            want = rr.kruskal_restricted(x, y, restricted)
            assert rr.contracted_model(x, y, restricted)[0] == want
            if size <= 1:
                assert want == fr.kruskal(x, y)
            for min_size in (1, 2, 3):
                assert rr.replay(x, y, want, restricted, min_size) == rr.full(x, y, want, restricted, min_size)


class RecordingEngine(pc.Engine):
    """pyref_cluster.Engine that keeps the arguments and the result of its last get_connections call: in run()
    that is the enrichment list (:788)."""

    def get_connections(self, pivots, min_score):
        out = super().get_connections(pivots, min_score)
        self.last = (list(pivots), min_score, out)
        return out


@pytest.fixture(scope="module")
def tails(hga_mod, tmp_path_factory):
    _, k, sdk, rec, idx, c = overlap_ref.tails_case(hga_mod, tmp_path_factory.mktemp("enrich_case"))
    offsets = np.asarray(rec["offsets"], np.uint64)
    lengths = np.diff(offsets)
    avg = int(lengths.sum() // len(lengths))
    cats = np.asarray(rec["category"], np.int32)

    def run(**kw):
        cfg = hga_mod.cluster_config(c["sc_min"], c["sc_max"], c["sc_fraction"], c["sc_score"], c["enrich"], c["tail"], 1,
                                     c["dims"])
        stats = {}
        return hga_mod.cluster_host(rec["bases"], offsets, cats, idx, avg, cfg, True, start=rec["start"], end=rec["end"],
                                    stats=stats, **kw), stats

    def restatement():
        eng = RecordingEngine(idx, lengths, cats, avg, True, c, start=rec["start"], end=rec["end"])
        return eng, eng.run()

    return run, restatement, c


def hashes(log):
    return [ln for ln in log.splitlines() if ln.startswith("#")]


def test_hooked_engine_equals_the_plain_run(tails):
    run, _, c = tails
    assert c["enrich"] == 20 and c["sc_max"] == -1
    plain, plain_stats = run()
    assert "enrich_forest_calls" not in plain_stats
    took = lambda log: [ln.split(" took ")[0] for ln in log.splitlines() if " took " in ln]
    for kw in (dict(), dict(device_forest=True), dict(device_sets=True, device_tails=True)):
        got, stats = run(device_enrich=True, **kw)
        assert stats["enrich_forest_calls"] == 1
        assert got[0].tolist() == plain[0].tolist() and len(got[0]) > 1
        assert np.array_equal(got[1], plain[1])
        assert hashes(got[2]) == hashes(plain[2]) and len(hashes(plain[2])) > 3
        assert took(got[2]) == took(plain[2])
        at = took(got[2]).index("Calculation of enrichment connections")
        assert took(got[2])[at + 1] == "Merging into core components"


def test_the_enrichment_step_of_the_workload_is_not_hollow(tails):
    """What the engine test above and tests/test_forest_restricted_gpu.py rely on for bin/categorization on this
    workload with default arguments: the enrichment list is longer than its accepted connections, the
    restricted rule itself rejects some (both sides holding a core), and reads are merged into cores."""
    run, restatement, c = tails
    eng, core = restatement()
    pivots, min_score, conns = eng.last
    assert min_score == c["enrich"] and len(pivots) >= 2
    x, y = [t[0] for t in conns], [t[1] for t in conns]
    by_rule = []
    acc = rr.kruskal_restricted(x, y, pivots, by_rule)
    assert len(conns) > len(acc) >= 1
    assert len(by_rule) >= 1
    # at least one read is merged into a core: an accepted connection with a non-core end
    assert any((x[p] in pivots) != (y[p] in pivots) for p in acc)
    assert rr.replay(x, y, acc, pivots, 2) == pc.union_find(conns, set(pivots), 2, -1)
    assert any(len(comp) >= 2 and set(comp) & set(pivots) for comp, _ in rr.replay(x, y, acc, pivots, 2))
    # and the restatement is the run the engine test compares against
    plain, _ = run()
    assert plain[0].tolist() == core
