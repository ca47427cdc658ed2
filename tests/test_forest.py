"""hga_spanning_forest on the CPU: the entries in the header and the binding, Kruskal's loop against the model
of the device's Borůvka rounds on every shape the GPU tests use, the replay argument (union_find over the
accepted connections alone equals union_find over the whole list), and the engine's HGA_DEVICE_FOREST=1
path through the host hook against the plain run."""
import os
import re

import numpy as np
import pytest

import forest_ref as fr
import oracle
import overlap_ref
import pyref_cluster as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_declared_and_bound(hga_mod):
    header = open(os.path.join(ROOT, "include", "hga.h")).read()
    assert re.search(r"hga_status\s+hga_spanning_forest\s*\(", header)
    assert re.search(r"hga_status\s+hga_spanning_forest_fetch\s*\(", header)
    assert "ReadClusteringEngine.cpp:424-489" in header and ":754-761" in header
    assert len(hga_mod.HGA_SYMBOLS["hga_spanning_forest"][1]) == 7
    assert len(hga_mod.HGA_SYMBOLS["hga_spanning_forest_fetch"][1]) == 4
    L = hga_mod.lib()
    assert hasattr(L, "hga_spanning_forest") and hasattr(L, "hga_spanning_forest_fetch")
    assert callable(getattr(hga_mod.Ctx, "spanning_forest", None))
    # a null context is rejected, not dereferenced
    assert L.hga_spanning_forest(None, None, None, 0, 0, 0, None) == 1
    assert L.hga_spanning_forest_fetch(None, None, None, None) == 1


def test_shapes_are_not_hollow():
    fr.check_not_hollow()


@pytest.mark.parametrize("name", sorted(fr.shapes()))
def test_kruskal_equals_the_round_model_and_replays(name):
    x, y = fr.shapes()[name]
    want = fr.expected(name)
    assert fr.model(name)[0] == want
    for min_size in (1, 3):
        assert fr.replay(x, y, want, min_size) == fr.full(x, y, min_size)


def test_replay_on_random_multigraphs():
    rng = np.random.default_rng(17)
    for _ in range(60):
        v, e = int(rng.integers(2, 40)), int(rng.integers(0, 120))
        xy = rng.integers(1, 1 + v, (e, 2))
        xy = np.concatenate([xy, xy[: e // 3, ::-1], xy[: e // 4]])   # both directions, repeats
        xy = xy[rng.permutation(len(xy))]
        x, y = xy[:, 0], xy[:, 1]
        want = fr.kruskal(x, y)
        assert fr.boruvka_model(x, y)[0] == want
        for min_size in (1, 2, 3):
            assert fr.replay(x, y, want, min_size) == fr.full(x, y, min_size)


@pytest.fixture(scope="module")
def tails(hga_mod, tmp_path_factory):
    _, k, sdk, rec, idx, c = overlap_ref.tails_case(hga_mod, tmp_path_factory.mktemp("forest_case"))
    offsets = np.asarray(rec["offsets"], np.uint64)
    avg = int(np.diff(offsets).sum() // (len(offsets) - 1))
    cats = np.asarray(rec["category"], np.int32)

    def run(sc_max=c["sc_max"], **kw):
        cfg = hga_mod.cluster_config(c["sc_min"], sc_max, c["sc_fraction"], c["sc_score"], c["enrich"], c["tail"], 1,
                                     c["dims"])
        stats = {}
        return hga_mod.cluster_host(rec["bases"], offsets, cats, idx, avg, cfg, True, start=rec["start"], end=rec["end"],
                                    stats=stats, **kw), stats

    return run, idx, c


def hashes(log):
    return [ln for ln in log.splitlines() if ln.startswith("#")]


def test_hooked_engine_equals_the_plain_run(tails):
    run, idx, c = tails
    assert c["sc_max"] == -1 and c["sc_fraction"] == 0.15 and c["sc_score"] == 0
    plain, plain_stats = run()
    assert "forest_calls" not in plain_stats
    for kw in (dict(), dict(device_sets=True, device_tails=True)):
        got, stats = run(device_forest=True, **kw)
        assert stats["forest_calls"] == 1
        assert got[0].tolist() == plain[0].tolist() and len(got[0]) > 1
        assert np.array_equal(got[1], plain[1])
        assert hashes(got[2]) == hashes(plain[2]) and len(hashes(plain[2])) > 3
        took = lambda log: [ln.split(" took ")[0] for ln in log.splitlines() if " took " in ln]
        assert took(got[2]) == took(plain[2])
        assert took(got[2])[:2] == ["Calculation of connections between reads", "Union-find"]


def test_a_size_cap_keeps_the_full_list(tails):
    run, _, _ = tails
    plain, _ = run(sc_max=40)
    got, stats = run(sc_max=40, device_forest=True)
    assert stats["forest_calls"] == 0
    assert got[0].tolist() == plain[0].tolist() and np.array_equal(got[1], plain[1])
    assert hashes(got[2]) == hashes(plain[2])


def test_the_cli_case_is_not_hollow(tails):
    """What tests/test_forest_gpu.py relies on for bin/categorization on this workload with default arguments:
    more than 1000 accepted connections, and a prefix more than twice as long."""
    _, idx, c = tails
    cx, cy, _, _ = oracle.connections(idx, min_score=1)
    prefix = int(len(cx) * c["sc_fraction"])
    edges = fr.kruskal(cx[:prefix], cy[:prefix])
    assert len(edges) > 1000 and prefix > 2 * len(edges)
    # and the replay on the real list, at the run's min size
    full = pc.union_find(list(zip(cx[:prefix].tolist(), cy[:prefix].tolist(), [0] * prefix)), set(), c["sc_min"], -1)
    assert fr.replay(cx[:prefix], cy[:prefix], edges, c["sc_min"]) == full and len(full) > 2
