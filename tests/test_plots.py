"""The debug plots of `categorization -d` (host/plots.cpp, the engine's plot sink): the wire strings the
reference pipes to scripts/plotting.py (src/clustering/ReadClusteringEngine.cpp:19-124) at its five sites
(:759, :773, :782, :787, :798).  Formatter known answers by hand, plot_spectral's format against the
reference's two recorded dumps, and the engine's (kind, wire) pairs against tests/plots_ref.py run beside
tests/pyref_cluster.py."""
import ast
import os

import numpy as np
import pytest

import oracle
import plots_ref as pr
from test_clustering import CFGS, fasta_haplotype_case

REF_LOG = os.path.join(os.path.dirname(__file__), "golden", "ref_log")


# ---------------------------------------------------------------- formatters, by hand
def test_connection_histogram_known_answers(hga_mod):
    assert hga_mod.plot_connection_histogram([], [], []) == "{}\n{}"
    assert hga_mod.plot_connection_histogram([7], [1], [0]) == "{7: 1}\n{}"          # one good row
    # a score present on one side only is left out of the other; scores ascending; good first (:32)
    assert hga_mod.plot_connection_histogram([2, 5, 2 ** 63], [0, 3, 1], [4, 1, 0]) == \
        f"{{5: 3, {2 ** 63}: 1}}\n{{2: 4, 5: 1}}"
    assert pr.connection_histogram([]) == "{}\n{}"
    assert pr.connection_histogram([(1, 2, 7, True)]) == "{7: 1}\n{}"
    conns = [(1, 2, 2 ** 63, True)] + [(1, 3, 5, True)] * 3 + [(2, 3, 5, False)] + [(4, 5, 2, False)] * 4
    assert pr.connection_histogram(conns) == f"{{5: 3, {2 ** 63}: 1}}\n{{2: 4, 5: 1}}"


def test_per_candidate_histogram_keeps_the_first_row_per_candidate():
    # :102-124: the entry of y is replaced only on a strictly larger score, so in a descending list the
    # first row with that y stays: y = 9 counts under (8, bad), not under the later (8, good) or (3, good)
    conns = [(1, 9, 8, False), (2, 9, 8, True), (3, 4, 8, True), (5, 9, 3, True), (6, 7, 3, False)]
    assert pr.connection_histogram(conns, True) == "{8: 1}\n{3: 1, 8: 1}"
    # a score of 0 never replaces the {0, false} the loop starts from (:105-108)
    assert pr.connection_histogram([(1, 2, 0, True)], True) == "{}\n{0: 1}"


def test_component_coverage_known_answers(hga_mod):
    cases = [
        # a single read at (0, 0): the close sorts first and 0 - (-1) = 1 base lands on coverage 0 (prev_pos
        # starts at -1, the difference is taken in uint32_t)
        ([[(0, 0)]], "[[(0, 1)]]"),
        # two nested reads: 11 bases up to the first start and 50 after the inner read at coverage 1, 10 + 30 at 2
        ([[(10, 100), (20, 50)]], "[[(1, 61), (2, 40)]]"),
        # two reads sharing an endpoint: the close at 10 sorts before the open at 10, coverage never reaches 2
        ([[(0, 10), (10, 20)]], "[[(1, 21)]]"),
        ([], "[]"),
        ([[], [(5, 6)]], "[[], [(1, 7)]]"),
        # prev_pos is an int: a position above 2^31 wraps through it and through the int sum
        ([[(2 ** 31 + 5, 2 ** 31 + 9)]], f"[[(1, {pr._as_int32(2 ** 31 + 6 + 4)})]]"),
    ]
    for comps, want in cases:
        assert hga_mod.plot_component_coverage(comps) == want
        assert pr.component_coverage(comps) == want


# ---------------------------------------------------------------- plot_spectral against the recorded dumps
def parse_spectral_dump(text):
    lines = text.split("\n")
    conns = [tuple(t) for t in ast.literal_eval(lines[0])]
    cats = [tuple(t) for t in ast.literal_eval(lines[1])]
    partition = [list(p) for p in ast.literal_eval(lines[2])]
    return conns, cats, partition, lines[3:]


@pytest.mark.parametrize("name,final_newline", [("ref_spectral.txt", False), ("ref_spectral2.txt", True)])
def test_spectral_graph_reproduces_the_reference_dumps(hga_mod, name, final_newline):
    """src/spectral and src/spectral2, plot_spectral's input as the reference recorded it (:77-98): parsed into
    (connections, categories, partition) and formatted back, the bytes are the file's.  src/spectral was saved
    without the final newline the source appends (:97); it is compared up to that one byte."""
    text = open(os.path.join(REF_LOG, name), newline="").read()
    conns, cats, partition, rest = parse_spectral_dump(text)
    assert rest == ([""] if final_newline else [])
    # line 2 is (id, category) for x then y of every connection, repeats included (:83-84)
    assert [c[0] for c in cats] == [v for c in conns for v in c[:2]]
    first_category = dict(cats)
    assert all(first_category[i] == c for i, c in cats)
    want = text if final_newline else text + "\n"
    assert hga_mod.plot_spectral_graph(conns, first_category, partition) == want
    assert pr.spectral_graph(conns, first_category, partition) == want


# ---------------------------------------------------------------- the engine's five plots
def mosaic_case(hga_mod, tmp_path):
    """test_clustering.py's workload that reaches the tail and spectral stages (haplotype B identical to A
    over 40 kb every 150 kb)."""
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
    offsets = np.asarray(rec["offsets"], np.uint64)
    idx = oracle.construct_indices(rec["bases"], offsets, k, sdk)
    return rec, offsets, idx


CASES = {"haplotypes": (fasta_haplotype_case, CFGS[0]),
         "haplotypes_score": (fasta_haplotype_case, CFGS[2]),
         "mosaic": (mosaic_case, dict(sc_min=30, sc_max=-1, sc_fraction=0.15, sc_score=0, enrich=20, tail=40, dims=16))}


@pytest.fixture(scope="module", params=list(CASES))
def plotted(request, hga_mod, tmp_path_factory):
    """(case name, the run's inputs, the restatement's (kind, wire) pairs), computed once per case."""
    make, c = CASES[request.param]
    rec, offsets, idx = make(hga_mod, tmp_path_factory.mktemp(request.param))
    lengths = np.diff(offsets)
    avg = int(lengths.sum() // len(lengths))
    cats = np.asarray(rec["category"], np.int32)
    eng = pr.PlotEngine(idx, lengths, cats, avg, True, c, start=rec["start"], end=rec["end"])
    want_ids = eng.run()
    return request.param, (rec, offsets, idx, cats, avg, c), want_ids, eng.plots


def run_plots(hga_mod, inputs, debug=True, **kw):
    rec, offsets, idx, cats, avg, c = inputs
    cfg = hga_mod.cluster_config(c["sc_min"], c["sc_max"], c["sc_fraction"], c["sc_score"], c["enrich"], c["tail"], 1,
                                 c["dims"])
    plots, stats = [], {}
    ids, owner, log = hga_mod.cluster_host(rec["bases"], offsets, cats, idx, avg, cfg, debug, start=rec["start"],
                                           end=rec["end"], plots=plots, stats=stats, **kw)
    return ids.tolist(), plots, stats, log


def test_restatement_reaches_every_site(plotted):
    name, _, _, want = plotted
    kinds = [k for k, _ in want]
    if name == "mosaic":   # more than 2 scaffold components and strong tail connections: all five sites
        assert kinds == ["connection_histogram", "spectral_graph", "component_coverage", "connection_histogram",
                         "component_coverage"]
    else:
        assert kinds == ["connection_histogram", "component_coverage", "connection_histogram", "component_coverage"]
    assert want[0][1] != "{}\n{}" and all(w != "[]" for k, w in want if k == "component_coverage")


@pytest.mark.parametrize("hooks", [dict(), dict(device_quality=True), dict(device_forest=True, device_enrich=True),
                                   dict(device_forest=True, device_enrich=True, device_quality=True)],
                         ids=["host", "hook32", "hooks8_16", "hooks8_16_32"])
def test_engine_plots_equal_the_restatement(hga_mod, plotted, hooks):
    """The (kind, wire) pairs of the engine equal plots_ref's, byte for byte, on the host path (the list is
    counted before it is cut to the fraction), through the quality hook (bit 32), and with the two forest
    replays (bits 8 and 16), where the engine never holds the lists.  Ties follow (pivot, candidate) in both."""
    name, inputs, want_ids, want = plotted
    ids, plots, stats, _ = run_plots(hga_mod, inputs, **hooks)
    assert ids == want_ids
    assert [k for k, _ in plots] == [k for k, _ in want]
    for (kind, got), (_, exp) in zip(plots, want):
        assert got == exp, kind
    calls = (stats["quality_calls_device"], stats["quality_calls_host"])
    first_on_fraction_path = inputs[5]["sc_score"] == 0
    if hooks.get("device_quality"):
        assert calls == ((2, 0) if first_on_fraction_path else (1, 1))
    else:
        assert calls == (0, 2)


def test_no_sink_no_quality_calls(hga_mod, plotted, capfd):
    """Without a sink nothing is computed: no quality call (the engine's counters, which HGA_TIMING=1 prints),
    no plot, and the same ids and log lines as the existing entry point."""
    _, inputs, want_ids, _ = plotted
    os.environ["HGA_TIMING"] = "1"
    try:
        capfd.readouterr()
        ids, plots, stats, log = run_plots(hga_mod, inputs, plot_sink=False, device_quality=True)
        err = capfd.readouterr().err
    finally:
        del os.environ["HGA_TIMING"]
    assert ids == want_ids and plots == []
    assert (stats["quality_calls_device"], stats["quality_calls_host"]) == (0, 0)
    timing = dict(ln.split()[1:3] for ln in err.splitlines() if ln.startswith("hga-timing quality."))
    assert timing == {"quality.device_calls": "0", "quality.host_calls": "0"}
    rec, offsets, idx, cats, avg, c = inputs
    cfg = hga_mod.cluster_config(c["sc_min"], c["sc_max"], c["sc_fraction"], c["sc_score"], c["enrich"], c["tail"], 1,
                                 c["dims"])
    ids0, _, log0 = hga_mod.cluster_host(rec["bases"], offsets, cats, idx, avg, cfg, True, start=rec["start"],
                                         end=rec["end"])
    strip = lambda t: [ln for ln in t.splitlines() if " took " not in ln]
    assert ids0.tolist() == ids and strip(log0) == strip(log)


def test_not_debug_emits_nothing(hga_mod, tmp_path):
    rec, offsets, idx = fasta_haplotype_case(hga_mod, tmp_path)
    lengths = np.diff(offsets)
    inputs = (rec, offsets, idx, np.asarray(rec["category"], np.int32), int(lengths.sum() // len(lengths)), CFGS[0])
    _, plots, stats, _ = run_plots(hga_mod, inputs, debug=False)
    assert plots == [] and (stats["quality_calls_device"], stats["quality_calls_host"]) == (0, 0)
