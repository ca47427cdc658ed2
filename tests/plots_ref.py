"""Independent Python restatement of the debug plots of run_clustering
(src/clustering/ReadClusteringEngine.cpp): plot_connection_quality over every connection (:19-34) and
over the best connection per candidate (:102-124), plot_read_coverage (:37-73), plot_spectral (:77-98),
and their five call sites (:759, :773, :782, :787, :798), run beside tests/pyref_cluster.py's Engine.
Written from the reference text; connections are (x, y, score, is_good) tuples in the project's order
(score descending, then x, then y), which decides the ties the reference leaves unspecified."""
import pyref_cluster as pc

M32 = 2 ** 32


def _hist_wire(good, bad):
    side = lambda d: ", ".join(f"{s}: {d[s]}" for s in sorted(d))
    return "{" + side(good) + "}\n{" + side(bad) + "}"


def quality_all(conns):   # :19-31
    m = {True: {}, False: {}}
    for _, _, s, g in conns:
        m[bool(g)][s] = m[bool(g)].get(s, 0) + 1
    return m[True], m[False]


def quality_per_candidate(conns):   # :102-114
    best = {}
    for _, y, s, g in conns:
        cur = best.setdefault(y, (0, False))
        if s > cur[0]:
            best[y] = (s, bool(g))
    m = {True: {}, False: {}}
    for s, g in best.values():
        m[g][s] = m[g].get(s, 0) + 1
    return m[True], m[False]


def connection_histogram(conns, per_candidate=False):
    return _hist_wire(*(quality_per_candidate(conns) if per_candidate else quality_all(conns)))


def _as_int32(v):
    v %= M32
    return v - M32 if v >= 2 ** 31 else v


def coverage_runs(spans):   # get_coverage_runs, :38-61
    ends = []
    for a, b in spans:
        ends += [(int(a), True), (int(b), False)]
    ends.sort()   # std::pair<uint32_t, bool>: (p, False) before (p, True)
    result, cov, prev = {}, 0, -1
    for pos, is_start in ends:
        d = (pos - prev) % M32   # uint32_t - int, in uint32_t
        if is_start:
            cov += 1
            result[cov] = _as_int32(result.get(cov, 0) + d)
        else:
            result[cov] = _as_int32(result.get(cov, 0) + d)
            cov -= 1
        prev = _as_int32(pos)
    return result


def component_coverage(components):   # :63-72
    out = []
    for spans in components:
        runs = coverage_runs(spans)
        out.append("[" + ", ".join(f"({c}, {runs[c]})" for c in sorted(runs)) + "]")
    return "[" + ", ".join(out) + "]"


def spectral_graph(conns, first_category, partition):   # :77-97
    l1 = ", ".join(f"({c[0]}, {c[1]}, {c[2]})" for c in conns)
    l2 = ", ".join(f"({v}, {first_category[v]})" for c in conns for v in (c[0], c[1]))
    l3 = ", ".join("[" + ", ".join(str(i) for i in comp) + "]" for comp in partition)
    return f"[{l1}]\n[{l2}]\n[{l3}]\n"


class PlotEngine(pc.Engine):
    """pyref_cluster.Engine.run (:737-801) with the debug plots at the reference's sites; self.plots
    receives the (kind, wire) pairs."""

    def coverage(self, ids):
        return component_coverage([[(self.start[r], self.end[r]) for r in self.comps[i]["reads"]] for i in ids])

    def run(self):
        c = self.cfg
        self.plots = []
        all_ids = sorted(self.comps)
        if c["sc_score"] > 0:
            ids = [i for i in all_ids if len(self.comps[i]["kmers"]) >= c["sc_score"]]
            conns = self.get_connections(ids, c["sc_score"])
            scaffold = [x for x in conns if x[2] > c["sc_score"]]
        else:
            conns = self.get_connections(all_ids, 1)
            scaffold = conns[:int(len(conns) * c["sc_fraction"])]
        if self.debug:
            self.plots.append(("connection_histogram", connection_histogram(conns)))   # :759
        cts = pc.union_find(scaffold, set(), c["sc_min"], c["sc_max"])
        sids = self.merge([x[0] for x in cts])
        self.print_components(sids)
        if len(sids) > 2:
            strong = [x for x in self.core_connections(cts) if x[2] > 5]
            if strong:
                spectral = pc.spectral_clustering(strong, c["dims"])
                if self.debug:   # :773
                    cat = {v: min(self.comps[v]["cats"]) for x in strong for v in x[:2]}
                    self.plots.append(("spectral_graph", spectral_graph(strong, cat, spectral)))
                self.merge(spectral)
            self.remove_merged()
        core = self.ids(c["sc_min"])
        self.print_components(core)
        if self.debug:
            self.plots.append(("component_coverage", self.coverage(core)))   # :782
        conns = self.get_connections(core, c["enrich"])
        if self.debug:
            self.plots.append(("connection_histogram", connection_histogram(conns, True)))   # :787
        cts = pc.union_find(conns, set(core), 2, -1)
        self.merge([x[0] for x in cts])
        self.remove_merged()
        core = self.ids(c["sc_min"])
        self.print_components(core)
        if self.debug:
            self.plots.append(("component_coverage", self.coverage(core)))   # :798
        return core
