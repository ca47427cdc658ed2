// cluster_api.cpp — C ABI of the host clustering stages (lib/libhga_cluster.so) for the ctypes
// mirror and the tests: the engine on construct_indices outputs, union_find, spectral
// clustering and the eigensolver.  Status 0 = ok, -1 = error (hgc_last_error()).
#include <cstdlib>
#include <cstring>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "clustering.h"

namespace {
thread_local std::string g_err;
thread_local uint64_t g_forest_calls = 0;   // of this thread's last hgc_cluster* call (hgc_forest_calls)
thread_local uint64_t g_enrich_calls = 0;   // likewise (hgc_enrich_forest_calls)

template <class F>
int guard(F&& f) {
    try {
        g_err.clear();
        f();
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}

template <class T>
T* dup(const T* p, size_t n) {
    T* q = static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1));
    if (!q) throw std::bad_alloc();
    if (n) std::memcpy(q, p, n * sizeof(T));
    return q;
}

std::vector<hgah::Connection> conns_of(const uint32_t* x, const uint32_t* y, const uint64_t* s, uint64_t n) {
    std::vector<hgah::Connection> c(n);
    for (uint64_t i = 0; i < n; ++i) c[i] = {x[i], y[i], s[i], false};
    return c;
}

// Components as a flat list: ids[] with ptr[] (CSR), caller frees both.
void put_components(const std::vector<hgah::ComponentList>& comps, uint64_t** ptr, uint32_t** ids, uint64_t* n) {
    std::vector<uint64_t> p{0};
    std::vector<uint32_t> v;
    for (auto& c : comps) {
        v.insert(v.end(), c.begin(), c.end());
        p.push_back(v.size());
    }
    *ptr = dup(p.data(), p.size());
    *ids = dup(v.data(), v.size());
    *n = comps.size();
}
}  // namespace

extern "C" {

struct hgc_config {   // ReadClusteringConfig (ReadClusteringEngine.h:138-148)
    int sc_min_size, sc_max_size;
    double sc_fraction;
    uint64_t sc_score, core_enrichment, tail_amplification;
    int threads, spectral_dims, force_spectral;
};

const char* hgc_last_error(void) { return g_err.c_str(); }
void hgc_free(void* p) { std::free(p); }

// run_clustering after construct_indices (host-only: no device state) on the lookup's CSR
// outputs; reads in reader order with ReadID = first_read_id + i.  Outputs: the returned
// component ids (ascending; under debug in print_components' order), per read the id of the returned
// component containing it (0 = none), the timing/log text (with print_components' blocks under debug).
// start / end: the reads' simulator-header coordinates (GenomeReadData start / end), null = 0.
// hgc_cluster_batched: the same with the tail stage's batched overlap hook (set_device_overlaps) set
// to the engine's host implementation of hga_read_overlaps when batched != 0 — the device path's
// batching and eligibility rule without a device; ov_edges[2] (may be null) receives the tail stage's
// edge counts {from the batch, from the host's approximate_read_overlap}.  batched is a set of bit flags:
// 1 is the hook above; 2 sets the component-overlap and set-score hooks (set_device_component_overlaps,
// set_device_set_scores) to the engine's host implementations, so that the tail stage runs the batching
// of HGA_DEVICE_SETS=1 (every edge in one call, one set-score call over ids filtered through the index);
// 4 sets the tree-tails hook (set_device_tree_tails) to host_tree_tails, so that the tail stage takes the
// tails of all trees from one call, as under HGA_DEVICE_TAILS=1;
// 8 sets the spanning-forest hook (set_device_forest) to host_forest, so that the first union_find replays
// only the connections it would accept, as under HGA_DEVICE_FOREST=1; hgc_forest_calls() then tells how
// many times this thread's last hgc_cluster* call took that path;
// 16 sets the enrichment-forest hook (set_device_enrich_forest) to host_enrich_forest, so that the
// enrichment union_find replays only the connections it would accept, as under HGA_DEVICE_ENRICH=1;
// hgc_enrich_forest_calls() then tells how many times this thread's last hgc_cluster* call took that path.
// 32 sets the quality hook (set_device_quality) to host_quality, so that the two connection histograms of
// the debug plots come through the hook, as where the list stays on the device; it is only ever called by
// an engine with a plot sink (hgc_cluster_plots).
// hgc_cluster_plots: the same run with a plot sink when with_sink != 0.  plots_out receives the plots in
// emission order as one buffer of plots_bytes bytes, "kind\0wire\0" per plot, n_plots their number;
// quality_calls[2] (may be null) the engine's {quality_calls_device, quality_calls_host}.
static int cluster_run(const char* bases, const uint64_t* offsets, const int32_t* category, const uint32_t* start,
                const uint32_t* end, uint64_t n_reads,
                uint64_t avg_read_length, uint32_t first_read_id, const uint64_t* hit_ptr, const uint32_t* sorted_kid,
                const uint64_t* first_ptr, const uint32_t* first_kid, const uint32_t* first_pos, const uint64_t* kci_ptr,
                const uint32_t* kci_read, uint32_t n_sdk, const hgc_config* cfg, int debug, uint32_t** ids_out,
                uint64_t* n_ids, uint32_t** comp_of_read, char** log_out, int batched, uint64_t* ov_edges,
                std::string* plots, uint64_t* n_plots, uint64_t* quality_calls) {
    return guard([&] {
        hgah::RecordSet rs;
        rs.bases.append(bases, n_reads ? offsets[n_reads] : 0);
        rs.offsets.assign(offsets, offsets + n_reads + 1);
        rs.category.assign(category, category + n_reads);
        if (start && end) {
            rs.start.assign(start, start + n_reads);
            rs.end.assign(end, end + n_reads);
        }
        rs.meta.avg_read_length = avg_read_length;
        hgah::ClusteringConfig c;
        c.scaffold_component_min_size = cfg->sc_min_size;
        c.scaffold_component_max_size = cfg->sc_max_size;
        c.scaffold_forming_fraction = cfg->sc_fraction;
        c.scaffold_forming_score = cfg->sc_score;
        c.enrichment_connections_min_score = cfg->core_enrichment;
        c.tail_amplification_min_score = cfg->tail_amplification;
        c.threads = cfg->threads;
        c.spectral_dims = cfg->spectral_dims;
        c.force_spectral = cfg->force_spectral != 0;
        const uint64_t H = hit_ptr[n_reads], U = first_ptr[n_reads], HK = kci_ptr[n_sdk];
        hgah::ClusteringEngine e(c, debug != 0, rs, first_read_id, std::vector<uint64_t>(hit_ptr, hit_ptr + n_reads + 1),
                                 std::vector<uint32_t>(sorted_kid, sorted_kid + H),
                                 std::vector<uint64_t>(first_ptr, first_ptr + n_reads + 1),
                                 std::vector<uint32_t>(first_kid, first_kid + U),
                                 std::vector<uint32_t>(first_pos, first_pos + U),
                                 std::vector<uint64_t>(kci_ptr, kci_ptr + n_sdk + 1),
                                 std::vector<uint32_t>(kci_read, kci_read + HK), nullptr);
        if (batched & 1)
            e.set_device_overlaps([&e](const std::vector<hgah::ComponentID>& x, const std::vector<hgah::ComponentID>& y) {
                return e.host_read_overlaps(x, y);
            });
        if (batched & 2) {
            e.set_device_component_overlaps([&e](const std::vector<hgah::ComponentID>& x, const std::vector<hgah::ComponentID>& y) {
                return e.host_component_overlaps(x, y);
            });
            e.set_device_set_scores([&e](const std::vector<hgah::ComponentList>& sets, const hgah::ClusteringEngine::SetPairs& pairs) {
                return e.host_set_scores(sets, pairs);
            });
        }
        if (batched & 4)
            e.set_device_tree_tails([&e](const hgah::ClusteringEngine::TreeList& cts) { return e.host_tree_tails(cts); });
        if (batched & 8)
            e.set_device_forest([&e](hgah::Score min_score, uint32_t min_kmers, double keep_fraction) {
                return e.host_forest(min_score, min_kmers, keep_fraction);
            });
        if (batched & 16)
            e.set_device_enrich_forest([&e](const std::vector<hgah::ComponentID>& pivots, hgah::Score min_score) {
                return e.host_enrich_forest(pivots, min_score);
            });
        if (batched & 32)
            e.set_device_quality([&e](const std::vector<hgah::ComponentID>& pivots, hgah::Score min_score, bool per_candidate) {
                return e.host_quality(pivots, min_score, per_candidate);
            });
        if (plots)
            e.set_plot_sink([&](const char* kind, const std::string& wire) {
                plots->append(kind);
                plots->push_back('\0');
                plots->append(wire);
                plots->push_back('\0');
                ++*n_plots;
            });
        std::ostringstream log;
        g_forest_calls = g_enrich_calls = 0;
        const auto ids = e.run(log);
        if (quality_calls) {
            quality_calls[0] = e.quality_calls_device();
            quality_calls[1] = e.quality_calls_host();
        }
        g_forest_calls = e.forest_calls();
        g_enrich_calls = e.enrich_forest_calls();
        if (ov_edges) {
            ov_edges[0] = e.overlap_edges_device();
            ov_edges[1] = e.overlap_edges_host();
        }
        std::vector<uint32_t> owner(n_reads, 0);
        for (auto id : ids)
            for (uint32_t r : e.components().at(id).reads) owner[r - first_read_id] = id;
        *ids_out = dup(ids.data(), ids.size());
        *n_ids = ids.size();
        *comp_of_read = dup(owner.data(), owner.size());
        const std::string s = log.str();
        *log_out = dup(s.c_str(), s.size() + 1);
    });
}

int hgc_cluster_batched(const char* bases, const uint64_t* offsets, const int32_t* category, const uint32_t* start,
                const uint32_t* end, uint64_t n_reads,
                uint64_t avg_read_length, uint32_t first_read_id, const uint64_t* hit_ptr, const uint32_t* sorted_kid,
                const uint64_t* first_ptr, const uint32_t* first_kid, const uint32_t* first_pos, const uint64_t* kci_ptr,
                const uint32_t* kci_read, uint32_t n_sdk, const hgc_config* cfg, int debug, uint32_t** ids_out,
                uint64_t* n_ids, uint32_t** comp_of_read, char** log_out, int batched, uint64_t* ov_edges) {
    return cluster_run(bases, offsets, category, start, end, n_reads, avg_read_length, first_read_id, hit_ptr, sorted_kid,
                       first_ptr, first_kid, first_pos, kci_ptr, kci_read, n_sdk, cfg, debug, ids_out, n_ids, comp_of_read,
                       log_out, batched, ov_edges, nullptr, nullptr, nullptr);
}

int hgc_cluster_plots(const char* bases, const uint64_t* offsets, const int32_t* category, const uint32_t* start,
                const uint32_t* end, uint64_t n_reads,
                uint64_t avg_read_length, uint32_t first_read_id, const uint64_t* hit_ptr, const uint32_t* sorted_kid,
                const uint64_t* first_ptr, const uint32_t* first_kid, const uint32_t* first_pos, const uint64_t* kci_ptr,
                const uint32_t* kci_read, uint32_t n_sdk, const hgc_config* cfg, int debug, uint32_t** ids_out,
                uint64_t* n_ids, uint32_t** comp_of_read, char** log_out, int batched, uint64_t* ov_edges, int with_sink,
                char** plots_out, uint64_t* plots_bytes, uint64_t* n_plots, uint64_t* quality_calls) {
    std::string plots;
    uint64_t n = 0;
    const int st = cluster_run(bases, offsets, category, start, end, n_reads, avg_read_length, first_read_id, hit_ptr,
                               sorted_kid, first_ptr, first_kid, first_pos, kci_ptr, kci_read, n_sdk, cfg, debug, ids_out, n_ids,
                               comp_of_read, log_out, batched, ov_edges, with_sink ? &plots : nullptr, &n, quality_calls);
    if (st != 0) return st;
    return guard([&] {
        *plots_out = dup(plots.data(), plots.size());
        *plots_bytes = plots.size();
        *n_plots = n;
    });
}

// The wire-string formatters of the debug plots (host/plots.h), for the tests.  Each returns a malloc'ed
// NUL-terminated string in *out (hgc_free).
int hgc_plot_connection_histogram(const uint64_t* score, const uint64_t* good, const uint64_t* bad, uint64_t n, char** out) {
    return guard([&] {
        hgah::QualityHist h;
        h.score.assign(score, score + n);
        h.good.assign(good, good + n);
        h.bad.assign(bad, bad + n);
        const std::string s = hgah::connection_histogram(h);
        *out = dup(s.c_str(), s.size() + 1);
    });
}

// components: CSR over reads (comp_ptr[n_comp + 1]), start / end per listed read
int hgc_plot_component_coverage(const uint64_t* comp_ptr, const uint32_t* start, const uint32_t* end, uint64_t n_comp,
                                char** out) {
    return guard([&] {
        std::vector<hgah::ReadSpans> comps(n_comp);
        for (uint64_t c = 0; c < n_comp; ++c)
            for (uint64_t i = comp_ptr[c]; i < comp_ptr[c + 1]; ++i) comps[c].emplace_back(start[i], end[i]);
        const std::string s = hgah::component_coverage(comps);
        *out = dup(s.c_str(), s.size() + 1);
    });
}

// cat_x / cat_y: *categories.begin() of each connection's two components; part_ptr / part_ids: the partition (CSR)
int hgc_plot_spectral_graph(const uint32_t* x, const uint32_t* y, const uint64_t* s, const int32_t* cat_x,
                            const int32_t* cat_y, uint64_t n, const uint64_t* part_ptr, const uint32_t* part_ids,
                            uint64_t n_parts, char** out) {
    return guard([&] {
        std::vector<hgah::SpectralEdge> edges(n);
        std::map<uint32_t, int32_t> cat;
        for (uint64_t i = 0; i < n; ++i) {
            edges[i] = {x[i], y[i], s[i]};
            cat[x[i]] = cat_x[i];
            cat[y[i]] = cat_y[i];
        }
        std::vector<std::vector<uint32_t>> parts(n_parts);
        for (uint64_t p = 0; p < n_parts; ++p) parts[p].assign(part_ids + part_ptr[p], part_ids + part_ptr[p + 1]);
        const std::string w = hgah::spectral_graph(edges, [&](uint32_t id) { return cat.at(id); }, parts);
        *out = dup(w.c_str(), w.size() + 1);
    });
}

int hgc_cluster(const char* bases, const uint64_t* offsets, const int32_t* category, const uint32_t* start,
                const uint32_t* end, uint64_t n_reads,
                uint64_t avg_read_length, uint32_t first_read_id, const uint64_t* hit_ptr, const uint32_t* sorted_kid,
                const uint64_t* first_ptr, const uint32_t* first_kid, const uint32_t* first_pos, const uint64_t* kci_ptr,
                const uint32_t* kci_read, uint32_t n_sdk, const hgc_config* cfg, int debug, uint32_t** ids_out,
                uint64_t* n_ids, uint32_t** comp_of_read, char** log_out) {
    return hgc_cluster_batched(bases, offsets, category, start, end, n_reads, avg_read_length, first_read_id, hit_ptr,
                               sorted_kid, first_ptr, first_kid, first_pos, kci_ptr, kci_read, n_sdk, cfg, debug, ids_out,
                               n_ids, comp_of_read, log_out, 0, nullptr);
}

uint64_t hgc_forest_calls(void) { return g_forest_calls; }
uint64_t hgc_enrich_forest_calls(void) { return g_enrich_calls; }

// union_find (ReadClusteringEngine.cpp:424-489) of an ordered connection list.
int hgc_union_find(const uint32_t* x, const uint32_t* y, const uint64_t* s, uint64_t n, const uint32_t* restricted,
                   uint64_t n_restricted, int min_size, int max_size, uint64_t** comp_ptr, uint32_t** comp_ids,
                   uint64_t* n_comp, uint64_t** tree_ptr, uint32_t** tree_xy) {
    return guard([&] {
        const std::set<hgah::ComponentID> r(restricted, restricted + n_restricted);
        const auto res = hgah::union_find(conns_of(x, y, s, n), r, min_size, max_size);
        std::vector<hgah::ComponentList> comps;
        std::vector<uint64_t> tp{0};
        std::vector<uint32_t> txy;
        for (auto& ct : res) {
            comps.push_back(ct.first);
            for (auto& e : ct.second) {
                txy.push_back(e.first);
                txy.push_back(e.second);
            }
            tp.push_back(txy.size() / 2);
        }
        put_components(comps, comp_ptr, comp_ids, n_comp);
        *tree_ptr = dup(tp.data(), tp.size());
        *tree_xy = dup(txy.data(), txy.size());
    });
}

// spectral_clustering (ReadClusteringEngine.cpp:653-697).
int hgc_spectral(const uint32_t* x, const uint32_t* y, const uint64_t* s, uint64_t n, int dims, uint64_t** comp_ptr,
                 uint32_t** comp_ids, uint64_t* n_comp) {
    return guard([&] { put_components(hgah::spectral_clustering(conns_of(x, y, s, n), dims), comp_ptr, comp_ids, n_comp); });
}

// Symmetric eigen-decomposition used by spectral_clustering (values ascending, vectors as
// columns of a row-major n x n matrix); caller-allocated outputs.
int hgc_sym_eigen(const double* a, int n, double* values, double* vectors) {
    return guard([&] {
        std::vector<double> v, w;
        hgah::sym_eigen(std::vector<double>(a, a + (size_t)n * n), n, v, w);
        std::memcpy(values, v.data(), (size_t)n * sizeof(double));
        std::memcpy(vectors, w.data(), (size_t)n * n * sizeof(double));
    });
}

}  // extern "C"
