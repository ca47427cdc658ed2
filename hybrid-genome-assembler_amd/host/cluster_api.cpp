// cluster_api.cpp — C ABI of the host clustering stages (lib/libhga_cluster.so) for the ctypes
// mirror and the tests: the engine on construct_indices outputs, union_find, spectral
// clustering and the eigensolver.  Status 0 = ok, -1 = error (hgc_last_error()).
#include <cstdlib>
#include <cstring>
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
int hgc_cluster_batched(const char* bases, const uint64_t* offsets, const int32_t* category, const uint32_t* start,
                const uint32_t* end, uint64_t n_reads,
                uint64_t avg_read_length, uint32_t first_read_id, const uint64_t* hit_ptr, const uint32_t* sorted_kid,
                const uint64_t* first_ptr, const uint32_t* first_kid, const uint32_t* first_pos, const uint64_t* kci_ptr,
                const uint32_t* kci_read, uint32_t n_sdk, const hgc_config* cfg, int debug, uint32_t** ids_out,
                uint64_t* n_ids, uint32_t** comp_of_read, char** log_out, int batched, uint64_t* ov_edges) {
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
        std::ostringstream log;
        g_forest_calls = g_enrich_calls = 0;
        const auto ids = e.run(log);
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
