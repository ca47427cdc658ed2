// clustering.h — the stages of `categorization` after index construction
// (ReadClusteringEngine::run_clustering / export_components,
// src/clustering/ReadClusteringEngine.cpp:301-826).
//
// The engine starts from the state construct_indices leaves (one component per read with >= 1
// SDK hit; kmer_component_index; read metadata), which the GPU lookup produced.  The all-reads
// connection pass (get_all_connections / the filtered get_connections call at :750-755) runs on
// the GPU (hga_connections_run) on the device-resident indices.  With a device ctx the later
// get_connections calls, on merged components and the edited kmer_component_index, run there too:
// merge_components keeps the members, KmerID unions and categories of the components on the host
// (the tail stage needs them) and hands the call's groups to hga_components_merge, which edits the
// device's copy of kmer_component_index; get_connections then calls hga_components_connections.  The
// engine builds no host kmer_component_index in that mode (kmer_component_index() fetches it on
// demand).  HGA_HOST_CONNECTIONS=1 in the environment, or an engine without a ctx, keeps the host
// index and runs those calls on the host.
// The spanning-tree edge overlaps of the tail stage (approximate_read_overlap, :491-513) run on the
// GPU too (hga_read_overlaps), in one batch over all trees, for the edges whose two endpoints were
// never merged into: those components' KmerID lists are still the reads' own, which is what the
// device's first-occurrence lists describe.  Edges touching a merge survivor stay on the host.
// HGA_DEVICE_SETS=1 (opt-in, with the component state on the device) moves the remaining readers of the
// components' KmerID lists there as well — every tree edge through hga_components_overlaps, the tail
// sets' unions and intersections through hga_components_set_scores — and the engine then keeps no
// KmerID list per component at all (see set_device_component_overlaps below).  In that mode the three
// distance passes over every scaffold tree run there as well (hga_tree_tails, one call; HGA_DEVICE_TAILS=0
// keeps them on the host), so the stage is three device calls that exchange small id lists.
//
// Determinism: the reference iterates tsl::robin_map / std::unordered_map containers and sorts
// connections with an unstable std::sort on the score only, so ties and container orders are
// unspecified there.  Here components are visited in ascending ComponentID order, connections
// are ordered by (score descending, x ascending, y ascending) — the GPU's order — and ties of
// max_element take the smallest id.  With those orders fixed, every rule below follows the
// reference statement by statement, including its edge behaviour (kmer_component_index
// removal drops the tail of a list once the removal list is exhausted, :405-416; unsigned BFS
// distances, :529; merged components carry de-duplicated KmerIDs, Utils.h merge_n_vectors).
// Spectral clustering uses a Jacobi eigensolver (Eigen2's SelfAdjointEigenSolver in the
// reference) and the Evrot rotation (src/lib/clustering/Evrot.cpp, method 1: true gradient):
// floating-point results can differ in degenerate eigenspaces, so the final read->component
// assignment is "parity unpinned" (SURVEY.md §8(c)).
#pragma once

#include <cstdint>
#include <map>
#include <ostream>
#include <set>
#include <string>
#include <utility>
#include <functional>
#include <vector>

#include "hga.h"
#include "plots.h"
#include "seqio.h"

namespace hgah {

using ComponentID = uint32_t;
using KmerID = uint32_t;
using Score = uint64_t;

struct Connection {   // ComponentConnection, ReadClusteringEngine.h:127-136
    ComponentID x, y;
    Score score;
    bool is_good;
};
using SpanningTree = std::vector<std::pair<ComponentID, ComponentID>>;
using ComponentList = std::vector<ComponentID>;

struct ClusteringConfig {   // ReadClusteringConfig, ReadClusteringEngine.h:138-148
    int scaffold_component_min_size = 30;
    int scaffold_component_max_size = -1;
    double scaffold_forming_fraction = 0.15;
    Score scaffold_forming_score = 0;
    Score enrichment_connections_min_score = 20;
    Score tail_amplification_min_score = 40;
    int threads = 1;
    int spectral_dims = 16;
    bool force_spectral = false;
};

// (score desc, x asc, y asc) — the order of hga_connections_fetch.
void sort_connections(std::vector<Connection>& c);

// union_find (:424-489).  Components in ascending order of their root id.
std::vector<std::pair<ComponentList, SpanningTree>> union_find(const std::vector<Connection>& connections,
                                                               const std::set<ComponentID>& restricted,
                                                               int min_component_size, int max_component_size);

// spectral_clustering (:653-697) with SpectralClustering + ClusterRotate + Evrot.
std::vector<ComponentList> spectral_clustering(const std::vector<Connection>& connections, int dims);

// Symmetric eigen-decomposition (cyclic Jacobi): eigenvalues ascending, eigenvectors as columns
// of the row-major n x n `vectors`.
void sym_eigen(std::vector<double> a, int n, std::vector<double>& values, std::vector<double>& vectors);

class ClusteringEngine {
   public:
    // State after construct_indices (ReadClusteringEngine.cpp:234-299) from the lookup's CSR
    // outputs (hga_lookup_result): read i has ReadID first_read_id + i.  `gpu` (may be null)
    // holds the same lookup on the device for the first connection pass and, unless
    // HGA_HOST_CONNECTIONS=1, the component state after merges; kci_ptr / kci_read are not read then.
    ClusteringEngine(const ClusteringConfig& cfg, bool debug, const RecordSet& reads, uint32_t first_read_id,
                     std::vector<uint64_t> hit_ptr, std::vector<uint32_t> sorted_kid, std::vector<uint64_t> first_ptr,
                     std::vector<uint32_t> first_kid, std::vector<uint32_t> first_pos,
                     const std::vector<uint64_t>& kci_ptr, const std::vector<uint32_t>& kci_read, hga_ctx* gpu);

    // run_clustering after construct_indices (:737-801); the timing lines go to `out`.
    std::vector<ComponentID> run(std::ostream& out);

    // print_components (:189-198) under debug: ids sorted in place by size, largest first (ties by
    // ascending id; std::sort leaves them unspecified there), then one ReadComponent::to_string line
    // each (ReadClusteringEngine.h:52-112): "#<id> : <per-category read counts a/b/..> [<per-category
    // simulator-coordinate intervals>]".
    void print_components(std::vector<ComponentID>& ids, std::ostream& out) const;
    std::string component_string(ComponentID id) const;

    // export_components (:804-826).
    void export_components(const std::vector<ComponentID>& ids, const std::string& dir, std::ostream& out) const;

    // Stages, public for the tests.
    // keep_fraction >= 0: return only the first (size_t)(n * keep_fraction) entries of the sorted list
    // (the device path fetches just that prefix, hga_connections_fetch_range).
    std::vector<Connection> get_connections(const std::vector<ComponentID>& pivots, Score min_score,
                                            uint32_t min_kmers = 0, double keep_fraction = -1.0);
    std::vector<Connection> get_all_connections(Score min_score, double keep_fraction = -1.0);
    std::vector<ComponentID> merge_components(const std::vector<ComponentList>& components);
    void remove_merged_components();
    std::vector<ComponentID> component_ids(uint64_t threshold_size) const;

    struct Component {   // ReadComponent, ReadClusteringEngine.h:36-113
        std::vector<uint32_t> reads;   // contained_read_ids
        std::vector<KmerID> kmers;     // discriminative_kmer_ids (sorted)
        std::set<int32_t> categories;
    };
    const std::map<ComponentID, Component>& components() const { return index_; }
    // (with the component state on the device: fetched with hga_components_fetch_index on every call)
    const std::vector<std::vector<ComponentID>>& kmer_component_index() const;
    // get_connections calls after the first merge answered by the device / by the host
    uint64_t connection_calls_device() const { return conn_dev_calls_; }
    uint64_t connection_calls_host() const { return conn_host_calls_; }
    bool used_gpu() const { return gpu_calls_ > 0; }
    // Spanning-tree edges of the tail stage whose overlap came from the batch (device or hook) / from
    // the host's approximate_read_overlap.
    uint64_t overlap_edges_device() const { return ov_edges_dev_; }
    uint64_t overlap_edges_host() const { return ov_edges_host_; }
    // Device connection pass over several ranks (categorization --gpus N): fn(pivots or empty for
    // "every read", min_score, min_kmers) -> connections in the reference order; replaces the
    // single-ctx call while the device indices describe the state.
    using DeviceConnections = std::function<std::vector<Connection>(const std::vector<ComponentID>&, Score, uint32_t)>;
    void set_device_connections(DeviceConnections fn) { dev_conn_ = std::move(fn); }
    // Batched overlaps of the tail stage: fn(x, y) -> approximate_read_overlap of each ReadID pair
    // (x[i], y[i]), both one-read components; replaces the single-ctx hga_read_overlaps call.
    // HGA_HOST_OVERLAPS=1 in the environment keeps every edge on the host.
    using DeviceOverlaps = std::function<std::vector<int>(const std::vector<ComponentID>& x, const std::vector<ComponentID>& y)>;
    void set_device_overlaps(DeviceOverlaps fn) { dev_ov_ = std::move(fn); }
    // hga_read_overlaps' semantics on the host, from the first-occurrence lists (the hook of the
    // device-less tests): the intersection of the two reads' distinct KmerID lists.
    std::vector<int> host_read_overlaps(const std::vector<ComponentID>& x, const std::vector<ComponentID>& y) const;
    // The tail stage without host KmerID lists (HGA_DEVICE_SETS=1 with the component state on the
    // device, or both hooks below set): every spanning-tree edge goes in one batch to
    // hga_components_overlaps (one call: its kernel takes hga_read_overlaps' path for a never-merged pair
    // by itself, so splitting the edges would only add a launch, a synchronisation and the bookkeeping),
    // and core_component_connections makes one hga_components_set_scores call over the amplified left
    // and right tail vertices of every scaffold component that are still in the index.  Under
    // HGA_DEVICE_SETS=1 the engine also builds no Component::kmers, its sorted_kid argument may be
    // empty, and merge_components skips the host union.
    // fn(x, y) -> approximate_read_overlap of each id pair on the CURRENT component lists.
    void set_device_component_overlaps(DeviceOverlaps fn) { dev_cov_ = std::move(fn); }
    // fn(sets, pairs) -> per pair (a, b) of set indices, |accumulate_kmer_ids(sets[a]) ∩ accumulate_kmer_ids(sets[b])|.
    using SetPairs = std::vector<std::pair<uint32_t, uint32_t>>;
    using DeviceSetScores = std::function<std::vector<Score>(const std::vector<ComponentList>& sets, const SetPairs& pairs)>;
    void set_device_set_scores(DeviceSetScores fn) { dev_sets_fn_ = std::move(fn); }
    // The two hooks' semantics on the host lists (the hooks of the device-less tests).
    std::vector<int> host_component_overlaps(const std::vector<ComponentID>& x, const std::vector<ComponentID>& y) const;
    std::vector<Score> host_set_scores(const std::vector<ComponentList>& sets, const SetPairs& pairs) const;
    // HGA_DEVICE_SETS=1 and neither HGA_HOST_CONNECTIONS=1 nor HGA_HOST_OVERLAPS=1: what an engine with
    // a ctx runs (the CLI then leaves sorted_kid on the device).
    static bool device_sets_requested();
    bool device_sets() const { return dev_sets_; }
    uint64_t set_score_calls() const { return sets_calls_; }
    // The spanning-tree tails of every scaffold tree in one call (hga_tree_tails with overlap = NULL and
    // the reads' lengths): under HGA_DEVICE_SETS=1, HGA_DEVICE_TAILS=1 / 0 selects it / the per-tree host
    // passes fed by the batched overlaps (unset: the device call).  The call then replaces
    // tree_overlaps and spanning_tree_tails; the overlaps never reach the host.
    // fn(components with their trees) -> per tree (left, right), each ascending.
    using TreeTails = std::vector<std::pair<std::vector<ComponentID>, std::vector<ComponentID>>>;
    using TreeList = std::vector<std::pair<ComponentList, SpanningTree>>;
    using DeviceTreeTails = std::function<TreeTails(const TreeList& comps_and_trees)>;
    void set_device_tree_tails(DeviceTreeTails fn) { dev_tt_fn_ = std::move(fn); }
    // The hook's semantics on the host (the hook of the device-less tests): the overlaps of every edge as
    // the engine's mode computes them, then spanning_tree_tails per tree.
    TreeTails host_tree_tails(const TreeList& comps_and_trees);
    static bool device_tails_requested();
    bool device_tails() const { return dev_tails_; }
    uint64_t tree_tails_calls() const { return tt_calls_; }
    // The first union_find call from a spanning forest (HGA_DEVICE_FOREST=1, opt-in).  With
    // scaffold_component_max_size = -1 and nothing restricted the loop (:424-489) rejects a connection only
    // when both ends are already in one component, so the accepted connections are the minimum spanning
    // forest of the list with the position as weight, and replaying union_find over them alone, in
    // position order, repeats the full list's merges (every other connection was a no-op).  run() then
    // leaves the sorted list on the device, has hga_spanning_forest find the accepted connections of the
    // scaffold-forming prefix and fetches only those (at most n_reads - 1) for the unchanged union_find.
    // Applies while the engine is pristine with a ctx (or the hook below), on the fraction path
    // (scaffold_forming_score == 0) with scaffold_component_max_size == -1; every other call runs as before.
    // fn(min_score, min_kmers, keep_fraction) -> the accepted (x, y) in position order and the prefix length.
    struct ForestEdges {
        SpanningTree edges;
        uint64_t connections = 0;   // the length of the list they were taken from (the scaffold-forming prefix; the enrichment list)
    };
    using DeviceForest = std::function<ForestEdges(Score min_score, uint32_t min_kmers, double keep_fraction)>;
    void set_device_forest(DeviceForest fn) { dev_forest_fn_ = std::move(fn); }
    // The hook's semantics on the host (the hook of the device-less tests): get_all_connections' prefix,
    // then the connections that join two components.
    ForestEdges host_forest(Score min_score, uint32_t min_kmers, double keep_fraction);
    // HGA_DEVICE_FOREST=1 without HGA_HOST_CONNECTIONS=1: what an engine with a ctx runs.
    static bool device_forest_requested();
    uint64_t forest_calls() const { return forest_calls_; }
    // The enrichment union_find (:785-794) from a restricted spanning forest (HGA_DEVICE_ENRICH=1, opt-in).
    // union_find(conns, restricted = core ids, 2, -1) also rejects a connection whose two components both
    // hold a restricted id (:456); with all restricted ids contracted into one vertex that is again the
    // minimum spanning forest of the list (hga.h, "Spanning forest"), and the replay over the accepted
    // connections with the same restricted set repeats the full list's merges.  When the step would read
    // the device's component state (merges done, no HGA_HOST_CONNECTIONS=1) run() leaves
    // hga_components_connections' list on the device, has hga_spanning_forest_restricted find the
    // accepted connections and fetches only those; a pristine engine, one without a ctx and one with only
    // a connection hook run the step as before.
    // fn(pivots = the core ids, also the restricted set; min_score) -> the accepted (x, y) in position
    // order and the length of the enrichment list.
    using DeviceEnrichForest = std::function<ForestEdges(const std::vector<ComponentID>& pivots, Score min_score)>;
    void set_device_enrich_forest(DeviceEnrichForest fn) { dev_enrich_fn_ = std::move(fn); }
    // The hook's semantics on the host (the hook of the device-less tests): get_connections' list, then the
    // loop's two rejection rules.
    ForestEdges host_enrich_forest(const std::vector<ComponentID>& pivots, Score min_score);
    // HGA_DEVICE_ENRICH=1 without HGA_HOST_CONNECTIONS=1: what an engine with a ctx runs.
    static bool device_enrich_requested();
    uint64_t enrich_forest_calls() const { return enrich_calls_; }
    // The debug plots (:759, :773, :782, :787, :798).  With a sink set, run() under debug hands it the wire
    // string of each plot the reference pipes to scripts/plotting.py, at the reference's sites and in its
    // order, with the kinds "connection_histogram" (:759), "spectral_graph" (:773, only when the spectral
    // stage runs), "component_coverage" (:782), "connection_histogram" (:787), "component_coverage" (:798);
    // force_spectral emits nothing (:739-746).  Without a sink nothing is computed and run() makes the calls
    // it made before, one for one.
    // The two connection histograms are statistics over a whole connection list.  Where the engine holds
    // that list (the host path, before it is cut to the scaffold-forming fraction; a connection hook's
    // fetch; get_connections' fetch for the enrichment) it counts on the host; where the list stays on the
    // device (the first pass's prefix fetch, HGA_DEVICE_FOREST=1, HGA_DEVICE_ENRICH=1) it calls
    // hga_connections_quality on the ctx's result, for the enrichment with one class per id numbering the
    // components' distinct category sets (is_good compares those sets, :319, and only the host holds them).
    using PlotSink = std::function<void(const char* kind, const std::string& wire)>;
    void set_plot_sink(PlotSink fn) { plot_sink_ = std::move(fn); }
    // fn(pivots, min_score, per_candidate) -> the histogram of the list the site plots in the current state:
    // per_candidate false (:759): get_all_connections(min_score), every row, pivots not read;
    // per_candidate true (:787): get_connections(pivots, min_score), the best row per candidate.
    // Replaces both the device call and the host count at :787, and at :759 on the fraction path (with
    // scaffold_forming_score > 0 the whole list is on the host and is counted there).
    using DeviceQuality = std::function<QualityHist(const std::vector<ComponentID>& pivots, Score min_score, bool per_candidate)>;
    void set_device_quality(DeviceQuality fn) { dev_quality_fn_ = std::move(fn); }
    // The hook's semantics on the host (the hook of the device-less tests): the list, then quality_of.
    QualityHist host_quality(const std::vector<ComponentID>& pivots, Score min_score, bool per_candidate);
    // plot_connection_quality's two loops (:19-31, :102-121) over an ordered list.
    static QualityHist quality_of(const std::vector<Connection>& connections, bool per_candidate);
    uint64_t quality_calls_device() const { return quality_dev_calls_; }
    uint64_t quality_calls_host() const { return quality_host_calls_; }

   private:
    bool plots_on() const { return debug_ && (bool)plot_sink_; }
    // hga_connections_quality on the ctx's current connection result
    QualityHist device_quality(bool per_candidate);
    std::string coverage_wire(const std::vector<ComponentID>& ids) const;
    bool forest_applies() const;
    bool enrich_forest_applies() const;
    // quality (may be null): filled from the list on the device, before the forest call reads it
    ForestEdges device_enrich_forest(const std::vector<ComponentID>& pivots, Score min_score, QualityHist* quality = nullptr);
    ForestEdges device_forest(Score min_score, uint32_t min_kmers, double keep_fraction, QualityHist* quality = nullptr);
    // hga_connections_run of the pristine state as get_connections calls it; returns the list's length
    uint64_t device_connections_run(const std::vector<ComponentID>& pivots, Score min_score, uint32_t min_kmers);
    bool sets_mode() const;
    size_t kmer_count(ComponentID id) const;
    std::vector<KmerID> accumulate_kmer_ids(const std::vector<ComponentID>& ids) const;
    uint32_t kmer_position(ComponentID read, KmerID kid) const;
    uint32_t read_length(ComponentID read) const;
    int approximate_read_overlap(ComponentID x, ComponentID y) const;
    // per tree, per edge: approximate_read_overlap (the batch where eligible, the host otherwise)
    std::vector<std::vector<int>> tree_overlaps(const std::vector<std::pair<ComponentList, SpanningTree>>& comps_and_trees);
    std::pair<std::vector<ComponentID>, std::vector<ComponentID>> spanning_tree_tails(const SpanningTree& tree,
                                                                                      const std::vector<int>& ov) const;
    TreeTails device_tree_tails(const TreeList& comps_and_trees);
    std::vector<ComponentID> amplify_component(const std::vector<ComponentID>& comp, Score min_score);
    std::vector<Connection> core_component_connections(
        const std::vector<std::pair<ComponentList, SpanningTree>>& comps_and_trees);
    bool is_good(ComponentID x, ComponentID y) const;
    std::vector<Connection> host_connections(const std::vector<ComponentID>& pivots, Score min_score) const;

    ClusteringConfig cfg_;
    bool debug_;
    const RecordSet& reads_;
    uint32_t first_id_;
    std::vector<uint64_t> hit_ptr_, first_ptr_;
    std::vector<uint32_t> first_kid_, first_pos_;
    std::map<ComponentID, Component> index_;
    mutable std::vector<std::vector<ComponentID>> kci_;
    size_t n_sdk_ = 0;          // KmerIDs (kci_.size() when the host holds the index)
    hga_ctx* gpu_;
    bool dev_comp_ = false;     // merges and post-merge connections on gpu_ (hga_components_*)
    uint64_t conn_dev_calls_ = 0, conn_host_calls_ = 0;
    DeviceConnections dev_conn_;
    DeviceOverlaps dev_ov_, dev_cov_;
    DeviceSetScores dev_sets_fn_;
    bool dev_sets_ = false;     // HGA_DEVICE_SETS=1 on the device component state: no KmerID lists here
    uint64_t sets_calls_ = 0;
    DeviceTreeTails dev_tt_fn_;
    bool dev_tails_ = false;    // dev_sets_ and the tree tails through hga_tree_tails
    std::vector<uint32_t> read_len_;   // by id - first_id_, built once when dev_tails_
    uint64_t tt_calls_ = 0;
    DeviceForest dev_forest_fn_;
    bool dev_forest_ = false;   // HGA_DEVICE_FOREST=1 with the component state on the device
    uint64_t forest_calls_ = 0, forest_conns_ = 0, forest_edges_ = 0;
    DeviceEnrichForest dev_enrich_fn_;
    bool dev_enrich_ = false;   // HGA_DEVICE_ENRICH=1 with the component state on the device
    uint64_t enrich_calls_ = 0, enrich_conns_ = 0, enrich_edges_ = 0;
    PlotSink plot_sink_;
    DeviceQuality dev_quality_fn_;
    uint64_t quality_dev_calls_ = 0, quality_host_calls_ = 0;
    uint64_t ov_edges_dev_ = 0, ov_edges_host_ = 0;
    bool pristine_ = true;   // no merge yet: the device indices still describe the state
    int gpu_calls_ = 0;
};

}  // namespace hgah
