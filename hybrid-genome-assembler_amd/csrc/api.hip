// api.hip — the extern "C" surface declared in include/hga.h.  Catches every
// exception and maps it to an hga_status + thread-local message.
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "hga_internal.hpp"

namespace {
thread_local std::string g_err;

template <class F>
hga_status guard(F&& f) {
    // a body that returns a value on one path would fall off its end on the others (undefined)
    static_assert(std::is_void<decltype(f())>::value, "guarded bodies return nothing");
    try {
        g_err.clear();
        f();
        return HGA_OK;
    } catch (const hga::Error& e) {
        g_err = e.what();
        return e.code;
    } catch (const std::bad_alloc&) {
        g_err = "host allocation failed";
        return HGA_ERR_OOM;
    } catch (const std::exception& e) {
        g_err = e.what();
        return HGA_ERR_INVALID;
    }
}

hga_status need_ctx(hga_ctx* c) {
    if (!c) {
        g_err = "null context";
        return HGA_ERR_INVALID;
    }
    return HGA_OK;
}

template <class T>
T* host_dup(const T* src, size_t n) {
    T* p = static_cast<T*>(std::malloc(n ? n * sizeof(T) : 1));
    if (!p) throw std::bad_alloc();
    if (n) std::memcpy(p, src, n * sizeof(T));
    return p;
}

// Between hga_lookup_begin and hga_lookup_finish there is no lookup result and no resident read set.
void no_session(hga_ctx* c, const char* fn) {
    HGA_REQUIRE(!c->lookup.batch.open, HGA_ERR_STATE,
                std::string(fn) + ": a read-batch session is open (hga_lookup_begin without hga_lookup_finish)");
}
}  // namespace

#define HGA_CTX_GUARD(c, ...)                               \
    do {                                                    \
        if (need_ctx(c) != HGA_OK) return HGA_ERR_INVALID;  \
        return guard([&] {                                  \
            HGA_HIP(hipSetDevice((c)->device));             \
            __VA_ARGS__;                                    \
        });                                                 \
    } while (0)
// the same for a call that reads a lookup result or the resident reads: not inside a read-batch session
#define HGA_RESULT_GUARD(c, fn, ...) HGA_CTX_GUARD(c, { no_session(c, fn); __VA_ARGS__; })

extern "C" {

const char* hga_last_error(void) { return g_err.c_str(); }
void hga_free(void* p) { std::free(p); }
const char* hga_version(void) { return "hga-mi355x 0.1 (gfx950)"; }

hga_status hga_device_count(int* n) {
    return guard([&] {
        HGA_REQUIRE(n, HGA_ERR_INVALID, "null out pointer");
        int d = 0;
        HGA_HIP(hipGetDeviceCount(&d));
        *n = d;
    });
}

hga_status hga_ctx_create(hga_ctx** out, int device) {
    return guard([&] {
        HGA_REQUIRE(out, HGA_ERR_INVALID, "null out pointer");
        int nd = 0;
        HGA_HIP(hipGetDeviceCount(&nd));
        HGA_REQUIRE(device >= 0 && device < nd, HGA_ERR_INVALID, "no such HIP device");
        HGA_HIP(hipSetDevice(device));
        auto* c = new hga_ctx();
        c->device = device;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
            c->num_cu = prop.multiProcessorCount;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.totalGlobalMem > 0)
            c->total_mem = prop.totalGlobalMem;
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete c;
            throw hga::Error(HGA_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
        }
        *out = c;
    });
}

hga_status hga_ctx_destroy(hga_ctx* c) {
    if (!c) return HGA_OK;
    return guard([&] {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        if (c->side) (void)hipStreamSynchronize(c->side);
        hipStream_t s = c->stream, s2 = c->side;
        hipEvent_t e1 = c->ev_fork, e2 = c->ev_join, e3 = c->ev_sel;
        delete c;
        if (e3) (void)hipEventDestroy(e3);
        (void)hipStreamDestroy(s);
        if (s2) {
            (void)hipEventDestroy(e1);
            (void)hipEventDestroy(e2);
            (void)hipStreamDestroy(s2);
        }
    });
}

hga_status hga_count_begin(hga_ctx* c, int k, uint32_t n_files) {
    HGA_CTX_GUARD(c, hga::count_begin(c, k, n_files));
}

hga_status hga_count_add(hga_ctx* c, uint32_t file, const char* seq, uint64_t n_bytes) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(seq || n_bytes == 0, HGA_ERR_INVALID, "null sequence pointer");
        hga::count_add(c, file, seq, n_bytes);
    });
}

hga_status hga_count_add_file(hga_ctx* c, uint32_t file, const char* bytes, uint64_t n_bytes, hga_ingest_info* info) {
    HGA_CTX_GUARD(c, hga::count_add_file(c, file, bytes, n_bytes, info));
}

hga_status hga_count_seq(hga_ctx* c, uint32_t file, char** bytes, uint64_t* n) {
    HGA_CTX_GUARD(c, hga::count_seq(c, file, bytes, n));
}

uint32_t hga_ingest_tile(void) { return hga::ingest_tile(); }

hga_status hga_connections_run(hga_ctx* c, const uint32_t* pivots, uint64_t n_pivots, uint32_t min_kmers,
                               uint64_t min_score, const int32_t* categories, uint64_t* n) {
    HGA_RESULT_GUARD(c, "hga_connections_run", {
        HGA_REQUIRE(n, HGA_ERR_INVALID, "null out pointer");
        HGA_REQUIRE(pivots || n_pivots == 0, HGA_ERR_INVALID, "null pivots with n_pivots > 0");
        hga::connections_run(c, pivots, n_pivots, min_kmers, min_score, categories, n);
    });
}

hga_status hga_connections_fetch(hga_ctx* c, uint32_t* x, uint32_t* y, uint64_t* score, uint8_t* is_good) {
    HGA_CTX_GUARD(c, hga::connections_fetch(c, x, y, score, is_good));
}

hga_status hga_connections_fetch_range(hga_ctx* c, uint64_t first, uint64_t count, uint32_t* x, uint32_t* y,
                                       uint64_t* score, uint8_t* is_good) {
    HGA_CTX_GUARD(c, hga::connections_fetch(c, x, y, score, is_good, first, count));
}

hga_status hga_read_overlaps(hga_ctx* c, const uint32_t* x, const uint32_t* y, uint64_t n, int32_t* overlap,
                             uint32_t* shared) {
    HGA_RESULT_GUARD(c, "hga_read_overlaps", hga::read_overlaps(c, x, y, n, overlap, shared));
}

hga_status hga_components_merge(hga_ctx* c, const uint64_t* group_ptr, const uint32_t* ids, uint64_t n_groups) {
    HGA_RESULT_GUARD(c, "hga_components_merge", hga::components_merge(c, group_ptr, ids, n_groups));
}

hga_status hga_components_connections(hga_ctx* c, const uint32_t* pivots, uint64_t n_pivots, uint64_t min_score,
                                      uint64_t* n) {
    HGA_RESULT_GUARD(c, "hga_components_connections", {
        HGA_REQUIRE(n, HGA_ERR_INVALID, "null out pointer");
        HGA_REQUIRE(pivots || n_pivots == 0, HGA_ERR_INVALID, "null pivots with n_pivots > 0");
        hga::components_connections(c, pivots, n_pivots, min_score, n);
    });
}

hga_status hga_components_overlaps(hga_ctx* c, const uint32_t* x, const uint32_t* y, uint64_t n, int32_t* overlap,
                                   uint32_t* shared) {
    HGA_RESULT_GUARD(c, "hga_components_overlaps", hga::components_overlaps(c, x, y, n, overlap, shared));
}

hga_status hga_tree_tails(hga_ctx* c, const uint64_t* tree_ptr, const uint32_t* ex, const uint32_t* ey, uint64_t n_trees,
                          const int32_t* overlap, const uint32_t* read_length, uint64_t tail_length, uint64_t* left_ptr,
                          uint32_t* left, uint64_t* right_ptr, uint32_t* right, hga_tree_ends* ends) {
    HGA_RESULT_GUARD(c, "hga_tree_tails", hga::tree_tails(c, tree_ptr, ex, ey, n_trees, overlap, read_length, tail_length, left_ptr, left,
                                     right_ptr, right, ends));
}

hga_status hga_spanning_forest(hga_ctx* c, const uint32_t* x, const uint32_t* y, uint64_t n, uint64_t first, uint64_t count,
                               uint64_t* n_edges) {
    HGA_RESULT_GUARD(c, "hga_spanning_forest", hga::spanning_forest(c, x, y, n, first, count, n_edges));
}

hga_status hga_spanning_forest_restricted(hga_ctx* c, const uint32_t* x, const uint32_t* y, uint64_t n, uint64_t first,
                                          uint64_t count, const uint32_t* restricted, uint64_t n_restricted,
                                          uint64_t* n_edges) {
    HGA_RESULT_GUARD(c, "hga_spanning_forest_restricted", hga::spanning_forest_restricted(c, x, y, n, first, count, restricted, n_restricted, n_edges));
}

hga_status hga_spanning_forest_fetch(hga_ctx* c, uint64_t* pos, uint32_t* x, uint32_t* y) {
    HGA_CTX_GUARD(c, hga::spanning_forest_fetch(c, pos, x, y));
}

hga_status hga_connections_quality(hga_ctx* c, const uint32_t* x, const uint32_t* y, const uint64_t* score,
                                   const uint8_t* is_good, uint64_t n, int per_candidate, const int32_t* vertex_class,
                                   uint64_t** out_score, uint64_t** out_good, uint64_t** out_bad, uint64_t* n_rows) {
    HGA_RESULT_GUARD(c, "hga_connections_quality", hga::connections_quality(c, x, y, score, is_good, n, per_candidate, vertex_class, out_score, out_good,
                                              out_bad, n_rows));
}

uint32_t hga_connections_quality_tile(void) { return hga::connections_quality_tile(); }

hga_status hga_components_set_scores(hga_ctx* c, const uint64_t* set_ptr, const uint32_t* ids, uint64_t n_sets,
                                     const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, uint64_t* score,
                                     uint64_t* set_size) {
    HGA_RESULT_GUARD(c, "hga_components_set_scores", hga::components_set_scores(c, set_ptr, ids, n_sets, pair_a, pair_b, n_pairs, score, set_size));
}

hga_status hga_components_get_sizes(hga_ctx* c, hga_components_sizes* out) {
    HGA_RESULT_GUARD(c, "hga_components_get_sizes", {
        HGA_REQUIRE(out, HGA_ERR_INVALID, "null out pointer");
        hga::components_sizes(c, out);
    });
}

hga_status hga_components_fetch_index(hga_ctx* c, uint64_t* ptr, uint32_t* ids) {
    HGA_RESULT_GUARD(c, "hga_components_fetch_index", hga::components_fetch_index(c, ptr, ids));
}

hga_status hga_components_fetch_kmers(hga_ctx* c, uint32_t id, uint32_t* kmers, uint64_t* n) {
    HGA_RESULT_GUARD(c, "hga_components_fetch_kmers", {
        HGA_REQUIRE(n, HGA_ERR_INVALID, "null out pointer");
        hga::components_fetch_kmers(c, id, kmers, n);
    });
}

hga_status hga_components_reset(hga_ctx* c) {
    HGA_RESULT_GUARD(c, "hga_components_reset", {
        HGA_REQUIRE(c->lookup.ran, HGA_ERR_STATE, "hga_lookup_run not called");
        hga::components_drop(c);
    });
}

hga_status hga_count_add_rows(hga_ctx* c, uint32_t file, const uint64_t* keys, const uint32_t* counts,
                              uint64_t n) {
    HGA_CTX_GUARD(c, hga::count_add_rows(c, file, keys, counts, n));
}

hga_status hga_count_run(hga_ctx* c, uint32_t min_per_file) {
    HGA_CTX_GUARD(c, hga::count_run(c, min_per_file));
}

hga_status hga_count_set_passes(hga_ctx* c, uint32_t passes, uint64_t budget_bytes) {
    HGA_CTX_GUARD(c, hga::count_set_passes(c, passes, budget_bytes));
}

hga_status hga_count_estimate(hga_ctx* c, uint32_t min_per_file, uint32_t passes, uint64_t* bytes) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(bytes, HGA_ERR_INVALID, "null out pointer");
        *bytes = hga::count_estimate(c, min_per_file, passes);
    });
}

hga_status hga_count_get_pass_stats(hga_ctx* c, hga_count_pass_stats* out) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(out, HGA_ERR_INVALID, "null out pointer");
        auto& s = c->count;
        hga::count_settle(c);
        HGA_REQUIRE(s.ran, HGA_ERR_STATE, "hga_count_run not called");
        out->passes = s.run_passes;
        out->pad = 0;
        out->work_bytes = s.work_bytes;
        out->max_pass_instances = s.pass_max;
        out->min_pass_instances = s.pass_min;
    });
}

hga_status hga_count_get_stats(hga_ctx* c, hga_count_stats* out) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(out, HGA_ERR_INVALID, "null out pointer");
        auto& s = c->count;
        hga::count_settle(c);
        HGA_REQUIRE(s.ran, HGA_ERR_STATE, "hga_count_run not called");
        out->instances = s.instances;
        out->distinct_rows = s.rows;
        uint64_t b = 0;
        for (auto l : s.seq_len) b += l;
        out->bytes = b;
        if (s.dist) {   // after hga_count_exchange: the whole input over all ranks (no collective)
            out->distinct_rows = hga::count_global_rows(c);
            out->instances = s.g_instances;
            out->bytes = s.g_bytes;
        }
        out->buckets = s.buckets;
        out->max_split = s.max_split;
    });
}

hga_status hga_count_spec_hist(hga_ctx* c, const double* thr, uint32_t n_thr, int64_t** triples,
                               uint64_t* n) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(thr && triples && n, HGA_ERR_INVALID, "null pointer");
        std::vector<int64_t> v;
        if (c->count.dist) hga::count_spec_hist_global(c, thr, n_thr, v);
        else hga::count_spec_hist(c, thr, n_thr, v);
        *triples = host_dup(v.data(), v.size());
        *n = v.size() / 3;
    });
}

hga_status hga_count_select(hga_ctx* c, int64_t lower, int64_t upper, uint64_t** keys, uint64_t* n,
                            uint64_t* n_discriminative) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(keys && n && n_discriminative, HGA_ERR_INVALID, "null pointer");
        uint64_t m = 0, d = 0;
        if (c->count.dist) {
            hga::count_select_global(c, lower, upper, &m, &d);
            std::vector<uint64_t> k;
            std::vector<uint8_t> f;
            hga::count_fetch_selected_global(c, k, f);
            *keys = host_dup(k.data(), k.size());
            const bool leaf = hga::comm_is_gather_leaf(c);   // (hga_comm_set_root: an empty list here)
            *n = leaf ? 0 : m;
            *n_discriminative = leaf ? 0 : d;
            return;
        }
        hga::count_select(c, lower, upper, &m, &d);
        uint64_t* out = static_cast<uint64_t*>(std::malloc(m ? m * 8 : 8));
        if (!out) throw std::bad_alloc();
        hga::count_fetch_selected(c, out, nullptr);
        *keys = out;
        *n = m;
        *n_discriminative = d;
    });
}

hga_status hga_count_select_ex(hga_ctx* c, int64_t lower, int64_t upper, uint64_t** keys, uint8_t** disc,
                               uint64_t* n, uint64_t* n_discriminative) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(keys && disc && n && n_discriminative, HGA_ERR_INVALID, "null pointer");
        uint64_t m = 0, d = 0;
        if (c->count.dist) {
            hga::count_select_global(c, lower, upper, &m, &d);
            std::vector<uint64_t> k;
            std::vector<uint8_t> f;
            hga::count_fetch_selected_global(c, k, f);
            *keys = host_dup(k.data(), k.size());
            *disc = host_dup(f.data(), f.size());
            const bool leaf = hga::comm_is_gather_leaf(c);   // (hga_comm_set_root: an empty list here)
            *n = leaf ? 0 : m;
            *n_discriminative = leaf ? 0 : d;
            return;
        }
        hga::count_select(c, lower, upper, &m, &d);
        uint64_t* out = static_cast<uint64_t*>(std::malloc(m ? m * 8 : 8));
        uint8_t* fl = static_cast<uint8_t*>(std::malloc(m ? m : 1));
        if (!out || !fl) { std::free(out); std::free(fl); throw std::bad_alloc(); }
        hga::count_fetch_selected(c, out, fl);
        *keys = out;
        *disc = fl;
        *n = m;
        *n_discriminative = d;
    });
}

hga_status hga_count_select_device(hga_ctx* c, int64_t lower, int64_t upper, uint64_t* n,
                                   uint64_t* n_discriminative) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(n && n_discriminative, HGA_ERR_INVALID, "null pointer");
        if (c->count.dist) hga::count_select_global(c, lower, upper, n, n_discriminative);
        else hga::count_select(c, lower, upper, n, n_discriminative);
    });
}

hga_status hga_count_partition(hga_ctx* c, const uint64_t* splitters, uint32_t n_owners, uint64_t* keys_out,
                               uint32_t* counts_out, uint64_t* rows_per_owner) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(rows_per_owner && (n_owners <= 1 || splitters), HGA_ERR_INVALID, "null pointer");
        hga::count_partition(c, splitters, n_owners, keys_out, counts_out, rows_per_owner);
    });
}

hga_status hga_count_merge(hga_ctx* c, const uint64_t* keys, const uint32_t* counts, uint64_t n,
                           uint32_t min_per_file) {
    HGA_CTX_GUARD(c, { hga::count_merge(c, keys, counts, n, min_per_file); });
}

hga_status hga_count_pack_bits(hga_ctx* c, int* bits) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(bits, HGA_ERR_INVALID, "null pointer");
        HGA_REQUIRE(c->count.begun, HGA_ERR_STATE, "hga_count_begin not called");
        hga::count_settle(c);   // (a failed count reports here)
        *bits = hga::count_pack_bits(c);
    });
}

hga_status hga_count_partition_packed(hga_ctx* c, const uint64_t* splitters, uint32_t n_owners, uint64_t* out,
                                      uint64_t capacity, uint64_t* pieces_per_owner, uint64_t* total) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(pieces_per_owner && total && (n_owners <= 1 || splitters), HGA_ERR_INVALID, "null pointer");
        *total = hga::count_partition_packed(c, splitters, n_owners, out, capacity, pieces_per_owner);
        HGA_REQUIRE(*total <= capacity, HGA_ERR_OOM, "output capacity too small (see *total)");
    });
}

hga_status hga_count_merge_packed(hga_ctx* c, const uint64_t* pieces, uint64_t n, uint32_t min_per_file) {
    HGA_CTX_GUARD(c, { hga::count_merge_packed(c, pieces, n, min_per_file); });
}

hga_status hga_count_rows(hga_ctx* c, uint64_t** keys, uint32_t** counts, uint64_t* rows) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(keys && counts && rows, HGA_ERR_INVALID, "null pointer");
        // (no early return: the guarded lambda returns void on every path)
        if (!c->count.dist) {   // sorted on the device, copied straight into the returned buffers
            hga::count_rows_to(c, keys, counts, rows);
        } else {
            std::vector<uint64_t> k;
            std::vector<uint32_t> v;
            hga::count_rows_global(c, -1, k, v);
            *keys = host_dup(k.data(), k.size());
            *counts = host_dup(v.data(), v.size());
            *rows = k.size();
        }
    });
}

hga_status hga_count_dump(hga_ctx* c, uint32_t file, uint64_t** keys, uint32_t** counts, uint64_t* rows) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(keys && counts && rows, HGA_ERR_INVALID, "null pointer");
        HGA_REQUIRE(file < c->count.n_files, HGA_ERR_INVALID, "file index out of range");
        std::vector<uint64_t> k;
        std::vector<uint32_t> v;
        if (c->count.dist) hga::count_rows_global(c, (int)file, k, v);
        else hga::count_rows(c, (int)file, k, v);
        *keys = host_dup(k.data(), k.size());
        *counts = host_dup(v.data(), v.size());
        *rows = k.size();
    });
}

hga_status hga_lookup_load(hga_ctx* c, int k, const uint64_t* keys, uint32_t n) {
    HGA_RESULT_GUARD(c, "hga_lookup_load", {
        HGA_REQUIRE(keys || n == 0, HGA_ERR_INVALID, "null keys");
        hga::components_drop(c);
        hga::lookup_load(c, k, keys, n);
    });
}

hga_status hga_lookup_set_reads(hga_ctx* c, const char* bases, const uint64_t* offsets, uint64_t n_reads,
                                uint32_t first_read_id) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(offsets, HGA_ERR_INVALID, "null offsets");
        HGA_REQUIRE(bases || offsets[n_reads] == 0, HGA_ERR_INVALID, "null bases");
        hga::components_drop(c);
        hga::lookup_set_reads(c, bases, offsets, n_reads, first_read_id);
    });
}

hga_status hga_lookup_run(hga_ctx* c) {
    HGA_RESULT_GUARD(c, "hga_lookup_run", {
        hga::components_drop(c);
        hga::lookup_run(c);
    });
}

hga_status hga_lookup_get_sizes(hga_ctx* c, hga_lookup_sizes* out) {
    HGA_RESULT_GUARD(c, "hga_lookup_get_sizes", {
        HGA_REQUIRE(out, HGA_ERR_INVALID, "null out pointer");
        hga::lookup_sizes(c, out);
    });
}

hga_status hga_lookup_fetch(hga_ctx* c, const hga_lookup_result* out) {
    HGA_RESULT_GUARD(c, "hga_lookup_fetch", {
        HGA_REQUIRE(out, HGA_ERR_INVALID, "null out pointer");
        hga::lookup_fetch(c, out);
    });
}

hga_status hga_lookup_begin(hga_ctx* c, uint32_t first_read_id) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(c->lookup.loaded, HGA_ERR_STATE, "hga_lookup_load not called");
        hga::components_drop(c);
        hga::lookup_begin(c, first_read_id);
    });
}

hga_status hga_lookup_add_reads(hga_ctx* c, const char* bases, const uint64_t* offsets, uint64_t n_reads) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(offsets, HGA_ERR_INVALID, "null offsets");
        HGA_REQUIRE(bases || offsets[n_reads] == 0, HGA_ERR_INVALID, "null bases");
        hga::lookup_add_reads(c, bases, offsets, n_reads);
    });
}

hga_status hga_lookup_finish(hga_ctx* c) {
    HGA_CTX_GUARD(c, hga::lookup_finish(c));
}

hga_status hga_lookup_batch_estimate(hga_ctx* c, uint64_t batch_bases, uint64_t batch_reads, uint64_t* slot_bytes) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(slot_bytes, HGA_ERR_INVALID, "null out pointer");
        *slot_bytes = hga::lookup_batch_estimate(batch_bases, batch_reads);
    });
}

hga_status hga_lookup_get_batch_stats(hga_ctx* c, hga_lookup_batch_stats* out) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(out, HGA_ERR_INVALID, "null out pointer");
        HGA_REQUIRE(c->lookup.batch.ever, HGA_ERR_STATE, "hga_lookup_begin not called");
        *out = c->lookup.batch.stats;
    });
}

hga_status hga_hll_registers(hga_ctx* c, int k, uint32_t b, uint8_t* registers) {
    HGA_RESULT_GUARD(c, "hga_hll_registers", {
        HGA_REQUIRE(registers, HGA_ERR_INVALID, "null registers");
        hga::hll_registers(c, k, (int)b, registers);
    });
}

hga_status hga_profile_enable(hga_ctx* c, int on) {
    HGA_CTX_GUARD(c, {
        c->prof.drain();
        c->prof.on = on != 0;
    });
}

hga_status hga_profile_select(hga_ctx* c, const char* names) {
    HGA_CTX_GUARD(c, {
        c->prof.drain();
        c->prof.only.clear();
        std::string cur;
        for (const char* p = names ? names : ""; ; ++p) {
            if (*p == ',' || *p == 0) {
                if (!cur.empty()) c->prof.only.push_back(cur);
                cur.clear();
                if (*p == 0) break;
            } else {
                cur += *p;
            }
        }
    });
}

hga_status hga_profile_reset(hga_ctx* c) {
    HGA_CTX_GUARD(c, {
        c->prof.drain();
        c->prof.acc.clear();
    });
}

hga_status hga_profile_get(hga_ctx* c, const char* name, double* ms, uint64_t* launches) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(name && ms && launches, HGA_ERR_INVALID, "null pointer");
        c->prof.drain();
        auto it = c->prof.acc.find(name);
        *ms = it == c->prof.acc.end() ? 0.0 : it->second.first;
        *launches = it == c->prof.acc.end() ? 0 : it->second.second;
    });
}

hga_status hga_sync(hga_ctx* c) { HGA_CTX_GUARD(c, c->sync()); }

hga_status hga_comm_init(hga_ctx* c, const void* unique_id, int rank, int nranks) {
    HGA_CTX_GUARD(c, hga::comm_init_rccl(c, unique_id, rank, nranks));
}

hga_status hga_comm_init_host(hga_ctx* c, int rank, int nranks, const hga_transport* t) {
    HGA_CTX_GUARD(c, hga::comm_init_host(c, rank, nranks, t));
}

hga_status hga_comm_info(hga_ctx* c, int* rank, int* nranks) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(rank && nranks, HGA_ERR_INVALID, "null pointer");
        *rank = c->comm ? c->comm->rank : 0;
        *nranks = c->comm ? c->comm->nranks : 1;
    });
}

hga_status hga_comm_set_root(hga_ctx* c, int root) {
    HGA_CTX_GUARD(c, { hga::comm_set_root(c, root); });
}

hga_status hga_comm_destroy(hga_ctx* c) {
    HGA_CTX_GUARD(c, {
        c->sync();
        c->comm.reset();
        c->count.dist = false;
    });
}

hga_status hga_count_exchange(hga_ctx* c, uint32_t min_per_file) {
    HGA_CTX_GUARD(c, hga::count_exchange(c, min_per_file));
}

hga_status hga_lookup_gather(hga_ctx* c) {
    HGA_RESULT_GUARD(c, "hga_lookup_gather", {
        hga::components_drop(c);
        hga::lookup_gather(c);
    });
}

hga_status hga_connections_gather(hga_ctx* c, uint64_t* n) {
    HGA_CTX_GUARD(c, {
        HGA_REQUIRE(n, HGA_ERR_INVALID, "null out pointer");
        hga::connections_gather(c, n);
    });
}

}  // extern "C"
