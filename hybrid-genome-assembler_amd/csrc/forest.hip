// forest.hip — hga_spanning_forest[_restricted]: the connections union_find accepts
// (src/clustering/ReadClusteringEngine.cpp:424-489) when it has no size cap, i.e. the positions p of an
// ordered connection list at which get_parent(x) != get_parent(y) and (with restricted ids, :456) the two
// components do not both hold one.
//
// With an edge's weight its position in the list (all distinct), the edges of the unrestricted call are
// the unique minimum spanning forest of the multigraph, so any order of finding them gives the same set.
// The restricted call is the same on the multigraph with all restricted ids contracted into one vertex
// (hga.h, "Spanning forest"): only the start differs.  Borůvka rounds:
//
//   sf_init   comp[v] = v, best[v] = none.
//   sf_restrict   (restricted call only) comp[r] = R for every restricted vertex r, R the smallest of them.
//   sf_min    one pass over the live edges (round 0: the range itself).  cx = comp[x], cy = comp[y]; an
//             edge inside one component is dropped for good, any other is kept for the next round
//             (compacted through LDS, one cursor add per workgroup) and offered to both components:
//             best[c] = min(best[c], position).  The offers of late rounds meet on a handful of words,
//             and one word takes about 88 device atomics per µs chip-wide, so an offer
//             first reads best[c] (relaxed, agent scope; best only decreases, so a stale value costs
//             an atomic, never a minimum), and the lanes of a wave that share the first offering lane's
//             target send one atomic for their minimum.  Threads take edges in ascending position, so
//             the first waves set small minima and most later offers stop at the read.
//   sf_hook   per root c with a best edge e: other = the component across e.  When both chose e the
//             smaller id stays the root; every other root sets comp[c] = other and appends e, one edge
//             per hook (distinct weights: the chosen edges close no cycle but that pair).  comp is
//             read from one buffer and written to the other, as a root another thread reads may hook.
//   sf_jump   comp[v] = comp[comp[v]] for every vertex, double-buffered, until every vertex points at a
//             root: pointer doubling, since a chain listed in ascending order hooks into one path of
//             depth V - 1 in a single round.  A launch reports whether its RESULT still has a vertex
//             two steps from its root, so a path of depth d takes ceil(log2 d) launches and no
//             launch only to notice the end.  The first launch of a round also clears best and
//             publishes the round's counters into the mapped staging.
//   finish    the accepted positions sorted ascending (at most V - 1), x and y gathered at them.
//
// One host synchronisation per sf_jump launch, the first of which is the round's own.
//
// The contracted start.  After sf_restrict the pointer forest has depth <= 1: R is a root, every other
// restricted vertex points at it, every other vertex at itself.  That is a state the rounds already meet
// (it is what a star round leaves once flattened), so the kernels run as they are:
//   - "offers only ever go to roots": sf_min offers to comp[x] and comp[y], and every round starts flat (each
//     comp value is a root), the first one now by construction instead of by identity.  A restricted vertex
//     other than R is never a comp value, so it gets no offer, its best stays none, sf_hook copies its
//     pointer, and it is never a root again (sf_jump only moves pointers towards roots).
//   - acc holds at most V - 1: the hooks of all rounds are a forest of the contracted graph, which has
//     V - (distinct restricted ids) + 1 <= V vertices.
//   - "live edges but no hook": a live edge joins two roots, so both have a best; the smallest live position
//     is the best of both its ends, and the end with the larger id hooks.  No word of that depends on the start.
//   - max_jumps: a pointer path visits distinct vertices, so its depth is at most V - 1 whatever the start, and
//     ceil(log2 V) + 1 doublings flatten it.
// An edge between two restricted ids has cx == cy == R in round 0 and is dropped like a self-loop.
// In the enrichment list (:788-789) nearly every live edge has R on one side, so best[R] is the hot word of
// round 0: the restricted call relies on sf_offer's read before the atomic and on its one atomic per wave
// and target, which were written for the star shapes (one word takes ~88 device atomics per µs chip-wide).
#include "hga_internal.hpp"

namespace hga {
namespace {

constexpr uint32_t SF_NIL = 0xFFFFFFFFu;
constexpr int SF_T = 256;
constexpr int SF_EI = 8, SF_ETILE = SF_T * SF_EI;   // edges per thread / per workgroup of sf_min
constexpr int SF_VI = 4, SF_VTILE = SF_T * SF_VI;   // vertices per thread / per workgroup of sf_hook, sf_jump

// device words of one call
enum { SF_LIVE = 0, SF_ACC = 1, SF_WORDS = 2 };
// words of the mapped staging
enum { SF_H_LIVE = 0, SF_H_ACC = 1, SF_H_CHANGED = 2, SF_H_WORDS = 4 };

inline unsigned sf_grid(uint64_t n, int tile) { return (unsigned)((n + tile - 1) / tile); }

__global__ void __launch_bounds__(SF_T) sf_init(uint32_t* __restrict__ comp, uint32_t* __restrict__ best, uint32_t V,
                                                uint32_t* __restrict__ ctr) {
    const uint32_t v = blockIdx.x * SF_T + threadIdx.x;
    if (v < V) {
        comp[v] = v;
        best[v] = SF_NIL;
    }
    if (v < SF_WORDS) ctr[v] = 0;
}

// comp[r - first_id] = R for the n restricted ids (checked on the host; duplicates write the same word twice)
__global__ void __launch_bounds__(SF_T) sf_restrict(uint32_t* __restrict__ comp, const uint32_t* __restrict__ restricted,
                                                    uint32_t n, uint32_t first_id, uint32_t V, uint32_t R) {
    const uint32_t j = blockIdx.x * SF_T + threadIdx.x;
    if (j >= n) return;
    const uint32_t v = restricted[j] - first_id;
    if (v < V) comp[v] = R;
}

// best[t] = min(best[t], i) for the lanes with want set.  Called by every lane of the wave.
__device__ __forceinline__ void sf_offer(uint32_t* __restrict__ best, uint32_t t, uint32_t i, bool want, int lane) {
    if (want) want = __hip_atomic_load(&best[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > i;
    const unsigned long long m = __ballot(want);
    if (m == 0) return;   // (wave-uniform)
    const int lead = __ffsll((long long)m) - 1;
    const uint32_t t0 = __shfl(t, lead, 64);
    const bool grp = want && t == t0;
    if (__popcll(__ballot(grp)) > 1) {   // (wave-uniform) lanes that share a target: one atomic for their minimum
        uint32_t v = grp ? i : SF_NIL;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) v = min(v, (uint32_t)__shfl_xor(v, o, 64));
        if (lane == lead) atomicMin(&best[t0], v);
        want = want && !grp;
    }
    if (want) atomicMin(&best[t], i);
}

// live_in == nullptr: the positions are [0, n) themselves (round 0)
__global__ void __launch_bounds__(SF_T) sf_min(const uint32_t* __restrict__ ex, const uint32_t* __restrict__ ey,
                                               const uint32_t* __restrict__ live_in, uint32_t n, uint32_t first_id,
                                               uint32_t V, const uint32_t* __restrict__ comp, uint32_t* __restrict__ best,
                                               uint32_t* __restrict__ live_out, uint32_t* __restrict__ ctr) {
    __shared__ uint32_t kept[SF_ETILE];
    __shared__ uint32_t n_kept, base;
    const int lane = (int)(threadIdx.x & 63u);
    if (threadIdx.x == 0) n_kept = 0;
    __syncthreads();
    const uint64_t at = (uint64_t)blockIdx.x * SF_ETILE + threadIdx.x;
#pragma unroll 1
    for (int k = 0; k < SF_EI; ++k) {   // (static stride, the same trip count in every lane)
        const uint64_t j = at + (uint64_t)k * SF_T;
        uint32_t i = SF_NIL, cx = 0, cy = 0;
        bool keep = false;
        if (j < n) {
            i = live_in ? live_in[j] : (uint32_t)j;
            const uint32_t x = ex[i] - first_id, y = ey[i] - first_id;
            if (x < V && y < V) {
                cx = comp[x];
                cy = comp[y];
                keep = cx != cy;
            }
        }
        const unsigned long long km = __ballot(keep);
        if (km) {   // (wave-uniform)
            uint32_t wb = 0;
            if (lane == 0) wb = atomicAdd(&n_kept, (uint32_t)__popcll(km));
            wb = __shfl(wb, 0, 64);
            if (keep) kept[wb + (uint32_t)__popcll(km & ((1ull << lane) - 1))] = i;
        }
        sf_offer(best, cx, i, keep, lane);
        sf_offer(best, cy, i, keep, lane);
    }
    __syncthreads();
    const uint32_t m = n_kept;   // <= SF_ETILE
    if (threadIdx.x == 0 && m) base = atomicAdd(&ctr[SF_LIVE], m);
    __syncthreads();
    if (m == 0) return;
    const uint32_t b = base;     // the kept counts of all workgroups sum to at most n: inside live_out
    for (uint32_t q = threadIdx.x; q < m; q += SF_T) live_out[b + q] = kept[q];
}

__global__ void __launch_bounds__(SF_T) sf_hook(const uint32_t* __restrict__ ex, const uint32_t* __restrict__ ey,
                                                uint32_t first_id, uint32_t V, const uint32_t* __restrict__ best,
                                                const uint32_t* __restrict__ comp_in, uint32_t* __restrict__ comp_out,
                                                uint32_t* __restrict__ acc, uint32_t* __restrict__ ctr) {
    __shared__ uint32_t hooked[SF_VTILE];
    __shared__ uint32_t n_hooked, base;
    const int lane = (int)(threadIdx.x & 63u);
    if (threadIdx.x == 0) n_hooked = 0;
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < SF_VI; ++k) {
        const uint32_t v = blockIdx.x * SF_VTILE + k * SF_T + threadIdx.x;
        bool hook = false;
        uint32_t e = SF_NIL;
        if (v < V) {
            uint32_t to = comp_in[v];
            e = best[v];
            if (e != SF_NIL && to == v) {   // (offers only ever go to roots)
                const uint32_t cx = comp_in[ex[e] - first_id], cy = comp_in[ey[e] - first_id];
                const uint32_t other = cx == v ? cy : cx;
                if (other != v && !(best[other] == e && v < other)) {
                    to = other;
                    hook = true;
                }
            }
            comp_out[v] = to;
        }
        const unsigned long long hm = __ballot(hook);
        if (hm) {   // (wave-uniform)
            uint32_t wb = 0;
            if (lane == 0) wb = atomicAdd(&n_hooked, (uint32_t)__popcll(hm));
            wb = __shfl(wb, 0, 64);
            if (hook) hooked[wb + (uint32_t)__popcll(hm & ((1ull << lane) - 1))] = e;
        }
    }
    __syncthreads();
    const uint32_t m = n_hooked;   // <= SF_VTILE
    if (threadIdx.x == 0 && m) base = atomicAdd(&ctr[SF_ACC], m);
    __syncthreads();
    if (m == 0) return;
    const uint32_t b = base;
    // a forest on V vertices has at most V - 1 edges; acc holds V entries
    for (uint32_t q = threadIdx.x; q < m; q += SF_T)
        if (b + q < V) acc[b + q] = hooked[q];
}

// best != nullptr: the round's first launch (clears best, publishes the counters)
__global__ void __launch_bounds__(SF_T) sf_jump(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t V,
                                                uint32_t* __restrict__ best, const uint32_t* __restrict__ ctr,
                                                uint32_t* __restrict__ host_words) {
    int far = 0;
#pragma unroll
    for (int k = 0; k < SF_VI; ++k) {
        const uint32_t v = blockIdx.x * SF_VTILE + k * SF_T + threadIdx.x;
        if (v < V) {
            const uint32_t g = in[in[v]];
            out[v] = g;
            if (in[g] != g) far = 1;
            if (best) best[v] = SF_NIL;
        }
    }
    far = __syncthreads_or(far);
    if (threadIdx.x == 0) {
        if (far) host_words[SF_H_CHANGED] = 1;   // (the host zeroes it before the launch)
        if (best && blockIdx.x == 0) {
            host_words[SF_H_LIVE] = ctr[SF_LIVE];
            host_words[SF_H_ACC] = ctr[SF_ACC];
        }
    }
}

__global__ void __launch_bounds__(SF_T) sf_gather(const uint32_t* __restrict__ ex, const uint32_t* __restrict__ ey,
                                                  const uint32_t* __restrict__ acc, uint32_t m, uint64_t first,
                                                  uint64_t* __restrict__ pos, uint32_t* __restrict__ x,
                                                  uint32_t* __restrict__ y) {
    const uint32_t j = blockIdx.x * SF_T + threadIdx.x;
    if (j >= m) return;
    const uint32_t e = acc[j];
    pos[j] = first + e;
    x[j] = ex[e];
    y[j] = ey[e];
}

// n_restricted == 0: nothing of the restricted call is read or launched
void spanning_forest_run(hga_ctx* c, const uint32_t* x, const uint32_t* y, uint64_t n_given, uint64_t first, uint64_t count,
                         const uint32_t* restricted, uint64_t n_restricted, uint64_t* n_edges) {
    auto& L = c->lookup;
    auto& F = c->forest;
    HGA_REQUIRE(n_edges, HGA_ERR_INVALID, "null n_edges");
    HGA_REQUIRE(restricted || n_restricted == 0, HGA_ERR_INVALID, "null restricted list with a count");
    HGA_REQUIRE((x == nullptr) == (y == nullptr), HGA_ERR_INVALID, "exactly one of x and y is null");
    HGA_REQUIRE(L.ran, HGA_ERR_STATE, "hga_lookup_run not called");
    HGA_REQUIRE(x || c->conn.ready, HGA_ERR_STATE, "no connection result: hga_connections_run not called");
    const uint64_t total = x ? n_given : c->conn.n;
    const uint64_t a = std::min<uint64_t>(first, total), n64 = std::min<uint64_t>(count, total - a);
    HGA_REQUIRE(n64 <= 0xFFFFFFFEull, HGA_ERR_INVALID, "more than 2^32 - 2 entries: positions are 32-bit on the device");
    HGA_REQUIRE(L.n_reads < (1ull << 31), HGA_ERR_INVALID, "too many reads");
    const uint32_t n = (uint32_t)n64, V = (uint32_t)L.n_reads, first_id = L.first_read_id;
    if (x)
        for (uint64_t i = a; i < a + n64; ++i)
            HGA_REQUIRE(x[i] >= first_id && x[i] - first_id < V && y[i] >= first_id && y[i] - first_id < V, HGA_ERR_INVALID,
                        "id outside the lookup's reads");
    HGA_REQUIRE(n_restricted <= 0xFFFFFFFFull, HGA_ERR_INVALID, "more than 2^32 - 1 restricted ids");
    uint32_t R = SF_NIL;   // the smallest restricted vertex
    for (uint64_t i = 0; i < n_restricted; ++i) {
        HGA_REQUIRE(restricted[i] >= first_id && restricted[i] - first_id < V, HGA_ERR_INVALID,
                    "restricted id outside the lookup's reads");
        R = std::min(R, restricted[i] - first_id);
    }
    F.have = false;
    F.n = 0;
    F.first = a;
    if (n == 0 || V == 0) {
        F.have = true;
        *n_edges = 0;
        return;
    }
    const uint32_t *ex, *ey;
    if (x) {
        uint32_t* dx = static_cast<uint32_t*>(F.ex.ensure((uint64_t)n * 4));
        uint32_t* dy = static_cast<uint32_t*>(F.ey.ensure((uint64_t)n * 4));
        HGA_HIP(hipMemcpyAsync(dx, x + a, (uint64_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HGA_HIP(hipMemcpyAsync(dy, y + a, (uint64_t)n * 4, hipMemcpyHostToDevice, c->stream));
        ex = dx;
        ey = dy;
    } else {   // read in place: the connection result is not written
        ex = c->conn.ox.as<uint32_t>() + a;
        ey = c->conn.oy.as<uint32_t>() + a;
    }
    uint32_t* comp_a = static_cast<uint32_t*>(F.comp_a.ensure((uint64_t)V * 4));
    uint32_t* comp_b = static_cast<uint32_t*>(F.comp_b.ensure((uint64_t)V * 4));
    uint32_t* best = static_cast<uint32_t*>(F.best.ensure((uint64_t)V * 4));
    uint32_t* acc = static_cast<uint32_t*>(F.acc.ensure((uint64_t)V * 4));
    uint32_t* live_a = static_cast<uint32_t*>(F.live_a.ensure((uint64_t)n * 4));
    uint32_t* live_b = static_cast<uint32_t*>(F.live_b.ensure((uint64_t)n * 4));
    uint32_t* ctr = static_cast<uint32_t*>(F.ctr.ensure(SF_WORDS * 4));
    volatile uint32_t* hs = static_cast<uint32_t*>(c->pinned.ensure(SF_H_WORDS * 4));
    uint32_t* d_hs = c->pinned.dev(const_cast<uint32_t*>(hs));
    const unsigned vgrid = sf_grid(V, SF_VTILE);
    c->launch("sf_init", [&] { hipLaunchKernelGGL(sf_init, dim3(sf_grid(V, SF_T)), dim3(SF_T), 0, c->stream, comp_a, best, V, ctr); });
    c->check_launch("sf_init");
    if (n_restricted) {   // the contracted start: every restricted vertex points at R
        const uint32_t nr = (uint32_t)n_restricted;
        uint32_t* dr = static_cast<uint32_t*>(F.restricted.ensure((uint64_t)nr * 4));
        HGA_HIP(hipMemcpyAsync(dr, restricted, (uint64_t)nr * 4, hipMemcpyHostToDevice, c->stream));
        c->launch("sf_restrict", [&] {
            hipLaunchKernelGGL(sf_restrict, dim3(sf_grid(nr, SF_T)), dim3(SF_T), 0, c->stream, comp_a, dr, nr, first_id, V, R);
        });
        c->check_launch("sf_restrict");
    }

    int max_jumps = 1;   // ceil(log2 V) + 1
    while ((1ull << (max_jumps - 1)) < V) ++max_jumps;
    const uint32_t* live_in = nullptr;
    uint32_t live_n = n, accepted = 0;
    for (int round = 0;; ++round) {
        // (a round at least halves the components that still have a live edge)
        HGA_REQUIRE(round <= 33, HGA_ERR_HIP, "spanning forest: the rounds did not end");
        HGA_HIP(hipMemsetAsync(ctr + SF_LIVE, 0, 4, c->stream));
        c->launch("sf_min", [&] {
            hipLaunchKernelGGL(sf_min, dim3(sf_grid(live_n, SF_ETILE)), dim3(SF_T), 0, c->stream, ex, ey, live_in, live_n,
                               first_id, V, comp_a, best, live_a, ctr);
        });
        c->check_launch("sf_min");
        c->launch("sf_hook", [&] {
            hipLaunchKernelGGL(sf_hook, dim3(vgrid), dim3(SF_T), 0, c->stream, ex, ey, first_id, V, best, comp_a, comp_b, acc,
                               ctr);
        });
        c->check_launch("sf_hook");
        std::swap(comp_a, comp_b);
        bool flat = false;
        for (int j = 0; j < max_jumps && !flat; ++j) {
            hs[SF_H_CHANGED] = 0;
            c->launch("sf_jump", [&] {
                hipLaunchKernelGGL(sf_jump, dim3(vgrid), dim3(SF_T), 0, c->stream, comp_a, comp_b, V, j == 0 ? best : nullptr,
                                   ctr, d_hs);
            });
            c->check_launch("sf_jump");
            std::swap(comp_a, comp_b);
            c->sync();
            flat = hs[SF_H_CHANGED] == 0;
        }
        HGA_REQUIRE(flat, HGA_ERR_HIP, "spanning forest: the component pointers did not settle");
        const uint32_t kept = hs[SF_H_LIVE], acc_n = hs[SF_H_ACC];
        HGA_REQUIRE(kept <= live_n && acc_n >= accepted && acc_n < V, HGA_ERR_HIP, "spanning forest: counters out of range");
        const bool hooks = acc_n != accepted;
        accepted = acc_n;
        if (kept == 0) break;
        HGA_REQUIRE(hooks, HGA_ERR_HIP, "spanning forest: live edges but no hook");
        live_in = live_a;
        live_n = kept;
        std::swap(live_a, live_b);
    }

    if (accepted) {
        int bits = 1;
        while (bits < 32 && ((uint64_t)(n - 1) >> bits)) ++bits;
        radix_sort_u32(c, acc, nullptr, accepted, bits, F.sort);
        uint64_t* pos = static_cast<uint64_t*>(F.pos.ensure((uint64_t)accepted * 8));
        uint32_t* gx = static_cast<uint32_t*>(F.x.ensure((uint64_t)accepted * 4));
        uint32_t* gy = static_cast<uint32_t*>(F.y.ensure((uint64_t)accepted * 4));
        c->launch("sf_gather", [&] {
            hipLaunchKernelGGL(sf_gather, dim3(sf_grid(accepted, SF_T)), dim3(SF_T), 0, c->stream, ex, ey, acc, accepted, a, pos,
                               gx, gy);
        });
        c->check_launch("sf_gather");
        c->sync();
    }
    F.n = accepted;
    F.have = true;
    *n_edges = accepted;
}

}  // namespace

void spanning_forest(hga_ctx* c, const uint32_t* x, const uint32_t* y, uint64_t n, uint64_t first, uint64_t count,
                     uint64_t* n_edges) {
    spanning_forest_run(c, x, y, n, first, count, nullptr, 0, n_edges);
}

void spanning_forest_restricted(hga_ctx* c, const uint32_t* x, const uint32_t* y, uint64_t n, uint64_t first,
                                uint64_t count, const uint32_t* restricted, uint64_t n_restricted, uint64_t* n_edges) {
    c->forest.have = false;   // a failed call leaves no result to fetch
    spanning_forest_run(c, x, y, n, first, count, restricted, n_restricted, n_edges);
}

void spanning_forest_fetch(hga_ctx* c, uint64_t* pos, uint32_t* x, uint32_t* y) {
    auto& F = c->forest;
    HGA_REQUIRE(F.have, HGA_ERR_STATE, "hga_spanning_forest not called");
    if (F.n) {
        if (pos) HGA_HIP(hipMemcpyAsync(pos, F.pos.p, F.n * 8, hipMemcpyDeviceToHost, c->stream));
        if (x) HGA_HIP(hipMemcpyAsync(x, F.x.p, F.n * 4, hipMemcpyDeviceToHost, c->stream));
        if (y) HGA_HIP(hipMemcpyAsync(y, F.y.p, F.n * 4, hipMemcpyDeviceToHost, c->stream));
    }
    c->sync();
}

}  // namespace hga
