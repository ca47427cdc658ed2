// tails.hip — hga_tree_tails: get_spanning_tree_tails (src/clustering/ReadClusteringEngine.cpp:509-573)
// for every scaffold tree in one call.
//
// The reference runs three BFS passes per tree over hash containers: from the first vertex to the
// farthest one, from there to the "right" end, from there to the "left" end, each time with
//     dist(start) = length(start),  dist(child) = dist(parent) + length(child) - overlap(parent, child)
// in uint64 arithmetic (:529).  In a tree the distance of a vertex is a sum along its one path from the
// start, so no traversal order matters and the three passes are three prefix sums over one Euler tour:
//
//   tt_expand   2E directed edges keyed by (tree, source id); the stable radix sort groups every vertex's
//               out-edges, trees in input order, vertices in ascending id.  (The destination is left out
//               of the key: any fixed cyclic order of a vertex's out-edges gives a valid tour, and the
//               stable sort makes that order the input order.)
//   tt_inv      where each directed edge went, so that an edge finds its twin (the same edge reversed).
//   tt_link     next(u->v) = the out-edge of v after v->u, cyclically: the Euler tour of the tree.  The
//               cycle is cut in front of the tree's first sorted edge, an out-edge of its smallest id.
//   tt_jump     list ranking by pointer jumping, double-buffered, ceil(log2(2 * E_max)) rounds whatever
//               the depth of the trees; run once.  pos = the edge's place in the tour.
//   per pass    the tour rotated to an out-edge of the pass's start vertex is a depth-first walk from it:
//     tt_weigh    edge u->v is a down edge iff it precedes its twin; it weighs length(v) - overlap, the
//                 matching up edge the negative of that, scattered into tour order;
//     tt_scan_*   prefix sum modulo 2^64 over all tours at once (a tour's own sum is the difference to
//                 the prefix at its first slot; the library's single-pass scan carries 40 bits only);
//     tt_far_dist dist(v) = length(start) + prefix at v's down edge; the largest per tree, reduced over
//                 the lanes of a wave that share a tree before the one atomic per wave and tree;
//     tt_far_id   among the vertices at that distance the smallest id (= the smallest sorted position of
//                 a vertex's first out-edge), the same way; passes 2 and 3 also flag the vertices with
//                 dist + tail_length > max.  The next pass reads its start from this result on the device.
//   tt_compact  the flagged vertices per tree in ascending id (sorted order) behind an exclusive scan.
//
// The tree structure is checked on the host before anything is launched (union-find per tree: a
// repeated edge, a self-loop or a cycle joins two ids that are already joined; E + 1 distinct ids then
// mean one connected part), so the kernels only ever see forests.
#include "hga_internal.hpp"

namespace hga {
namespace {

constexpr uint32_t TT_NIL = 0xFFFFFFFFu;
constexpr int TT_SCAN_T = 256, TT_SCAN_I = 8, TT_SCAN_TILE = TT_SCAN_T * TT_SCAN_I;

inline unsigned tt_grid(uint64_t n) { return (unsigned)((n + 255) / 256); }
inline int tt_bits(uint64_t n) {   // bits to hold values in [0, n)
    int b = 1;
    while (b < 64 && ((n - 1) >> b)) ++b;
    return b;
}

// What the per-pass kernels read of the sorted directed edges.
struct TtEdges {
    const uint64_t* key;     // (tree << idb) | (source id - first_id), ascending
    const uint32_t* val;     // 2 * edge + orientation (1: the source is ey)
    const uint32_t* twin;    // sorted position of the reversed edge
    const uint32_t* head;    // sorted position of the source vertex's first out-edge
    const uint32_t* pos;     // place in the tree's tour as cut for pass 1
    const uint64_t* tptr2;   // 2 * tree_ptr: tree t's directed edges are [tptr2[t], tptr2[t + 1])
    const uint32_t* lx;      // read length of ex[q] / ey[q]
    const uint32_t* ly;
    const int32_t* ov;       // overlap of edge q
    uint32_t n2;
    int idb;
};

__global__ void __launch_bounds__(256) tt_expand(const uint32_t* __restrict__ ex, const uint32_t* __restrict__ ey,
                                                 const uint32_t* __restrict__ et, uint32_t n2, uint32_t first_id,
                                                 int idb, uint64_t* __restrict__ key, uint32_t* __restrict__ val) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n2) return;
    const uint32_t q = i >> 1;
    const uint32_t src = (i & 1u) ? ey[q] : ex[q];
    key[i] = ((uint64_t)et[q] << idb) | (uint64_t)(src - first_id);
    val[i] = i;
}

__global__ void __launch_bounds__(256) tt_inv(const uint32_t* __restrict__ val, uint32_t n2, uint32_t* __restrict__ where) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n2) where[val[i]] = i;
}

__device__ __forceinline__ uint32_t tt_lower_bound(const uint64_t* __restrict__ key, uint32_t lo, uint32_t hi, uint64_t k) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] < k) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// link[i] = (successor in the tour or TT_NIL at its end, hops to the end so far)
__global__ void __launch_bounds__(256) tt_link(const uint64_t* __restrict__ key, const uint32_t* __restrict__ val,
                                               const uint32_t* __restrict__ where, const uint64_t* __restrict__ tptr2,
                                               uint32_t n2, int idb, uint32_t* __restrict__ twin,
                                               uint32_t* __restrict__ head, uint2* __restrict__ link) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n2) return;
    const uint64_t k = key[i];
    const uint32_t t = (uint32_t)(k >> idb);
    const uint32_t base = (uint32_t)tptr2[t], end = (uint32_t)tptr2[t + 1];
    const uint32_t j = where[val[i] ^ 1u];
    twin[i] = j;
    head[i] = tt_lower_bound(key, base, i, k);
    const uint64_t kj = key[j];
    const uint32_t nxt = (j + 1 < end && key[j + 1] == kj) ? j + 1 : tt_lower_bound(key, base, j, kj);
    link[i] = nxt == base ? make_uint2(TT_NIL, 0u) : make_uint2(nxt, 1u);
}

__global__ void __launch_bounds__(256) tt_jump(const uint2* __restrict__ in, uint2* __restrict__ out, uint32_t n2) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n2) return;
    uint2 a = in[i];
    if (a.x != TT_NIL) {
        const uint2 b = in[a.x];
        a = make_uint2(b.x, a.y + b.y);
    }
    out[i] = a;
}

__global__ void __launch_bounds__(256) tt_pos(const uint2* __restrict__ link, const uint64_t* __restrict__ key,
                                              const uint64_t* __restrict__ tptr2, uint32_t n2, int idb,
                                              uint32_t* __restrict__ pos) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n2) return;
    const uint32_t t = (uint32_t)(key[i] >> idb);
    pos[i] = (uint32_t)(tptr2[t + 1] - tptr2[t]) - 1u - link[i].y;
}

// The pass's start edge of tree t: pass 0 the tree's first sorted edge, later the previous pass's farthest vertex.
__device__ __forceinline__ uint32_t tt_start(const uint32_t* __restrict__ prev_far, uint32_t t, uint32_t base) {
    return prev_far ? prev_far[t] : base;
}
__device__ __forceinline__ uint32_t tt_src_len(const TtEdges& g, uint32_t i) {
    const uint32_t v = g.val[i];
    return (v & 1u) ? g.ly[v >> 1] : g.lx[v >> 1];
}

// rp[i] = the edge's place in the tour rotated to the start edge, bit 31: a down edge
__global__ void __launch_bounds__(256) tt_weigh(TtEdges g, const uint32_t* __restrict__ prev_far, uint32_t* __restrict__ rp,
                                                uint64_t* __restrict__ w) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= g.n2) return;
    const uint32_t t = (uint32_t)(g.key[i] >> g.idb);
    const uint32_t base = (uint32_t)g.tptr2[t], len = (uint32_t)g.tptr2[t + 1] - base;
    const uint32_t ph = g.pos[tt_start(prev_far, t, base)];
    const uint32_t pi = g.pos[i], pj = g.pos[g.twin[i]];
    const uint32_t ri = pi >= ph ? pi - ph : pi + len - ph;
    const uint32_t rj = pj >= ph ? pj - ph : pj + len - ph;
    const bool down = ri < rj;
    const uint32_t v = g.val[i], q = v >> 1;
    const uint32_t lsrc = (v & 1u) ? g.ly[q] : g.lx[q], ldst = (v & 1u) ? g.lx[q] : g.ly[q];
    const uint64_t o = (uint64_t)(int64_t)g.ov[q];   // sign-extended, as the host's (uint64_t)(int64_t)
    w[base + ri] = down ? (uint64_t)ldst - o : o - (uint64_t)lsrc;
    rp[i] = ri | (down ? 0x80000000u : 0u);
}

// ---- prefix sum modulo 2^64: tile sums, their scan by one workgroup, the tiles' own scans on top
__device__ __forceinline__ uint64_t tt_block_excl(uint64_t v, uint64_t* lds, uint64_t& total) {
    const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
    uint64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t u = __shfl_up((unsigned long long)inc, o, 64);
        if (lane >= o) inc += u;
    }
    if (lane == 63) lds[wv] = inc;
    __syncthreads();
    uint64_t carry = 0, all = 0;
#pragma unroll
    for (int k = 0; k < TT_SCAN_T / 64; ++k) {
        if (k < wv) carry += lds[k];
        all += lds[k];
    }
    __syncthreads();   // lds is reused by the caller's next round
    total = all;
    return carry + inc - v;
}

__global__ void __launch_bounds__(TT_SCAN_T) tt_scan_sum(const uint64_t* __restrict__ w, uint64_t n, uint64_t* __restrict__ part) {
    __shared__ uint64_t lds[TT_SCAN_T / 64];
    const uint64_t at = (uint64_t)blockIdx.x * TT_SCAN_TILE;
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < TT_SCAN_I; ++k) {
        const uint64_t i = at + (uint64_t)k * TT_SCAN_T + threadIdx.x;
        if (i < n) s += w[i];
    }
    uint64_t total;
    (void)tt_block_excl(s, lds, total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

__global__ void __launch_bounds__(TT_SCAN_T) tt_scan_part(uint64_t* __restrict__ part, uint64_t nb) {
    __shared__ uint64_t lds[TT_SCAN_T / 64];
    uint64_t carry = 0;
    for (uint64_t at = 0; at < nb; at += TT_SCAN_T) {
        const uint64_t i = at + threadIdx.x;
        const uint64_t v = i < nb ? part[i] : 0;
        uint64_t total;
        const uint64_t e = tt_block_excl(v, lds, total);
        if (i < nb) part[i] = carry + e;
        carry += total;
    }
}

// in place: w[i] <- sum of w[0 .. i)
__global__ void __launch_bounds__(TT_SCAN_T) tt_scan_apply(uint64_t* __restrict__ w, uint64_t n, const uint64_t* __restrict__ part) {
    __shared__ uint64_t lds[TT_SCAN_T / 64];
    const uint64_t at = (uint64_t)blockIdx.x * TT_SCAN_TILE + (uint64_t)threadIdx.x * TT_SCAN_I;
    uint64_t v[TT_SCAN_I], s = 0;
#pragma unroll
    for (int k = 0; k < TT_SCAN_I; ++k) {
        v[k] = at + k < n ? w[at + k] : 0;
        s += v[k];
    }
    uint64_t total;
    uint64_t run = part[blockIdx.x] + tt_block_excl(s, lds, total);
#pragma unroll
    for (int k = 0; k < TT_SCAN_I; ++k) {
        if (at + k < n) w[at + k] = run;
        run += v[k];
    }
}

// ---- farthest vertex per tree.  Lanes of a wave hold consecutive sorted edges, so the lanes of one tree
// are contiguous: a shuffle-down reduction that only combines lanes of the same tree leaves each tree's
// result in its first lane of the wave, which issues the wave's one atomic for that tree.
struct TtLane {
    uint32_t t;       // tree, TT_NIL past the end
    bool down, root;  // the edge reaches its destination first / is the pass's start edge
    uint64_t d;       // distance of the destination (down edges)
    uint64_t lr;      // length of the start vertex (root)
    uint32_t start;
};
__device__ __forceinline__ TtLane tt_lane(const TtEdges& g, const uint32_t* __restrict__ prev_far, const uint32_t* __restrict__ rp,
                                          const uint64_t* __restrict__ x, uint32_t i) {
    TtLane r{TT_NIL, false, false, 0, 0, 0};
    if (i >= g.n2) return r;
    r.t = (uint32_t)(g.key[i] >> g.idb);
    const uint32_t base = (uint32_t)g.tptr2[r.t];
    r.start = tt_start(prev_far, r.t, base);
    r.lr = tt_src_len(g, r.start);
    r.root = i == r.start;
    const uint32_t p = rp[i];
    r.down = (p & 0x80000000u) != 0;
    if (r.down) r.d = r.lr + x[base + (p & 0x7FFFFFFFu) + 1] - x[base];
    return r;
}

__global__ void __launch_bounds__(256) tt_far_dist(TtEdges g, const uint32_t* __restrict__ prev_far, const uint32_t* __restrict__ rp,
                                                   const uint64_t* __restrict__ x, unsigned long long* __restrict__ tmax) {
    const int lane = (int)(threadIdx.x & 63u);
    const TtLane r = tt_lane(g, prev_far, rp, x, blockIdx.x * 256u + threadIdx.x);
    uint64_t c = r.down ? r.d : 0;   // 0: the identity of an unsigned maximum
    if (r.root && r.lr > c) c = r.lr;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t oc = __shfl_down((unsigned long long)c, o, 64);
        const uint32_t ot = __shfl_down(r.t, o, 64);
        if (lane + o < 64 && ot == r.t && oc > c) c = oc;
    }
    const uint32_t pt = __shfl_up(r.t, 1, 64);
    if (r.t != TT_NIL && (lane == 0 || pt != r.t)) atomicMax(&tmax[r.t], (unsigned long long)c);
}

__global__ void __launch_bounds__(256) tt_far_id(TtEdges g, const uint32_t* __restrict__ prev_far, const uint32_t* __restrict__ rp,
                                                 const uint64_t* __restrict__ x, const unsigned long long* __restrict__ tmax,
                                                 uint64_t tail, uint32_t* __restrict__ tfar, uint64_t* __restrict__ flag) {
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const TtLane r = tt_lane(g, prev_far, rp, x, i);
    const uint64_t mx = r.t != TT_NIL ? tmax[r.t] : 0;
    uint32_t c = TT_NIL;
    if (r.down) {
        const uint32_t hv = g.head[g.twin[i]];   // the destination vertex, by its first out-edge
        if (r.d == mx) c = hv;
        if (flag) flag[hv] = r.d + tail > mx ? 1 : 0;
    }
    if (r.root) {
        if (r.lr == mx && r.start < c) c = r.start;
        if (flag) flag[r.start] = r.lr + tail > mx ? 1 : 0;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t oc = __shfl_down(c, o, 64);
        const uint32_t ot = __shfl_down(r.t, o, 64);
        if (lane + o < 64 && ot == r.t && oc < c) c = oc;
    }
    const uint32_t pt = __shfl_up(r.t, 1, 64);
    if (r.t != TT_NIL && c != TT_NIL && (lane == 0 || pt != r.t)) atomicMin(&tfar[r.t], c);
}

// s: the exclusive scan of the vertex flags (n2 + 1 entries)
__global__ void __launch_bounds__(256) tt_compact(const uint64_t* __restrict__ key, const uint64_t* __restrict__ s, uint32_t n2,
                                                  int idb, uint32_t first_id, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n2) return;
    const uint64_t a = s[i];
    if (s[i + 1] != a) out[a] = (uint32_t)(key[i] & ((1ull << idb) - 1)) + first_id;
}

// per tree: where its two lists start, and the ids of the passes' farthest vertices (0 for a tree without edges)
__global__ void __launch_bounds__(256) tt_finish(const uint64_t* __restrict__ key, const uint64_t* __restrict__ tptr2,
                                                 const uint64_t* __restrict__ sl, const uint64_t* __restrict__ sr,
                                                 const uint32_t* __restrict__ tfar, uint32_t n_trees, int idb,
                                                 uint32_t first_id, uint64_t* __restrict__ ptr_l, uint64_t* __restrict__ ptr_r,
                                                 uint32_t* __restrict__ far_id) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t > n_trees) return;
    const uint64_t at = tptr2[t];
    ptr_l[t] = sl[at];
    ptr_r[t] = sr[at];
    if (t == n_trees) return;
    for (uint32_t p = 0; p < 3; ++p) {
        const uint32_t f = tfar[(uint64_t)p * n_trees + t];
        far_id[(uint64_t)p * n_trees + t] = f == TT_NIL ? 0u : (uint32_t)(key[f] & ((1ull << idb) - 1)) + first_id;
    }
}

void tt_prefix_sum(hga_ctx* c, uint64_t* w, uint64_t n, DevBuf& part_buf) {
    const uint64_t nb = (n + TT_SCAN_TILE - 1) / TT_SCAN_TILE;
    uint64_t* part = static_cast<uint64_t*>(part_buf.ensure(nb * 8));
    c->launch("tt_scan_sum", [&] { hipLaunchKernelGGL(tt_scan_sum, dim3((unsigned)nb), dim3(TT_SCAN_T), 0, c->stream, w, n, part); });
    c->check_launch("tt_scan_sum");
    c->launch("tt_scan_part", [&] { hipLaunchKernelGGL(tt_scan_part, dim3(1), dim3(TT_SCAN_T), 0, c->stream, part, nb); });
    c->check_launch("tt_scan_part");
    c->launch("tt_scan_apply", [&] { hipLaunchKernelGGL(tt_scan_apply, dim3((unsigned)nb), dim3(TT_SCAN_T), 0, c->stream, w, n, part); });
    c->check_launch("tt_scan_apply");
}

// find with path halving on the per-read parent array
inline uint32_t tt_find(std::vector<uint32_t>& parent, uint32_t r) {
    while (parent[r] != r) {
        parent[r] = parent[parent[r]];
        r = parent[r];
    }
    return r;
}

}  // namespace

void tree_tails(hga_ctx* c, const uint64_t* tree_ptr, const uint32_t* ex, const uint32_t* ey, uint64_t n_trees,
                const int32_t* overlap, const uint32_t* read_length, uint64_t tail_length, uint64_t* left_ptr,
                uint32_t* left, uint64_t* right_ptr, uint32_t* right, hga_tree_ends* ends) {
    auto& L = c->lookup;
    auto& S = c->tails;
    HGA_REQUIRE(L.ran, HGA_ERR_STATE, "hga_lookup_run not called");
    if (n_trees == 0) return;
    HGA_REQUIRE(tree_ptr && left_ptr && right_ptr, HGA_ERR_INVALID, "null tree_ptr / left_ptr / right_ptr");
    HGA_REQUIRE(n_trees < 0xFFFFFFFFull, HGA_ERR_INVALID, "too many trees");
    for (uint64_t t = 0; t < n_trees; ++t)
        HGA_REQUIRE(tree_ptr[t] <= tree_ptr[t + 1], HGA_ERR_INVALID, "tree_ptr decreases");
    const uint64_t e0 = tree_ptr[0], E = tree_ptr[n_trees] - e0;
    HGA_REQUIRE(E < (1ull << 30), HGA_ERR_INVALID, "too many tree edges");
    HGA_REQUIRE(E == 0 || (ex && ey && left && right), HGA_ERR_INVALID, "null edge or output list");
    const uint64_t first = L.first_read_id, nr = L.n_reads;
    if (!read_length) {
        HGA_REQUIRE(!(L.gathered && c->comm && c->comm->nranks > 1), HGA_ERR_STATE,
                    "read_length is required on a gathered ctx: the other ranks' reads are not here");
        HGA_REQUIRE(L.h_offsets.size() == nr + 1, HGA_ERR_STATE, "the ctx's read set does not match the lookup result");
    }
    ex = ex ? ex + e0 : ex;
    ey = ey ? ey + e0 : ey;
    if (overlap) overlap += e0;

    // ---- the structural check, and the per-edge tree and endpoint lengths
    std::vector<uint32_t> et(E), lx(E), ly(E);
    std::vector<uint64_t> tptr2(n_trees + 1);
    uint64_t e_max = 0;
    {
        std::vector<uint32_t> owner(nr, TT_NIL), parent(nr);
        auto len_of = [&](uint64_t r) {
            return read_length ? read_length[r] : (uint32_t)(L.h_offsets[r + 1] - L.h_offsets[r]);
        };
        for (uint64_t t = 0; t < n_trees; ++t) {
            const uint64_t a = tree_ptr[t] - e0, b = tree_ptr[t + 1] - e0;
            tptr2[t] = 2 * a;
            e_max = std::max(e_max, b - a);
            uint64_t vertices = 0;
            for (uint64_t q = a; q < b; ++q) {
                const uint32_t id[2] = {ex[q], ey[q]};
                uint32_t r[2];
                for (int s = 0; s < 2; ++s) {
                    HGA_REQUIRE(id[s] >= first && id[s] - first < nr, HGA_ERR_INVALID, "id outside the lookup's reads");
                    r[s] = (uint32_t)(id[s] - first);
                    if (owner[r[s]] == TT_NIL) {
                        owner[r[s]] = (uint32_t)t;
                        parent[r[s]] = r[s];
                        ++vertices;
                    }
                    HGA_REQUIRE(owner[r[s]] == (uint32_t)t, HGA_ERR_INVALID, "an id occurs in two trees");
                }
                const uint32_t ra = tt_find(parent, r[0]), rb = tt_find(parent, r[1]);
                HGA_REQUIRE(ra != rb, HGA_ERR_INVALID, "not a tree: self-loop, repeated edge or cycle");
                parent[ra] = rb;
                et[q] = (uint32_t)t;
                lx[q] = len_of(r[0]);
                ly[q] = len_of(r[1]);
            }
            HGA_REQUIRE(b == a || vertices == b - a + 1, HGA_ERR_INVALID, "not a tree: more than one connected part");
        }
        tptr2[n_trees] = 2 * E;
    }
    auto zero_ends = [&] {
        if (ends) std::memset(ends, 0, n_trees * sizeof(hga_tree_ends));
    };
    if (E == 0) {
        std::memset(left_ptr, 0, (n_trees + 1) * 8);
        std::memset(right_ptr, 0, (n_trees + 1) * 8);
        zero_ends();
        return;
    }

    // ---- upload
    const uint32_t n2 = (uint32_t)(2 * E), T = (uint32_t)n_trees;
    const uint32_t first_id = L.first_read_id;
    const int idb = tt_bits(std::max<uint64_t>(nr, 2)), bits = idb + tt_bits(std::max<uint64_t>(n_trees, 2));
    HGA_REQUIRE(bits <= 64, HGA_ERR_INVALID, "tree count and id range exceed the 64-bit sort key");
    uint32_t* dex = static_cast<uint32_t*>(S.ex.ensure(E * 4));
    uint32_t* dey = static_cast<uint32_t*>(S.ey.ensure(E * 4));
    uint32_t* det = static_cast<uint32_t*>(S.et.ensure(E * 4));
    uint32_t* dlx = static_cast<uint32_t*>(S.lx.ensure(E * 4));
    uint32_t* dly = static_cast<uint32_t*>(S.ly.ensure(E * 4));
    int32_t* dov = static_cast<int32_t*>(S.ov.ensure(E * 4));
    uint64_t* dtp = static_cast<uint64_t*>(S.tptr.ensure((n_trees + 1) * 8));
    HGA_HIP(hipMemcpyAsync(dex, ex, E * 4, hipMemcpyHostToDevice, c->stream));
    HGA_HIP(hipMemcpyAsync(dey, ey, E * 4, hipMemcpyHostToDevice, c->stream));
    HGA_HIP(hipMemcpyAsync(det, et.data(), E * 4, hipMemcpyHostToDevice, c->stream));
    HGA_HIP(hipMemcpyAsync(dlx, lx.data(), E * 4, hipMemcpyHostToDevice, c->stream));
    HGA_HIP(hipMemcpyAsync(dly, ly.data(), E * 4, hipMemcpyHostToDevice, c->stream));
    HGA_HIP(hipMemcpyAsync(dtp, tptr2.data(), (n_trees + 1) * 8, hipMemcpyHostToDevice, c->stream));
    if (overlap) HGA_HIP(hipMemcpyAsync(dov, overlap, E * 4, hipMemcpyHostToDevice, c->stream));
    else components_overlaps_device(c, dex, dey, E, dov);   // the weights never leave the device

    // ---- the tour
    uint64_t* key = static_cast<uint64_t*>(S.key.ensure((uint64_t)n2 * 8));
    uint32_t* val = static_cast<uint32_t*>(S.val.ensure((uint64_t)n2 * 4));
    uint32_t* where = static_cast<uint32_t*>(S.where.ensure((uint64_t)n2 * 4));
    uint32_t* twin = static_cast<uint32_t*>(S.twin.ensure((uint64_t)n2 * 4));
    uint32_t* head = static_cast<uint32_t*>(S.head.ensure((uint64_t)n2 * 4));
    uint32_t* pos = static_cast<uint32_t*>(S.pos.ensure((uint64_t)n2 * 4));
    uint32_t* rp = static_cast<uint32_t*>(S.rp.ensure((uint64_t)n2 * 4));
    uint2* la = static_cast<uint2*>(S.link_a.ensure((uint64_t)n2 * 8));
    uint2* lb = static_cast<uint2*>(S.link_b.ensure((uint64_t)n2 * 8));
    uint64_t* w = static_cast<uint64_t*>(S.w.ensure(((uint64_t)n2 + 1) * 8));
    uint64_t* fl = static_cast<uint64_t*>(S.flag_l.ensure(((uint64_t)n2 + 1) * 8));
    uint64_t* fr = static_cast<uint64_t*>(S.flag_r.ensure(((uint64_t)n2 + 1) * 8));
    unsigned long long* tmax = static_cast<unsigned long long*>(S.tmax.ensure(3ull * T * 8));
    uint32_t* tfar = static_cast<uint32_t*>(S.tfar.ensure(3ull * T * 4));
    uint32_t* far_id = static_cast<uint32_t*>(S.far_id.ensure(3ull * T * 4));
    uint64_t* ptr_l = static_cast<uint64_t*>(S.ptr_l.ensure((n_trees + 1) * 8));
    uint64_t* ptr_r = static_cast<uint64_t*>(S.ptr_r.ensure((n_trees + 1) * 8));
    uint32_t* out_l = static_cast<uint32_t*>(S.out_l.ensure((E + n_trees) * 4));
    uint32_t* out_r = static_cast<uint32_t*>(S.out_r.ensure((E + n_trees) * 4));
    HGA_HIP(hipMemsetAsync(w + n2, 0, 8, c->stream));
    HGA_HIP(hipMemsetAsync(fl, 0, ((uint64_t)n2 + 1) * 8, c->stream));
    HGA_HIP(hipMemsetAsync(fr, 0, ((uint64_t)n2 + 1) * 8, c->stream));
    HGA_HIP(hipMemsetAsync(tmax, 0, 3ull * T * 8, c->stream));
    HGA_HIP(hipMemsetAsync(tfar, 0xFF, 3ull * T * 4, c->stream));
    const unsigned grid = tt_grid(n2);
    c->launch("tt_expand", [&] {
        hipLaunchKernelGGL(tt_expand, dim3(grid), dim3(256), 0, c->stream, dex, dey, det, n2, first_id, idb, key, val);
    });
    c->check_launch("tt_expand");
    radix_sort_u64(c, key, val, n2, bits, S.sort);
    c->launch("tt_inv", [&] { hipLaunchKernelGGL(tt_inv, dim3(grid), dim3(256), 0, c->stream, val, n2, where); });
    c->check_launch("tt_inv");
    c->launch("tt_link", [&] {
        hipLaunchKernelGGL(tt_link, dim3(grid), dim3(256), 0, c->stream, key, val, where, dtp, n2, idb, twin, head, la);
    });
    c->check_launch("tt_link");
    int rounds = 0;
    while ((1ull << rounds) < 2 * e_max) ++rounds;   // ceil(log2(2 * E_max))
    for (int r = 0; r < rounds; ++r) {
        c->launch("tt_jump", [&] { hipLaunchKernelGGL(tt_jump, dim3(grid), dim3(256), 0, c->stream, la, lb, n2); });
        c->check_launch("tt_jump");
        std::swap(la, lb);
    }
    c->launch("tt_pos", [&] { hipLaunchKernelGGL(tt_pos, dim3(grid), dim3(256), 0, c->stream, la, key, dtp, n2, idb, pos); });
    c->check_launch("tt_pos");

    // ---- the three passes
    const TtEdges g{key, val, twin, head, pos, dtp, dlx, dly, dov, n2, idb};
    for (uint32_t p = 0; p < 3; ++p) {
        const uint32_t* prev = p ? tfar + (uint64_t)(p - 1) * T : nullptr;
        unsigned long long* pmax = tmax + (uint64_t)p * T;
        uint32_t* pfar = tfar + (uint64_t)p * T;
        uint64_t* flag = p == 0 ? nullptr : (p == 1 ? fr : fl);
        c->launch("tt_weigh", [&] { hipLaunchKernelGGL(tt_weigh, dim3(grid), dim3(256), 0, c->stream, g, prev, rp, w); });
        c->check_launch("tt_weigh");
        tt_prefix_sum(c, w, (uint64_t)n2 + 1, S.part);
        c->launch("tt_far_dist", [&] {
            hipLaunchKernelGGL(tt_far_dist, dim3(grid), dim3(256), 0, c->stream, g, prev, rp, w, pmax);
        });
        c->check_launch("tt_far_dist");
        c->launch("tt_far_id", [&] {
            hipLaunchKernelGGL(tt_far_id, dim3(grid), dim3(256), 0, c->stream, g, prev, rp, w, pmax, tail_length, pfar, flag);
        });
        c->check_launch("tt_far_id");
    }

    // ---- the tails, per tree in ascending id
    exclusive_scan_u64(c, fl, (uint64_t)n2 + 1, S.part);
    exclusive_scan_u64(c, fr, (uint64_t)n2 + 1, S.part);
    c->launch("tt_compact", [&] {
        hipLaunchKernelGGL(tt_compact, dim3(grid), dim3(256), 0, c->stream, key, fl, n2, idb, first_id, out_l);
        hipLaunchKernelGGL(tt_compact, dim3(grid), dim3(256), 0, c->stream, key, fr, n2, idb, first_id, out_r);
    });
    c->check_launch("tt_compact");
    c->launch("tt_finish", [&] {
        hipLaunchKernelGGL(tt_finish, dim3(tt_grid(n_trees + 1)), dim3(256), 0, c->stream, key, dtp, fl, fr, tfar, T, idb,
                           first_id, ptr_l, ptr_r, far_id);
    });
    c->check_launch("tt_finish");

    // ---- results: staged on the host, so that a failure on the way leaves the caller's arrays alone
    std::vector<uint64_t> h_pl(n_trees + 1), h_pr(n_trees + 1), h_max(3ull * T);
    std::vector<uint32_t> h_fid(3ull * T);
    HGA_HIP(hipMemcpyAsync(h_pl.data(), ptr_l, (n_trees + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HGA_HIP(hipMemcpyAsync(h_pr.data(), ptr_r, (n_trees + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HGA_HIP(hipMemcpyAsync(h_max.data(), tmax, 3ull * T * 8, hipMemcpyDeviceToHost, c->stream));
    HGA_HIP(hipMemcpyAsync(h_fid.data(), far_id, 3ull * T * 4, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    const uint64_t nl = h_pl[n_trees], nrt = h_pr[n_trees];
    HGA_REQUIRE(nl <= E + n_trees && nrt <= E + n_trees, HGA_ERR_HIP, "tree tails: list sizes out of range");
    std::vector<uint32_t> h_l(nl), h_r(nrt);
    if (nl) HGA_HIP(hipMemcpyAsync(h_l.data(), out_l, nl * 4, hipMemcpyDeviceToHost, c->stream));
    if (nrt) HGA_HIP(hipMemcpyAsync(h_r.data(), out_r, nrt * 4, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    std::memcpy(left_ptr, h_pl.data(), (n_trees + 1) * 8);
    std::memcpy(right_ptr, h_pr.data(), (n_trees + 1) * 8);
    if (nl) std::memcpy(left, h_l.data(), nl * 4);
    if (nrt) std::memcpy(right, h_r.data(), nrt * 4);
    if (ends) {
        zero_ends();
        for (uint64_t t = 0; t < n_trees; ++t) {
            if (tree_ptr[t] == tree_ptr[t + 1]) continue;
            ends[t].right_id = h_fid[T + t];
            ends[t].right_dist = h_max[T + t];
            ends[t].left_id = h_fid[2ull * T + t];
            ends[t].left_dist = h_max[2ull * T + t];
        }
    }
}

}  // namespace hga
