// quality.hip — hga_connections_quality: the two histograms plot_connection_quality pipes to the
// plotting script under -d (src/clustering/ReadClusteringEngine.cpp:19-34 over every connection, :102-124
// over the best connection per candidate), taken over an ordered connection list where it lies, on the
// device.
//
// The list is score-descending, so the rows of one score are one contiguous run and the histogram row of a
// connection follows from its position.  A row "counts" when it is kept (every row at :19-34; at :102-124
// the row of the smallest position among the rows with its y, which is the one the reference loop keeps:
// it replaces only on a strictly larger score) and it counts as good or bad.  With
//   b[i] = score[i] != score[i - 1]   (run start),   k[i] = kept,   g[i] = kept and good
// the counts of run r are differences of the exclusive prefix sums of k and g at the run starts.  So there
// is no histogram to add into: no atomic on a run's word, however many rows the run holds (one score holds
// most of a real list, and one word takes about 88 device atomics per µs chip-wide).
//
//   cq_first   (:102-124 only) first[y] = min(first[y], position), sf_min's offer: the word is read first
//              (relaxed, agent scope; it only decreases, so a stale value costs an atomic, never a minimum)
//              and the lanes of a wave that share the first offering lane's y send one atomic.  Rows are taken
//              in ascending position, so the first waves set small minima and later offers stop at the read.
//   cq_tile    per workgroup of CQ_TILE rows: the numbers of b, k and g in the tile (plain stores).
//   cq_scan    exclusive prefix sums of the three per-tile arrays, one workgroup each; entry n_tiles is the total.
//   cq_runs    per tile again, now with a prefix inside the tile: every run start writes its run's score and
//              the prefixes of k and g there, at the run's index (tile prefix of b + prefix inside the tile).
// The host reads the totals (one synchronisation: the number of runs sizes the buffers), then the runs, takes
// the differences, drops a run that kept no row and returns the rest score-ascending.
// Every ballot and shuffle is at the top level of a loop whose trip count is the same in every lane; no
// lane takes work from a device counter; every store is a plain vector store.
#include "hga_internal.hpp"

namespace hga {
namespace {

constexpr int CQ_T = 256, CQ_I = 8;
constexpr int CQ_TILE = CQ_T * CQ_I;   // rows per workgroup (hga_connections_quality_tile)
enum { CQ_B = 0, CQ_K = 1, CQ_G = 2, CQ_ARRAYS = 3 };

struct CqList {
    const uint32_t* x;
    const uint32_t* y;
    const uint64_t* s;
    const uint8_t* g;
    const int32_t* vc;      // class per vertex, or null: the stored flag
    const uint32_t* first;  // smallest position per vertex, or null: every row is kept
    uint32_t n, first_id, V;
};

// (b, k, g) of row i < n as bits 0, 1, 2
__device__ __forceinline__ uint32_t cq_flags(const CqList& L, uint32_t i) {
    const uint64_t s = L.s[i];
    const uint32_t b = (i == 0 || L.s[i - 1] != s) ? 1u : 0u;
    const uint32_t vx = L.x[i] - L.first_id, vy = L.y[i] - L.first_id;
    bool keep = true, good;
    if (L.first) {
        keep = vy < L.V && L.first[vy] == i;
        // the reference inserts {0, false} and replaces it only on a score above 0 (:105-108)
        if (s == 0) {
            good = false;
            return b | (keep ? 2u : 0u);
        }
    }
    if (L.vc)
        good = vx < L.V && vy < L.V && L.vc[vx] == L.vc[vy];
    else
        good = L.g[i] != 0;
    return b | (keep ? 2u : 0u) | (keep && good ? 4u : 0u);
}

// packed counts of a tile: b | k << 16 | g << 32 (each at most CQ_TILE = 2^11)
__device__ __forceinline__ unsigned long long cq_pack(uint32_t f) {
    return (unsigned long long)(f & 1u) | ((unsigned long long)((f >> 1) & 1u) << 16) |
           ((unsigned long long)((f >> 2) & 1u) << 32);
}

// inclusive scan over the workgroup; *total = the sum.  lds: CQ_T / 64 words.  Called by every thread.
__device__ __forceinline__ unsigned long long cq_block_scan(unsigned long long v, unsigned long long* lds,
                                                            unsigned long long* total) {
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    __syncthreads();   // (the previous call's readers are done with lds)
    if (lane == 63) lds[wave] = v;
    __syncthreads();
    unsigned long long before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < CQ_T / 64; ++w) {
        const unsigned long long t = lds[w];
        if (w < wave) before += t;
        all += t;
    }
    *total = all;
    return v + before;
}

__global__ void __launch_bounds__(CQ_T) cq_first(const uint32_t* __restrict__ y, uint32_t n, uint32_t first_id, uint32_t V,
                                                 uint32_t* __restrict__ first) {
    const int lane = (int)(threadIdx.x & 63u);
    const uint64_t at = (uint64_t)blockIdx.x * CQ_TILE + threadIdx.x;
#pragma unroll 1
    for (int k = 0; k < CQ_I; ++k) {   // (static stride, the same trip count in every lane)
        const uint64_t j = at + (uint64_t)k * CQ_T;
        uint32_t t = 0;
        bool want = false;
        if (j < n) {
            t = y[j] - first_id;
            want = t < V;
        }
        const uint32_t i = (uint32_t)j;
        if (want) want = __hip_atomic_load(&first[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > i;
        const unsigned long long m = __ballot(want);
        if (m == 0) continue;   // (wave-uniform)
        const int lead = __ffsll((long long)m) - 1;
        const uint32_t t0 = __shfl(t, lead, 64);
        const bool grp = want && t == t0;
        // the lanes that share the leader's y: positions ascend with the lane, so the leader's is their minimum
        if (lane == lead) atomicMin(&first[t0], i);
        if (want && !grp) atomicMin(&first[t], i);
    }
}

__global__ void __launch_bounds__(CQ_T) cq_tile(CqList L, uint32_t n_tiles, uint32_t* __restrict__ cnt) {
    __shared__ unsigned long long lds[CQ_T / 64];
    const uint64_t at = (uint64_t)blockIdx.x * CQ_TILE + threadIdx.x;
    unsigned long long sum = 0;
#pragma unroll 1
    for (int k = 0; k < CQ_I; ++k) {
        const uint64_t j = at + (uint64_t)k * CQ_T;
        if (j < L.n) sum += cq_pack(cq_flags(L, (uint32_t)j));
    }
    unsigned long long total;
    (void)cq_block_scan(sum, lds, &total);
    if (threadIdx.x == 0) {
        const size_t stride = (size_t)n_tiles + 1;
        cnt[CQ_B * stride + blockIdx.x] = (uint32_t)(total & 0xFFFFu);
        cnt[CQ_K * stride + blockIdx.x] = (uint32_t)((total >> 16) & 0xFFFFu);
        cnt[CQ_G * stride + blockIdx.x] = (uint32_t)(total >> 32);
    }
}

// workgroup a: cnt[a][0 .. n_tiles] becomes its exclusive prefix sums (entry n_tiles, zero before: the total)
__global__ void __launch_bounds__(CQ_T) cq_scan(uint32_t* __restrict__ cnt, uint32_t n_tiles) {
    __shared__ unsigned long long lds[CQ_T / 64];
    const uint64_t len = (uint64_t)n_tiles + 1;
    uint32_t* a = cnt + (size_t)blockIdx.x * len;
    unsigned long long carry = 0;
    const uint64_t chunks = (len + CQ_T - 1) / CQ_T;
#pragma unroll 1
    for (uint64_t q = 0; q < chunks; ++q) {   // (the same trip count in every thread)
        const uint64_t j = q * CQ_T + threadIdx.x;
        const unsigned long long v = j < len ? a[j] : 0;
        unsigned long long total;
        const unsigned long long inc = cq_block_scan(v, lds, &total);
        if (j < len) a[j] = (uint32_t)(carry + inc - v);
        carry += total;
    }
}

// thread t takes the CQ_I consecutive rows from tile start + t * CQ_I
__global__ void __launch_bounds__(CQ_T) cq_runs(CqList L, uint32_t n_tiles, const uint32_t* __restrict__ cnt, uint32_t R,
                                                uint64_t* __restrict__ run_score, uint32_t* __restrict__ run_k,
                                                uint32_t* __restrict__ run_g) {
    __shared__ unsigned long long lds[CQ_T / 64];
    const uint64_t j0 = (uint64_t)blockIdx.x * CQ_TILE + (uint64_t)threadIdx.x * CQ_I;
    uint32_t f[CQ_I];
    unsigned long long sum = 0;
#pragma unroll
    for (int k = 0; k < CQ_I; ++k) {
        f[k] = j0 + k < L.n ? cq_flags(L, (uint32_t)(j0 + k)) : 0u;
        sum += cq_pack(f[k]);
    }
    unsigned long long total;
    const unsigned long long before = cq_block_scan(sum, lds, &total) - sum;
    const size_t stride = (size_t)n_tiles + 1;
    uint32_t pb = cnt[CQ_B * stride + blockIdx.x] + (uint32_t)(before & 0xFFFFu);
    uint32_t pk = cnt[CQ_K * stride + blockIdx.x] + (uint32_t)((before >> 16) & 0xFFFFu);
    uint32_t pg = cnt[CQ_G * stride + blockIdx.x] + (uint32_t)(before >> 32);
#pragma unroll
    for (int k = 0; k < CQ_I; ++k) {
        if ((f[k] & 1u) && pb < R) {   // (pb < R: the totals come from the same flags)
            run_score[pb] = L.s[j0 + k];
            run_k[pb] = pk;
            run_g[pb] = pg;
        }
        pb += f[k] & 1u;
        pk += (f[k] >> 1) & 1u;
        pg += (f[k] >> 2) & 1u;
    }
}

inline unsigned cq_grid(uint64_t n) { return (unsigned)((n + CQ_TILE - 1) / CQ_TILE); }

template <class T>
T* cq_alloc(uint64_t n) {
    T* p = static_cast<T*>(std::malloc(std::max<uint64_t>(n, 1) * sizeof(T)));
    if (!p) throw std::bad_alloc();
    return p;
}

}  // namespace

uint32_t connections_quality_tile() { return (uint32_t)CQ_TILE; }

void connections_quality(hga_ctx* c, const uint32_t* x, const uint32_t* y, const uint64_t* score, const uint8_t* is_good,
                         uint64_t n_given, int per_candidate, const int32_t* vertex_class, uint64_t** out_score,
                         uint64_t** out_good, uint64_t** out_bad, uint64_t* n_rows) {
    auto& L = c->lookup;
    auto& Q = c->quality;
    HGA_REQUIRE(out_score && out_good && out_bad && n_rows, HGA_ERR_INVALID, "null out pointer");
    const bool given = x && y && score;
    HGA_REQUIRE(given || (!x && !y && !score), HGA_ERR_INVALID, "x, y and score are all null or all given");
    HGA_REQUIRE(L.ran, HGA_ERR_STATE, "hga_lookup_run not called");
    HGA_REQUIRE(given || c->conn.ready, HGA_ERR_STATE, "no connection result: hga_connections_run not called");
    const uint64_t n64 = given ? n_given : c->conn.n;
    HGA_REQUIRE(n64 <= 0xFFFFFFFEull, HGA_ERR_INVALID, "more than 2^32 - 2 entries: positions are 32-bit on the device");
    HGA_REQUIRE(L.n_reads < (1ull << 31), HGA_ERR_INVALID, "too many reads");
    const uint32_t n = (uint32_t)n64, V = (uint32_t)L.n_reads, first_id = L.first_read_id;
    if (given)
        for (uint64_t i = 0; i < n64; ++i) {
            HGA_REQUIRE(x[i] >= first_id && x[i] - first_id < V && y[i] >= first_id && y[i] - first_id < V, HGA_ERR_INVALID,
                        "id outside the lookup's reads");
            HGA_REQUIRE(i == 0 || score[i - 1] >= score[i], HGA_ERR_INVALID, "the list is not in result order (score descending)");
        }
    uint64_t *hs = nullptr, *hg = nullptr, *hb = nullptr;
    if (n == 0) {
        *out_score = cq_alloc<uint64_t>(0);
        *out_good = cq_alloc<uint64_t>(0);
        *out_bad = cq_alloc<uint64_t>(0);
        *n_rows = 0;
        return;
    }
    CqList D{};
    D.n = n;
    D.first_id = first_id;
    D.V = V;
    if (given) {
        uint32_t* dx = static_cast<uint32_t*>(Q.ex.ensure((uint64_t)n * 4));
        uint32_t* dy = static_cast<uint32_t*>(Q.ey.ensure((uint64_t)n * 4));
        uint64_t* ds = static_cast<uint64_t*>(Q.es.ensure((uint64_t)n * 8));
        uint8_t* dg = static_cast<uint8_t*>(Q.eg.ensure(n));
        HGA_HIP(hipMemcpyAsync(dx, x, (uint64_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HGA_HIP(hipMemcpyAsync(dy, y, (uint64_t)n * 4, hipMemcpyHostToDevice, c->stream));
        HGA_HIP(hipMemcpyAsync(ds, score, (uint64_t)n * 8, hipMemcpyHostToDevice, c->stream));
        if (is_good)
            HGA_HIP(hipMemcpyAsync(dg, is_good, n, hipMemcpyHostToDevice, c->stream));
        else
            HGA_HIP(hipMemsetAsync(dg, 0, n, c->stream));
        D.x = dx;
        D.y = dy;
        D.s = ds;
        D.g = dg;
    } else {   // read in place: the connection result is not written
        D.x = c->conn.ox.as<uint32_t>();
        D.y = c->conn.oy.as<uint32_t>();
        D.s = c->conn.os.as<uint64_t>();
        D.g = c->conn.og.as<uint8_t>();
    }
    if (vertex_class) {
        int32_t* dv = static_cast<int32_t*>(Q.vc.ensure((uint64_t)V * 4));
        HGA_HIP(hipMemcpyAsync(dv, vertex_class, (uint64_t)V * 4, hipMemcpyHostToDevice, c->stream));
        D.vc = dv;
    }
    const uint32_t nt = cq_grid(n);
    if (per_candidate) {
        uint32_t* first = static_cast<uint32_t*>(Q.first.ensure((uint64_t)V * 4));
        HGA_HIP(hipMemsetAsync(first, 0xFF, (uint64_t)V * 4, c->stream));   // ~0: no row yet
        c->launch("cq_first", [&] {
            hipLaunchKernelGGL(cq_first, dim3(nt), dim3(CQ_T), 0, c->stream, D.y, n, first_id, V, first);
        });
        c->check_launch("cq_first");
        D.first = first;
    }
    const size_t stride = (size_t)nt + 1;
    uint32_t* cnt = static_cast<uint32_t*>(Q.cnt.ensure(stride * CQ_ARRAYS * 4));
    HGA_HIP(hipMemsetAsync(cnt, 0, stride * CQ_ARRAYS * 4, c->stream));
    c->launch("cq_tile", [&] { hipLaunchKernelGGL(cq_tile, dim3(nt), dim3(CQ_T), 0, c->stream, D, nt, cnt); });
    c->check_launch("cq_tile");
    c->launch("cq_scan", [&] { hipLaunchKernelGGL(cq_scan, dim3(CQ_ARRAYS), dim3(CQ_T), 0, c->stream, cnt, nt); });
    c->check_launch("cq_scan");
    uint32_t* tot = static_cast<uint32_t*>(c->pinned.ensure(CQ_ARRAYS * 4));
    for (int a = 0; a < CQ_ARRAYS; ++a)
        HGA_HIP(hipMemcpyAsync(tot + a, cnt + a * stride + nt, 4, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    const uint32_t R = tot[CQ_B], tot_k = tot[CQ_K], tot_g = tot[CQ_G];
    HGA_REQUIRE(R >= 1 && R <= n && tot_k <= n && tot_g <= tot_k, HGA_ERR_HIP, "connection quality: counters out of range");
    uint64_t* rs = static_cast<uint64_t*>(Q.rs.ensure((uint64_t)R * 8));
    uint32_t* rk = static_cast<uint32_t*>(Q.rk.ensure((uint64_t)R * 4));
    uint32_t* rg = static_cast<uint32_t*>(Q.rg.ensure((uint64_t)R * 4));
    c->launch("cq_runs", [&] { hipLaunchKernelGGL(cq_runs, dim3(nt), dim3(CQ_T), 0, c->stream, D, nt, cnt, R, rs, rk, rg); });
    c->check_launch("cq_runs");
    std::vector<uint64_t> h_s(R);
    std::vector<uint32_t> h_k((size_t)R + 1), h_g((size_t)R + 1);
    HGA_HIP(hipMemcpyAsync(h_s.data(), rs, (uint64_t)R * 8, hipMemcpyDeviceToHost, c->stream));
    HGA_HIP(hipMemcpyAsync(h_k.data(), rk, (uint64_t)R * 4, hipMemcpyDeviceToHost, c->stream));
    HGA_HIP(hipMemcpyAsync(h_g.data(), rg, (uint64_t)R * 4, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    h_k[R] = tot_k;
    h_g[R] = tot_g;
    uint64_t rows = 0;
    for (uint32_t r = 0; r < R; ++r) {
        HGA_REQUIRE(h_k[r + 1] >= h_k[r] && h_g[r + 1] >= h_g[r] && h_g[r + 1] - h_g[r] <= h_k[r + 1] - h_k[r] &&
                        (r == 0 || h_s[r] < h_s[r - 1]),
                    HGA_ERR_HIP, "connection quality: runs out of order");
        rows += h_k[r + 1] > h_k[r];
    }
    try {
        hs = cq_alloc<uint64_t>(rows);
        hg = cq_alloc<uint64_t>(rows);
        hb = cq_alloc<uint64_t>(rows);
    } catch (...) {
        std::free(hs);
        std::free(hg);
        std::free(hb);
        throw;
    }
    uint64_t o = 0;
    for (uint32_t r = R; r-- > 0;) {   // the runs descend; the result ascends
        const uint64_t k = h_k[r + 1] - h_k[r], g = h_g[r + 1] - h_g[r];
        if (k == 0) continue;
        hs[o] = h_s[r];
        hg[o] = g;
        hb[o] = k - g;
        ++o;
    }
    *out_score = hs;
    *out_good = hg;
    *out_bad = hb;
    *n_rows = rows;
}

}  // namespace hga
