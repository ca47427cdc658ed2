// components.hip — hga_components_*: ReadClusteringEngine::merge_components
// (src/clustering/ReadClusteringEngine.cpp:341-422) and get_connections (:301-333) on the state merges
// leave, on the device.
//
// State (ComponentState, hga_internal.hpp).  The lookup's arrays are only read.  The view keeps
//   idx / len   a copy of kci_val at the lookup's kci_ptr offsets plus the current length of every
//               KmerID's list: the reference's edit only ever removes entries, so a list shrinks in place;
//   pool        the merge survivors' KmerID unions, appended call by call;
//   ovr_off/len per read: where its current list is in the pool (~0: the read's own sorted_kid slice).
//
// One merge call.
//   cm_expand    every entry of every member's current list -> (group << 32 | KmerID) for the unions, and,
//                for the non-survivors, the removal pair (KmerID << 32 | read) at a host-scanned offset;
//   radix sort + cm_uniq_flag / scan / cm_uniq_put: the distinct (group, KmerID) pairs are the unions,
//                group by group and ascending; each also gives the survivor's removal pair;
//   radix sort of the removal pairs, cm_seg: the per-KmerID segments of the sorted pairs;
//   cm_edit      one wave per KmerID applies the two-pointer loop of :400-412 in closed form: the j-th
//                occurrence (from 0) of read c in the list is kept exactly when c < max(R) and
//                j >= mult_R(c), R the KmerID's removal multiset.  The loop stops when R is exhausted,
//                hence the bound by max(R): later entries are dropped whoever they belong to.
//
// Connections.  After merges the pivots are few and a survivor's list may hold most KmerIDs, so the work
// is split inside a pivot: one workgroup per 256 entries of a pivot's list flattens their index lists
// (cc_accum, block scan as connect.hip's cn_local does) and adds into a dense u32 score row per pivot,
// n_reads wide, in HBM.  cc_pairs counts, then emits (pivot, candidate, score) with score >= min_score
// into the ctx's connection buffers; connections_order (connect.hip) sorts and decodes them.
//
// Overlaps on the current lists (hga_components_overlaps: approximate_read_overlap :491-507 with merge
// survivors).  co_wave, one wave per pair in ov_wave's shape (overlap.hip): the shared KmerIDs are those of
// the two current lists, their positions each id's own read's (first_kid / first_pos), 0 when absent.
//
// Set scores (hga_components_set_scores: accumulate_kmer_ids :341-347 and the tail intersections
// :621-624).  Bitmaps, not sorted merges: a row of one bit per KmerID per set in HBM.  cs_bounds cuts every
// member list at the KmerID tile borders, cs_mark ORs a tile's share of every member list into its set's
// row (1024 entries per workgroup, so a union of most of K spreads over many), cs_pairs takes
// popcount(row a & row b) with 16-byte loads, one workgroup per pair; the sizes are the pairs (s, s).  The
// rows of one tile stay within CS_ROW_BYTES (HGA_SETS_BYTES); the host adds the tiles' counts up.
//
// Every loop runs over static wave or workgroup strides with wave-uniform bounds; no kernel draws work
// from a device counter.
#include <climits>
#include <cstdlib>

#include "hga_internal.hpp"

namespace hga {
namespace {

constexpr uint64_t CC_ROW_BYTES = 256ull << 20;   // score rows of one batch of pivots
constexpr int CC_T = 256;                         // cc_accum: list entries per workgroup
constexpr uint64_t CO_CHUNK = 1ull << 22;         // co_wave: pairs per launch (16 MiB per scratch array)
constexpr uint64_t CS_ROW_BYTES = 256ull << 20;   // set scores: the bitmap rows of one KmerID tile (HGA_SETS_BYTES)
constexpr int CS_E = 1024;                        // cs_mark: list entries per workgroup
constexpr uint64_t CS_CHUNK = 1ull << 22;         // cs_pairs: pairs per launch

inline unsigned cm_blocks(uint64_t n, uint64_t t, uint64_t cap) {
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + t - 1) / t, cap));
}
inline int cm_bits(uint64_t n) {   // bits to hold values in [0, n)
    int b = 1;
    while (b < 64 && ((n - 1) >> b)) ++b;
    return b;
}

// Where the current KmerID lists are.
struct CmLists {
    const uint64_t* hit_ptr;
    const uint32_t* skid;
    const uint64_t* ovr_off;
    const uint32_t* ovr_len;
    const uint32_t* pool;
};
__device__ __forceinline__ const uint32_t* cm_list(const CmLists& v, uint32_t r, uint32_t& n) {
    const uint64_t o = v.ovr_off[r];
    if (o != ~0ull) {
        n = v.ovr_len[r];
        return v.pool + o;
    }
    const uint64_t a = v.hit_ptr[r];
    n = (uint32_t)(v.hit_ptr[r + 1] - a);
    return v.skid + a;
}

// Members m of the call's groups: read mread[m], group mgrp[m]; moff[m] = entries of the members before m
// (moff[M] = T), roff[m] = the same over non-survivors only (~0 for a survivor).
__global__ void __launch_bounds__(256) cm_expand(CmLists v, const uint32_t* __restrict__ mread,
                                                 const uint32_t* __restrict__ mgrp, const uint64_t* __restrict__ moff,
                                                 const uint64_t* __restrict__ roff, uint32_t M, uint64_t T,
                                                 uint64_t* __restrict__ gk, uint64_t* __restrict__ rm) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < T; i += stride) {
        uint32_t a = 0, z = M;   // the member with moff[a] <= i < moff[a + 1]
        while (z - a > 1) {
            const uint32_t m = (a + z) >> 1;
            if (moff[m] <= i) a = m; else z = m;
        }
        uint32_t n;
        const uint32_t r = mread[a];
        const uint32_t* l = cm_list(v, r, n);
        const uint64_t e = i - moff[a];
        const uint32_t kid = l[e];
        gk[i] = ((uint64_t)mgrp[a] << 32) | kid;
        const uint64_t ro = roff[a];
        if (ro != ~0ull) rm[ro + e] = ((uint64_t)kid << 32) | r;
    }
}

__global__ void __launch_bounds__(256) cm_uniq_flag(const uint64_t* __restrict__ gk, uint64_t T,
                                                    uint64_t* __restrict__ flag) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < T; i += stride)
        flag[i] = (i == 0 || gk[i] != gk[i - 1]) ? 1ull : 0ull;
}

// pos: the exclusive scan of the flags.  The distinct pairs in order are the unions; gstart[g] = where
// group g's union starts, gstart[G] = their total.
__global__ void __launch_bounds__(256) cm_uniq_put(const uint64_t* __restrict__ gk, const uint64_t* __restrict__ pos,
                                                   uint64_t T, const uint32_t* __restrict__ surv, uint32_t G,
                                                   uint32_t* __restrict__ ubuf, uint64_t* __restrict__ rm_tail,
                                                   uint64_t* __restrict__ gstart) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < T; i += stride) {
        const uint64_t k = gk[i];
        const bool first = i == 0 || k != gk[i - 1];
        const uint64_t p = pos[i];
        if (first) {
            const uint32_t g = (uint32_t)(k >> 32), kid = (uint32_t)k;
            ubuf[p] = kid;
            rm_tail[p] = ((uint64_t)kid << 32) | surv[g];
            if (i == 0 || (uint32_t)(gk[i - 1] >> 32) != g) gstart[g] = p;
        }
        if (i == T - 1) gstart[G] = p + (first ? 1 : 0);
    }
}

// seg[2 * kid], seg[2 * kid + 1]: the KmerID's range of the sorted removal pairs (zeroed before: empty).
__global__ void __launch_bounds__(256) cm_seg(const uint64_t* __restrict__ rm, uint64_t R, uint32_t* __restrict__ seg) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < R; i += stride) {
        const uint32_t kid = (uint32_t)(rm[i] >> 32);
        if (i == 0 || (uint32_t)(rm[i - 1] >> 32) != kid) seg[2 * (uint64_t)kid] = (uint32_t)i;
        if (i == R - 1 || (uint32_t)(rm[i + 1] >> 32) != kid) seg[2 * (uint64_t)kid + 1] = (uint32_t)(i + 1);
    }
}

// One wave per KmerID with removal pairs.  The list is read in passes of 64 entries and written back
// compacted in place: a pass's kept entries land at or before the pass's own positions, and all of a
// pass's loads are issued before its stores.  The occurrence rank of an entry is its index minus the
// first index of its run of equal reads; the run start is carried across pass boundaries (carry_v,
// carry_f), not looked up in the list, whose front is already overwritten.
__global__ void __launch_bounds__(256) cm_edit(const uint64_t* __restrict__ kci_ptr, uint32_t* __restrict__ idx,
                                               uint32_t* __restrict__ len, const uint64_t* __restrict__ rm,
                                               const uint32_t* __restrict__ seg, uint32_t K,
                                               unsigned long long* __restrict__ removed) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t waves = gridDim.x * 4u;
    uint32_t gone = 0;   // entries this wave removed: one atomic per wave (same-address atomics serialise)
    for (uint32_t kid = wave; kid < K; kid += waves) {
        const uint32_t rs = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg[2 * (uint64_t)kid]);
        const uint32_t re = (uint32_t)__builtin_amdgcn_readfirstlane((int)seg[2 * (uint64_t)kid + 1]);
        if (re <= rs) continue;
        const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)len[kid]);
        if (n == 0) continue;
        uint32_t* __restrict__ L = idx + kci_ptr[kid];
        const uint64_t* __restrict__ R = rm + rs;
        const uint32_t nR = re - rs;
        const uint32_t maxR = (uint32_t)R[nR - 1];
        uint32_t out = 0, carry_v = 0, carry_f = 0;
        for (uint32_t base = 0; base < n; base += 64u) {
            const uint32_t i = base + lane;
            const bool act = i < n;
            const uint32_t v = act ? L[i] : 0xFFFFFFFFu;
            const uint32_t pv = __shfl_up(v, 1, 64);
            const bool start = lane == 0 ? (base == 0 || v != carry_v) : v != pv;
            uint32_t f = start ? i : (lane == 0 ? carry_f : 0u);   // inclusive max-scan: the run's first index
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t t = __shfl_up(f, o, 64);
                if ((int)lane >= o) f = max(f, t);
            }
            carry_v = __shfl(v, 63, 64);   // read again only when a further pass exists: lane 63 is active then
            carry_f = __shfl(f, 63, 64);
            bool keep = false;
            if (act && v < maxR) {
                uint32_t lo = 0, hi = nR;   // lower_bound(R, v)
                while (lo < hi) {
                    const uint32_t m = lo + ((hi - lo) >> 1);
                    if ((uint32_t)R[m] < v) lo = m + 1; else hi = m;
                }
                uint32_t up = lo, hi2 = nR;   // upper_bound(R, v)
                while (up < hi2) {
                    const uint32_t m = up + ((hi2 - up) >> 1);
                    if ((uint32_t)R[m] <= v) up = m + 1; else hi2 = m;
                }
                keep = (i - f) >= (up - lo);
            }
            const unsigned long long mask = __ballot(keep);
            if (keep) L[out + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = v;
            out += (uint32_t)__popcll(mask);
        }
        if (lane == 0) len[kid] = out;
        gone += n - out;
    }
    if (lane == 0 && gone) atomicAdd(removed, (unsigned long long)gone);
}

__global__ void cm_set_ovr(const uint32_t* __restrict__ surv, const uint64_t* __restrict__ gstart, uint32_t G,
                           uint64_t pool_base, uint64_t* __restrict__ ovr_off, uint32_t* __restrict__ ovr_len) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    ovr_off[surv[g]] = pool_base + gstart[g];
    ovr_len[surv[g]] = (uint32_t)(gstart[g + 1] - gstart[g]);
}

__global__ void __launch_bounds__(256) cm_len_init(const uint64_t* __restrict__ kci_ptr, uint32_t K,
                                                   uint32_t* __restrict__ len) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < K) len[k] = (uint32_t)(kci_ptr[k + 1] - kci_ptr[k]);
}

// Work item w: entries [wstart[w], wstart[w] + 256) of the list of pivot slot wslot[w].
__global__ void __launch_bounds__(CC_T) cc_accum(CmLists v, const uint64_t* __restrict__ kci_ptr,
                                                 const uint32_t* __restrict__ idx, const uint32_t* __restrict__ len,
                                                 const uint32_t* __restrict__ wslot, const uint32_t* __restrict__ wstart,
                                                 uint32_t W, const uint32_t* __restrict__ piv, uint64_t nr,
                                                 uint32_t* __restrict__ rows) {
    __shared__ uint32_t pre[CC_T + 1];
    __shared__ uint64_t st[CC_T];
    __shared__ uint32_t wsum[CC_T / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    for (uint32_t w = blockIdx.x; w < W; w += gridDim.x) {
        const uint32_t slot = wslot[w];
        uint32_t n;
        const uint32_t* l = cm_list(v, piv[slot], n);
        const uint32_t e = wstart[w] + t;
        uint32_t ln = 0;
        uint64_t s0 = 0;
        if (e < n) {
            const uint32_t kid = l[e];
            ln = len[kid];
            s0 = kci_ptr[kid];
        }
        uint32_t inc = ln;   // inclusive scan inside the wave, then over the four waves
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t x = __shfl_up(inc, o, 64);
            if ((int)lane >= o) inc += x;
        }
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        uint32_t wbase = 0;
        for (uint32_t q = 0; q < wv; ++q) wbase += wsum[q];
        pre[t] = wbase + inc - ln;
        st[t] = s0;
        if (t == CC_T - 1) pre[CC_T] = wbase + inc;
        __syncthreads();
        const uint32_t total = pre[CC_T];
        uint32_t* __restrict__ row = rows + (uint64_t)slot * nr;
        for (uint32_t j = t; j < total; j += CC_T) {
            uint32_t a = 0, z = CC_T;   // the entry with pre[a] <= j < pre[a + 1]
            while (z - a > 1) {
                const uint32_t m = (a + z) >> 1;
                if (pre[m] <= j) a = m; else z = m;
            }
            atomicAdd(&row[idx[st[a] + (j - pre[a])]], 1u);
        }
        __syncthreads();   // pre / st / wsum are reused by the next work item
    }
}

// ctr[0] pairs, ctr[1] largest score (EMIT = false); ctr[2] output cursor (EMIT = true).
template <bool EMIT>
__global__ void __launch_bounds__(256) cc_pairs(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ piv,
                                                uint64_t nr, uint64_t cells, uint32_t ms, uint64_t out_base,
                                                unsigned long long* __restrict__ ctr, uint32_t* __restrict__ ox,
                                                uint32_t* __restrict__ oy, uint32_t* __restrict__ os) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    // every lane of a wave runs the same number of rounds: the bound is on the wave's first cell
    for (uint64_t b = (uint64_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u); b < cells; b += stride) {
        const uint64_t i = b + lane;
        uint32_t s = 0, p = 0, cnd = 0;
        bool keep = false;
        if (i < cells) {
            s = rows[i];
            p = piv[i / nr];
            cnd = (uint32_t)(i % nr);
            keep = s >= ms && cnd != p;
        }
        const unsigned long long mask = __ballot(keep);
        if (!mask) continue;
        const uint32_t cnt = (uint32_t)__popcll(mask);
        if (!EMIT) {
            uint32_t mx = keep ? s : 0u;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, o, 64));
            if (lane == 0) {
                atomicAdd(&ctr[0], (unsigned long long)cnt);
                atomicMax(&ctr[1], (unsigned long long)mx);
            }
        } else {
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(&ctr[2], (unsigned long long)cnt);
            at = __shfl(at, 0, 64);
            if (keep) {
                const uint64_t o = out_base + at + (uint64_t)__popcll(mask & ((1ull << lane) - 1ull));
                ox[o] = p;
                oy[o] = cnd;
                os[o] = s;
            }
        }
    }
}

// kmer_positions[kid] of read r: the position in its own first_kid slice, 0 when the read lacks the KmerID
__device__ __forceinline__ int co_pos(const uint64_t* __restrict__ fptr, const uint32_t* __restrict__ fkid,
                                      const uint32_t* __restrict__ fpos, uint32_t r, uint32_t kid) {
    uint64_t lo = fptr[r], hi = fptr[r + 1];
    const uint64_t end = hi;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (fkid[mid] < kid) lo = mid + 1;
        else hi = mid;
    }
    return lo < end && fkid[lo] == kid ? (int)fpos[lo] : 0;
}

// One wave per pair, as ov_wave (overlap.hip): the lanes stride over the shorter current list, skip an
// entry equal to its predecessor and binary-search the longer list.  A pair of ids without an override
// takes the two first_kid lists (distinct, their positions beside them); any other pair looks each
// shared KmerID up in either read's own first_kid slice.
__global__ __launch_bounds__(256) void co_wave(CmLists v, const uint64_t* __restrict__ fptr,
                                               const uint32_t* __restrict__ fkid, const uint32_t* __restrict__ fpos,
                                               const uint32_t* __restrict__ ex, const uint32_t* __restrict__ ey,
                                               uint32_t n, uint32_t first_id, int32_t* __restrict__ ov,
                                               uint32_t* __restrict__ sh) {
    const int lane = (int)(threadIdx.x & 63u);
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
    const uint32_t waves = gridDim.x * 4u;
    for (uint32_t e = wave; e < n; e += waves) {
        uint32_t ra = ex[e] - first_id, rb = ey[e] - first_id;   // validated on the host
        const bool plain = v.ovr_off[ra] == ~0ull && v.ovr_off[rb] == ~0ull;   // the same in every lane
        const uint32_t *A, *B;
        uint32_t la, lb;
        if (plain) {
            A = fkid + fptr[ra];
            la = (uint32_t)(fptr[ra + 1] - fptr[ra]);
            B = fkid + fptr[rb];
            lb = (uint32_t)(fptr[rb + 1] - fptr[rb]);
        } else {
            A = cm_list(v, ra, la);
            B = cm_list(v, rb, lb);
        }
        if (la > lb) {   // a: the shorter list; pa / pb below follow the swap, the result is symmetric
            const uint32_t* tp = A;
            A = B;
            B = tp;
            const uint32_t tl = la;
            la = lb;
            lb = tl;
            const uint32_t tr = ra;
            ra = rb;
            rb = tr;
        }
        const uint64_t a0 = fptr[ra], b0 = fptr[rb];
        int cnt = 0, min_a = INT_MAX, max_a = INT_MIN, min_b = INT_MAX, max_b = INT_MIN;
        uint32_t lo = 0;   // a lane's KmerIDs do not descend: each search starts where its last one ended
        for (uint32_t i = (uint32_t)lane; i < la; i += 64u) {
            const uint32_t kid = A[i];
            if (i > 0 && A[i - 1] == kid) continue;
            uint32_t hi = lb;
            while (lo < hi) {   // lower_bound(B, kid)
                const uint32_t mid = lo + ((hi - lo) >> 1);
                if (B[mid] < kid) lo = mid + 1;
                else hi = mid;
            }
            if (lo < lb && B[lo] == kid) {
                const int pa = plain ? (int)fpos[a0 + i] : co_pos(fptr, fkid, fpos, ra, kid);
                const int pb = plain ? (int)fpos[b0 + lo] : co_pos(fptr, fkid, fpos, rb, kid);
                ++cnt;
                min_a = min(min_a, pa);
                max_a = max(max_a, pa);
                min_b = min(min_b, pb);
                max_b = max(max_b, pb);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cnt += __shfl_xor(cnt, o, 64);
            min_a = min(min_a, __shfl_xor(min_a, o, 64));
            max_a = max(max_a, __shfl_xor(max_a, o, 64));
            min_b = min(min_b, __shfl_xor(min_b, o, 64));
            max_b = max(max_b, __shfl_xor(max_b, o, 64));
        }
        if (lane == 0) {
            ov[e] = cnt ? max(max_a - min_a, max_b - min_b) : 0;
            sh[e] = (uint32_t)cnt;
        }
    }
}

// Set scores.  Member m of the call: read mread[m] in set mset[m].  bnd[m * (T + 1) + t]: the first entry
// of the member's current (ascending) list with KmerID >= t * tile_k, so tile t's share of the list is
// [bnd[.. + t], bnd[.. + t + 1]).
__global__ void __launch_bounds__(256) cs_bounds(CmLists v, const uint32_t* __restrict__ mread, uint32_t M, uint32_t T1,
                                                 uint64_t tile_k, uint32_t* __restrict__ bnd) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (uint64_t)M * T1) return;
    const uint32_t m = (uint32_t)(j / T1), t = (uint32_t)(j % T1);
    uint32_t n;
    const uint32_t* l = cm_list(v, mread[m], n);
    const uint64_t want = (uint64_t)t * tile_k;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((uint64_t)l[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    bnd[j] = lo;
}

// Work item w: entries [wstart[w], wstart[w] + CS_E) of tile t's share of member wmem[w]'s list, each
// ORed as a bit into the member's set row (roww words wide, bit 0 = KmerID k0).  The work items cover a
// member's whole list; those past the tile's share do nothing.
__global__ void __launch_bounds__(256) cs_mark(CmLists v, const uint32_t* __restrict__ mread,
                                               const uint32_t* __restrict__ mset, const uint32_t* __restrict__ wmem,
                                               const uint32_t* __restrict__ wstart, uint32_t W,
                                               const uint32_t* __restrict__ bnd, uint32_t T1, uint32_t t, uint32_t k0,
                                               uint64_t roww, uint32_t* __restrict__ rows) {
    for (uint32_t w = blockIdx.x; w < W; w += gridDim.x) {
        const uint32_t m = wmem[w];
        const uint64_t lo = bnd[(uint64_t)m * T1 + t], hi = bnd[(uint64_t)m * T1 + t + 1];
        uint32_t n;
        const uint32_t* l = cm_list(v, mread[m], n);
        uint32_t* __restrict__ row = rows + (uint64_t)mset[m] * roww;
        const uint64_t s = lo + wstart[w];
#pragma unroll
        for (uint32_t j = 0; j < (uint32_t)CS_E; j += 256u) {
            const uint64_t e = s + j + threadIdx.x;
            if (e < hi) {
                const uint32_t d = l[e] - k0;
                atomicOr(&row[d >> 5], 1u << (d & 31u));
            }
        }
    }
}

// One workgroup per pair: popcount(row a & row b), rows of row4 16-byte words.
__global__ void __launch_bounds__(256) cs_pairs(const uint4* __restrict__ rows, uint64_t row4,
                                                const uint32_t* __restrict__ pa, const uint32_t* __restrict__ pb,
                                                uint32_t n, unsigned long long* __restrict__ out) {
    __shared__ uint32_t ws[4];
    const uint32_t t = threadIdx.x, lane = t & 63u;
    for (uint32_t p = blockIdx.x; p < n; p += gridDim.x) {
        const uint4* __restrict__ A = rows + (uint64_t)pa[p] * row4;
        const uint4* __restrict__ B = rows + (uint64_t)pb[p] * row4;
        uint32_t c = 0;   // a row holds fewer than 2^32 bits
        for (uint64_t i = t; i < row4; i += 256u) {
            const uint4 a = A[i], b = B[i];
            c += (uint32_t)(__popc(a.x & b.x) + __popc(a.y & b.y) + __popc(a.z & b.z) + __popc(a.w & b.w));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) ws[t >> 6] = c;
        __syncthreads();
        if (t == 0) out[p] = (unsigned long long)ws[0] + ws[1] + ws[2] + ws[3];
        __syncthreads();   // ws is reused by the next pair
    }
}

// grows b to new_bytes keeping its first keep_bytes
void grow_keep(hga_ctx* c, DevBuf& b, size_t keep_bytes, size_t new_bytes) {
    if (new_bytes <= b.cap && b.p) return;
    void* np = nullptr;
    HGA_HIP(hipMalloc(&np, new_bytes));
    if (keep_bytes && b.p) {
        hipError_t e = hipMemcpyAsync(np, b.p, keep_bytes, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {
            (void)hipFree(np);
            HGA_HIP(e);
        }
    }
    b.release();
    b.p = np;
    b.cap = new_bytes;
}

// Creates the view from the current lookup result.
void ensure_view(hga_ctx* c) {
    auto& L = c->lookup;
    auto& V = c->comp;
    HGA_REQUIRE(L.ran, HGA_ERR_STATE, "hga_lookup_run not called");
    if (V.live) return;
    const uint64_t nr = L.n_reads, H = L.hits, K = L.n_sdk;
    HGA_REQUIRE(nr < 0xFFFFFFFFull && H < (1ull << 32), HGA_ERR_INVALID, "lookup result too large for the component view");
    uint32_t* idx = static_cast<uint32_t*>(V.idx.ensure(std::max<uint64_t>(H, 1) * 4));
    uint32_t* len = static_cast<uint32_t*>(V.len.ensure(std::max<uint64_t>(K, 1) * 4));
    uint64_t* oo = static_cast<uint64_t*>(V.ovr_off.ensure(std::max<uint64_t>(nr, 1) * 8));
    uint32_t* ol = static_cast<uint32_t*>(V.ovr_len.ensure(std::max<uint64_t>(nr, 1) * 4));
    V.pool.ensure(16);
    V.pool_cap = V.pool.cap / 4;
    V.pool_used = 0;
    if (H) HGA_HIP(hipMemcpyAsync(idx, L.kci_val.p, H * 4, hipMemcpyDeviceToDevice, c->stream));
    if (nr) {
        HGA_HIP(hipMemsetAsync(oo, 0xFF, nr * 8, c->stream));
        HGA_HIP(hipMemsetAsync(ol, 0, nr * 4, c->stream));
    }
    if (K) {
        c->launch("cm_len_init", [&] {
            hipLaunchKernelGGL(cm_len_init, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, c->stream,
                               L.kci_ptr.as<uint64_t>(), (uint32_t)K, len);
        });
        c->check_launch("cm_len_init");
    }
    V.h_hit_ptr.assign(nr + 1, 0);
    if (H) HGA_HIP(hipMemcpyAsync(V.h_hit_ptr.data(), L.hit_ptr.p, (nr + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    V.ovr.clear();
    V.index_entries = H;
    V.survivor_kmers = 0;
    V.merges = 0;
    V.live = true;
}

inline uint32_t cur_len(const ComponentState& V, uint32_t r) {
    auto it = V.ovr.find(r);
    return it != V.ovr.end() ? it->second.second : (uint32_t)(V.h_hit_ptr[r + 1] - V.h_hit_ptr[r]);
}

inline CmLists lists_of(hga_ctx* c) {
    auto& L = c->lookup;
    auto& V = c->comp;
    return CmLists{L.hit_ptr.as<uint64_t>(), L.s_val2.as<uint32_t>(), V.ovr_off.as<uint64_t>(), V.ovr_len.as<uint32_t>(),
                   V.pool.as<uint32_t>()};
}

}  // namespace

void components_drop(hga_ctx* c) { c->comp.live = false; }

void components_merge(hga_ctx* c, const uint64_t* group_ptr, const uint32_t* ids, uint64_t n_groups) {
    auto& L = c->lookup;
    auto& V = c->comp;
    HGA_REQUIRE(L.ran, HGA_ERR_STATE, "hga_lookup_run not called");
    if (n_groups == 0) return;
    HGA_REQUIRE(group_ptr, HGA_ERR_INVALID, "null group_ptr with n_groups > 0");
    const uint64_t first = L.first_read_id, nr = L.n_reads;
    const uint64_t n_ids = group_ptr[n_groups] - group_ptr[0];
    HGA_REQUIRE(ids || n_ids == 0, HGA_ERR_INVALID, "null ids");
    for (uint64_t g = 0; g < n_groups; ++g)
        HGA_REQUIRE(group_ptr[g + 1] >= group_ptr[g], HGA_ERR_INVALID, "group_ptr must be non-decreasing");
    ensure_view(c);
    // everything is checked before anything is launched or changed
    {
        std::vector<uint32_t> all;
        all.reserve(n_ids);
        for (uint64_t g = 0; g < n_groups; ++g) {
            const uint64_t a = group_ptr[g], b = group_ptr[g + 1];
            for (uint64_t i = a; i < b; ++i) {
                HGA_REQUIRE(ids[i] >= first && ids[i] - first < nr, HGA_ERR_INVALID, "id outside the lookup's reads");
                const uint32_t r = (uint32_t)(ids[i] - first);
                HGA_REQUIRE(b - a < 2 || cur_len(V, r) > 0, HGA_ERR_INVALID, "id without hits in a group of two or more");
                all.push_back(r);
            }
        }
        std::sort(all.begin(), all.end());
        HGA_REQUIRE(std::adjacent_find(all.begin(), all.end()) == all.end(), HGA_ERR_INVALID,
                    "id listed twice in one merge call");
    }
    // the members of the groups of two or more, their list offsets (moff) and removal offsets (roff)
    std::vector<uint32_t> mread, mgrp, surv;
    std::vector<uint64_t> moff, roff;
    uint64_t T = 0, Tr = 0;
    for (uint64_t g = 0; g < n_groups; ++g) {
        const uint64_t a = group_ptr[g], b = group_ptr[g + 1];
        if (b - a < 2) continue;
        const uint32_t gi = (uint32_t)surv.size();
        surv.push_back((uint32_t)(ids[a] - first));
        for (uint64_t i = a; i < b; ++i) {
            const uint32_t r = (uint32_t)(ids[i] - first);
            const uint32_t ln = cur_len(V, r);
            mread.push_back(r);
            mgrp.push_back(gi);
            moff.push_back(T);
            T += ln;
            if (i == a) {
                roff.push_back(~0ull);
            } else {
                roff.push_back(Tr);
                Tr += ln;
            }
        }
    }
    const uint64_t G = surv.size(), M = mread.size();
    if (G == 0) return;
    moff.push_back(T);
    HGA_REQUIRE(T + Tr < (1ull << 32) && M < (1ull << 32), HGA_ERR_OOM, "too many removal pairs for one merge call");
    const uint64_t K = L.n_sdk;
    // uploads: mread | mgrp | surv (u32), then moff | roff | gstart (u64)
    const size_t u32n = 2 * M + G, off64 = (u32n * 4 + 7) & ~7ull;
    char* mem = static_cast<char*>(V.mem.ensure(off64 + (2 * M + 1 + G + 1) * 8));
    uint32_t* d_mread = reinterpret_cast<uint32_t*>(mem);
    uint32_t* d_mgrp = d_mread + M;
    uint32_t* d_surv = d_mgrp + M;
    uint64_t* d_moff = reinterpret_cast<uint64_t*>(mem + off64);
    uint64_t* d_roff = d_moff + M + 1;
    uint64_t* d_gstart = d_roff + M;
    HGA_HIP(hipMemcpyAsync(d_mread, mread.data(), M * 4, hipMemcpyHostToDevice, c->stream));
    HGA_HIP(hipMemcpyAsync(d_mgrp, mgrp.data(), M * 4, hipMemcpyHostToDevice, c->stream));
    HGA_HIP(hipMemcpyAsync(d_surv, surv.data(), G * 4, hipMemcpyHostToDevice, c->stream));
    HGA_HIP(hipMemcpyAsync(d_moff, moff.data(), (M + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HGA_HIP(hipMemcpyAsync(d_roff, roff.data(), M * 8, hipMemcpyHostToDevice, c->stream));
    uint64_t* gk = static_cast<uint64_t*>(V.gk.ensure(T * 8));
    uint64_t* rm = static_cast<uint64_t*>(V.rm.ensure((Tr + T) * 8));   // the unions hold at most T KmerIDs
    uint64_t* flag = static_cast<uint64_t*>(V.flag.ensure(T * 8));
    uint32_t* ubuf = static_cast<uint32_t*>(V.ubuf.ensure(T * 4));
    uint32_t* seg = static_cast<uint32_t*>(V.seg.ensure(std::max<uint64_t>(K, 1) * 8));
    auto* ctr = static_cast<unsigned long long*>(V.ctr.ensure(64));
    const uint64_t gcap = (uint64_t)c->num_cu * 16;
    const CmLists lists = lists_of(c);
    c->launch("cm_expand", [&] {
        hipLaunchKernelGGL(cm_expand, dim3(cm_blocks(T, 256, gcap)), dim3(256), 0, c->stream, lists, d_mread, d_mgrp,
                           d_moff, d_roff, (uint32_t)M, T, gk, rm);
    });
    c->check_launch("cm_expand");
    radix_sort_u64(c, gk, nullptr, T, 32 + cm_bits(G), V.scratch);
    c->launch("cm_union", [&] {
        hipLaunchKernelGGL(cm_uniq_flag, dim3(cm_blocks(T, 256, gcap)), dim3(256), 0, c->stream, gk, T, flag);
    });
    c->check_launch("cm_uniq_flag");
    exclusive_scan_u64(c, flag, T, V.scratch);
    c->launch("cm_union", [&] {
        hipLaunchKernelGGL(cm_uniq_put, dim3(cm_blocks(T, 256, gcap)), dim3(256), 0, c->stream, gk, flag, T, d_surv,
                           (uint32_t)G, ubuf, rm + Tr, d_gstart);
    });
    c->check_launch("cm_uniq_put");
    std::vector<uint64_t> gstart(G + 1);
    HGA_HIP(hipMemcpyAsync(gstart.data(), d_gstart, (G + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    const uint64_t U = gstart[G], R = Tr + U;
    HGA_REQUIRE(U >= G && U <= T, HGA_ERR_HIP, "component merge: inconsistent union sizes");
    // the pool is grown before the state changes: a failed allocation leaves the view as it was
    if (V.pool_used + U > V.pool_cap) {
        const uint64_t want = std::max<uint64_t>(V.pool_used + U, V.pool_cap * 2);
        grow_keep(c, V.pool, V.pool_used * 4, want * 4);
        V.pool_cap = want;
    }
    HGA_HIP(hipMemcpyAsync(V.pool.as<uint32_t>() + V.pool_used, ubuf, U * 4, hipMemcpyDeviceToDevice, c->stream));
    radix_sort_u64(c, rm, nullptr, R, 32 + cm_bits(std::max<uint64_t>(K, 1)), V.scratch);
    HGA_HIP(hipMemsetAsync(seg, 0, std::max<uint64_t>(K, 1) * 8, c->stream));
    HGA_HIP(hipMemsetAsync(ctr, 0, 64, c->stream));
    c->launch("cm_seg", [&] {
        hipLaunchKernelGGL(cm_seg, dim3(cm_blocks(R, 256, gcap)), dim3(256), 0, c->stream, rm, R, seg);
    });
    c->check_launch("cm_seg");
    c->launch("cm_edit", [&] {
        hipLaunchKernelGGL(cm_edit, dim3(cm_blocks(K, 4, gcap)), dim3(256), 0, c->stream, L.kci_ptr.as<uint64_t>(),
                           V.idx.as<uint32_t>(), V.len.as<uint32_t>(), rm, seg, (uint32_t)K, ctr + 3);
    });
    c->check_launch("cm_edit");
    hipLaunchKernelGGL(cm_set_ovr, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, c->stream, d_surv, d_gstart,
                       (uint32_t)G, V.pool_used, V.ovr_off.as<uint64_t>(), V.ovr_len.as<uint32_t>());
    c->check_launch("cm_set_ovr");
    unsigned long long removed = 0;
    HGA_HIP(hipMemcpyAsync(&removed, ctr + 3, 8, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    for (uint64_t g = 0; g < G; ++g) {
        const uint32_t ln = (uint32_t)(gstart[g + 1] - gstart[g]);
        auto it = V.ovr.find(surv[g]);
        if (it != V.ovr.end()) V.survivor_kmers -= it->second.second;
        V.ovr[surv[g]] = {V.pool_used + gstart[g], ln};
        V.survivor_kmers += ln;
    }
    V.pool_used += U;
    V.index_entries -= removed;
    V.merges += G;
}

void components_connections(hga_ctx* c, const uint32_t* pivots, uint64_t n_piv, uint64_t min_score, uint64_t* n_out) {
    auto& L = c->lookup;
    auto& V = c->comp;
    auto& S = c->conn;
    HGA_REQUIRE(L.ran, HGA_ERR_STATE, "hga_lookup_run not called");
    const uint64_t first = L.first_read_id, nr = L.n_reads;
    for (uint64_t i = 0; i < n_piv; ++i)
        HGA_REQUIRE(pivots[i] >= first && pivots[i] - first < nr, HGA_ERR_INVALID, "pivot ReadID outside the lookup's reads");
    S.n = 0;
    S.ready = false;
    *n_out = 0;
    if (min_score > 0xFFFFFFFFull || nr == 0 || L.hits == 0 || n_piv == 0) {
        S.ready = true;
        return;
    }
    ensure_view(c);
    const uint32_t ms = std::max<uint32_t>((uint32_t)min_score, 1u);   // a candidate shares at least one entry
    const uint64_t bmax = std::max<uint64_t>(1, CC_ROW_BYTES / 4 / nr);
    const uint64_t B = std::min<uint64_t>(bmax, n_piv);
    HGA_REQUIRE(B * nr < (1ull << 32), HGA_ERR_OOM, "too many reads for one score row");
    uint32_t* rows = static_cast<uint32_t*>(V.rows.ensure(B * nr * 4));
    auto* ctr = static_cast<unsigned long long*>(V.ctr.ensure(64));
    const CmLists lists = lists_of(c);
    uint64_t n = 0, cap = 0;
    uint32_t mxs = 0;
    std::vector<uint32_t> piv, wslot, wstart;
    for (uint64_t p0 = 0; p0 < n_piv; p0 += B) {
        const uint64_t nb = std::min<uint64_t>(B, n_piv - p0);
        piv.clear();
        wslot.clear();
        wstart.clear();
        for (uint64_t i = 0; i < nb; ++i) {
            const uint32_t r = (uint32_t)(pivots[p0 + i] - first);
            piv.push_back(r);
            const uint32_t ln = cur_len(V, r);
            for (uint32_t at = 0; at < ln; at += CC_T) {
                wslot.push_back((uint32_t)i);
                wstart.push_back(at);
                if (ln - at <= (uint32_t)CC_T) break;   // no wrap for lists near 2^32
            }
        }
        const uint64_t W = wslot.size();
        if (W == 0) continue;
        uint32_t* d_piv = static_cast<uint32_t*>(V.work.ensure((nb + 2 * W) * 4));
        uint32_t* d_wslot = d_piv + nb;
        uint32_t* d_wstart = d_wslot + W;
        HGA_HIP(hipMemcpyAsync(d_piv, piv.data(), nb * 4, hipMemcpyHostToDevice, c->stream));
        HGA_HIP(hipMemcpyAsync(d_wslot, wslot.data(), W * 4, hipMemcpyHostToDevice, c->stream));
        HGA_HIP(hipMemcpyAsync(d_wstart, wstart.data(), W * 4, hipMemcpyHostToDevice, c->stream));
        const uint64_t cells = nb * nr;
        HGA_HIP(hipMemsetAsync(rows, 0, cells * 4, c->stream));
        HGA_HIP(hipMemsetAsync(ctr, 0, 24, c->stream));
        c->launch("cc_accum", [&] {
            hipLaunchKernelGGL(cc_accum, dim3(cm_blocks(W, 1, (uint64_t)c->num_cu * 8)), dim3(CC_T), 0, c->stream, lists,
                               L.kci_ptr.as<uint64_t>(), V.idx.as<uint32_t>(), V.len.as<uint32_t>(), d_wslot, d_wstart,
                               (uint32_t)W, d_piv, nr, rows);
        });
        c->check_launch("cc_accum");
        const unsigned pg = cm_blocks(cells, 256, (uint64_t)c->num_cu * 16);
        c->launch("cc_pairs", [&] {
            hipLaunchKernelGGL(cc_pairs<false>, dim3(pg), dim3(256), 0, c->stream, rows, d_piv, nr, cells, ms, 0ull, ctr,
                               (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr);
        });
        c->check_launch("cc_pairs");
        unsigned long long h[2] = {0, 0};
        HGA_HIP(hipMemcpyAsync(h, ctr, 16, hipMemcpyDeviceToHost, c->stream));
        c->sync();   // also: the staged pivots and work items are reused by the next batch
        if (h[0] == 0) continue;
        HGA_REQUIRE(n + h[0] < (1ull << 32), HGA_ERR_OOM, "too many connections for one sort");
        if (n + h[0] > cap) {
            const uint64_t want = std::max<uint64_t>(n + h[0], cap * 2);
            grow_keep(c, S.x, n * 4, want * 4);
            grow_keep(c, S.y, n * 4, want * 4);
            grow_keep(c, S.s, n * 4, want * 4);
            cap = std::min<uint64_t>({S.x.cap, S.y.cap, S.s.cap}) / 4;
        }
        c->launch("cc_pairs", [&] {
            hipLaunchKernelGGL(cc_pairs<true>, dim3(pg), dim3(256), 0, c->stream, rows, d_piv, nr, cells, ms, n, ctr,
                               S.x.as<uint32_t>(), S.y.as<uint32_t>(), S.s.as<uint32_t>());
        });
        c->check_launch("cc_pairs");
        c->sync();
        n += h[0];
        mxs = std::max<uint32_t>(mxs, (uint32_t)h[1]);
    }
    connections_order(c, n, mxs, ms);
    *n_out = n;
}

void components_overlaps(hga_ctx* c, const uint32_t* x, const uint32_t* y, uint64_t n, int32_t* overlap,
                         uint32_t* shared) {
    auto& L = c->lookup;
    auto& S = c->overlap;
    HGA_REQUIRE(L.ran, HGA_ERR_STATE, "hga_lookup_run not called");
    if (n == 0) return;
    HGA_REQUIRE(x && y, HGA_ERR_INVALID, "null id list with n > 0");
    const uint64_t first = L.first_read_id, nr = L.n_reads;
    for (uint64_t i = 0; i < n; ++i)   // before anything is launched
        HGA_REQUIRE(x[i] >= first && x[i] - first < nr && y[i] >= first && y[i] - first < nr, HGA_ERR_INVALID,
                    "id outside the lookup's reads");
    ensure_view(c);
    if (L.hits == 0) {   // no read has a hit: every list is empty
        if (overlap) std::memset(overlap, 0, n * sizeof(int32_t));
        if (shared) std::memset(shared, 0, n * sizeof(uint32_t));
        return;
    }
    const uint64_t cap = std::min(n, CO_CHUNK);
    uint32_t* dx = static_cast<uint32_t*>(S.x.ensure(cap * 4));
    uint32_t* dy = static_cast<uint32_t*>(S.y.ensure(cap * 4));
    int32_t* dov = static_cast<int32_t*>(S.ov.ensure(cap * 4));
    uint32_t* dsh = static_cast<uint32_t*>(S.sh.ensure(cap * 4));
    const CmLists lists = lists_of(c);
    for (uint64_t at = 0; at < n; at += CO_CHUNK) {
        const uint64_t m = std::min(CO_CHUNK, n - at);
        HGA_HIP(hipMemcpyAsync(dx, x + at, m * 4, hipMemcpyHostToDevice, c->stream));
        HGA_HIP(hipMemcpyAsync(dy, y + at, m * 4, hipMemcpyHostToDevice, c->stream));
        const unsigned grid = (unsigned)std::min<uint64_t>((m + 3) / 4, (uint64_t)c->num_cu * 8);
        c->launch("co_wave", [&] {
            hipLaunchKernelGGL(co_wave, dim3(grid), dim3(256), 0, c->stream, lists, L.first_ptr.as<uint64_t>(),
                               L.first_kid.as<uint32_t>(), L.first_pos.as<uint32_t>(), dx, dy, (uint32_t)m,
                               L.first_read_id, dov, dsh);
        });
        c->check_launch("co_wave");
        if (overlap) HGA_HIP(hipMemcpyAsync(overlap + at, dov, m * 4, hipMemcpyDeviceToHost, c->stream));
        if (shared) HGA_HIP(hipMemcpyAsync(shared + at, dsh, m * 4, hipMemcpyDeviceToHost, c->stream));
        c->sync();   // the scratch is reused by the next chunk
    }
}

// The ids were validated by the caller; nothing is copied back and the stream is not synchronised.
void components_overlaps_device(hga_ctx* c, const uint32_t* dx, const uint32_t* dy, uint64_t n, int32_t* dov) {
    auto& L = c->lookup;
    auto& S = c->overlap;
    HGA_REQUIRE(L.ran, HGA_ERR_STATE, "hga_lookup_run not called");
    if (n == 0) return;
    ensure_view(c);
    if (L.hits == 0) {   // no read has a hit: every list is empty
        HGA_HIP(hipMemsetAsync(dov, 0, n * 4, c->stream));
        return;
    }
    uint32_t* dsh = static_cast<uint32_t*>(S.sh.ensure(std::min(n, CO_CHUNK) * 4));
    const CmLists lists = lists_of(c);
    for (uint64_t at = 0; at < n; at += CO_CHUNK) {
        const uint64_t m = std::min(CO_CHUNK, n - at);
        const unsigned grid = (unsigned)std::min<uint64_t>((m + 3) / 4, (uint64_t)c->num_cu * 8);
        c->launch("co_wave", [&] {
            hipLaunchKernelGGL(co_wave, dim3(grid), dim3(256), 0, c->stream, lists, L.first_ptr.as<uint64_t>(),
                               L.first_kid.as<uint32_t>(), L.first_pos.as<uint32_t>(), dx + at, dy + at, (uint32_t)m,
                               L.first_read_id, dov + at, dsh);
        });
        c->check_launch("co_wave");
    }
}

// One bitmap row per set, a bit per KmerID.  When n_sets rows of all K bits exceed the byte budget the
// call runs over KmerID tiles of tile_k ids: each tile marks its share of every member list, the pair
// kernel counts it, and the host adds the tiles' counts up.  A row is never narrower than one 16-byte
// word, so more than budget / 16 sets exceed the budget by that much.
void components_set_scores(hga_ctx* c, const uint64_t* set_ptr, const uint32_t* ids, uint64_t n_sets,
                           const uint32_t* pair_a, const uint32_t* pair_b, uint64_t n_pairs, uint64_t* score,
                           uint64_t* set_size) {
    auto& L = c->lookup;
    auto& V = c->comp;
    HGA_REQUIRE(L.ran, HGA_ERR_STATE, "hga_lookup_run not called");
    if (n_sets == 0) {
        HGA_REQUIRE(n_pairs == 0, HGA_ERR_INVALID, "pair index outside the sets");
        return;
    }
    HGA_REQUIRE(set_ptr, HGA_ERR_INVALID, "null set_ptr with n_sets > 0");
    HGA_REQUIRE(n_pairs == 0 || (pair_a && pair_b && score), HGA_ERR_INVALID, "null pair list or score with n_pairs > 0");
    HGA_REQUIRE(n_sets < 0xFFFFFFFFull, HGA_ERR_INVALID, "too many sets");
    for (uint64_t s = 0; s < n_sets; ++s)
        HGA_REQUIRE(set_ptr[s + 1] >= set_ptr[s], HGA_ERR_INVALID, "set_ptr must be non-decreasing");
    HGA_REQUIRE(ids || set_ptr[n_sets] == set_ptr[0], HGA_ERR_INVALID, "null ids");
    const uint64_t first = L.first_read_id, nr = L.n_reads;
    for (uint64_t i = set_ptr[0]; i < set_ptr[n_sets]; ++i)
        HGA_REQUIRE(ids[i] >= first && ids[i] - first < nr, HGA_ERR_INVALID, "id outside the lookup's reads");
    for (uint64_t p = 0; p < n_pairs; ++p)
        HGA_REQUIRE(pair_a[p] < n_sets && pair_b[p] < n_sets, HGA_ERR_INVALID, "pair index outside the sets");
    ensure_view(c);
    // the pairs asked for, then (s, s) per set for the sizes
    const uint64_t P = n_pairs + (set_size ? n_sets : 0);
    if (n_pairs) std::memset(score, 0, n_pairs * 8);
    if (set_size) std::memset(set_size, 0, n_sets * 8);
    const uint64_t K = L.n_sdk;
    if (P == 0 || K == 0 || L.hits == 0) return;
    // members with a non-empty current list, and their lists cut into work items of CS_E entries
    std::vector<uint32_t> mread, mset, wmem, wstart;
    for (uint64_t s = 0; s < n_sets; ++s)
        for (uint64_t i = set_ptr[s]; i < set_ptr[s + 1]; ++i) {
            const uint32_t r = (uint32_t)(ids[i] - first);
            const uint32_t ln = cur_len(V, r);
            if (!ln) continue;
            HGA_REQUIRE(mread.size() < 0xFFFFFFFFull, HGA_ERR_OOM, "too many set members");
            const uint32_t m = (uint32_t)mread.size();
            mread.push_back(r);
            mset.push_back((uint32_t)s);
            for (uint32_t at = 0; at < ln; at += CS_E) {
                wmem.push_back(m);
                wstart.push_back(at);
                if (ln - at <= (uint32_t)CS_E) break;   // no wrap for lists near 2^32
            }
        }
    const uint64_t M = mread.size(), W = wmem.size();
    HGA_REQUIRE(W < (1ull << 32), HGA_ERR_OOM, "too many list entries for one set-score call");
    uint64_t budget = CS_ROW_BYTES;
    if (const char* e = std::getenv("HGA_SETS_BYTES")) {
        char* end = nullptr;
        const unsigned long long b = std::strtoull(e, &end, 10);
        if (end != e && b > 0) budget = b;
    }
    const uint64_t full4 = (K + 127) / 128;   // 16-byte words of a row that holds every KmerID
    const uint64_t row4 = std::min(full4, std::max<uint64_t>(1, budget / 16 / n_sets));
    const uint64_t tile_k = row4 * 128, roww = row4 * 4;
    const uint64_t T = (K + tile_k - 1) / tile_k;
    HGA_REQUIRE(M * (T + 1) < (1ull << 32), HGA_ERR_OOM, "too many KmerID tiles for one set-score call");
    uint32_t* rows = static_cast<uint32_t*>(V.rows.ensure(n_sets * row4 * 16));
    const uint64_t pcap = std::min(P, CS_CHUNK);
    // uploads: mread | mset | wmem | wstart | bnd (u32), then the pairs and scores of one chunk
    uint32_t* d_mread = static_cast<uint32_t*>(V.work.ensure(std::max<uint64_t>(1, 2 * M + 2 * W + M * (T + 1)) * 4));
    uint32_t* d_mset = d_mread + M;
    uint32_t* d_wmem = d_mset + M;
    uint32_t* d_wstart = d_wmem + W;
    uint32_t* d_bnd = d_wstart + W;
    char* mem = static_cast<char*>(V.mem.ensure(pcap * 16));
    auto* d_out = reinterpret_cast<unsigned long long*>(mem);
    uint32_t* d_pa = reinterpret_cast<uint32_t*>(mem + pcap * 8);
    uint32_t* d_pb = d_pa + pcap;
    const CmLists lists = lists_of(c);
    if (M) {
        HGA_HIP(hipMemcpyAsync(d_mread, mread.data(), M * 4, hipMemcpyHostToDevice, c->stream));
        HGA_HIP(hipMemcpyAsync(d_mset, mset.data(), M * 4, hipMemcpyHostToDevice, c->stream));
        HGA_HIP(hipMemcpyAsync(d_wmem, wmem.data(), W * 4, hipMemcpyHostToDevice, c->stream));
        HGA_HIP(hipMemcpyAsync(d_wstart, wstart.data(), W * 4, hipMemcpyHostToDevice, c->stream));
        c->launch("cs_bounds", [&] {
            hipLaunchKernelGGL(cs_bounds, dim3((unsigned)((M * (T + 1) + 255) / 256)), dim3(256), 0, c->stream, lists,
                               d_mread, (uint32_t)M, (uint32_t)(T + 1), tile_k, d_bnd);
        });
        c->check_launch("cs_bounds");
    }
    std::vector<uint32_t> ha(pcap), hb(pcap);
    std::vector<unsigned long long> got(pcap);
    for (uint64_t t = 0; t < T; ++t) {
        HGA_HIP(hipMemsetAsync(rows, 0, n_sets * row4 * 16, c->stream));
        if (M) {
            c->launch("cs_mark", [&] {
                hipLaunchKernelGGL(cs_mark, dim3(cm_blocks(W, 1, (uint64_t)c->num_cu * 8)), dim3(256), 0, c->stream, lists,
                                   d_mread, d_mset, d_wmem, d_wstart, (uint32_t)W, d_bnd, (uint32_t)(T + 1), (uint32_t)t,
                                   (uint32_t)(t * tile_k), roww, rows);
            });
            c->check_launch("cs_mark");
        }
        for (uint64_t at = 0; at < P; at += CS_CHUNK) {
            const uint64_t m = std::min(CS_CHUNK, P - at);
            for (uint64_t i = 0; i < m; ++i) {
                const uint64_t p = at + i;
                ha[i] = p < n_pairs ? pair_a[p] : (uint32_t)(p - n_pairs);
                hb[i] = p < n_pairs ? pair_b[p] : (uint32_t)(p - n_pairs);
            }
            HGA_HIP(hipMemcpyAsync(d_pa, ha.data(), m * 4, hipMemcpyHostToDevice, c->stream));
            HGA_HIP(hipMemcpyAsync(d_pb, hb.data(), m * 4, hipMemcpyHostToDevice, c->stream));
            c->launch("cs_pairs", [&] {
                hipLaunchKernelGGL(cs_pairs, dim3(cm_blocks(m, 1, (uint64_t)c->num_cu * 8)), dim3(256), 0, c->stream,
                                   reinterpret_cast<const uint4*>(rows), row4, d_pa, d_pb, (uint32_t)m, d_out);
            });
            c->check_launch("cs_pairs");
            HGA_HIP(hipMemcpyAsync(got.data(), d_out, m * 8, hipMemcpyDeviceToHost, c->stream));
            c->sync();   // the staged pairs are reused by the next chunk
            for (uint64_t i = 0; i < m; ++i) {
                const uint64_t p = at + i;
                if (p < n_pairs) score[p] += got[i];
                else set_size[p - n_pairs] += got[i];
            }
        }
    }
}

void components_sizes(hga_ctx* c, hga_components_sizes* out) {
    ensure_view(c);
    auto& V = c->comp;
    out->index_entries = V.index_entries;
    out->survivors = V.ovr.size();
    out->survivor_kmers = V.survivor_kmers;
    out->merges = V.merges;
}

void components_fetch_index(hga_ctx* c, uint64_t* ptr, uint32_t* ids) {
    ensure_view(c);
    auto& L = c->lookup;
    auto& V = c->comp;
    const uint64_t K = L.n_sdk, H = L.hits;
    if (!ptr && !ids) return;
    std::vector<uint32_t> len(K);
    std::vector<uint64_t> kp(K + 1, 0);
    if (K) HGA_HIP(hipMemcpyAsync(len.data(), V.len.p, K * 4, hipMemcpyDeviceToHost, c->stream));
    if (K && ids) HGA_HIP(hipMemcpyAsync(kp.data(), L.kci_ptr.p, (K + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    std::vector<uint32_t> all;
    if (ids && H) {   // the lists keep the lookup's offsets: packed on the host
        all.resize(H);
        HGA_HIP(hipMemcpyAsync(all.data(), V.idx.p, H * 4, hipMemcpyDeviceToHost, c->stream));
    }
    c->sync();
    uint64_t at = 0;
    for (uint64_t k = 0; k < K; ++k) {
        if (ptr) ptr[k] = at;
        if (ids)
            for (uint32_t i = 0; i < len[k]; ++i) ids[at + i] = all[kp[k] + i] + L.first_read_id;
        at += len[k];
    }
    if (ptr) ptr[K] = at;
}

void components_fetch_kmers(hga_ctx* c, uint32_t id, uint32_t* kmers, uint64_t* n) {
    ensure_view(c);
    auto& L = c->lookup;
    auto& V = c->comp;
    HGA_REQUIRE(id >= L.first_read_id && (uint64_t)(id - L.first_read_id) < L.n_reads, HGA_ERR_INVALID,
                "id outside the lookup's reads");
    const uint32_t r = id - L.first_read_id;
    const uint32_t ln = cur_len(V, r);
    *n = ln;
    if (!kmers || !ln) return;
    auto it = V.ovr.find(r);
    const uint32_t* src = it != V.ovr.end() ? V.pool.as<uint32_t>() + it->second.first
                                            : L.s_val2.as<uint32_t>() + V.h_hit_ptr[r];
    HGA_HIP(hipMemcpyAsync(kmers, src, (size_t)ln * 4, hipMemcpyDeviceToHost, c->stream));
    c->sync();
}

}  // namespace hga
