// count_sizing.hpp — every size-derived choice of count_run (count.hip) and the device bytes it
// requests, as host arithmetic only (no HIP): hga_count_estimate and count_run call the same
// function, and tests/native/count_sizing_check.cpp runs it stand-alone under the host sanitizers.
//
// One pass (P = 1) is the pipeline of DESIGN §4 on the whole input.  With P = 2^pb passes the top
// pb bits of the mixed key select the pass; every pass counts a disjoint key range of about
// total / P instances with region / bucket / remainder taken from the 2k - pb bits below, so all
// per-instance buffers are sized by the pass's share times a margin.
#pragma once
#include <algorithm>
#include <cstdint>

#ifndef HGA_MAX_FB
#define HGA_MAX_FB 12
#endif
#ifndef HGA_MAX_FB1
#define HGA_MAX_FB1 6
#endif
#ifndef HGA_PB_P
#define HGA_PB_P 65536
#endif
#ifndef HGA_B1_PER_CU
#define HGA_B1_PER_CU 2   // bin1 super-tiles per CU
#endif

namespace hga {
namespace sizing {

constexpr uint32_t kMaxFb = HGA_MAX_FB, kMaxFb1 = HGA_MAX_FB1;
constexpr uint64_t kBlk = 8192;         // level-1 block = one kc_bin1 tile (count.hip BLK)
constexpr uint32_t kMaxSf3 = 4096;      // kc_split3: (sub-bucket, file) pairs
constexpr uint32_t kSlack3 = 64;        // kc_split3: extra slots per sub-bucket slab
constexpr uint32_t kMaxPasses = 256;
constexpr uint64_t kBinFileBytes = 24, kBlkEntryBytes = 16;   // sizeof(BinFile), sizeof(Blk)
constexpr uint32_t kMargin16 = 20;      // a pass's buffers hold 1.25x its expected share (in 1/16)
constexpr uint64_t kMarginSlack = 65536;   // + this many instances (small inputs spread unevenly)

// The test / tuning hooks count_run reads from the environment (HGA_FB_MAX, HGA_FB_MIN,
// HGA_COUNT_LEGACY, HGA_B1_SOLE, HGA_ROW_CAP, HGA_SPLIT3_TARGET, HGA_SPLIT3_FORCE).
struct Hooks {
    uint32_t fb_max = kMaxFb, fb_min = 0;
    bool legacy = false, sole = true;
    uint64_t row_cap = 0;   // 0: none
    uint64_t split3_target = 32768;
    int split3_force = -1;  // < 0: none
};

struct Plan {
    uint32_t P = 1, pb = 0;      // passes (clamped), log2
    uint32_t nbits = 0;          // key bits below the pass bits: 2k - pb
    uint64_t total_bytes = 0;    // resident bases (>= instances)
    uint64_t pass_bytes = 0;     // expected instances of one pass: total_bytes / P
    uint32_t margin16 = 16;      // P > 1: the share a pass's buffers hold, in 1/16 of pass_bytes
    bool packed = false, e1_32 = false, e32 = false;
    uint64_t per_bucket = 0;
    uint32_t fb = 0, fb1 = 0, fb2 = 0, fb3 = 0;
    uint32_t rbits = 0, r1bits = 0;   // before the third split level
    uint64_t st_pos = 0;         // bases per kc_bin1 super-tile
    uint32_t W = 0;              // super-tiles = kc_bin1 workgroups
    uint64_t n_first = 0, table_cap = 0, pool_cap = 0;   // level-1 blocks
    uint64_t binned_cap = 0, binned3_cap = 0;            // elements
    uint64_t rows_cap = 0;
    // the bytes of every request, in count_run's order
    uint64_t b_gstat = 0, b_fs = 0, b_wcnt = 0, b_off = 0, b_nblk = 0, b_tab = 0, b_binned = 0, b_binned1 = 0, b_table = 0,
             b_binned3 = 0, b_fs3 = 0, b_rows_key = 0, b_rows_cnt = 0, b_blist = 0, b_pinst = 0;
    uint64_t work_bytes = 0;     // their sum
    uint64_t rows_bytes = 0;     // b_rows_key + b_rows_cnt
    bool rows_full = true;       // the rows got their full capacity total_bytes / min_per_file
};

inline uint32_t ceil_log2(uint32_t v) {
    uint32_t b = 0;
    while (b < 31 && (1u << b) < v) ++b;
    return b;
}

// The pass bits a k allows: at least one key bit stays below the pass bits and the level-1 region
// bits (2k - pb - MAX_FB1 >= 1); for k <= 3, whose keys are shorter than that, at most two passes
// (plan() then leaves a remainder bit below the bucket bits).
inline uint32_t clamp_pb(int k, uint32_t pb) {
    const uint32_t nbits = 2u * (uint32_t)k;
    const uint32_t lim = nbits > kMaxFb1 + 1 ? nbits - kMaxFb1 - 1 : 1;
    return std::min(std::min(pb, lim), ceil_log2(kMaxPasses));
}

// margin16: P > 1 only; the share of pass_bytes the per-instance buffers hold (16 P: any input).
// rows_budget: P > 1 only; bytes the rows may take (~0: their full capacity).
inline Plan plan(int k, uint32_t F, const uint64_t* seq_len, uint32_t min_per_file, uint32_t num_cu, const Hooks& hk,
                 uint32_t passes, uint32_t margin16 = kMargin16, uint64_t rows_budget = ~0ull) {
    Plan pl;
    const uint32_t full = 2u * (uint32_t)k;
    pl.pb = clamp_pb(k, ceil_log2(std::max(1u, passes)));
    pl.P = 1u << pl.pb;
    const uint32_t P = pl.P;
    const uint32_t nbits = pl.nbits = full - pl.pb;
    uint64_t total = 0;
    for (uint32_t f = 0; f < F; ++f) total += seq_len[f];
    pl.total_bytes = total;
    const uint64_t share = pl.pass_bytes = total / P;
    pl.margin16 = P > 1 ? std::min(std::max(margin16, 16u), 16u * P) : 16u;

    // fan-out: ~16K windows per fine bucket (packed counting: ~64K), at most 2^MAX_FB buckets, never
    // more bits than the key (one pass) / than leave a remainder bit (passes)
    pl.packed = F <= 2 && nbits - std::min<uint32_t>(kMaxFb, nbits) <= 31 && !hk.legacy;
    pl.per_bucket = pl.packed ? HGA_PB_P : 16384;
    const uint32_t fb_lim = P > 1 ? nbits - 1 : nbits;
    uint32_t fb = 0;
    const uint32_t fb_max = std::min(hk.fb_max, kMaxFb);
    while (fb < fb_max && fb < fb_lim && ((share >> fb) > pl.per_bucket || fb < hk.fb_min)) ++fb;
    if (nbits == 64 && fb == 0) fb = 1;   // k = 32, one pass: see count_run
    pl.fb = fb;
    pl.rbits = nbits - fb;
    pl.fb1 = std::min(fb, kMaxFb1);
    pl.r1bits = nbits - pl.fb1;
    pl.fb2 = fb - pl.fb1;
    pl.e1_32 = pl.r1bits <= 32;
    pl.e32 = pl.rbits <= 31;
    const uint64_t nb = 1ull << fb, nb1 = 1ull << pl.fb1;

    // super-tiles: ~HGA_B1_PER_CU per CU; far larger inputs take more, smaller ones so that each
    // (workgroup, region) still fits one block — sized by the instances a super-tile keeps, which is
    // 1/P of its bases, so the pool's first blocks shrink with P
    uint64_t st_pos = total / ((uint64_t)num_cu * HGA_B1_PER_CU) + 1;
    const uint64_t st_cap = kBlk * nb1 * 15 / 16 * P;
    if (hk.sole && st_pos > st_cap + st_cap / 2) st_pos = st_cap;
    st_pos = std::max<uint64_t>(kBlk, (st_pos + kBlk - 1) / kBlk * kBlk);
    pl.st_pos = st_pos;
    uint64_t W = 0;
    for (uint32_t f = 0; f < F; ++f) W += (seq_len[f] + st_pos - 1) / st_pos;
    pl.W = (uint32_t)W;

    // what one pass may hold: everything (one pass), or its share times the margin
    const uint64_t held =
        P > 1 ? std::min<uint64_t>(total, share / 16 * pl.margin16 + share % 16 * pl.margin16 / 16 + kMarginSlack) : total;
    pl.binned_cap = std::max<uint64_t>(held, 1);
    pl.n_first = W * nb1;
    pl.table_cap = pl.n_first + held / kBlk + 2;
    pl.pool_cap = pl.table_cap * kBlk;

    // third split level: fine buckets far above one LDS table
    uint32_t fb3 = 0;
    {
        const uint64_t avg = share >> fb;
        if (hk.split3_force >= 0) {
            while (fb3 < (uint32_t)hk.split3_force && fb3 < 8 && ((2u << fb3) * F) <= kMaxSf3 && pl.rbits - fb3 > 1) ++fb3;
        } else if (avg > 2 * pl.per_bucket && fb == kMaxFb) {
            while (fb3 < 8 && (avg >> fb3) > hk.split3_target && ((2u << fb3) * F) <= kMaxSf3 && pl.rbits - fb3 > 10) ++fb3;
        }
    }
    pl.fb3 = fb3;
    const uint64_t nbc = nb << fb3;
    pl.binned3_cap = fb3 ? held + held / 4 + nbc * kSlack3 + 64 : 0;

    uint64_t cap = (total / std::max<uint32_t>(1, min_per_file) + 4) & ~3ull;   // x4: 16-B row groups
    if (hk.row_cap) cap = std::max<uint64_t>(4, hk.row_cap & ~3ull);
    const uint64_t row_b = 8 + 4ull * F;
    if (P > 1 && rows_budget != ~0ull && cap > rows_budget / row_b) {
        cap = std::max<uint64_t>(4, (rows_budget / row_b) & ~3ull);
        pl.rows_full = false;
    }
    pl.rows_cap = cap;

    const uint64_t esz1 = pl.e1_32 ? 4 : 8, esz = pl.e32 ? 4 : 8;
    const uint64_t Wm = std::max<uint64_t>(W, 1);
    pl.b_gstat = 8 * 8;
    pl.b_fs = nb * (F + 1) * 8;
    pl.b_wcnt = Wm * nb * 4;
    pl.b_off = (W * nb + 1) * 8;
    pl.b_nblk = Wm * nb1 * 4;
    pl.b_tab = (kBinFileBytes + 4) * F;
    pl.b_binned = pl.binned_cap * esz;
    pl.b_binned1 = pl.pool_cap * esz1;
    pl.b_table = pl.table_cap * kBlkEntryBytes;
    pl.b_binned3 = pl.binned3_cap * esz;
    pl.b_fs3 = fb3 ? nbc * (F + 1) * 8 : 0;
    pl.b_rows_key = cap * 8;
    pl.b_rows_cnt = cap * 4 * F;
    pl.b_blist = pl.packed && pl.e32 ? nbc * 4 : 0;
    pl.b_pinst = (uint64_t)kMaxPasses * 8;   // (the same at any P: a budget of the one-pass request fits every P)
    pl.rows_bytes = pl.b_rows_key + pl.b_rows_cnt;
    pl.work_bytes = pl.b_gstat + pl.b_fs + pl.b_wcnt + pl.b_off + pl.b_nblk + pl.b_tab + pl.b_binned + pl.b_binned1 +
                    pl.b_table + pl.b_binned3 + pl.b_fs3 + pl.rows_bytes + pl.b_blist + pl.b_pinst;
    return pl;
}

// The plan of a run: `passes` >= 1 is taken as given (rounded up to a power of two, clamped);
// 0 picks the smallest P whose request at the base margin, full rows included, fits `budget`.
// With a budget and more than one pass, the rows get what the work buffers leave when their full
// capacity does not fit, and the margin grows as far as the budget allows — up to P, where every
// buffer holds the whole input and no key range can be too heavy.  budget 0: no limit (one pass
// when passes is 0), the base margin.  fits: the request is within the budget.
inline Plan plan_run(int k, uint32_t F, const uint64_t* seq_len, uint32_t min_per_file, uint32_t num_cu, const Hooks& hk,
                     uint32_t passes, uint64_t budget, bool* fits = nullptr) {
    if (fits) *fits = true;
    if (!budget) return plan(k, F, seq_len, min_per_file, num_cu, hk, std::max(1u, passes));
    uint32_t P = passes;
    if (!P) {
        const uint32_t pmax = 1u << clamp_pb(k, 31);
        for (P = 1; P < pmax; P <<= 1)
            if (plan(k, F, seq_len, min_per_file, num_cu, hk, P).work_bytes <= budget) break;
    }
    Plan pl = plan(k, F, seq_len, min_per_file, num_cu, hk, P);
    if (pl.P == 1) {
        if (fits) *fits = pl.work_bytes <= budget;
        return pl;
    }
    auto with = [&](uint32_t m16) {
        const Plan a = plan(k, F, seq_len, min_per_file, num_cu, hk, pl.P, m16);
        if (a.work_bytes <= budget) return a;
        const uint64_t rest = a.work_bytes - a.rows_bytes;   // the rows take what is left
        return plan(k, F, seq_len, min_per_file, num_cu, hk, pl.P, m16, budget > rest ? budget - rest : 0);
    };
    pl = with(kMargin16);
    if (pl.work_bytes > budget) {
        if (fits) *fits = false;
        return pl;
    }
    // the largest margin whose request, with the rows as they are now, still fits
    uint32_t lo = kMargin16, hi = 16u * pl.P;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        const Plan a = with(mid);
        if (a.work_bytes <= budget && a.rows_cap >= pl.rows_cap) lo = mid;
        else hi = mid - 1;
    }
    return lo > kMargin16 ? with(lo) : pl;
}

}  // namespace sizing
}  // namespace hga
