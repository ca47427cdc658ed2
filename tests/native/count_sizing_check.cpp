// Stand-alone check of the count's sizing arithmetic (csrc/count_sizing.hpp: pure host code, what
// hga_count_estimate and count_run share).  tests/test_count_sizing.py builds it with
// -fsanitize=address,undefined and runs it; it prints one line per failed property and exits 1.
//
// Properties, over k x files x input sizes x min_per_file x passes:
//   - P is a power of two <= 256, >= 1 key bit is left below the pass bits and the region bits
//     (k >= 4), and P equals the request when k allows it;
//   - every buffer that a kernel indexes by a count is large enough for it by construction
//     (the pool holds its first blocks, the table at least two spill blocks, binned >= 1);
//   - the requests sum to work_bytes, and a pass's buffers shrink with P for large inputs;
//   - plan_run: the auto choice is the smallest P that fits, the result is within the budget, a
//     budget of the one-pass request makes every buffer hold the whole input, and no budget
//     changes a one-pass plan.
#include <cstdio>
#include <vector>

#include "../../hybrid-genome-assembler_amd/csrc/count_sizing.hpp"

using namespace hga::sizing;

static int fails = 0;
#define CHECK(cond, ...)                         \
    do {                                         \
        if (!(cond)) {                           \
            std::printf("FAIL %s: ", #cond);     \
            std::printf(__VA_ARGS__);            \
            std::printf("\n");                   \
            ++fails;                             \
        }                                        \
    } while (0)

static uint64_t sum_requests(const Plan& p) {
    return p.b_gstat + p.b_fs + p.b_wcnt + p.b_off + p.b_nblk + p.b_tab + p.b_binned + p.b_binned1 + p.b_table +
           p.b_binned3 + p.b_fs3 + p.b_rows_key + p.b_rows_cnt + p.b_blist + p.b_pinst;
}

int main() {
    const int ks[] = {1, 2, 3, 4, 5, 12, 15, 16, 17, 19, 21, 22, 31, 32};
    const uint64_t totals[] = {0, 1, 7, 100, 65536, 65537, 1000003, 15000000, 268435456ull, 3770000000ull, 30000000000ull};
    const uint32_t Fs[] = {1, 2, 3, 5, 64};
    const uint32_t passes[] = {1, 2, 3, 4, 8, 64, 256, 1000};
    Hooks hooks[3];
    hooks[1].fb_min = 12;
    hooks[2].split3_force = 3;
    hooks[2].legacy = true;
    uint64_t cases = 0;
    for (int k : ks)
        for (uint64_t total : totals)
            for (uint32_t F : Fs)
                for (const Hooks& hk : hooks)
                    for (uint32_t mn : {1u, 2u, 3u}) {
                        std::vector<uint64_t> len(F, total / F);
                        len[0] += total % F;
                        const uint32_t cu = 256;
                        const Plan one = plan(k, F, len.data(), mn, cu, hk, 1);
                        for (uint32_t want : passes) {
                            const Plan p = plan(k, F, len.data(), mn, cu, hk, want);
                            ++cases;
                            const uint32_t nbits = 2u * (uint32_t)k;
                            CHECK(p.P >= 1 && p.P <= kMaxPasses && (p.P & (p.P - 1)) == 0 && p.P == (1u << p.pb), "k=%d P=%u", k, p.P);
                            CHECK(p.nbits + p.pb == nbits && p.nbits >= 1, "k=%d", k);
                            if (k >= 4) CHECK(p.nbits >= kMaxFb1 + 1, "k=%d pb=%u", k, p.pb);
                            if (k >= 12 && want <= kMaxPasses) CHECK(p.P >= want && p.P < 2 * want, "k=%d want=%u P=%u", k, want, p.P);
                            CHECK(p.P <= std::max(1u, want) * 2 - (want > 1), "k=%d want=%u P=%u", k, want, p.P);
                            CHECK(p.fb + p.rbits == p.nbits && p.fb1 + p.r1bits == p.nbits && p.fb1 + p.fb2 == p.fb, "bits k=%d", k);
                            CHECK(p.fb <= kMaxFb && p.fb1 <= kMaxFb1, "fb k=%d", k);
                            if (p.P > 1) CHECK(p.rbits >= 1 && p.rbits <= 63, "k=%d P=%u rbits=%u", k, p.P, p.rbits);
                            if (nbits == 64 && p.P == 1) CHECK(p.fb >= 1, "k=32 needs a bucket bit");
                            CHECK((p.e1_32 && p.r1bits <= 32) || (!p.e1_32 && p.r1bits > 32), "e1 k=%d", k);
                            CHECK((p.e32 && p.rbits <= 31) || (!p.e32 && p.rbits > 31), "e k=%d", k);
                            CHECK(p.st_pos % kBlk == 0 && p.st_pos >= kBlk, "st_pos");
                            uint64_t W = 0;
                            for (uint64_t l : len) W += (l + p.st_pos - 1) / p.st_pos;
                            CHECK(W == p.W && p.W * p.st_pos >= total, "W covers every base");
                            if (total >= 15000000) CHECK(p.W >= cu, "W=%u keeps the chip busy (total=%llu P=%u)", p.W, (unsigned long long)total, p.P);
                            CHECK(p.n_first == (uint64_t)p.W << p.fb1 && p.table_cap >= p.n_first + 2 && p.pool_cap == p.table_cap * kBlk, "pool");
                            CHECK(p.binned_cap >= 1 && p.binned_cap <= std::max<uint64_t>(total, 1), "binned");
                            if (p.P == 1) CHECK(p.binned_cap == std::max<uint64_t>(total, 1) && p.table_cap == p.n_first + total / kBlk + 2, "one pass holds all");
                            else CHECK(p.binned_cap >= std::min<uint64_t>(total, p.pass_bytes + p.pass_bytes / 4), "margin");
                            if (p.fb3) CHECK(p.binned3_cap >= p.binned_cap + p.binned_cap / 4 + (((uint64_t)kSlack3 << p.fb) << p.fb3), "binned3");
                            CHECK(p.rows_cap % 4 == 0 && p.rows_cap >= 4, "rows");
                            CHECK(sum_requests(p) == p.work_bytes, "sum");
                            if (p.P > 1 && total >= 268435456ull && hk.fb_min == 0)
                                CHECK(p.work_bytes - p.rows_bytes < one.work_bytes - one.rows_bytes, "passes shrink the work buffers k=%d P=%u", k, p.P);
                            // budgets
                            bool fits = false;
                            const Plan b1 = plan_run(k, F, len.data(), mn, cu, hk, want, one.work_bytes, &fits);
                            // (HGA_FB_MIN on an input of a few bases: the shorter key can bring in the packed
                            // kernel's bucket list, 16 KB that one pass does not have)
                            if (hk.fb_min == 0 || total >= 65536)
                                CHECK(fits && b1.work_bytes <= one.work_bytes, "k=%d F=%u total=%llu want=%u: %llu > %llu", k, F,
                                  (unsigned long long)total, want, (unsigned long long)b1.work_bytes, (unsigned long long)one.work_bytes);
                            CHECK(b1.P == p.P, "budget keeps the requested P");
                            if (b1.P > 1 && hk.fb_min == 0)
                                CHECK(b1.rows_full && b1.binned_cap == std::max<uint64_t>(total, 1) && b1.table_cap >= b1.n_first + total / kBlk + 2,
                                      "the one-pass budget holds any key range: k=%d F=%u total=%llu P=%u margin=%u", k, F,
                                      (unsigned long long)total, b1.P, b1.margin16);
                        }
                        // auto choice under a third of the one-pass request
                        const uint64_t third = one.work_bytes / 3;
                        bool fits = false;
                        const Plan a = plan_run(k, F, len.data(), mn, cu, hk, 0, third, &fits);
                        if (fits) {
                            CHECK(a.work_bytes <= third, "auto within budget");
                            if (a.P > 1) {
                                const Plan h = plan(k, F, len.data(), mn, cu, hk, a.P / 2);
                                CHECK(h.work_bytes > third || !a.rows_full, "auto picks the smallest P: k=%d total=%llu P=%u", k, (unsigned long long)total, a.P);
                            }
                            const Plan again = plan_run(k, F, len.data(), mn, cu, hk, a.P, third, nullptr);
                            CHECK(again.work_bytes == a.work_bytes, "the estimate at the chosen P equals the run's request");
                        }
                        const Plan nob = plan_run(k, F, len.data(), mn, cu, hk, 0, 0, nullptr);
                        CHECK(nob.P == 1 && nob.work_bytes == one.work_bytes, "no budget: one pass");
                    }
    std::printf("%llu cases, %d failures\n", (unsigned long long)cases, fails);
    return fails ? 1 : 0;
}
