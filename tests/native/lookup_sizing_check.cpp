// Stand-alone check of the read-batch slot arithmetic of the SDK lookup (csrc/lookup_sizing.hpp: pure host
// code, what hga_lookup_batch_estimate and hga_lookup_add_reads share).  tests/test_lookup_sizing.py builds
// it with -fsanitize=address,undefined and runs it; it prints one line per failed property and exits 1.
//
// Properties, over bases x reads (0 and 1 base; 31 / 32 / 33 bases = one scan thread's frame; one tile of
// 256 threads x 32 bases +- 1; 2^32 - 1 reads; sizes near 2^40 bases):
//   - threads = ceil(bases / 32), tiles = ceil(threads / 256), computed without 32-bit wrap;
//   - every part holds what its kernel indexes: a byte per base + a 16-B group, reads + 1 offsets, a start
//     bit per base with a pad word in front and one behind the last word the scan reads, a read index per
//     32-base word, a mask and 32 KmerIDs per thread, a count per tile + the total;
//   - the parts start on 256-B boundaries in the order of the header, do not overlap and sum to `bytes`;
//   - sizes are monotone in bases and in reads, two slots are twice one, and the slots of a batch are
//     smaller than the one-shot buffers of a read set of four or more such batches;
//   - grow_hits never shrinks, holds the need, and at least doubles when it grows.
#include <cstdio>
#include <initializer_list>

#include "../../hybrid-genome-assembler_amd/csrc/lookup_sizing.hpp"

using namespace hga::lksizing;

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

static void check_slot(uint64_t bases, uint64_t reads) {
    const Slot s = slot(bases, reads);
    const unsigned long long B = bases, R = reads;
    // 128-bit reference for the counts
    const unsigned __int128 b128 = bases;
    const uint64_t threads = (uint64_t)((b128 + 31) / 32), tiles = (uint64_t)(((unsigned __int128)threads + 255) / 256);
    const uint64_t words = threads;   // 32-base words = scan threads (kP == 32)
    CHECK(s.n_threads == threads && s.n_tiles == tiles, "bases %llu reads %llu", B, R);
    CHECK(s.n_threads * kP >= bases && (s.n_threads == 0 || (s.n_threads - 1) * kP < bases), "bases %llu", B);
    CHECK(s.b_bases >= bases + 16, "bases %llu", B);
    CHECK(s.b_offsets == (reads + 1) * 8, "reads %llu", R);
    // lk_scan reads start words kSbPad + p0 / 32 - 1 and kSbPad + p0 / 32 for every p0 = 32 t < bases
    CHECK(s.b_starts >= (kSbPad + words + 1) * 4, "bases %llu", B);
    CHECK(s.b_word_read >= 4 && s.b_word_read >= words * 4, "bases %llu", B);
    CHECK(s.b_hmask >= 4 && s.b_hmask >= threads * 4, "bases %llu", B);
    CHECK(s.b_win_kid >= 4 && s.b_win_kid / 4 / kP >= threads, "bases %llu", B);
    CHECK(s.b_tile == (tiles + 1) * 8, "bases %llu", B);
    const uint64_t off[7] = {s.o_bases, s.o_offsets, s.o_starts, s.o_word_read, s.o_hmask, s.o_win_kid, s.o_tile};
    const uint64_t len[7] = {s.b_bases, s.b_offsets, s.b_starts, s.b_word_read, s.b_hmask, s.b_win_kid, s.b_tile};
    CHECK(off[0] == 0, "bases %llu reads %llu", B, R);
    for (int i = 0; i < 7; ++i) {
        CHECK(off[i] % kAlign == 0, "part %d bases %llu reads %llu", i, B, R);
        const uint64_t end = i < 6 ? off[i + 1] : s.bytes;
        CHECK(off[i] + len[i] <= end && end - off[i] - len[i] < kAlign, "part %d bases %llu reads %llu", i, B, R);
    }
    CHECK(s.bytes % kAlign == 0 && s.bytes > 0, "bases %llu reads %llu", B, R);
    CHECK(slot_bytes(bases, reads) == 2 * s.bytes, "bases %llu reads %llu", B, R);
    CHECK(s.o_stage_offsets >= bases && s.o_stage_offsets % 8 == 0 && s.stage_bytes == s.o_stage_offsets + s.b_offsets,
          "bases %llu reads %llu", B, R);
    CHECK(oneshot_bytes(bases, reads) <= s.bytes, "bases %llu reads %llu", B, R);
    // the leading term: 1 (bases) + 1/8 (starts) + 1/8 (word_read) + 1/8 (hmask) + 4 (win_kid) B per base
    if (bases >= (1ull << 20))
        CHECK(s.bytes >= bases * 5 && s.bytes - (reads + 1) * 8 <= bases * 6, "bases %llu reads %llu: %llu", B, R,
              (unsigned long long)s.bytes);
}

int main() {
    const uint64_t tile = kP * kT;
    const uint64_t bases[] = {0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 4096, tile - 1, tile, tile + 1, 2 * tile - 1,
                              2 * tile, 2 * tile + 1, 1000003,   // (ascending: the monotone check below) (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 1,
                              (1ull << 37) - 1, (1ull << 40) - 33, (1ull << 40) - 1, 1ull << 40, (1ull << 40) + 1,
                              (1ull << 40) + tile + 5, 3ull << 40};
    const uint64_t reads[] = {0, 1, 2, 31, 32, 33, 1000, (1ull << 31) - 1, 1ull << 31, kMaxReads - 1, kMaxReads};
    uint64_t cases = 0;
    for (uint64_t b : bases)
        for (uint64_t r : reads) {
            check_slot(b, r);
            ++cases;
        }
    // monotone in either argument
    for (size_t i = 0; i + 1 < sizeof(bases) / 8; ++i)
        for (uint64_t r : reads) CHECK(slot(bases[i], r).bytes <= slot(bases[i + 1], r).bytes, "bases %zu", i);
    for (uint64_t b : bases)
        for (size_t j = 0; j + 1 < sizeof(reads) / 8; ++j)
            CHECK(slot(b, reads[j]).bytes <= slot(b, reads[j + 1]).bytes, "reads %zu", j);
    // a session's two slots against the one-shot buffers of a read set of n such batches
    for (uint64_t b : {1ull << 24, 1ull << 26, 1ull << 28})
        for (uint64_t n : {4ull, 16ull, 1000ull})
            CHECK(slot_bytes(b, b / 1000) < oneshot_bytes(n * b, n * (b / 1000)), "batch %llu x %llu",
                  (unsigned long long)b, (unsigned long long)n);
    // the hit arrays' capacity
    for (uint64_t cap : {0ull, 1ull, 86ull, 1ull << 20, (1ull << 40) + 3, ~0ull >> 1, (~0ull >> 1) + 1, ~0ull})
        for (uint64_t need : {0ull, 1ull, 85ull, 86ull, 87ull, 173ull, (1ull << 20) + 1, 1ull << 41, ~0ull}) {
            const uint64_t g = grow_hits(cap, need);
            CHECK(g >= cap && g >= need, "cap %llu need %llu", (unsigned long long)cap, (unsigned long long)need);
            if (need <= cap) CHECK(g == cap, "cap %llu need %llu", (unsigned long long)cap, (unsigned long long)need);
            else CHECK(g == ~0ull || g >= 2 * cap, "cap %llu need %llu", (unsigned long long)cap, (unsigned long long)need);
            ++cases;
        }
    CHECK(kHitBytes == 24, "hit bytes");
    std::printf("%llu cases, %d failures\n", (unsigned long long)cases, fails);
    return fails ? 1 : 0;
}
