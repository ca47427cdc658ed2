// lookup_sizing.hpp — every size of one read-batch slot of the SDK lookup (lookup.hip, hga_lookup_begin /
// _add_reads / _finish), as host arithmetic only (no HIP): hga_lookup_batch_estimate and the run call the
// same function, and tests/native/lookup_sizing_check.cpp runs it stand-alone under the host sanitizers.
//
// A slot holds what lk_read_map, lk_scan<false,...> and lk_scan<true,0> read and write for one batch of
// whole reads: the ASCII bases, the batch-local CSR offsets, the read-start bitmap, the word -> read map,
// the per-thread hit masks, the per-window KmerIDs and the per-tile hit counts.  A session keeps two
// slots (the next batch's upload and count scan are queued while this one's emit runs), each backed by
// one device allocation cut at kAlign boundaries, plus a pinned host staging area for the upload.
#pragma once
#include <cstdint>

namespace hga {
namespace lksizing {

constexpr uint64_t kP = 32;        // window ends per scan thread (lookup.hip LK_P)
constexpr uint64_t kT = 256;       // scan threads per tile (lookup.hip LK_T)
constexpr uint64_t kSbPad = 1;     // leading zero words of the read-start bitmap (SB_PAD)
constexpr uint64_t kSbTail = 64;   // trailing zero words of the read-start bitmap
constexpr uint64_t kAlign = 256;   // every part starts on this boundary (16-B loads of the bases)
constexpr uint64_t kSlots = 2;
constexpr uint64_t kMaxReads = (1ull << 32) - 1;   // reads of a session (ReadIDs are 32-bit)

struct Slot {
    uint64_t n_threads = 0, n_tiles = 0;
    // bytes of each part, then its offset inside the slot's allocation
    uint64_t b_bases = 0, b_offsets = 0, b_starts = 0, b_word_read = 0, b_hmask = 0, b_win_kid = 0, b_tile = 0;
    uint64_t o_bases = 0, o_offsets = 0, o_starts = 0, o_word_read = 0, o_hmask = 0, o_win_kid = 0, o_tile = 0;
    uint64_t bytes = 0;        // one slot's device allocation
    uint64_t stage_bytes = 0;  // one slot's pinned host staging: the bases, then the offsets
    uint64_t o_stage_offsets = 0;
};

inline uint64_t ceil_div(uint64_t a, uint64_t b) { return a / b + (a % b != 0); }
inline uint64_t align_up(uint64_t v) { return ceil_div(v, kAlign) * kAlign; }
inline uint64_t at_least_one(uint64_t v) { return v ? v : 1; }

// The slot of a batch of `reads` whole reads with `bases` bases in all (reads <= kMaxReads; bases far
// below 2^58, so no product here overflows 64 bits).
inline Slot slot(uint64_t bases, uint64_t reads) {
    Slot s;
    s.n_threads = ceil_div(bases, kP);
    s.n_tiles = ceil_div(s.n_threads, kT);
    const uint64_t words = ceil_div(bases, 32);   // 32-base words: starts bitmap, word_read
    s.b_bases = bases + 16;                       // lk_scan loads 16-B groups up to the last base
    s.b_offsets = (reads + 1) * 8;
    s.b_starts = (kSbPad + words + kSbTail) * 4;
    s.b_word_read = at_least_one(words) * 4;
    s.b_hmask = at_least_one(s.n_threads) * 4 + 256;
    s.b_win_kid = at_least_one(s.n_threads) * kP * 4;
    s.b_tile = (s.n_tiles + 1) * 8;
    uint64_t o = 0;
    auto put = [&](uint64_t& off, uint64_t b) {
        off = o;
        o += align_up(b);
    };
    put(s.o_bases, s.b_bases);
    put(s.o_offsets, s.b_offsets);
    put(s.o_starts, s.b_starts);
    put(s.o_word_read, s.b_word_read);
    put(s.o_hmask, s.b_hmask);
    put(s.o_win_kid, s.b_win_kid);
    put(s.o_tile, s.b_tile);
    s.bytes = o;
    s.o_stage_offsets = align_up(bases);
    s.stage_bytes = s.o_stage_offsets + s.b_offsets;
    return s;
}

// Device bytes of a session's slots for batches of at most `bases` bases and `reads` reads.
inline uint64_t slot_bytes(uint64_t bases, uint64_t reads) { return kSlots * slot(bases, reads).bytes; }

// The scan buffers of the one-shot path (hga_lookup_set_reads + hga_lookup_run) for the same input:
// what a session's slots replace.
inline uint64_t oneshot_bytes(uint64_t bases, uint64_t reads) {
    const Slot s = slot(bases, reads);
    return s.b_bases + s.b_offsets + s.b_starts + s.b_word_read + s.b_hmask + s.b_win_kid + s.b_tile;
}

// Capacity (in hits) of the appended hit arrays once `need` hits must fit: unchanged while they do,
// else doubled, or `need` itself when that is more.
inline uint64_t grow_hits(uint64_t cap, uint64_t need) {
    if (need <= cap) return cap;
    const uint64_t twice = cap > (~0ull >> 1) ? ~0ull : 2 * cap;
    return need > twice ? need : twice;
}
constexpr uint64_t kHitBytes = 4 + 4 + 4 + 8 + 4;   // hit_read, hit_kid, hit_pos, s_key, s_val per hit

}  // namespace lksizing
}  // namespace hga
