// ingest.hip — hga_count_add_file: the '\n'-separated read stream of a FASTA / FASTQ file, made on the
// device from the file's raw bytes and appended to seq[file], where hga_count_add would have put it.
//
// The specification is jf_stream_fast (host/fastio.cpp): lines as std::getline sees them, the layout taken
// from the first non-empty line, FASTA and 4-line FASTQ produced, everything else refused (layout 3, the
// ctx untouched, the caller parses on the host).  Both accepted layouts keep or drop each input byte by a
// rule that only looks at the byte's line, and the kept bytes stay in input order:
//   FASTA   a header line ('>' first) keeps its '>' as one '\n' (the first header keeps nothing); every
//           other line keeps all its bytes but the '\n';
//   FASTQ   line 4r + 1 keeps all its bytes but the '\n'; line 4r, r > 0, keeps its '@' as one '\n'.
// So the stream is a byte compaction, and every pass takes a fixed tile of IG_TILE input bytes per
// workgroup whatever the lines are (one 5 MB line and millions of 1-byte lines are the same grid):
//   ig_count    newlines per tile; the position of the first byte that is not '\n' (the first non-empty
//               line starts there): the word is read first and one atomic per workgroup follows only when
//               the tile's candidate beats it
//   (scan)      exclusive_scan_u64: each tile's first line index, the number of newlines at the end
//   -- first host read: {newlines, first position}; with the caller's byte there and the last byte the host
//      knows the line count and the layout up to FASTQ's per-record rules, and sizes the line table
//   ig_starts   the u32 line-start table (a call is at most 2^32 - 1 bytes)
//   ig_lines    FASTQ only, one thread per line: the four per-record rules of jf_stream_fast; a wave vote,
//               then at most one atomic per workgroup ORs the refusal word, and none for a valid file
//   ig_kept     kept bytes per tile, and the header lines that begin in it (FASTA: the records)
//   (scan)      each tile's output offset, the total at the end (and the headers' total)
//   -- second host read: {refusal word, out_bytes, records}; seq[file] grows as count_add grows it
//   ig_scatter  the tile's kept bytes compacted in LDS at the destination's offset mod 16, then written as
//               16-byte stores where a whole aligned chunk is the tile's, single bytes at its two ends
// The walk over a thread's 32 bytes (ig_walk) is one function for ig_kept and ig_scatter, so the two agree.
// Every ballot, shuffle and barrier is outside divergent code; no lane takes work from a device counter;
// every store is a plain vector store; the two control words are zeroed on the stream in each call.
#include "hga_internal.hpp"

namespace hga {
namespace {

constexpr int IG_T = 256;                  // threads per workgroup
constexpr int IG_B = 32;                   // input bytes per thread: two 16-byte loads
constexpr int IG_TILE = IG_T * IG_B;       // input bytes per workgroup (hga_ingest_tile)
enum { IG_FIRST = 0, IG_BAD = 1, IG_CTL = 2 };   // control words
enum { LAYOUT_EMPTY = 0, LAYOUT_FASTA = 1, LAYOUT_FASTQ = 2, LAYOUT_REFUSED = 3 };

// inclusive scan of v over the workgroup, *total = the sum; lds: IG_T / 64 words.  Called by every thread.
__device__ __forceinline__ uint32_t ig_block_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    __syncthreads();   // (the previous call's readers are done with lds)
    if (lane == 63) lds[wave] = v;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < IG_T / 64; ++w) {
        const uint32_t t = lds[w];
        if (w < wave) before += t;
        all += t;
    }
    *total = all;
    return v + before;
}

// The thread's 32 bytes of the staging buffer (padded so that every chunk starting below n is allocated)
// as 8 words; valid = how many of them lie below n.
struct IgChunk {
    uint32_t w[IG_B / 4];
    uint32_t p0, valid;
    __device__ __forceinline__ uint32_t byte(int j) const { return (w[j >> 2] >> ((j & 3) * 8)) & 0xFFu; }
};

__device__ __forceinline__ IgChunk ig_load(const uint8_t* __restrict__ d, uint32_t n) {
    IgChunk c;
    const uint64_t p = (uint64_t)blockIdx.x * IG_TILE + (uint64_t)threadIdx.x * IG_B;
    c.p0 = (uint32_t)p;
    c.valid = p < n ? (uint32_t)min((uint64_t)IG_B, (uint64_t)n - p) : 0u;
    if (c.valid) {
        const uint4 a = *reinterpret_cast<const uint4*>(d + p), b = *reinterpret_cast<const uint4*>(d + p + 16);
        c.w[0] = a.x, c.w[1] = a.y, c.w[2] = a.z, c.w[3] = a.w;
        c.w[4] = b.x, c.w[5] = b.y, c.w[6] = b.z, c.w[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < IG_B / 4; ++j) c.w[j] = 0;
    }
    return c;
}

// bit j: byte j of the chunk is a valid '\n'
__device__ __forceinline__ uint32_t ig_newlines(const IgChunk& c) {
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < IG_B; ++j) m |= (c.byte(j) == (uint32_t)'\n' ? 1u : 0u) << j;
    return c.valid >= (uint32_t)IG_B ? m : (m & ((1u << c.valid) - 1u));
}

__global__ void __launch_bounds__(IG_T) ig_count(const uint8_t* __restrict__ d, uint32_t n, uint64_t* __restrict__ cnt,
                                                 uint32_t* __restrict__ ctl) {
    __shared__ uint32_t lds[IG_T / 64];
    __shared__ uint32_t lds_first[IG_T / 64];
    const IgChunk c = ig_load(d, n);
    const uint32_t nl = ig_newlines(c);
    const uint32_t vmask = c.valid >= (uint32_t)IG_B ? ~0u : ((1u << c.valid) - 1u);
    const uint32_t other = ~nl & vmask;   // valid bytes that are not '\n'
    // candidates are held as ~position, zero: none, so the zeroed word needs no other initial value
    uint32_t cand = other ? ~(c.p0 + (uint32_t)(__ffs((int)other) - 1)) : 0u;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) cand = max(cand, (uint32_t)__shfl_xor(cand, o, 64));
    if ((threadIdx.x & 63u) == 0) lds_first[threadIdx.x >> 6] = cand;
    uint32_t total;
    (void)ig_block_scan((uint32_t)__popc(nl), lds, &total);   // (its barriers also publish lds_first)
    if (threadIdx.x == 0) {
        cnt[blockIdx.x] = total;
        uint32_t best = 0;
#pragma unroll
        for (int w = 0; w < IG_T / 64; ++w) best = max(best, lds_first[w]);
        if (best && __hip_atomic_load(&ctl[IG_FIRST], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < best)
            atomicMax(&ctl[IG_FIRST], best);
    }
}

// st[0] = 0, st[j + 1] = the position behind the j-th '\n' (NL + 1 entries; at most n <= 2^32 - 1)
__global__ void __launch_bounds__(IG_T) ig_starts(const uint8_t* __restrict__ d, uint32_t n, const uint64_t* __restrict__ first_line,
                                                  uint32_t NL, uint32_t* __restrict__ st) {
    __shared__ uint32_t lds[IG_T / 64];
    const IgChunk c = ig_load(d, n);
    uint32_t nl = ig_newlines(c);
    const uint32_t mine = (uint32_t)__popc(nl);
    uint32_t total;
    const uint32_t before = ig_block_scan(mine, lds, &total) - mine;
    uint64_t at = first_line[blockIdx.x] + before + 1;
    if (blockIdx.x == 0 && threadIdx.x == 0) st[0] = 0;
    while (nl) {
        const int j = __ffs((int)nl) - 1;
        nl &= nl - 1;
        if (at <= NL) st[at] = c.p0 + (uint32_t)j + 1u;   // (at <= NL: the count came from the same bytes)
        ++at;
    }
}

// What the passes share: the staged bytes and their line table.
struct IgIn {
    const uint8_t* d;
    const uint32_t* st;
    const uint64_t* first_line;   // per tile: the index of the line its first byte lies in
    uint32_t n, NL, nl;           // bytes, newlines, lines (nl = NL, + 1 when the last byte is not '\n')
    uint32_t layout, first_pos;   // FASTA: the position of the first header
    __device__ __forceinline__ uint32_t begin(uint32_t i) const { return st[i]; }
    __device__ __forceinline__ uint32_t len(uint32_t i) const { return (i < NL ? st[i + 1] - 1u : n) - st[i]; }
    __device__ __forceinline__ uint32_t c0(uint32_t i) const { return len(i) ? d[st[i]] : 0u; }
};

// jf_stream_fast's acceptance of 4-line FASTQ, one thread per line (the host has checked the first line's
// position and the line count)
__global__ void __launch_bounds__(IG_T) ig_lines(IgIn in, uint32_t* __restrict__ ctl) {
    __shared__ uint32_t lds_bad;
    if (threadIdx.x == 0) lds_bad = 0;
    __syncthreads();
    const uint64_t i64 = (uint64_t)blockIdx.x * IG_T + threadIdx.x;
    bool bad = false;
    if (i64 < in.nl) {
        const uint32_t i = (uint32_t)i64;
        switch (i & 3u) {
        case 0: bad = in.c0(i) != (uint32_t)'@'; break;
        case 1: bad = in.c0(i) == (uint32_t)'+'; break;
        case 2: bad = in.c0(i) != (uint32_t)'+'; break;
        default: bad = in.len(i) != in.len(i - 2); break;
        }
    }
    const unsigned long long m = __ballot(bad);
    if (m && (threadIdx.x & 63u) == 0) lds_bad = 1;   // (plain store of the same value by up to four waves)
    __syncthreads();
    if (threadIdx.x == 0 && lds_bad) atomicOr(&ctl[IG_BAD], 1u);
}

// The walk over the thread's chunk.  `before` = newlines of the tile in front of the chunk.  Returns the
// number of kept bytes and adds the headers met to *hdrs; with WRITE the kept bytes go to out[0 ..].
template <bool WRITE>
__device__ __forceinline__ uint32_t ig_walk(const IgIn& in, const IgChunk& c, uint32_t before, uint32_t* hdrs,
                                            uint8_t* out) {
    if (!c.valid) return 0;
    uint32_t line = (uint32_t)in.first_line[blockIdx.x] + before;
    bool at_start = c.p0 == 0 || in.d[c.p0 - 1] == (uint8_t)'\n';
    uint32_t kept = 0;
    if (in.layout == LAYOUT_FASTA) {
        // header: the chunk's first byte lies in a header line (looked up when the line began earlier)
        bool header = !at_start && in.d[in.begin(line)] == (uint8_t)'>';
#pragma unroll
        for (int j = 0; j < IG_B; ++j) {
            if ((uint32_t)j < c.valid) {
                const uint32_t b = c.byte(j);
                if (b == (uint32_t)'\n') {
                    at_start = true;
                    header = false;
                } else {
                    bool keep = !header;
                    uint32_t v = b;
                    if (at_start && b == (uint32_t)'>') {
                        header = true;
                        ++*hdrs;
                        keep = c.p0 + (uint32_t)j != in.first_pos;
                        v = (uint32_t)'\n';
                    }
                    at_start = false;
                    if (keep) {
                        if (WRITE) out[kept] = (uint8_t)v;
                        ++kept;
                    }
                }
            }
        }
    } else {   // FASTQ, already accepted by ig_lines: line 4r is not empty
#pragma unroll
        for (int j = 0; j < IG_B; ++j) {
            if ((uint32_t)j < c.valid) {
                const uint32_t b = c.byte(j);
                if (b == (uint32_t)'\n') {
                    at_start = true;
                    ++line;
                } else {
                    const uint32_t q = line & 3u;
                    const bool sep = q == 0 && at_start && line != 0;
                    at_start = false;
                    if (q == 1 || sep) {
                        if (WRITE) out[kept] = (uint8_t)(sep ? (uint32_t)'\n' : b);
                        ++kept;
                    }
                }
            }
        }
    }
    return kept;
}

// kept[tile] = the tile's kept bytes, hdr[tile] = the header lines that begin in it
__global__ void __launch_bounds__(IG_T) ig_kept(IgIn in, uint64_t* __restrict__ kept, uint64_t* __restrict__ hdr) {
    __shared__ uint32_t lds[IG_T / 64];
    const IgChunk c = ig_load(in.d, in.n);
    const uint32_t mine = (uint32_t)__popc(ig_newlines(c));
    uint32_t total;
    const uint32_t before = ig_block_scan(mine, lds, &total) - mine;
    uint32_t hdrs = 0;
    const uint32_t k = ig_walk<false>(in, c, before, &hdrs, nullptr);
    uint32_t tot_k, tot_h;
    (void)ig_block_scan(k, lds, &tot_k);
    (void)ig_block_scan(hdrs, lds, &tot_h);
    if (threadIdx.x == 0) {
        kept[blockIdx.x] = tot_k;
        hdr[blockIdx.x] = tot_h;
    }
}

// dst: where the call's output begins; out_off[tile]: the tile's offset in it (below out_total < 2^32)
__global__ void __launch_bounds__(IG_T) ig_scatter(IgIn in, const uint64_t* __restrict__ out_off, uint32_t out_total,
                                                   uint8_t* __restrict__ dst) {
    __shared__ uint32_t lds[IG_T / 64];
    __shared__ __attribute__((aligned(16))) uint8_t buf[IG_TILE + 16];
    const IgChunk c = ig_load(in.d, in.n);
    const uint32_t mine = (uint32_t)__popc(ig_newlines(c));
    uint32_t total;
    const uint32_t before = ig_block_scan(mine, lds, &total) - mine;
    uint32_t hdrs = 0;
    const uint32_t k = ig_walk<false>(in, c, before, &hdrs, nullptr);
    uint32_t m;
    const uint32_t at = ig_block_scan(k, lds, &m) - k;
    const uint64_t o0 = out_off[blockIdx.x];
    if (o0 > out_total || m > out_total - o0) return;   // (never: the offsets are ig_kept's; uniform in the workgroup)
    uint8_t* g0 = dst + o0;
    // buf index = destination address mod 16 + offset in the tile's output, so that an aligned 16-byte chunk
    // of the destination is an aligned chunk of buf; at + k <= m <= IG_TILE: the walk stays inside buf
    const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(g0) & 15u);
    (void)ig_walk<true>(in, c, before, &hdrs, buf + a + at);
    __syncthreads();
    const uint32_t end = a + m, chunks = (end + 15u) / 16u;
    uint8_t* gbase = g0 - a;   // 16-byte aligned
    for (uint32_t q = threadIdx.x; q < chunks; q += IG_T) {
        const uint32_t lo = q * 16u;
        if (lo >= a && lo + 16u <= end) {
            *reinterpret_cast<uint4*>(gbase + lo) = *reinterpret_cast<const uint4*>(buf + lo);
        } else {
            for (uint32_t x = max(lo, a); x < min(lo + 16u, end); ++x) gbase[x] = buf[x];
        }
    }
}

inline unsigned ig_grid(uint64_t n) { return (unsigned)((n + IG_TILE - 1) / IG_TILE); }

}  // namespace

uint32_t ingest_tile() { return (uint32_t)IG_TILE; }

void ingest_release(hga_ctx* c) {
    auto& s = c->count;
    s.ing_raw.release();
    s.ing_st.release();
    s.ing_cnt.release();
    s.ing_kept.release();
    s.ing_ctl.release();
}

void count_add_file(hga_ctx* c, uint32_t file, const char* bytes, uint64_t n64, hga_ingest_info* info) {
    auto& s = c->count;
    HGA_REQUIRE(s.begun, HGA_ERR_STATE, "hga_count_begin not called");
    HGA_REQUIRE(file < s.n_files, HGA_ERR_INVALID, "file index out of range");
    HGA_REQUIRE(info, HGA_ERR_INVALID, "null info pointer");
    HGA_REQUIRE(bytes || n64 == 0, HGA_ERR_INVALID, "null bytes pointer");
    HGA_REQUIRE(n64 <= 0xFFFFFFFFull, HGA_ERR_INVALID,
                "more than 2^32 - 1 bytes in one call: cut the file at record starts (line starts are 32-bit on the device)");
    *info = hga_ingest_info{};
    if (n64 == 0) return;
    const uint32_t n = (uint32_t)n64;
    const uint32_t nt = ig_grid(n);
    // Every error below leaves through here: nothing of this call is still in flight when a buffer goes
    // (the caller may free its bytes, hga_count_run releases the staging).
    struct Drain {
        hga_ctx* c;
        bool armed = true;
        ~Drain() {
            if (armed) (void)hipStreamSynchronize(c->stream);
        }
    } drain{c};

    // every chunk of 32 bytes that starts below n is allocated
    uint8_t* d = static_cast<uint8_t*>(s.ing_raw.ensure(((uint64_t)n + IG_B - 1) / IG_B * IG_B + IG_B));
    uint64_t* cnt = static_cast<uint64_t*>(s.ing_cnt.ensure(((uint64_t)nt + 1) * 8));
    uint64_t* kept = static_cast<uint64_t*>(s.ing_kept.ensure(((uint64_t)nt + 1) * 16));
    uint64_t* hdr = kept + nt + 1;
    uint32_t* ctl = static_cast<uint32_t*>(s.ing_ctl.ensure(IG_CTL * 4));
    HGA_HIP(hipMemcpyAsync(d, bytes, n, hipMemcpyHostToDevice, c->stream));
    HGA_HIP(hipMemsetAsync(ctl, 0, IG_CTL * 4, c->stream));
    HGA_HIP(hipMemsetAsync(cnt + nt, 0, 8, c->stream));
    HGA_HIP(hipMemsetAsync(kept + nt, 0, 8, c->stream));
    HGA_HIP(hipMemsetAsync(hdr + nt, 0, 8, c->stream));
    c->launch("ig_count", [&] { hipLaunchKernelGGL(ig_count, dim3(nt), dim3(IG_T), 0, c->stream, d, n, cnt, ctl); });
    c->check_launch("ig_count");
    exclusive_scan_u64(c, cnt, (uint64_t)nt + 1, s.scratch);
    struct Head {
        uint64_t newlines, kept, headers;
        uint32_t ctl[IG_CTL];
    };
    Head* h = static_cast<Head*>(c->pinned.ensure(sizeof(Head)));
    HGA_HIP(hipMemcpyAsync(&h->newlines, cnt + nt, 8, hipMemcpyDeviceToHost, c->stream));
    HGA_HIP(hipMemcpyAsync(h->ctl, ctl, IG_CTL * 4, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    HGA_REQUIRE(h->newlines <= n, HGA_ERR_HIP, "ingest: newline count out of range");
    const uint32_t NL = (uint32_t)h->newlines;
    const uint64_t nl = (uint64_t)NL + (bytes[n - 1] != '\n' ? 1 : 0);
    info->lines = nl;
    if (h->ctl[IG_FIRST] == 0) {   // only empty lines
        info->layout = LAYOUT_EMPTY;
        drain.armed = false;
        return;
    }
    const uint32_t first_pos = ~h->ctl[IG_FIRST];
    HGA_REQUIRE(first_pos < n, HGA_ERR_HIP, "ingest: first line out of range");
    const char head = bytes[first_pos];
    uint32_t layout = LAYOUT_REFUSED;
    if (head == '>') layout = LAYOUT_FASTA;
    else if (head == '@' && first_pos == 0 && nl % 4 == 0) layout = LAYOUT_FASTQ;
    info->layout = layout;
    if (layout == LAYOUT_REFUSED) {
        drain.armed = false;
        return;
    }

    uint32_t* st = static_cast<uint32_t*>(s.ing_st.ensure(((uint64_t)NL + 1) * 4));
    c->launch("ig_starts", [&] { hipLaunchKernelGGL(ig_starts, dim3(nt), dim3(IG_T), 0, c->stream, d, n, cnt, NL, st); });
    c->check_launch("ig_starts");
    IgIn in{};
    in.d = d;
    in.st = st;
    in.first_line = cnt;
    in.n = n;
    in.NL = NL;
    in.nl = (uint32_t)nl;   // (nl <= n)
    in.layout = layout;
    in.first_pos = first_pos;
    if (layout == LAYOUT_FASTQ) {
        c->launch("ig_lines", [&] {
            hipLaunchKernelGGL(ig_lines, dim3((unsigned)((nl + IG_T - 1) / IG_T)), dim3(IG_T), 0, c->stream, in, ctl);
        });
        c->check_launch("ig_lines");
    }
    // (a FASTQ file ig_lines refuses is still walked: the walk reads only the table and the bytes, and its
    // result is dropped below — one synchronisation instead of two)
    c->launch("ig_kept", [&] { hipLaunchKernelGGL(ig_kept, dim3(nt), dim3(IG_T), 0, c->stream, in, kept, hdr); });
    c->check_launch("ig_kept");
    exclusive_scan_u64(c, kept, (uint64_t)nt + 1, s.scratch);
    if (layout == LAYOUT_FASTA) exclusive_scan_u64(c, hdr, (uint64_t)nt + 1, s.scratch);
    HGA_HIP(hipMemcpyAsync(&h->kept, kept + nt, 8, hipMemcpyDeviceToHost, c->stream));
    HGA_HIP(hipMemcpyAsync(&h->headers, hdr + nt, 8, hipMemcpyDeviceToHost, c->stream));
    HGA_HIP(hipMemcpyAsync(h->ctl, ctl, IG_CTL * 4, hipMemcpyDeviceToHost, c->stream));
    c->sync();
    if (layout == LAYOUT_FASTQ && h->ctl[IG_BAD]) {
        info->layout = LAYOUT_REFUSED;
        drain.armed = false;
        return;
    }
    const uint64_t out_bytes = h->kept;
    HGA_REQUIRE(out_bytes <= n && h->headers <= nl, HGA_ERR_HIP, "ingest: output size out of range");
    info->records = layout == LAYOUT_FASTQ ? nl / 4 : h->headers;
    info->seq_bytes = out_bytes;
    if (out_bytes == 0) {
        drain.armed = false;
        return;
    }
    // as count_add: grown to twice the capacity at least, one separator between calls
    const uint64_t old = s.seq_len[file];
    const uint64_t need = old + (old ? 1 : 0) + out_bytes;
    DevBuf* b = s.seq[file];
    if (need > b->cap) {
        size_t cap = std::max<size_t>(need + 64, b->cap ? b->cap * 2 : 0);
        std::unique_ptr<DevBuf> nb(new DevBuf());
        nb->ensure(cap);
        if (old) HGA_HIP(hipMemcpyAsync(nb->p, b->p, old, hipMemcpyDeviceToDevice, c->stream));
        c->sync();
        delete b;
        s.seq[file] = b = nb.release();
    }
    uint8_t* dst = b->as<uint8_t>();
    if (old) HGA_HIP(hipMemsetAsync(dst + old, '\n', 1, c->stream));
    c->launch("ig_scatter", [&] {
        hipLaunchKernelGGL(ig_scatter, dim3(nt), dim3(IG_T), 0, c->stream, in, kept, (uint32_t)out_bytes, dst + (need - out_bytes));
    });
    c->check_launch("ig_scatter");
    c->sync();
    drain.armed = false;
    s.seq_len[file] = need;
    s.ran = false;
    s.dist = false;
}

void count_seq(hga_ctx* c, uint32_t file, char** bytes, uint64_t* n) {
    auto& s = c->count;
    HGA_REQUIRE(s.begun, HGA_ERR_STATE, "hga_count_begin not called");
    HGA_REQUIRE(file < s.n_files, HGA_ERR_INVALID, "file index out of range");
    HGA_REQUIRE(bytes && n, HGA_ERR_INVALID, "null out pointer");
    const uint64_t len = s.seq_len[file];
    char* p = static_cast<char*>(std::malloc(len ? len : 1));
    if (!p) throw std::bad_alloc();
    if (len) {
        const hipError_t e = hipMemcpyAsync(p, s.seq[file]->p, len, hipMemcpyDeviceToHost, c->stream);
        const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(c->stream) : e;
        if (e2 != hipSuccess) {
            (void)hipStreamSynchronize(c->stream);
            std::free(p);
            HGA_HIP(e2);
        }
    }
    *bytes = p;
    *n = len;
}

}  // namespace hga
