// ingest_cut_check.cpp — cut_records (host/fastio.cpp) as a stand-alone host program, meant to be built with
// AddressSanitizer + UBSan (tests/test_ingest_cut.py builds and runs it).  Every input lies in a heap block of
// exactly its size, so a read past the end or before the start is reported.  Checked for seeded FASTA, 4-line
// FASTQ and other files, whole and truncated at every length near the end, at several piece sizes:
//   * the starts begin at 0, ascend strictly and lie inside the data;
//   * every later start is a record start by the definition in seqio.h, and the first one at or after the
//     next multiple of the piece size above the previous start;
//   * a first byte other than '>' / '@' (after leading newlines) gives the single start 0.
// Prints "<n> checks, <f> failures".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "seqio.h"

namespace {
uint64_t checks = 0, failures = 0;
void expect(bool ok, const char* what, size_t n, size_t piece) {
    ++checks;
    if (!ok) {
        ++failures;
        if (failures <= 20) std::fprintf(stderr, "FAIL %s (n = %zu, piece = %zu)\n", what, n, piece);
    }
}

std::string bases(std::mt19937_64& rng, size_t n) {
    std::string s(n, 'A');
    for (auto& c : s) c = "ACGTNacgt"[rng() % 9];
    return s;
}

std::string make(std::mt19937_64& rng, int family, size_t size) {
    std::string d;
    if (family == 2) d = bases(rng, 5) + "\n";   // neither '>' nor '@' first
    if (rng() % 4 == 0) d += "\n\n";
    while (d.size() < size) {
        const size_t len = rng() % 70;
        if (family == 1) {   // 4-line FASTQ; quality lines may start with '@' or '+'
            std::string q(len, 'I');
            if (len && rng() % 3 == 0) q[0] = rng() % 2 ? '@' : '+';
            d += "@r" + std::to_string(rng() % 1000) + "\n" + bases(rng, len) + "\n+\n" + q + "\n";
        } else {             // multi-line FASTA with '@' / '+' / empty lines
            d += ">h" + std::to_string(rng() % 1000) + "\n";
            for (int l = (int)(rng() % 4); l > 0; --l) {
                const int kind = (int)(rng() % 8);
                d += (kind == 0 ? "" : kind == 1 ? "@" + bases(rng, len) : kind == 2 ? "+" + bases(rng, len) : bases(rng, len)) + "\n";
            }
        }
    }
    return d;
}

size_t next_line(const char* d, size_t n, size_t b) {
    while (b < n && d[b] != '\n') ++b;
    return b < n ? b + 1 : n;
}

bool record_start(const char* d, size_t n, size_t b, bool fastq) {
    if (b >= n || (b && d[b - 1] != '\n')) return false;
    if (!fastq) return d[b] == '>';
    if (d[b] != '@') return false;
    const size_t l2 = next_line(d, n, next_line(d, n, b));
    return l2 < n && d[l2] == '+';
}

void check_one(const std::string& src, size_t n, size_t piece) {
    std::unique_ptr<char[]> blk(new char[n ? n : 1]);   // exactly n bytes: the sanitizer sees any overrun
    if (n) std::memcpy(blk.get(), src.data(), n);
    const char* d = blk.get();
    const std::vector<uint64_t> cuts = hgah::cut_records(n ? d : nullptr, n, piece);
    expect(!cuts.empty() && cuts[0] == 0, "starts begin at 0", n, piece);
    size_t q = 0;
    while (q < n && d[q] == '\n') ++q;
    const bool known = q < n && (d[q] == '>' || d[q] == '@');
    if (!known) {
        expect(cuts.size() == 1, "unknown first byte: the single start 0", n, piece);
        return;
    }
    const bool fastq = d[q] == '@';
    for (size_t i = 1; i < cuts.size(); ++i) {
        const size_t c = cuts[i], prev = cuts[i - 1];
        expect(c > prev && c < n, "ascending, inside the data", n, piece);
        expect(record_start(d, n, c, fastq), "a record start", n, piece);
        const size_t m = (prev / piece + 1) * piece;
        bool first = m <= c;
        for (size_t x = m; first && x < c; ++x) first = !record_start(d, n, x, fastq);
        expect(first, "the first record start at or after the multiple", n, piece);
    }
    // and none was left out behind the last start
    const size_t m = (cuts.back() / piece + 1) * piece;
    bool none = true;
    for (size_t x = m; none && x < n; ++x) none = !record_start(d, n, x, fastq);
    expect(none, "no record start left behind the last one", n, piece);
}
}  // namespace

int main() {
    std::mt19937_64 rng(20260101);
    const size_t pieces[] = {1, 2, 7, 64, 333, 4096, SIZE_MAX};
    for (int family = 0; family < 3; ++family)
        for (int rep = 0; rep < 6; ++rep) {
            const std::string src = make(rng, family, 200 + 700 * (size_t)rep);
            for (size_t piece : pieces) {
                check_one(src, src.size(), piece);
                for (size_t cut = 0; cut <= 12 && cut <= src.size(); ++cut) check_one(src, src.size() - cut, piece);
                for (size_t n = 0; n <= 12 && n <= src.size(); ++n) check_one(src, n, piece);
            }
        }
    bool threw = false;
    try {
        (void)hgah::cut_records(">a\n", 3, 0);
    } catch (const std::invalid_argument&) {
        threw = true;
    }
    expect(threw, "piece 0 is refused", 3, 0);
    std::printf("%llu checks, %llu failures\n", (unsigned long long)checks, (unsigned long long)failures);
    return failures ? 1 : 0;
}
