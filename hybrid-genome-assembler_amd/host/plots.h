// plots.h — the wire strings `categorization -d` pipes to scripts/plotting.py
// (src/clustering/ReadClusteringEngine.cpp:19-124): pure formatters, byte for byte what the reference's
// fmt::format / boost::algorithm::join calls produce, and the pipe itself.
#pragma once

#include <cstdint>
#include <functional>
#include <string>
#include <utility>
#include <vector>

namespace hgah {

// run_command_with_input (src/common/Utils.cpp:24-45): popen(cmd, "w"), write, pclose.
int run_command_with_input(const std::string& cmd, const std::string& in);

// plot_connection_quality's histogram (:19-34 over every connection, :102-124 over the best connection per
// candidate) as rows: the scores strictly ascending, per score the good and the bad connections counted.
struct QualityHist {
    std::vector<uint64_t> score, good, bad;
};

// "{" good "}\n{" bad "}" (:32, :122): each side "score: count" joined by ", ", scores ascending, a
// side's count of 0 left out (the reference's per-side std::map never holds it).
std::string connection_histogram(const QualityHist& h);

// plot_read_coverage (:37-73).  Per component the (start, end) simulator coordinates of its reads.  The
// endpoints (position, is_start) are sorted as std::pair<uint32_t, bool>, and the coverage runs keep the
// reference's arithmetic: prev_pos is an int starting at -1, endpoint.first - prev_pos is evaluated in
// uint32_t and added to an int, a start is credited to the coverage after its increment.
// "[(c, b), ...]" per component, joined into "[...]".
using ReadSpans = std::vector<std::pair<uint32_t, uint32_t>>;
std::string component_coverage(const std::vector<ReadSpans>& components);

// plot_spectral (:77-98), three lines each ending in '\n': "(x, y, score)" per connection; "(id, category)"
// for x then y of every connection, repeats included, category = *categories.begin() of the component;
// the partition as "[[...], ...]".
struct SpectralEdge {
    uint32_t x, y;
    uint64_t score;
};
std::string spectral_graph(const std::vector<SpectralEdge>& connections,
                           const std::function<int32_t(uint32_t)>& first_category,
                           const std::vector<std::vector<uint32_t>>& partition);

}  // namespace hgah
