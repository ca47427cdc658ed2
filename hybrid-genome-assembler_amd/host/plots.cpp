// plots.cpp — see plots.h.
#include "plots.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>

namespace hgah {

int run_command_with_input(const std::string& cmd, const std::string& in) {
    std::FILE* p = popen(cmd.c_str(), "w");
    if (!p) {
        std::fprintf(stderr, "incorrect parameters or too many files.\n");
        return EXIT_FAILURE;
    }
    std::fprintf(p, "%s", in.c_str());
    if (std::ferror(p)) {
        std::fprintf(stderr, "Output to stream failed.\n");
        std::exit(EXIT_FAILURE);
    }
    if (pclose(p) != 0) std::fprintf(stderr, "Could not run more or other error.\n");
    return EXIT_SUCCESS;
}

namespace {
void join_to(std::string& out, const std::vector<std::string>& parts) {   // boost::algorithm::join(parts, ", ")
    for (size_t i = 0; i < parts.size(); ++i) {
        if (i) out += ", ";
        out += parts[i];
    }
}
}  // namespace

std::string connection_histogram(const QualityHist& h) {
    std::vector<std::string> good, bad;
    for (size_t i = 0; i < h.score.size(); ++i) {
        if (h.good[i]) good.push_back(std::to_string(h.score[i]) + ": " + std::to_string(h.good[i]));
        if (h.bad[i]) bad.push_back(std::to_string(h.score[i]) + ": " + std::to_string(h.bad[i]));
    }
    std::string s = "{";
    join_to(s, good);
    s += "}\n{";
    join_to(s, bad);
    s += "}";
    return s;
}

std::string component_coverage(const std::vector<ReadSpans>& components) {
    std::vector<std::string> component_strings;
    for (const ReadSpans& reads : components) {
        std::vector<std::pair<uint32_t, bool>> endpoints;   // Endpoint
        for (const auto& r : reads) {
            endpoints.emplace_back(r.first, true);
            endpoints.emplace_back(r.second, false);
        }
        std::sort(endpoints.begin(), endpoints.end());
        std::map<int, int> result;
        int current_coverage = 0;
        int prev_pos = -1;
        for (const auto& endpoint : endpoints) {
            // (endpoint.first - prev_pos): uint32_t - int, evaluated in uint32_t, added to an int (:52, :55)
            const uint32_t d = endpoint.first - (uint32_t)prev_pos;
            if (endpoint.second) {
                current_coverage++;
                int& v = result.insert({current_coverage, 0}).first->second;
                v = (int)((uint32_t)v + d);
            } else {
                int& v = result.insert({current_coverage, 0}).first->second;
                v = (int)((uint32_t)v + d);
                current_coverage--;
            }
            prev_pos = (int)endpoint.first;
        }
        std::vector<std::string> coverage_strings;
        for (const auto& cb : result)
            coverage_strings.push_back("(" + std::to_string(cb.first) + ", " + std::to_string(cb.second) + ")");
        std::string s = "[";
        join_to(s, coverage_strings);
        s += "]";
        component_strings.push_back(std::move(s));
    }
    std::string s = "[";
    join_to(s, component_strings);
    s += "]";
    return s;
}

std::string spectral_graph(const std::vector<SpectralEdge>& connections,
                           const std::function<int32_t(uint32_t)>& first_category,
                           const std::vector<std::vector<uint32_t>>& partition) {
    std::vector<std::string> conn_strings, category_strings;
    for (const SpectralEdge& c : connections) {
        conn_strings.push_back("(" + std::to_string(c.x) + ", " + std::to_string(c.y) + ", " + std::to_string(c.score) + ")");
        category_strings.push_back("(" + std::to_string(c.x) + ", " + std::to_string(first_category(c.x)) + ")");
        category_strings.push_back("(" + std::to_string(c.y) + ", " + std::to_string(first_category(c.y)) + ")");
    }
    std::string input = "[";
    join_to(input, conn_strings);
    input += "]\n[";
    join_to(input, category_strings);
    input += "]\n";
    std::vector<std::string> component_strings;
    for (const auto& comp : partition) {
        std::vector<std::string> temp;
        for (uint32_t id : comp) temp.push_back(std::to_string(id));
        std::string s = "[";
        join_to(s, temp);
        s += "]";
        component_strings.push_back(std::move(s));
    }
    input += "[";
    join_to(input, component_strings);
    input += "]\n";
    return input;
}

}  // namespace hgah
