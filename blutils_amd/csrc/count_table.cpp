// The feature x sample count table of blu_consensus_extras.count_table_path (include/blu_pipeline.h): the
// parser to CSR, and the join of its rows with the run's queries on their keys.  Host code: the file is small next to the
// hit table (one line per representative sequence), and the counting itself is the device's (report_kernel.hip).
#include <unordered_map>

#include "pipeline_internal.h"

namespace blu {
namespace {

int parse_error(const char* path, uint64_t line, uint64_t column, const char* what) {
    set_error("count table %s: line %llu, column %llu: %s", path, (unsigned long long)line, (unsigned long long)column, what);
    return BLU_ERR_PARSE;
}

// the cells of one line (no line end in it)
void split_tabs(std::string_view line, std::vector<std::string_view>& cells) {
    cells.clear();
    for (size_t at = 0;;) {
        const size_t tab = line.find('\t', at);
        cells.push_back(line.substr(at, tab == std::string_view::npos ? std::string_view::npos : tab - at));
        if (tab == std::string_view::npos) return;
        at = tab + 1;
    }
}

// ASCII digits, optionally '.' and one or more zeros; the value below 2^32
bool cell_value(std::string_view c, uint32_t* out) {
    size_t i = 0;
    uint64_t v = 0;
    while (i < c.size() && c[i] >= '0' && c[i] <= '9') {
        v = v * 10 + (uint64_t)(c[i] - '0');
        if (v >> 32) return false;
        ++i;
    }
    if (i == 0) return false;
    if (i < c.size()) {
        if (c[i] != '.' || i + 1 == c.size()) return false;
        for (++i; i < c.size(); ++i) if (c[i] != '0') return false;
    }
    *out = (uint32_t)v;
    return true;
}

std::string_view key_of(std::string_view name) { return name.substr(0, name.find(';')); }

}  // namespace

int parse_count_table(const char* path, CountTable& t) {
    MappedFile f;
    if (!f.open(path)) { set_error("cannot read the count table %s", path); return BLU_ERR_IO; }
    const std::string_view text(f.data, f.size);
    std::vector<std::string_view> cells;
    std::vector<uint32_t> rank;          // header column -> sample id (its position in ascending byte order)
    bool have_header = false;
    uint64_t line_no = 0;
    t.row_ptr.assign(1, 0);
    for (size_t at = 0; at < text.size();) {
        const size_t nl = text.find('\n', at);
        std::string_view line = text.substr(at, nl == std::string_view::npos ? std::string_view::npos : nl - at);
        at = nl == std::string_view::npos ? text.size() : nl + 1;
        ++line_no;
        if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
        if (line.empty()) continue;
        if (!have_header) {
            if (line[0] == '#' && line.find('\t') == std::string_view::npos) continue;   // a comment
            split_tabs(line, cells);
            if (cells.size() < 2) return parse_error(path, line_no, 2, "the header names no sample");
            std::unordered_map<std::string_view, uint32_t> seen;
            for (size_t c = 1; c < cells.size(); ++c) {
                if (cells[c].empty()) return parse_error(path, line_no, c + 1, "an empty sample name");
                if (!seen.emplace(cells[c], (uint32_t)c).second) return parse_error(path, line_no, c + 1, "a sample name for the second time");
            }
            const uint32_t ns = (uint32_t)cells.size() - 1;
            std::vector<uint32_t> order(ns);
            for (uint32_t i = 0; i < ns; ++i) order[i] = i;
            std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cells[a + 1] < cells[b + 1]; });
            rank.resize(ns);
            t.samples.resize(ns);
            for (uint32_t k = 0; k < ns; ++k) { rank[order[k]] = k; t.samples[k] = std::string(cells[order[k] + 1]); }
            have_header = true;
            continue;
        }
        split_tabs(line, cells);
        const size_t ns = t.samples.size();
        if (cells.size() < ns + 1) return parse_error(path, line_no, cells.size() + 1, "the row is short of a cell");
        if (cells.size() > ns + 1) return parse_error(path, line_no, ns + 2, "the row has a cell no sample heads");
        uint64_t sum = 0;
        for (size_t c = 1; c <= ns; ++c) {
            uint32_t v = 0;
            if (!cell_value(cells[c], &v)) return parse_error(path, line_no, c + 1, "a cell is not a whole number below 2^32 (digits, optionally `.0`)");
            if (v) { t.sample.push_back(rank[c - 1]); t.count.push_back(v); sum += v; }
        }
        t.row_names.emplace_back(cells[0]);
        t.row_sum.push_back(sum);
        t.row_ptr.push_back(t.sample.size());
    }
    if (!have_header) return parse_error(path, line_no + 1, 1, "no header line");
    return BLU_OK;
}

int join_count_table(const CountTable& t, const std::vector<std::string>& query_names, const std::vector<std::string>& extra,
                     CountJoin& j, blu_count_table_stats* st) {
    const size_t n_rows = t.row_names.size(), nq = query_names.size(), ns = t.samples.size();
    std::unordered_map<std::string_view, uint32_t> row_of;
    row_of.reserve(n_rows * 2);
    for (size_t i = 0; i < n_rows; ++i) {
        if (t.row_sum[i] >> 32) { set_error("count table: row `%s`: its counts add up to 2^32 or more", t.row_names[i].c_str()); return BLU_ERR_INVALID_ARG; }
        const auto it = row_of.emplace(key_of(t.row_names[i]), (uint32_t)i);
        if (!it.second) {
            set_error("count table: rows `%s` and `%s` have one key", t.row_names[it.first->second].c_str(), t.row_names[i].c_str());
            return BLU_ERR_INVALID_ARG;
        }
    }
    // the row of every query (with hits, then header-only); a key two queries share, or one no row has, fails here
    std::unordered_map<std::string_view, uint32_t> query_of;
    query_of.reserve((nq + extra.size()) * 2);
    std::vector<uint8_t> taken(n_rows, 0);
    j.row_ptr.assign(1, 0);
    j.row_ptr.reserve(nq + 1);
    j.weight.assign(nq, 0);
    j.unclassified.assign(ns, 0);
    j.unclassified_total = 0;
    auto name_at = [&](size_t k) -> const std::string& { return k < nq ? query_names[k] : extra[k - nq]; };
    for (size_t k = 0; k < nq + extra.size(); ++k) {
        const std::string& name = name_at(k);
        const std::string_view key = key_of(name);
        const auto seen = query_of.emplace(key, (uint32_t)k);
        if (!seen.second) {
            set_error("count table: queries `%s` and `%s` have one key", name_at(seen.first->second).c_str(), name.c_str());
            return BLU_ERR_INVALID_ARG;
        }
        const auto row = row_of.find(key);
        if (row == row_of.end()) { set_error("count table: no row for query `%s`", name.c_str()); return BLU_ERR_INVALID_ARG; }
        const uint32_t i = row->second;
        taken[i] = 1;
        if (k < nq) {
            j.sample.insert(j.sample.end(), t.sample.begin() + t.row_ptr[i], t.sample.begin() + t.row_ptr[i + 1]);
            j.count.insert(j.count.end(), t.count.begin() + t.row_ptr[i], t.count.begin() + t.row_ptr[i + 1]);
            j.row_ptr.push_back(j.sample.size());
            j.weight[k] = (uint32_t)t.row_sum[i];
        } else {
            // a header without hits: unclassified in every sample it was counted in
            for (uint64_t e = t.row_ptr[i]; e < t.row_ptr[i + 1]; ++e) j.unclassified[t.sample[e]] += t.count[e];
            j.unclassified_total += t.row_sum[i];
        }
    }
    uint64_t n_left = 0;
    for (size_t i = 0; i < n_rows; ++i) {
        if (taken[i]) continue;
        // a representative BLAST gave no line for
        ++n_left;
        for (uint64_t e = t.row_ptr[i]; e < t.row_ptr[i + 1]; ++e) j.unclassified[t.sample[e]] += t.count[e];
        j.unclassified_total += t.row_sum[i];
    }
    if (st) *st = blu_count_table_stats{n_rows, ns, n_rows - n_left, n_left};
    return BLU_OK;
}

}  // namespace blu
