// `build-distances` on the host (include/blu_pipeline.h): the features of a sample-table file at one rank as
// CSR, the rendering of a distance matrix from the pair integers, and the chain of the two around blu_sample_distances.  The
// file is small next to what precedes it in a run (one line per path); the pairwise pass is the device's (distance_kernel.hip).
// With a depth the chain has a step more: the features are rarefied on the device first (rarefy_kernel.hip) and
// the rarefied table is rendered here too.  `build-diversity` takes the same features to blu_sample_alpha
// (alpha_kernel.hip) and renders its integers here.
#include "pipeline_internal.h"

namespace blu {
namespace {

int malformed(const char* path, uint64_t line, const char* fmt, unsigned long long a = 0, unsigned long long b = 0) {
    char what[256];
    snprintf(what, sizeof what, fmt, a, b);
    set_error("sample table %s: line %llu: %s", path, (unsigned long long)line, what);
    return BLU_ERR_PARSE;
}

void split_tabs(std::string_view line, std::vector<std::string_view>& cells) {
    cells.clear();
    for (size_t at = 0;;) {
        const size_t tab = line.find('\t', at);
        cells.push_back(line.substr(at, tab == std::string_view::npos ? std::string_view::npos : tab - at));
        if (tab == std::string_view::npos) return;
        at = tab + 1;
    }
}

// ASCII digits, the value below 2^64
bool cell_u64(std::string_view c, uint64_t* out) {
    if (c.empty()) return false;
    unsigned __int128 v = 0;
    for (char ch : c) {
        if (ch < '0' || ch > '9') return false;
        v = v * 10 + (unsigned)(ch - '0');
        if (v >> 64) return false;
    }
    *out = (uint64_t)v;
    return true;
}

struct Row {
    uint64_t line;                  // 1-based line of the file
    std::string_view rank, taxonomy;
    int64_t parent = -1;            // row index, -1 = top-level
    std::vector<uint64_t> clade;    // [n_samples]; becomes the direct counts once the children are subtracted
};

struct Feature { std::string text; std::vector<uint64_t> cells; };

char* copy_text(std::string_view s) {
    char* p = (char*)malloc(s.size() + 1);
    if (!p) throw std::bad_alloc();
    memcpy(p, s.data(), s.size());
    p[s.size()] = 0;
    return p;
}

template <class T>
T* array_of(size_t n) {
    T* p = (T*)calloc(n ? n : 1, sizeof(T));
    if (!p) throw std::bad_alloc();
    return p;
}

int features_from_table(const char* path, const char* rank_arg, uint32_t flags, blu_distance_features* out) {
    if (flags & ~BLU_DISTANCE_DROP_UNCLASSIFIED) { set_error("build-distances: unknown bits in the flags"); return BLU_ERR_INVALID_ARG; }
    MappedFile f;
    if (!f.open(path)) { set_error("cannot read the sample table %s", path); return BLU_ERR_IO; }
    const std::string_view text(f.data, f.size);
    std::vector<std::string_view> cells;
    std::vector<std::string> names;
    std::vector<Row> rows;
    std::vector<uint64_t> fixed[2];                 // unclassified, unplaced
    std::unordered_map<std::string_view, uint32_t> row_of;
    bool have_header = false;
    uint64_t line_no = 0;
    size_t ns = 0;
    for (size_t at = 0; at < text.size();) {
        const size_t nl = text.find('\n', at);
        const std::string_view line = text.substr(at, nl == std::string_view::npos ? std::string_view::npos : nl - at);
        at = nl == std::string_view::npos ? text.size() : nl + 1;
        ++line_no;
        split_tabs(line, cells);
        if (!have_header) {
            if (cells.size() < 5 || cells[0] != "#rank" || cells[1] != "identifier" || cells[2] != "taxonomy" || cells[3] != "total")
                return malformed(path, line_no, "not the header `#rank identifier taxonomy total <sample>...` with at least one sample");
            for (size_t c = 4; c < cells.size(); ++c) names.emplace_back(cells[c]);
            ns = names.size();
            have_header = true;
            continue;
        }
        if (cells.size() != ns + 4) return malformed(path, line_no, "%llu cells where the header's samples ask for %llu", cells.size(), ns + 4);
        std::vector<uint64_t> per(ns);
        uint64_t total = 0;
        unsigned __int128 sum = 0;
        if (!cell_u64(cells[3], &total)) return malformed(path, line_no, "`total` is not a whole number below 2^64");
        for (size_t s = 0; s < ns; ++s) {
            if (!cell_u64(cells[4 + s], &per[s])) return malformed(path, line_no, "cell %llu is not a whole number below 2^64", s + 5);
            sum += per[s];
        }
        if (sum != (unsigned __int128)total) return malformed(path, line_no, "`total` %llu is not the sum of the line's cells", total);
        if (cells[0] == "-" && cells[2].empty() && (cells[1] == "unclassified" || cells[1] == "unplaced")) {
            std::vector<uint64_t>& slot = fixed[cells[1] == "unplaced" ? 1 : 0];
            if (!slot.empty()) return malformed(path, line_no, "the fixed row for the second time");
            slot = std::move(per);
            continue;
        }
        if (cells[2].empty()) return malformed(path, line_no, "a row without a taxonomy that is neither `- unclassified` nor `- unplaced`");
        if (rows.size() >= 0xFFFFFFFFull) return malformed(path, line_no, "2^32 rows or more");
        if (!row_of.emplace(cells[2], (uint32_t)rows.size()).second) return malformed(path, line_no, "a taxonomy for the second time");
        rows.push_back(Row{line_no, cells[0], cells[2], -1, std::move(per)});
    }
    if (!have_header) return malformed(path, 1, "no header line");
    for (auto& v : fixed) if (v.empty()) v.assign(ns, 0);

    // the expected per-sample sums, from the clade cells as read; then parents, and the direct counts in place
    std::vector<unsigned __int128> expect(ns, 0);
    for (size_t s = 0; s < ns; ++s) if (!(flags & BLU_DISTANCE_DROP_UNCLASSIFIED)) expect[s] = (unsigned __int128)fixed[0][s] + fixed[1][s];
    for (Row& r : rows) {
        const size_t semi = r.taxonomy.rfind(';');
        if (semi == std::string_view::npos) {
            for (size_t s = 0; s < ns; ++s) expect[s] += r.clade[s];
            continue;
        }
        const auto it = row_of.find(r.taxonomy.substr(0, semi));
        if (it == row_of.end()) return malformed(path, r.line, "the row's parent is missing");
        r.parent = it->second;
    }
    // rule (a) needs the clade cells of rank-R rows: taken before the subtraction
    const bool ranked = rank_arg != nullptr;
    const std::string want = ranked ? canonical_display(rank_arg) : std::string();
    std::vector<uint8_t> is_r(rows.size(), 0), under_r(rows.size(), 0);
    if (ranked) {
        bool any = false;
        for (size_t i = 0; i < rows.size(); ++i) any |= (is_r[i] = rows[i].rank == want);
        if (!any) { set_error("build-distances: no row of %s has the rank `%s`", path, rank_arg); return BLU_ERR_INVALID_ARG; }
        for (size_t i = 0; i < rows.size(); ++i)
            for (int64_t p = rows[i].parent; p >= 0 && !under_r[i]; p = rows[(size_t)p].parent) under_r[i] = is_r[(size_t)p] || under_r[(size_t)p];
    }
    std::vector<Feature> feats;
    if (!(flags & BLU_DISTANCE_DROP_UNCLASSIFIED)) {
        feats.push_back(Feature{"unclassified", fixed[0]});
        feats.push_back(Feature{"unplaced", fixed[1]});
    }
    std::vector<int64_t> feat_of(rows.size(), -1);
    for (size_t i = 0; i < rows.size(); ++i) {
        if (under_r[i]) continue;
        feat_of[i] = (int64_t)feats.size();
        feats.push_back(Feature{std::string(rows[i].taxonomy), rows[i].clade});
    }
    // direct = clade - the children's clade: a child takes its cells out of its parent's feature unless the parent keeps its
    // clade (rule (a)); checked on every row, featured or not
    {
        std::vector<std::vector<uint64_t>> left(rows.size());
        for (size_t i = 0; i < rows.size(); ++i) left[i] = rows[i].clade;
        for (size_t i = 0; i < rows.size(); ++i) {
            if (rows[i].parent < 0) continue;
            const size_t p = (size_t)rows[i].parent;
            for (size_t s = 0; s < ns; ++s) {
                if (left[p][s] < rows[i].clade[s])
                    return malformed(path, rows[p].line, "a negative direct count in sample column %llu: the children's counts pass the row's", s + 1);
                left[p][s] -= rows[i].clade[s];
            }
        }
        for (size_t i = 0; i < rows.size(); ++i)
            if (feat_of[i] >= 0 && !is_r[i]) feats[(size_t)feat_of[i]].cells = std::move(left[i]);
    }
    // the invariant, then the CSR without the all-zero features
    for (size_t s = 0; s < ns; ++s) {
        unsigned __int128 sum = 0;
        for (const Feature& ft : feats) sum += ft.cells[s];
        if (sum != expect[s]) {
            set_error("build-distances: %s: the features of sample column %llu do not add up to its unclassified, unplaced and top-level counts",
                      path, (unsigned long long)(s + 1));
            return BLU_ERR_PARSE;
        }
    }
    size_t kept = 0, nnz = 0;
    for (const Feature& ft : feats) {
        size_t n = 0;
        for (uint64_t v : ft.cells) n += v != 0;
        kept += n != 0;
        nnz += n;
    }
    out->n_features = kept;
    out->n_samples = (uint32_t)ns;
    out->n_dropped = feats.size() - kept;
    out->row_ptr = array_of<uint64_t>(kept + 1);
    out->sample = array_of<uint32_t>(nnz);
    out->count = array_of<uint64_t>(nnz);
    out->sample_names = array_of<char*>(ns);
    out->feature_text = array_of<char*>(kept);
    for (size_t s = 0; s < ns; ++s) out->sample_names[s] = copy_text(names[s]);
    size_t k = 0, e = 0;
    for (const Feature& ft : feats) {
        const size_t e0 = e;
        for (size_t s = 0; s < ns; ++s) if (ft.cells[s]) { out->sample[e] = (uint32_t)s; out->count[e] = ft.cells[s]; ++e; }
        if (e == e0) continue;
        out->feature_text[k] = copy_text(ft.text);
        out->row_ptr[++k] = e;
    }
    return BLU_OK;
}

// num / den with six decimals, half up; den > 0, num <= den
void six_decimals(std::string& o, uint64_t num, uint64_t den) {
    const unsigned __int128 q = ((unsigned __int128)num * 1000000u + den / 2) / den;
    char b[32];
    const int n = snprintf(b, sizeof b, "%llu.%06llu", (unsigned long long)(q / 1000000u), (unsigned long long)(q % 1000000u));
    o.append(b, (size_t)n);
}

int render_text(int metric, const char* const* names, const blu_sample_distance& d, std::string& o) {
    if (metric != BLU_DISTANCE_BRAY_CURTIS && metric != BLU_DISTANCE_JACCARD) { set_error("build-distances: unknown metric %d", metric); return BLU_ERR_INVALID_ARG; }
    const uint64_t S = d.n_samples;
    if (!names || (S && (!d.total || !d.richness || !d.min_sum || !d.shared))) { set_error("build-distances: null argument"); return BLU_ERR_INVALID_ARG; }
    for (uint64_t a = 0; a < S; ++a) { o.push_back('\t'); o += names[a]; }
    o.push_back('\n');
    for (uint64_t a = 0; a < S; ++a) {
        o += names[a];
        for (uint64_t b = 0; b < S; ++b) {
            o.push_back('\t');
            uint64_t num, den;
            if (metric == BLU_DISTANCE_BRAY_CURTIS) {
                if (d.total[a] >> 63 || d.total[b] >> 63) { set_error("build-distances: a total of 2^63 or more"); return BLU_ERR_INVALID_ARG; }
                den = d.total[a] + d.total[b];
                const uint64_t c = d.min_sum[a * S + b];
                if (c > den / 2) { set_error("build-distances: min_sum[%llu][%llu] passes the smaller total", (unsigned long long)a, (unsigned long long)b); return BLU_ERR_INVALID_ARG; }
                num = den - 2 * c;
            } else {
                const uint64_t i = d.shared[a * S + b], both = (uint64_t)d.richness[a] + d.richness[b];
                if (2 * i > both) { set_error("build-distances: shared[%llu][%llu] passes the smaller richness", (unsigned long long)a, (unsigned long long)b); return BLU_ERR_INVALID_ARG; }
                den = both - i;
                num = den - i;
            }
            if (den == 0) o += "nan";
            else six_decimals(o, num, den);
        }
        o.push_back('\n');
    }
    return BLU_OK;
}

// features -> rarefied features -> pair integers of the kept samples -> both texts, then both files
int rarefied_matrix(const blu_distance_features& ft, const blu_distance_desc& desc, int metric, uint64_t depth, uint64_t seed, const char* out_path,
                    const char* table_out, blu_rarefied& rf, blu_sample_distance& d, blu_distance_stats2* stats2) {
    const uint32_t S = ft.n_samples;
    {
        std::unordered_map<std::string_view, uint32_t> column_of;
        for (uint32_t a = 0; a < S; ++a) {
            const auto at = column_of.emplace(ft.sample_names[a], a);
            if (!at.second) {
                set_error("build-distances: sample columns %u and %u are both named `%s`: a sample's draw goes by its name", at.first->second + 1, a + 1,
                          ft.sample_names[a]);
                return BLU_ERR_INVALID_ARG;
            }
        }
    }
    std::vector<uint64_t> stream(S), total(S, 0);
    for (uint32_t a = 0; a < S; ++a) stream[a] = blu_rarefy_stream(seed, ft.sample_names[a], strlen(ft.sample_names[a]));
    blu_rarefy_desc rd{};
    rd.struct_size = sizeof rd;
    rd.device = desc.device;
    rd.n_features = ft.n_features;
    rd.n_samples = S;
    rd.row_ptr = ft.row_ptr; rd.sample = ft.sample; rd.count = ft.count;
    rd.sample_stream = stream.data();
    rd.depth = depth;
    if (const int rc = blu_sample_rarefy(&rd, &rf)) return rc;
    for (uint64_t e = 0; e < ft.row_ptr[ft.n_features]; ++e) total[ft.sample[e]] += ft.count[e];   // (no wrap: the call above checked)
    if (rf.n_kept == 0) {
        uint32_t top = 0;
        for (uint32_t a = 1; a < S; ++a) if (total[a] > total[top]) top = a;
        set_error("build-distances: no sample reaches the depth %llu: the largest, `%s`, has %llu reads", (unsigned long long)depth,
                  ft.sample_names[top], (unsigned long long)total[top]);
        return BLU_ERR_INVALID_ARG;
    }
    const uint32_t K = rf.n_kept;
    std::vector<const char*> names(K);
    uint64_t reads = 0;
    for (uint32_t k = 0; k < K; ++k) { names[k] = ft.sample_names[rf.kept_sample[k]]; reads += total[rf.kept_sample[k]]; }
    blu_distance_desc kd = desc;
    kd.n_samples = K;
    kd.row_ptr = rf.row_ptr; kd.sample = rf.sample; kd.count = rf.count;
    if (const int rc = blu_sample_distances(&kd, &d)) return rc;
    std::string matrix, table;
    if (const int rc = render_text(metric, names.data(), d, matrix)) return rc;
    uint64_t n_left = 0;
    for (uint64_t f = 0; f < ft.n_features; ++f) n_left += rf.row_ptr[f + 1] != rf.row_ptr[f];
    if (table_out) {
        table = "#feature\ttotal";
        for (uint32_t k = 0; k < K; ++k) { table.push_back('\t'); table += names[k]; }
        table.push_back('\n');
        std::vector<uint64_t> cells(K);
        for (uint64_t f = 0; f < ft.n_features; ++f) {
            if (rf.row_ptr[f + 1] == rf.row_ptr[f]) continue;
            std::fill(cells.begin(), cells.end(), 0);
            uint64_t sum = 0;
            for (uint64_t e = rf.row_ptr[f]; e < rf.row_ptr[f + 1]; ++e) { cells[rf.sample[e]] = rf.count[e]; sum += rf.count[e]; }
            table += ft.feature_text[f];
            table.push_back('\t');
            table += std::to_string(sum);
            for (uint32_t k = 0; k < K; ++k) { table.push_back('\t'); table += std::to_string(cells[k]); }
            table.push_back('\n');
        }
    }
    if (!write_text_file(out_path, matrix)) { set_error("cannot write %s", out_path); return BLU_ERR_IO; }
    if (table_out && !write_text_file(table_out, table)) {
        unlink(out_path);                           // nothing is left behind unless every step succeeded
        set_error("cannot write %s", table_out);
        return BLU_ERR_IO;
    }
    if (stats2)
        *stats2 = blu_distance_stats2{n_left, K, rf.row_ptr[ft.n_features], ft.n_dropped, depth, K, (uint64_t)S - K, ft.n_features - n_left, reads};
    return BLU_OK;
}

// num / den with six decimals, half up, in 128 bits; den > 0 (the quotient may pass 1: chao1)
void six_decimals_wide(std::string& o, unsigned __int128 num, unsigned __int128 den) {
    const unsigned __int128 q = (num * 1000000u + den / 2) / den;
    char b[48];
    const int n = snprintf(b, sizeof b, "%llu.%06llu", (unsigned long long)(q / 1000000u), (unsigned long long)(q % 1000000u));
    o.append(b, (size_t)n);
}

int impossible(const char* name, uint64_t depth, const char* what) {
    set_error("build-diversity: sample `%s` at depth %llu: %s: integers that cannot occur", name, (unsigned long long)depth, what);
    return BLU_ERR_INVALID_ARG;
}

// the alpha file (include/blu_pipeline.h: blu_alpha_render); *rows = its lines after the header
int alpha_text(const char* const* names, const uint64_t* reads, const uint64_t* depths, uint32_t n_depths, const blu_alpha& al, std::string& o,
               uint64_t* rows) {
    const uint64_t S = al.n_samples, NS = al.n_slots;
    if (NS != (n_depths ? n_depths : 1u)) { set_error("build-diversity: %u slots do not go with %u depths", al.n_slots, n_depths); return BLU_ERR_INVALID_ARG; }
    if (S && (!names || !reads || (n_depths && !depths) || !al.present || !al.n || !al.observed || !al.singletons || !al.doubletons || !al.sum_sq ||
              !al.sum_xlog)) {
        set_error("build-diversity: null argument");
        return BLU_ERR_INVALID_ARG;
    }
    o = "#sample\tdepth\treads\tobserved\tsingletons\tdoubletons\tchao1\tsimpson\tshannon\tgoods_coverage\n";
    *rows = 0;
    for (uint64_t a = 0; a < S; ++a) {
        for (uint64_t j = 0; j < NS; ++j) {
            const uint64_t at = a * NS + j;
            if (!al.present[at]) continue;
            const uint64_t depth = n_depths ? depths[j] : reads[a];
            const uint64_t n = al.n[at], obs = al.observed[at], f1 = al.singletons[at], f2 = al.doubletons[at];
            const unsigned __int128 n2 = (unsigned __int128)n * n;
            if (n >> 32) return impossible(names[a], depth, "n is 2^32 or more");
            if (al.sum_sq[at] > n2) return impossible(names[a], depth, "sum_sq passes n^2");
            if (f1 > n) return impossible(names[a], depth, "singletons pass n");
            if (f1 + f2 > obs) return impossible(names[a], depth, "singletons and doubletons pass observed");
            if (obs > n) return impossible(names[a], depth, "observed passes n");
            o += names[a];
            for (uint64_t v : {depth, reads[a], obs, f1, f2}) { o.push_back('\t'); o += std::to_string(v); }
            o.push_back('\t');
            const unsigned __int128 twice = 2 * ((unsigned __int128)f2 + 1);
            six_decimals_wide(o, (unsigned __int128)obs * twice + (f1 ? (unsigned __int128)f1 * (f1 - 1) : 0), twice);
            if (n == 0) { o += "\tnan\tnan\tnan\n"; ++*rows; continue; }
            o.push_back('\t');
            six_decimals_wide(o, n2 - al.sum_sq[at], n2);
            o.push_back('\t');
            const uint64_t whole = n * blu_alpha_log2(n);                 // (below 2^61)
            six_decimals_wide(o, whole > al.sum_xlog[at] ? whole - al.sum_xlog[at] : 0, (unsigned __int128)n << 24);
            o.push_back('\t');
            six_decimals_wide(o, n - f1, n);
            o.push_back('\n');
            ++*rows;
        }
    }
    return BLU_OK;
}

// features -> alpha integers -> the text, then the file
int alpha_table(const char* table_path, const char* rank, uint32_t flags, int device, const char* out_path, const blu_alpha_options* opt,
                blu_distance_features& ft, blu_alpha& al, blu_alpha_stats* stats) {
    if (const int rc = blu_distance_features_from_table(table_path, rank, flags, &ft)) return rc;
    const uint32_t S = ft.n_samples, K = opt ? opt->n_depths : 0u;
    if (K) {
        std::unordered_map<std::string_view, uint32_t> column_of;
        for (uint32_t a = 0; a < S; ++a) {
            const auto at = column_of.emplace(ft.sample_names[a], a);
            if (!at.second) {
                set_error("build-diversity: sample columns %u and %u are both named `%s`: a sample's draw goes by its name", at.first->second + 1, a + 1,
                          ft.sample_names[a]);
                return BLU_ERR_INVALID_ARG;
            }
        }
    }
    std::vector<uint64_t> stream(S), total(S, 0);
    for (uint32_t a = 0; a < S; ++a) stream[a] = blu_rarefy_stream(opt ? opt->seed : 0, ft.sample_names[a], strlen(ft.sample_names[a]));
    blu_alpha_desc ad{};
    ad.struct_size = sizeof ad;
    ad.device = device;
    ad.n_features = ft.n_features;
    ad.n_samples = S;
    ad.n_depths = K;
    ad.row_ptr = ft.row_ptr; ad.sample = ft.sample; ad.count = ft.count;
    ad.sample_stream = stream.data();
    ad.depths = K ? opt->depths : nullptr;
    if (const int rc = blu_sample_alpha(&ad, &al)) return rc;
    for (uint64_t e = 0; e < ft.row_ptr[ft.n_features]; ++e) total[ft.sample[e]] += ft.count[e];   // (no wrap: the call above checked)
    if (K) {
        uint32_t top = 0;
        for (uint32_t a = 1; a < S; ++a) if (total[a] > total[top]) top = a;
        if (total[top] < opt->depths[0]) {
            set_error("build-diversity: no sample reaches the first depth %llu: the largest, `%s`, has %llu reads", (unsigned long long)opt->depths[0],
                      ft.sample_names[top], (unsigned long long)total[top]);
            return BLU_ERR_INVALID_ARG;
        }
    }
    std::string text;
    uint64_t rows = 0;
    if (const int rc = alpha_text(ft.sample_names, total.data(), ad.depths, K, al, text, &rows)) return rc;
    if (!write_text_file(out_path, text)) { set_error("cannot write %s", out_path); return BLU_ERR_IO; }
    if (stats) *stats = blu_alpha_stats{ft.n_features, S, ft.row_ptr[ft.n_features], ft.n_dropped, K, rows, al.t_device_ms};
    return BLU_OK;
}

}  // namespace
}  // namespace blu

using namespace blu;

extern "C" {

int blu_alpha_render(const char* const* names, const uint64_t* reads, const uint64_t* depths, uint32_t n_depths, const blu_alpha* integers,
                     const char* out_path) {
    if (!integers || !out_path) { set_error("build-diversity: null argument"); return BLU_ERR_INVALID_ARG; }
    try {
        std::string text;
        uint64_t rows = 0;
        if (const int rc = alpha_text(names, reads, depths, n_depths, *integers, text, &rows)) return rc;
        if (!write_text_file(out_path, text)) { set_error("cannot write %s", out_path); return BLU_ERR_IO; }
        return BLU_OK;
    } catch (const std::bad_alloc&) { set_error("build-diversity: out of memory"); return BLU_ERR_ALLOC; }
}

int blu_alpha_table_file(const char* table_path, const char* rank, uint32_t flags, int device, const char* out_path,
                         const blu_alpha_options* options, blu_alpha_stats* stats) {
    if (!table_path || !out_path) { set_error("build-diversity: null argument"); return BLU_ERR_INVALID_ARG; }
    if (options && options->struct_size != sizeof(blu_alpha_options)) {
        set_error("build-diversity: options struct_size %llu is not one this library knows (%llu)", (unsigned long long)options->struct_size,
                  (unsigned long long)sizeof(blu_alpha_options));
        return BLU_ERR_INVALID_ARG;
    }
    if (options && options->n_depths && !options->depths) { set_error("build-diversity: depths is NULL"); return BLU_ERR_INVALID_ARG; }
    blu_distance_features ft{};
    blu_alpha al{};
    struct Free {
        blu_distance_features& f; blu_alpha& a;
        ~Free() { blu_distance_features_free(&f); blu_alpha_free(&a); }
    } guard{ft, al};
    try {
        return alpha_table(table_path, rank, flags, device, out_path, options, ft, al, stats);
    } catch (const std::bad_alloc&) { set_error("build-diversity: out of memory"); return BLU_ERR_ALLOC; }
}

void blu_distance_features_free(blu_distance_features* ft) {
    if (!ft) return;
    if (ft->sample_names) for (uint32_t s = 0; s < ft->n_samples; ++s) free(ft->sample_names[s]);
    if (ft->feature_text) for (uint64_t k = 0; k < ft->n_features; ++k) free(ft->feature_text[k]);
    free(ft->sample_names); free(ft->feature_text); free(ft->row_ptr); free(ft->sample); free(ft->count);
    memset(ft, 0, sizeof *ft);
}

int blu_distance_features_from_table(const char* table_path, const char* rank, uint32_t flags, blu_distance_features* out) {
    if (!table_path || !out) { set_error("build-distances: null argument"); return BLU_ERR_INVALID_ARG; }
    memset(out, 0, sizeof *out);
    try {
        const int rc = features_from_table(table_path, rank, flags, out);
        if (rc != BLU_OK) blu_distance_features_free(out);
        return rc;
    } catch (const std::bad_alloc&) {
        blu_distance_features_free(out);
        set_error("build-distances: out of memory");
        return BLU_ERR_ALLOC;
    }
}

int blu_distance_render(int metric, const char* const* names, const blu_sample_distance* integers, const char* out_path) {
    if (!integers || !out_path) { set_error("build-distances: null argument"); return BLU_ERR_INVALID_ARG; }
    try {
        std::string text;
        if (const int rc = render_text(metric, names, *integers, text)) return rc;
        if (!write_text_file(out_path, text)) { set_error("cannot write %s", out_path); return BLU_ERR_IO; }
        return BLU_OK;
    } catch (const std::bad_alloc&) { set_error("build-distances: out of memory"); return BLU_ERR_ALLOC; }
}

int blu_distance_matrix_file(const char* table_path, const char* rank, int metric, uint32_t flags, int device, const char* out_path,
                             blu_distance_stats* stats) {
    blu_distance_stats2 st{};
    const int rc = blu_distance_matrix_file_with(table_path, rank, metric, flags, device, out_path, nullptr, &st);
    if (rc == BLU_OK && stats) *stats = blu_distance_stats{st.n_features, st.n_samples, st.n_nonzeros, st.n_dropped};
    return rc;
}

int blu_distance_matrix_file_with(const char* table_path, const char* rank, int metric, uint32_t flags, int device, const char* out_path,
                                  const blu_distance_options* options, blu_distance_stats2* stats2) {
    if (!table_path || !out_path) { set_error("build-distances: null argument"); return BLU_ERR_INVALID_ARG; }
    if (metric != BLU_DISTANCE_BRAY_CURTIS && metric != BLU_DISTANCE_JACCARD) { set_error("build-distances: unknown metric %d", metric); return BLU_ERR_INVALID_ARG; }
    if (options && options->struct_size != sizeof(blu_distance_options)) {
        set_error("build-distances: options struct_size %llu is not one this library knows (%llu)", (unsigned long long)options->struct_size,
                  (unsigned long long)sizeof(blu_distance_options));
        return BLU_ERR_INVALID_ARG;
    }
    const uint64_t depth = options ? options->depth : 0;
    const char* table_out = options ? options->rarefied_table_path : nullptr;
    if (!depth && table_out) { set_error("build-distances: a rarefied table needs a depth"); return BLU_ERR_INVALID_ARG; }
    blu_distance_features ft{};
    blu_rarefied rf{};
    blu_sample_distance d{};
    struct Free {
        blu_distance_features& f; blu_rarefied& r; blu_sample_distance& d;
        ~Free() { blu_distance_features_free(&f); blu_rarefied_free(&r); blu_sample_distance_free(&d); }
    } guard{ft, rf, d};
    if (const int rc = blu_distance_features_from_table(table_path, rank, flags, &ft)) return rc;
    blu_distance_desc desc{};
    desc.struct_size = sizeof desc;
    desc.device = device;
    desc.n_features = ft.n_features;
    desc.n_samples = ft.n_samples;
    desc.row_ptr = ft.row_ptr; desc.sample = ft.sample; desc.count = ft.count;
    if (!depth) {
        if (const int rc = blu_sample_distances(&desc, &d)) return rc;
        if (const int rc = blu_distance_render(metric, ft.sample_names, &d, out_path)) return rc;
        if (stats2) *stats2 = blu_distance_stats2{ft.n_features, ft.n_samples, ft.row_ptr[ft.n_features], ft.n_dropped, 0, ft.n_samples, 0, 0, 0};
        return BLU_OK;
    }
    try {
        return rarefied_matrix(ft, desc, metric, depth, options->seed, out_path, table_out, rf, d, stats2);
    } catch (const std::bad_alloc&) { set_error("build-distances: out of memory"); return BLU_ERR_ALLOC; }
}

}  // extern "C"
