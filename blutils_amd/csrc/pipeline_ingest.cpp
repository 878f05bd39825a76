// The CPU ingest of the pipeline (include/blu_pipeline.h): outfmt-6 text -> grouped SoA columns.  Reference files followed:
//   core/src/use_cases/build_consensus_identities/mod.rs:134-221   fold_results_by_query: per-query rows in file order, quotes stripped, bit_score f64 -> i64
//   mod.rs:226-244   outfmt-6 schema (13 tab-separated columns, no header)
// Third-party edge not pinned by any reference test: polars' CSV number parsing (strtod/strtoll here).
#include <deque>
#include <iterator>

#include "pipeline_internal.h"

namespace blu {
namespace {

std::string strip_quotes(std::string_view v) {   // mod.rs:169-172 `.replace("\"", "")`
    std::string s;
    s.reserve(v.size());
    for (char c : v) if (c != '"') s.push_back(c);
    return s;
}

// Parses one number the way the columns are typed (mod.rs:226-244).  Fast path for what BLAST prints — [-]digits[.digits]
// with at most 15 significant digits: mantissa and 10^k are exact doubles and IEEE division rounds correctly (Clinger),
// so the value is the one strtod / Rust's parser gives.  Everything else (exponents, '+', inf/nan, longer digit
// strings) takes std::from_chars, then strtod for the forms from_chars refuses.  (libstdc++ 11's from_chars for
// doubles goes through strtod with a locale switch: ~4 of them per row were most of the ingest time.)
bool parse_f64(std::string_view v, double* out) {
    const char* b = v.data();
    const char* e = b + v.size();
    if (b == e) return false;
    {
        static const double p10[16] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15};
        const char* p = b;
        const bool neg = p < e && *p == '-';
        if (neg) ++p;
        uint64_t mant = 0;
        int digits = 0, frac = 0;
        const char* d0 = p;
        while (p < e && (unsigned)(*p - '0') < 10u) { mant = mant * 10 + (unsigned)(*p - '0'); ++p; ++digits; }
        const bool had_int = p > d0;
        if (p < e && *p == '.') {
            ++p;
            const char* f0 = p;
            while (p < e && (unsigned)(*p - '0') < 10u) { mant = mant * 10 + (unsigned)(*p - '0'); ++p; ++digits; ++frac; }
            if (!had_int && p == f0) digits = 99;      // "." alone: not a number
        } else if (!had_int) digits = 99;
        if (p == e && digits <= 15) {
            const double x = (double)mant / p10[frac];
            *out = neg ? -x : x;
            return true;
        }
    }
    auto r = std::from_chars(b, e, *out);
    if (r.ec == std::errc() && r.ptr == e) return true;
    if ((unsigned char)*b <= ' ') return false;         // (strtod would skip leading blanks; a typed CSV column does not)
    for (const char* q = b; q < e; ++q) if (*q == 'x' || *q == 'X') return false;   // (nor does it read C's hexadecimal floats)
    std::string tmp(v);
    char* endp = nullptr;
    *out = strtod(tmp.c_str(), &endp);
    return endp == tmp.c_str() + tmp.size();            // the whole field, or it is not a number ("12abc")
}

// subject_taxid and align_length are Int64 columns of the reference's schema (mod.rs:226-244): [+-]digits and nothing
// else — no fraction, exponent or blanks ("12.7" fails there, so it fails here)
bool parse_i64(std::string_view v, int64_t* out) {
    const char* p = v.data();
    const char* e = p + v.size();
    if (p == e) return false;
    const bool neg = *p == '-';
    if (*p == '-' || *p == '+') ++p;
    if (p == e) return false;
    uint64_t x = 0;                                        // the whole i64 range, leading zeros included; beyond it: not an Int64
    const uint64_t lim = neg ? (1ull << 63) : (1ull << 63) - 1;
    for (; p < e; ++p) {
        const unsigned d = (unsigned)(*p - '0');
        if (d >= 10u) return false;
        if (x > (lim - d) / 10) return false;
        x = x * 10 + d;
    }
    *out = neg ? (int64_t)(0 - x) : (int64_t)x;
    return true;
}

struct RawRow { uint32_t lq, la, tax; int32_t bs, aln; double pid; };   // lq / la: the chunk's own query / accession ids

inline uint64_t hash_sv(std::string_view s) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (s.size() * 0xFF51AFD7ED558CCDull);
    const char* p = s.data();
    size_t n = s.size();
    while (n >= 8) { uint64_t w; memcpy(&w, p, 8); h = (h ^ w) * 0x9FB21C651E98DF25ull; h ^= h >> 29; p += 8; n -= 8; }
    if (n) { uint64_t w = 0; memcpy(&w, p, n); h = (h ^ w) * 0x9FB21C651E98DF25ull; h ^= h >> 29; }
    return h ^ (h >> 32);
}

// string_view -> dense id in first-appearance order; open addressing.  A slot holds the hash, the id and the first 16
// bytes of the key, so a lookup of a short key (accessions, query ids) touches one cache line and never the text it
// was first seen in (random reads into a mapped file of many GB: that, not the parsing, was the ingest's cost).  Keys
// are views into the mapped file or into an arena that outlives the dictionary.
struct SvDict {
    struct Slot { uint64_t hash; uint32_t id1, len; char head[16]; };   // id1 = id + 1, 0 = empty
    std::vector<Slot> slot;
    std::vector<std::string_view> keys;      // by id
    uint64_t mask;
    explicit SvDict(size_t cap = 1024) : slot(cap, Slot{0, 0, 0, {0}}), mask(cap - 1) {}
    void grow() {
        std::vector<Slot> ns(slot.size() * 2, Slot{0, 0, 0, {0}});
        const uint64_t nm = ns.size() - 1;
        for (const Slot& e : slot) {
            if (!e.id1) continue;
            uint64_t i = e.hash & nm;
            while (ns[i].id1) i = (i + 1) & nm;
            ns[i] = e;
        }
        slot.swap(ns);
        mask = nm;
    }
    uint32_t intern(std::string_view s, bool* is_new = nullptr) {
        const uint64_t h = hash_sv(s);
        const size_t hl = s.size() < 16 ? s.size() : 16;
        uint64_t i = h & mask;
        while (slot[i].id1) {
            const Slot& e = slot[i];
            if (e.hash == h && e.len == s.size() && memcmp(e.head, s.data(), hl) == 0 &&
                (s.size() <= 16 || memcmp(keys[e.id1 - 1].data() + 16, s.data() + 16, s.size() - 16) == 0)) {
                if (is_new) *is_new = false;
                return e.id1 - 1;
            }
            i = (i + 1) & mask;
        }
        const uint32_t id = (uint32_t)keys.size();
        Slot& e = slot[i];
        e.hash = h; e.id1 = id + 1; e.len = (uint32_t)s.size();
        memcpy(e.head, s.data(), hl);
        keys.push_back(s);
        if (is_new) *is_new = true;
        if (keys.size() * 3 > slot.size() * 2) grow();
        return id;
    }
};

// One worker's share of the file: [begin, end) starts and ends on line boundaries.
struct Chunk {
    const char* begin = nullptr;
    const char* end = nullptr;
    std::vector<RawRow> rows;
    SvDict queries, accs;                    // this chunk's dictionaries (quotes already stripped)
    std::deque<std::string> arena;           // owned copies of the fields that had quotes in them
    std::vector<uint32_t> q_count;           // rows per local query
    std::vector<uint32_t> qmap, amap;        // local id -> global query id / global accession rank
    std::vector<uint64_t> at;                // local query -> next row slot in the grouped table
    std::vector<std::string_view> acc_sorted;
    uint64_t unmatched = 0, first_line = 0, n_lines = 0;
    uint64_t n_data_lines = 0, n_kept = 0;   // under a hit or taxon filter: non-empty lines, lines kept
    uint64_t n_below = 0;                    // under a query cover: lines below it, whatever the other filters say
    uint64_t n_not_only = 0;                 // under a taxon filter: lines failing only the only list, and per exclude element
    std::vector<uint64_t> excluded_by;       // the lines whose first matching element it is
    int rc = BLU_OK;
    std::string err;
    std::string_view clean(std::string_view v) {   // mod.rs:169-172 `.replace("\"", "")`
        if (!memchr(v.data(), '"', v.size())) return v;
        arena.push_back(strip_quotes(v));
        return arena.back();
    }
};

// The hit filter's predicate (include/blu_pipeline.h: blu_hit_filter) on the values parse_f64 / parse_i64 gave: plain IEEE
// comparisons, so a NaN on either side fails.  This is the definition the GPU parser's decisions are held to.
inline bool filter_keeps(const blu_hit_filter& f, double pid, int64_t aln, double e_value, double bs) {
    if ((f.mask & BLU_FILTER_MIN_PERC_IDENTITY) && !(pid >= f.min_perc_identity)) return false;
    if ((f.mask & BLU_FILTER_MIN_ALIGN_LENGTH) && !(aln >= f.min_align_length)) return false;
    if ((f.mask & BLU_FILTER_MAX_E_VALUE) && !(e_value <= f.max_e_value)) return false;
    if ((f.mask & BLU_FILTER_MIN_BIT_SCORE) && !(bs >= f.min_bit_score)) return false;   // as written: before the truncation
    return true;
}

// The query cover's predicate (include/blu_pipeline.h: blu_query_cover) on the values parse_i64 gave, each in
// 0 .. 2^31 - 1 and qlen > 0: 64-bit integers, both sides below 2^48.  a: the percent column, or qstart; b: qend.  This is the
// definition the GPU parser's decisions are held to.
inline bool cover_keeps(const blu_query_cover& c, int64_t a, int64_t b, int64_t qlen) {
    if (c.source != BLU_QUERY_COVER_QLEN) return a * 1000 >= (int64_t)c.min_cover_milli;
    const int64_t span = (a > b ? a - b : b - a) + 1;
    return span * 100000 >= (int64_t)c.min_cover_milli * qlen;
}

// LAID_OUT: the seven role fields are read through `lay` (blu_table_layout: a checked layout that is not the
// reference's own); otherwise the positions are the reference's literals and lay is not looked at.  cov (LAID_OUT only): the
// query cover, whose fields are read through their own columns.
template <bool LAID_OUT>
void parse_chunk_as(Chunk& c, const Db& db, const char* path, const blu_hit_filter* flt, const TaxonCodes* taxa, const blu_table_layout* lay,
                    const blu_query_cover* cov) {
    constexpr int MAX_COLS = LAID_OUT ? (int)BLU_TABLE_LAYOUT_MAX_COLUMNS : 13;
    const int n_cols = LAID_OUT ? (int)lay->n_columns : 13;
    const int c_q = LAID_OUT ? (int)lay->query : 0, c_a = LAID_OUT ? (int)lay->accession : 1, c_tax = LAID_OUT ? (int)lay->taxid : 2;
    const int c_pid = LAID_OUT ? (int)lay->perc_identity : 3, c_aln = LAID_OUT ? (int)lay->align_length : 4;
    const int c_e = LAID_OUT ? (int)lay->e_value : 11, c_bs = LAID_OUT ? (int)lay->bit_score : 12;   // (no e-value column: refused before the parse)
    const bool tax_list = LAID_OUT && lay->taxid_is_list != 0;
    if (taxa) c.excluded_by.assign(taxa->n_exclude, 0);
    const char* p = c.begin;
    uint64_t line_no = 0;
    c.rows.reserve((size_t)(c.end - c.begin) / 96 + 16);
    std::string_view last_q_raw, last_a_raw;
    uint32_t last_q = 0, last_a = 0;
    bool have_last = false;
    while (p < c.end) {
        const char* nl = (const char*)memchr(p, '\n', (size_t)(c.end - p));
        const char* le = nl ? nl : c.end;
        const char* lend = le;
        if (lend > p && lend[-1] == '\r') --lend;
        ++line_no;
        if (lend > p) {
            std::string_view col[MAX_COLS];
            int nc = 0;
            const char* s = p;
            while (nc < n_cols) {
                const char* tab = (const char*)memchr(s, '\t', (size_t)(lend - s));
                const char* ce = tab ? tab : lend;
                col[nc++] = std::string_view(s, (size_t)(ce - s));
                if (!tab) break;
                s = tab + 1;
            }
            char msg[512];
            if (nc < n_cols) {
                snprintf(msg, sizeof msg, "line %llu(+%llu) of %s has %d columns, outfmt-6 with %d expected (%s)",
                         (unsigned long long)line_no, (unsigned long long)c.first_line, path, nc, n_cols, LAID_OUT ? "the table layout" : "mod.rs:226-244");
                c.rc = BLU_ERR_PARSE; c.err = msg; return;
            }
            double pid, bs;
            int64_t taxid_i, aln;
            std::string_view tax_field = col[c_tax];
            if (tax_list) tax_field = tax_field.substr(0, tax_field.find(';'));   // `staxids`: the id before the first ';'
            if (!parse_i64(tax_field, &taxid_i) || !parse_f64(col[c_pid], &pid) || !parse_i64(col[c_aln], &aln) || !parse_f64(col[c_bs], &bs)) {
                snprintf(msg, sizeof msg, "line %llu(+%llu) of %s: numeric column does not parse", (unsigned long long)line_no,
                         (unsigned long long)c.first_line, path);
                c.rc = BLU_ERR_PARSE; c.err = msg; return;
            }
            const double bs_t = std::trunc(bs);               // mod.rs:184 AnyValue::Float64 -> try_extract::<i64>
            if (!(bs_t >= -2147483648.0 && bs_t <= 2147483647.0) || aln < INT32_MIN || aln > INT32_MAX) {
                snprintf(msg, sizeof msg, "line %llu(+%llu) of %s: bit_score / align_length outside the 32-bit range of the engine columns",
                         (unsigned long long)line_no, (unsigned long long)c.first_line, path);
                c.rc = BLU_ERR_PARSE; c.err = msg; return;
            }
            if (flt || taxa || (LAID_OUT && cov)) {           // (validated like every line; dropped before it reaches a dictionary)
                double ev = 0;
                if (flt && (flt->mask & BLU_FILTER_MAX_E_VALUE) && !parse_f64(col[c_e], &ev)) {
                    snprintf(msg, sizeof msg, "line %llu(+%llu) of %s: numeric column does not parse (e_value)", (unsigned long long)line_no,
                             (unsigned long long)c.first_line, path);
                    c.rc = BLU_ERR_PARSE; c.err = msg; return;
                }
                bool covered = true;
                if constexpr (LAID_OUT) if (cov) {            // the coverage fields: Int64 like `length`, 0 .. 2^31 - 1, qlen > 0 — on every line
                    const bool by_len = cov->source == BLU_QUERY_COVER_QLEN;
                    const uint32_t at[3] = {by_len ? cov->qstart : cov->cover_column, cov->qend, cov->qlen};
                    static const char* const what[3] = {"qstart", "qend", "qlen"};
                    int64_t v[3] = {0, 0, 1};
                    for (int k = 0; k < (by_len ? 3 : 1); ++k) {
                        const char* const name = by_len ? what[k] : cov->source == BLU_QUERY_COVER_QCOVS ? "qcovs" : "qcovhsp";
                        if (!parse_i64(col[at[k]], &v[k])) {
                            snprintf(msg, sizeof msg, "line %llu(+%llu) of %s: query cover column does not parse (%s)", (unsigned long long)line_no,
                                     (unsigned long long)c.first_line, path, name);
                            c.rc = BLU_ERR_PARSE; c.err = msg; return;
                        }
                        if (v[k] < 0 || v[k] > INT32_MAX || (k == 2 && v[k] == 0)) {
                            snprintf(msg, sizeof msg, "line %llu(+%llu) of %s: query cover column outside its range (%s: 0 to 2^31 - 1, qlen above 0)",
                                     (unsigned long long)line_no, (unsigned long long)c.first_line, path, name);
                            c.rc = BLU_ERR_PARSE; c.err = msg; return;
                        }
                    }
                    covered = cover_keeps(*cov, v[0], v[1], v[2]);
                    if (!covered) ++c.n_below;                // (whatever the other filters say)
                }
                ++c.n_data_lines;
                // the taxon verdict: the code of the row the line joins to, first and whatever the thresholds say.
                // This is the definition the GPU parser's verdicts are held to.
                uint16_t code = 0;
                if (taxa) {
                    const uint32_t row = db.row_of.find_or(taxid_i, BLU_UNMATCHED_TAXID);
                    code = row == BLU_UNMATCHED_TAXID ? taxa->unmatched : taxa->code[row];
                    if (code == TAXON_NOT_ONLY) ++c.n_not_only;
                    else if (code) ++c.excluded_by[code - 1];
                }
                if (code || !covered || (flt && !filter_keeps(*flt, pid, aln, ev, bs))) { p = nl ? nl + 1 : c.end; continue; }
                ++c.n_kept;
            }
            RawRow r;
            // rows of one query usually sit next to each other: the previous row's ids are tried before the dictionaries
            if (!have_last || col[c_q] != last_q_raw) {
                bool is_new = false;
                last_q = c.queries.intern(c.clean(col[c_q]), &is_new);
                if (is_new) c.q_count.push_back(0);
                last_q_raw = col[c_q];
            }
            if (!have_last || col[c_a] != last_a_raw) { last_a = c.accs.intern(c.clean(col[c_a])); last_a_raw = col[c_a]; }
            have_last = true;
            ++c.q_count[last_q];
            r.lq = last_q; r.la = last_a;
            r.tax = db.row_of.find_or(taxid_i, BLU_UNMATCHED_TAXID);    // left join (mod.rs:72-76)
            if (r.tax == BLU_UNMATCHED_TAXID) ++c.unmatched;
            r.bs = (int32_t)bs_t; r.aln = (int32_t)aln; r.pid = pid;
            c.rows.push_back(r);
            if (!db.dup_rows.empty()) {                                  // a subject listed m times: m joined rows, in the DB's order
                auto dit = db.dup_rows.find(taxid_i);
                if (dit != db.dup_rows.end())
                    for (size_t k = 1; k < dit->second.size(); ++k) { r.tax = dit->second[k]; c.rows.push_back(r); ++c.q_count[last_q]; }
            }
        }
        p = nl ? nl + 1 : c.end;
    }
    c.n_lines = line_no;
    // this chunk's accessions in byte order (String::cmp), for the merge below
    c.acc_sorted = c.accs.keys;
    std::sort(c.acc_sorted.begin(), c.acc_sorted.end());
}
void parse_chunk(Chunk& c, const Db& db, const char* path, const blu_hit_filter* flt = nullptr, const TaxonCodes* taxa = nullptr,
                 const blu_table_layout* lay = nullptr, const blu_query_cover* cov = nullptr) {
    if (lay) parse_chunk_as<true>(c, db, path, flt, taxa, lay, cov);
    else parse_chunk_as<false>(c, db, path, flt, taxa, nullptr, nullptr);
}

// ---- taxon filter (include/blu_pipeline.h: blu_taxon_filter): the two lists -> one code per taxonomy row.
// An element `RANK__IDENTIFIER` names the node a lineage element of that spelling is interned as (Display(rank), identifier);
// an identifier ending in '*' is a prefix over the identifiers of that rank.  Only nodes that some lineage holds count (a
// node met in front of a bad element of a refused lineage is in the dictionary but in no lineage).
struct TaxonElement { std::string rank, ident; bool prefix = false; };

int parse_taxon_element(const char* text, const char* list, TaxonElement* el) {
    const std::string s = text ? text : "";
    const size_t sep = s.find("__");
    if (sep == std::string::npos || sep == 0 || sep + 2 >= s.size() || s.find("__", sep + 2) != std::string::npos) {
        set_error("taxon filter: %s element `%s` is not RANK__IDENTIFIER (two non-empty parts around one `__`)", list, s.c_str());
        return BLU_ERR_INVALID_ARG;
    }
    el->rank = canonical_display(s.substr(0, sep));
    el->ident = s.substr(sep + 2);
    el->prefix = el->ident.back() == '*';
    if (el->prefix) el->ident.pop_back();
    return BLU_OK;
}

}  // namespace

int taxon_codes(const Db& db, const blu_taxon_filter& f, unsigned nthreads, TaxonCodes& tc) {
    if ((f.n_exclude && !f.exclude) || (f.n_only && !f.only)) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    if (f.n_exclude > BLU_TAXON_FILTER_MAX_EXCLUDE) {
        set_error("taxon filter: %llu exclude elements, at most %u are taken", (unsigned long long)f.n_exclude, BLU_TAXON_FILTER_MAX_EXCLUDE);
        return BLU_ERR_INVALID_ARG;
    }
    const size_t n_ex = (size_t)f.n_exclude, n_el = n_ex + (size_t)f.n_only, n_nodes = db.node_ident.size(), n_tax = db.taxid.size();
    // the elements: exact ones by key, patterns by rank; the first of equal spellings stands for all of them
    std::vector<TaxonElement> els(n_el);
    std::unordered_map<std::string, std::vector<uint32_t>> exact, patterns;   // key / rank -> element indices (exclude first, list order)
    for (size_t k = 0; k < n_el; ++k) {
        const bool ex = k < n_ex;
        if (int rc = parse_taxon_element(ex ? f.exclude[k] : f.only[k - n_ex], ex ? "exclude" : "only", &els[k]); rc != BLU_OK) return rc;
        if (els[k].prefix) patterns[els[k].rank].push_back((uint32_t)k);
        else exact[els[k].rank + '\x1f' + els[k].ident].push_back((uint32_t)k);
    }
    std::vector<uint8_t> in_lineage(n_nodes, 0);
    for (uint32_t node : db.lin_node) in_lineage[node] = 1;
    // per node: the first exclude element that names it (+ 1), whether an only element names it; per element: named a node?
    std::vector<uint16_t> node_ex(n_nodes, 0);
    std::vector<uint8_t> node_only(n_nodes, 0);
    if (nthreads < 1 || n_nodes + n_tax < (1u << 16)) nthreads = 1;
    std::vector<std::vector<uint8_t>> found(nthreads, std::vector<uint8_t>(n_el, 0));
    parallel_for(nthreads, nthreads, [&](unsigned t) {
        std::string key;
        auto take = [&](uint32_t node, uint32_t k) {
            found[t][k] = 1;
            if (k >= n_ex) node_only[node] = 1;
            else if (!node_ex[node] || k + 1 < node_ex[node]) node_ex[node] = (uint16_t)(k + 1);
        };
        for (size_t node = n_nodes * t / nthreads; node < n_nodes * (t + 1) / nthreads; ++node) {
            if (!in_lineage[node]) continue;
            const std::string& rank = db.rank_display[db.node_rank[node]];
            const std::string& ident = db.node_ident[node];
            if (!exact.empty()) {
                key.assign(rank); key.push_back('\x1f'); key += ident;
                if (auto it = exact.find(key); it != exact.end()) for (uint32_t k : it->second) take((uint32_t)node, k);
            }
            if (!patterns.empty())
                if (auto it = patterns.find(rank); it != patterns.end())
                    for (uint32_t k : it->second)
                        if (ident.size() >= els[k].ident.size() && memcmp(ident.data(), els[k].ident.data(), els[k].ident.size()) == 0) take((uint32_t)node, k);
        }
    });
    for (size_t k = 0; k < n_el; ++k) {
        bool any = false;
        for (unsigned t = 0; t < nthreads && !any; ++t) any = found[t][k] != 0;
        if (!any) {
            set_error("taxon filter: %s element `%s` names no taxon of the taxonomies file", k < n_ex ? "exclude" : "only", k < n_ex ? f.exclude[k] : f.only[k - n_ex]);
            return BLU_ERR_INVALID_ARG;
        }
    }
    // one pass over the CSR: a row's code from its nodes (a bad row's lineage is empty: no elements)
    tc.code.assign(n_tax, 0);
    tc.unmatched = f.n_only ? TAXON_NOT_ONLY : 0;
    tc.n_exclude = (uint32_t)n_ex;
    tc.n_excluded = tc.n_not_only = 0;
    tc.excluded_by.assign(n_ex, 0);
    const bool has_only = f.n_only != 0;
    parallel_for(nthreads, nthreads, [&](unsigned t) {
        for (size_t r = n_tax * t / nthreads; r < n_tax * (t + 1) / nthreads; ++r) {
            uint16_t ex = 0;
            bool only = false;
            for (uint64_t j = db.lin_off[r]; j < db.lin_off[r + 1]; ++j) {
                const uint32_t node = db.lin_node[j];
                if (node_ex[node] && (!ex || node_ex[node] < ex)) ex = node_ex[node];
                only |= node_only[node] != 0;
            }
            tc.code[r] = ex ? ex : (has_only && !only ? TAXON_NOT_ONLY : (uint16_t)0);
        }
    });
    return BLU_OK;
}

// ---- the table's column layout (include/blu_pipeline.h: blu_table_layout) ----------------------------------------
int check_table_layout(const blu_table_layout* lay, const blu_hit_filter* flt, const blu_table_layout** use, bool keep_reference) {
    *use = nullptr;
    if (!lay) return BLU_OK;
    if (lay->struct_size != sizeof(blu_table_layout)) {
        set_error("table layout: struct_size %u is not a blu_table_layout this library knows (%zu bytes)", lay->struct_size, sizeof(blu_table_layout));
        return BLU_ERR_INVALID_ARG;
    }
    if (lay->n_columns < 1 || lay->n_columns > BLU_TABLE_LAYOUT_MAX_COLUMNS) {
        set_error("table layout: %u columns, 1 to %u are taken", lay->n_columns, BLU_TABLE_LAYOUT_MAX_COLUMNS);
        return BLU_ERR_INVALID_ARG;
    }
    const uint32_t role[7] = {lay->query, lay->accession, lay->taxid, lay->perc_identity, lay->align_length, lay->bit_score, lay->e_value};
    static const char* const name[7] = {"query", "accession", "taxid", "perc_identity", "align_length", "bit_score", "e_value"};
    for (int a = 0; a < 7; ++a) {
        if (a == 6 && role[a] == BLU_TABLE_LAYOUT_NO_COLUMN) continue;
        if (role[a] >= lay->n_columns) { set_error("table layout: the %s column %u is not one of the %u columns", name[a], role[a], lay->n_columns); return BLU_ERR_INVALID_ARG; }
        for (int b = 0; b < a; ++b)
            if (role[a] == role[b]) { set_error("table layout: %s and %s are both column %u", name[b], name[a], role[a]); return BLU_ERR_INVALID_ARG; }
    }
    if (lay->taxid_is_list > 1) { set_error("table layout: taxid_is_list is %u, 0 or 1 is taken", lay->taxid_is_list); return BLU_ERR_INVALID_ARG; }
    if (lay->e_value == BLU_TABLE_LAYOUT_NO_COLUMN && flt && (flt->mask & BLU_FILTER_MAX_E_VALUE)) {
        set_error("table layout: the e-value threshold (max_e_value) needs an `evalue` column and the layout names none");
        return BLU_ERR_INVALID_ARG;
    }
    const bool reference = lay->n_columns == 13 && lay->query == 0 && lay->accession == 1 && lay->taxid == 2 && lay->perc_identity == 3 &&
                           lay->align_length == 4 && lay->e_value == 11 && lay->bit_score == 12 && !lay->taxid_is_list;
    if (!reference || keep_reference) *use = lay;
    return BLU_OK;
}

// ---- the query cover (include/blu_pipeline.h: blu_query_cover) ------------------------------------------------------
int check_query_cover(const blu_query_cover* cov, const blu_table_layout* lay) {
    if (!cov) return BLU_OK;
    if (cov->struct_size != sizeof(blu_query_cover)) {
        set_error("query cover: struct_size %u is not a blu_query_cover this library knows (%zu bytes)", cov->struct_size, sizeof(blu_query_cover));
        return BLU_ERR_INVALID_ARG;
    }
    if (cov->stats) *cov->stats = blu_query_cover_stats{};
    if (cov->source != BLU_QUERY_COVER_QCOVHSP && cov->source != BLU_QUERY_COVER_QLEN && cov->source != BLU_QUERY_COVER_QCOVS) {
        set_error("query cover: source %u is not qcovhsp (1), qlen (2) or qcovs (3); blu_query_cover_parse resolves `auto`", cov->source);
        return BLU_ERR_INVALID_ARG;
    }
    if (cov->min_cover_milli > BLU_QUERY_COVER_MAX_MILLI) {
        set_error("query cover: %u thousandths of a percent, 0 to %u are taken", cov->min_cover_milli, BLU_QUERY_COVER_MAX_MILLI);
        return BLU_ERR_INVALID_ARG;
    }
    if (!lay) {
        set_error("query cover: the reference's columns hold no query length; the table's columns have to be named (a blu_table_layout)");
        return BLU_ERR_INVALID_ARG;
    }
    if (lay->struct_size != sizeof(blu_table_layout)) return BLU_OK;   // (check_table_layout refuses it, with its own message)
    const bool by_len = cov->source == BLU_QUERY_COVER_QLEN;
    const uint32_t at[3] = {by_len ? cov->qstart : cov->cover_column, cov->qend, cov->qlen};
    static const char* const len_name[3] = {"qstart", "qend", "qlen"};
    const uint32_t role[7] = {lay->query, lay->accession, lay->taxid, lay->perc_identity, lay->align_length, lay->bit_score, lay->e_value};
    static const char* const role_name[7] = {"query", "accession", "taxid", "perc_identity", "align_length", "bit_score", "e_value"};
    for (int k = 0; k < (by_len ? 3 : 1); ++k) {
        const char* const name = by_len ? len_name[k] : "cover";
        if (at[k] >= lay->n_columns) { set_error("query cover: the %s column %u is not one of the %u columns", name, at[k], lay->n_columns); return BLU_ERR_INVALID_ARG; }
        for (int r = 0; r < 7; ++r)
            if (at[k] == role[r]) { set_error("query cover: the %s column %u is the layout's %s column", name, at[k], role_name[r]); return BLU_ERR_INVALID_ARG; }
        for (int j = 0; j < k; ++j)
            if (at[k] == at[j]) { set_error("query cover: %s and %s are both column %u", len_name[j], name, at[k]); return BLU_ERR_INVALID_ARG; }
    }
    return BLU_OK;
}

namespace {
// BLAST's format string -> layout (blu_table_layout_parse).  Roles by priority, not by position: the first name of each list
// that the string holds.
int spec_columns(const char* spec, std::vector<std::string>& cols) {
    static const char* const STD[12] = {"qseqid", "sseqid", "pident", "length", "mismatch", "gapopen", "qstart", "qend", "sstart", "send", "evalue", "bitscore"};
    const char* p = spec;
    bool first = true;
    while (*p) {
        if (*p == ' ' || *p == '\t') { ++p; continue; }
        const char* b = p;
        while (*p && *p != ' ' && *p != '\t') ++p;
        const std::string tok(b, (size_t)(p - b));
        bool digits = true, word = true;
        for (unsigned char ch : tok) {
            if (ch - '0' >= 10u) digits = false;
            if (!(ch - '0' < 10u || (ch | 32) - 'a' < 26u || ch == '_')) word = false;
        }
        if (!word) { set_error("blast outfmt: `%s` is not a format specifier (letters, digits and `_`)", tok.c_str()); return BLU_ERR_INVALID_ARG; }
        const bool lead = first;
        first = false;
        if (lead && digits) {
            if (tok != "6") { set_error("blast outfmt: format `%s` is not read, only the tabular format 6", tok.c_str()); return BLU_ERR_INVALID_ARG; }
            continue;
        }
        if (tok == "std") cols.insert(cols.end(), STD, STD + 12);
        else cols.push_back(tok);
    }
    if (cols.size() > BLU_TABLE_LAYOUT_MAX_COLUMNS) {
        set_error("blast outfmt: %zu columns, at most %u are taken (the first beyond them: `%s`)", cols.size(), BLU_TABLE_LAYOUT_MAX_COLUMNS,
                  cols[BLU_TABLE_LAYOUT_MAX_COLUMNS].c_str());
        return BLU_ERR_INVALID_ARG;
    }
    for (size_t a = 0; a < cols.size(); ++a)
        for (size_t b = 0; b < a; ++b)
            if (cols[a] == cols[b]) { set_error("blast outfmt: `%s` is named twice (columns %zu and %zu)", cols[a].c_str(), b + 1, a + 1); return BLU_ERR_INVALID_ARG; }
    return BLU_OK;
}
int parse_layout_spec(const char* spec, blu_table_layout* out, std::vector<std::string>* names = nullptr) {
    std::vector<std::string> cols;
    if (int rc = spec_columns(spec, cols)) return rc;
    auto find = [&](std::initializer_list<const char*> names, uint32_t* at, const char** which) {
        for (const char* n : names)
            for (size_t k = 0; k < cols.size(); ++k)
                if (cols[k] == n) { *at = (uint32_t)k; if (which) *which = n; return true; }
        return false;
    };
    blu_table_layout l{};
    l.struct_size = sizeof l;
    l.n_columns = (uint32_t)cols.size();
    const char* tax_name = nullptr;
    if (!find({"qseqid", "qacc", "qaccver"}, &l.query, nullptr)) { set_error("blast outfmt: no query column: one of `qseqid`, `qacc`, `qaccver` is needed"); return BLU_ERR_INVALID_ARG; }
    if (!find({"saccver", "sacc", "sseqid"}, &l.accession, nullptr)) { set_error("blast outfmt: no subject column: one of `saccver`, `sacc`, `sseqid` is needed"); return BLU_ERR_INVALID_ARG; }
    if (!find({"staxid", "staxids"}, &l.taxid, &tax_name)) { set_error("blast outfmt: no taxid column: `staxid` or `staxids` is needed"); return BLU_ERR_INVALID_ARG; }
    if (!find({"pident"}, &l.perc_identity, nullptr)) { set_error("blast outfmt: no `pident` column"); return BLU_ERR_INVALID_ARG; }
    if (!find({"length"}, &l.align_length, nullptr)) { set_error("blast outfmt: no `length` column"); return BLU_ERR_INVALID_ARG; }
    if (!find({"bitscore"}, &l.bit_score, nullptr)) { set_error("blast outfmt: no `bitscore` column"); return BLU_ERR_INVALID_ARG; }
    if (!find({"evalue"}, &l.e_value, nullptr)) l.e_value = BLU_TABLE_LAYOUT_NO_COLUMN;
    l.taxid_is_list = strcmp(tax_name, "staxids") == 0 ? 1u : 0u;
    *out = l;
    if (names) names->swap(cols);
    return BLU_OK;
}

// The format string and a source -> the cover's columns (blu_query_cover_parse): the string goes through parse_layout_spec first,
// so every refusal of the layout is a refusal here.
int parse_cover_spec(const char* spec, uint32_t source, blu_query_cover* out) {
    blu_table_layout lay{};
    std::vector<std::string> cols;
    if (int rc = parse_layout_spec(spec, &lay, &cols)) return rc;
    if (source > BLU_QUERY_COVER_QCOVS) { set_error("query cover: source %u is not auto (0), qcovhsp (1), qlen (2) or qcovs (3)", source); return BLU_ERR_INVALID_ARG; }
    auto at = [&](const char* n) { for (size_t k = 0; k < cols.size(); ++k) if (cols[k] == n) return (uint32_t)k; return BLU_TABLE_LAYOUT_NO_COLUMN; };
    const uint32_t c_hsp = at("qcovhsp"), c_s = at("qstart"), c_e = at("qend"), c_l = at("qlen"), c_subj = at("qcovs");
    const bool has_len = c_s != BLU_TABLE_LAYOUT_NO_COLUMN && c_e != BLU_TABLE_LAYOUT_NO_COLUMN && c_l != BLU_TABLE_LAYOUT_NO_COLUMN;
    std::string missing;                            // of what the asked source reads
    auto lacks = [&](uint32_t c, const char* n) { if (c == BLU_TABLE_LAYOUT_NO_COLUMN) { missing += missing.empty() ? "`" : ", `"; missing += n; missing += '`'; } };
    if (source == BLU_QUERY_COVER_AUTO) {
        source = c_hsp != BLU_TABLE_LAYOUT_NO_COLUMN ? BLU_QUERY_COVER_QCOVHSP : has_len ? BLU_QUERY_COVER_QLEN : c_subj != BLU_TABLE_LAYOUT_NO_COLUMN ? BLU_QUERY_COVER_QCOVS : BLU_QUERY_COVER_AUTO;
        if (source == BLU_QUERY_COVER_AUTO) {
            lacks(c_hsp, "qcovhsp"); lacks(c_s, "qstart"); lacks(c_e, "qend"); lacks(c_l, "qlen"); lacks(c_subj, "qcovs");
            set_error("query cover: the format string names no coverage column: `qcovhsp`, or `qstart` `qend` `qlen`, or `qcovs` is needed; it lacks %s", missing.c_str());
            return BLU_ERR_INVALID_ARG;
        }
    }
    if (source == BLU_QUERY_COVER_QCOVHSP) lacks(c_hsp, "qcovhsp");
    else if (source == BLU_QUERY_COVER_QCOVS) lacks(c_subj, "qcovs");
    else { lacks(c_s, "qstart"); lacks(c_e, "qend"); lacks(c_l, "qlen"); }
    if (!missing.empty()) {
        set_error("query cover: source %s needs %s, and the format string lacks %s", source == BLU_QUERY_COVER_QCOVHSP ? "qcovhsp" : source == BLU_QUERY_COVER_QCOVS ? "qcovs" : "qlen",
                  source == BLU_QUERY_COVER_QLEN ? "`qstart`, `qend` and `qlen`" : "that column", missing.c_str());
        return BLU_ERR_INVALID_ARG;
    }
    const bool by_len = source == BLU_QUERY_COVER_QLEN;
    out->source = source;
    out->cover_column = by_len ? BLU_TABLE_LAYOUT_NO_COLUMN : source == BLU_QUERY_COVER_QCOVHSP ? c_hsp : c_subj;
    out->qstart = by_len ? c_s : BLU_TABLE_LAYOUT_NO_COLUMN; out->qend = by_len ? c_e : BLU_TABLE_LAYOUT_NO_COLUMN; out->qlen = by_len ? c_l : BLU_TABLE_LAYOUT_NO_COLUMN;
    out->reserved = 0;
    return BLU_OK;
}
}  // namespace

static thread_local int g_last_ingest_path = 0;   // 0 = CPU parser, 1 = GPU parser (blu_last_ingest_path)

// a2 + a4 + a5: outfmt-6 text -> SoA columns.  The file is cut into line-aligned chunks; each worker parses its
// chunk (numbers, tab scanning, the taxid join) and interns query / accession strings in dictionaries of its own.
// Afterwards only the DISTINCT strings are merged — queries in file order (first appearance decides a query's
// position, mod.rs:192-208), accessions by a tree of sorted-list merges (their id is their rank in byte order) —
// and the workers scatter their rows into the grouped table.  The result does not depend on the thread count.
int load_hits(const char* path, const Db& db, HitTable& ht, int device, bool host_columns, const blu_hit_filter* flt, TaxonCodes* taxa,
              const blu_table_layout* lay, const blu_query_cover* cov) {
    g_last_ingest_path = 0;
    if (flt && !(flt->mask & 15u)) flt = nullptr;   // no threshold given: today's path
    if (int rc = check_query_cover(cov, lay)) return rc;
    if (int rc = check_table_layout(lay, flt, &lay, cov != nullptr)) return rc;   // (the reference's own columns: today's path)
    // GPU parser first (ingest_gpu.hip) when a device is given: same columns bit for bit; files it does not handle
    // (quotes, empty lines, unusual numbers), small files and BLU_INGEST=cpu take the CPU path below.  The GPU path
    // reads the file through its descriptor and never maps it.
    {
        const char* mode = getenv("BLU_INGEST");
        struct stat sb;
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0 || fstat(fd, &sb) != 0) { if (fd >= 0) ::close(fd); set_error("Unexpected error occurred on load table: %s", path); return BLU_ERR_IO; }
        const size_t fsize = (size_t)sb.st_size;
        // (a DB that lists a taxid more than once multiplies hit rows in the join: the CPU parser does that)
        const bool want_gpu = device >= 0 && db.dup_rows.empty() && !(mode && strcmp(mode, "cpu") == 0) && (fsize >= (1u << 20) || (mode && strcmp(mode, "gpu") == 0));
        int rc = BLU_INGEST_FALLBACK;
        std::string why;
        if (want_gpu) rc = load_hits_gpu(fd, fsize, db.row_of, device, host_columns, ht, &why, flt, taxa, lay, cov);
        ::close(fd);
        if (want_gpu) {
            if (rc == BLU_OK) { g_last_ingest_path = 1; return BLU_OK; }
            if (rc != BLU_INGEST_FALLBACK) return rc;
            if (getenv("BLU_INGEST_TRACE")) fprintf(stderr, "[ingest] GPU parser declined (%s): CPU path\n", why.c_str());
        }
    }
    MappedFile f;
    if (!f.open(path)) { set_error("Unexpected error occurred on load table: %s", path); return BLU_ERR_IO; }
    const unsigned nthreads = f.size < (1u << 20) ? 1 : worker_threads();
    std::vector<Chunk> chunks(nthreads);
    const char* base = f.data;
    const char* fend = f.data + f.size;
    const char* cur = base;
    for (unsigned t = 0; t < nthreads; ++t) {
        const char* target = t + 1 == nthreads ? fend : base + (f.size / nthreads) * (t + 1);
        if (target < cur) target = cur;
        if (target < fend) {
            const char* nl = (const char*)memchr(target, '\n', (size_t)(fend - target));
            target = nl ? nl + 1 : fend;
        }
        chunks[t].begin = cur;
        chunks[t].end = target;
        cur = target;
    }
    Trace tr{"[ingest]", 22};
    parallel_for(nthreads, nthreads, [&](unsigned t) { parse_chunk(chunks[t], db, path, flt, taxa, lay, cov); });
    tr.lap("parse (parallel)");
    uint64_t lines_before = 0;
    size_t nh = 0;
    if (taxa) { taxa->n_excluded = taxa->n_not_only = 0; taxa->excluded_by.assign(taxa->n_exclude, 0); }
    for (auto& c : chunks) {
        if (c.rc != BLU_OK) { set_error("%s (chunk starting at line %llu)", c.err.c_str(), (unsigned long long)(lines_before + 1)); return c.rc; }
        lines_before += c.n_lines;
        nh += c.rows.size();
        ht.unmatched += c.unmatched;
        ht.n_lines += c.n_data_lines; ht.n_kept += c.n_kept; ht.n_below += c.n_below;
        if (taxa) {
            taxa->n_not_only += c.n_not_only;
            for (uint32_t k = 0; k < taxa->n_exclude; ++k) { taxa->excluded_by[k] += c.excluded_by[k]; taxa->n_excluded += c.excluded_by[k]; }
        }
    }
    if (nh >= 0xFFFFFFFFull) { set_error("more than 2^32 - 2 hit rows in %s", path); return BLU_ERR_INVALID_ARG; }
    // queries: the chunks' distinct names in file order -> global ids, and each chunk's first slot inside every segment
    {
        SvDict global(1u << 16);
        std::vector<uint64_t> per_query;
        std::vector<std::vector<uint64_t>> prior(nthreads);
        for (unsigned t = 0; t < nthreads; ++t) {
            Chunk& c = chunks[t];
            c.qmap.resize(c.queries.keys.size());
            prior[t].resize(c.queries.keys.size());
            for (uint32_t l = 0; l < c.queries.keys.size(); ++l) {
                bool is_new = false;
                const uint32_t g = global.intern(c.queries.keys[l], &is_new);
                if (is_new) { ht.query_names.emplace_back(c.queries.keys[l]); per_query.push_back(0); }
                c.qmap[l] = g;
                prior[t][l] = per_query[g];
                per_query[g] += c.q_count[l];
            }
        }
        const size_t nq = ht.query_names.size();
        ht.seg_off.assign(nq + 1, 0);
        for (size_t q = 0; q < nq; ++q) ht.seg_off[q + 1] = ht.seg_off[q] + per_query[q];
        for (unsigned t = 0; t < nthreads; ++t) {
            Chunk& c = chunks[t];
            c.at.resize(c.qmap.size());
            for (uint32_t l = 0; l < c.qmap.size(); ++l) c.at[l] = ht.seg_off[c.qmap[l]] + prior[t][l];
        }
    }
    tr.lap("queries (merge)");
    // accessions: tree of merges of the chunks' sorted lists; rank in the merged list = acc_rank = index into ht.accessions
    {
        std::vector<std::vector<std::string_view>> lists(nthreads);
        for (unsigned t = 0; t < nthreads; ++t) lists[t] = chunks[t].acc_sorted;
        merge_tree(nthreads, nthreads, [&](unsigned i, unsigned step) {
            std::vector<std::string_view> out;
            out.reserve(lists[i].size() + lists[i + step].size());
            std::set_union(lists[i].begin(), lists[i].end(), lists[i + step].begin(), lists[i + step].end(), std::back_inserter(out));
            lists[i].swap(out);
            std::vector<std::string_view>().swap(lists[i + step]);
        });
        const std::vector<std::string_view>& all = lists[0];
        ht.accessions.resize(all.size());
        parallel_for(nthreads, nthreads, [&](unsigned t) {
            for (size_t k = all.size() * t / nthreads; k < all.size() * (t + 1) / nthreads; ++k) ht.accessions[k].assign(all[k]);
            Chunk& c = chunks[t];
            c.amap.resize(c.accs.keys.size());
            for (uint32_t l = 0; l < c.accs.keys.size(); ++l)
                c.amap[l] = (uint32_t)(std::lower_bound(all.begin(), all.end(), c.accs.keys[l]) - all.begin());
        });
    }
    tr.lap("accessions (merge)");
    // stable grouping: queries in first-appearance order, rows of a query in file order (mod.rs:192-208); the chunks
    // write disjoint slots
    ht.bitscore.resize(nh); ht.align_len.resize(nh); ht.tax_desc_row.resize(nh); ht.acc_rank.resize(nh); ht.pident.resize(nh);
    parallel_for(nthreads, nthreads, [&](unsigned t) {
        Chunk& c = chunks[t];
        for (const RawRow& r : c.rows) {
            const uint64_t d = c.at[r.lq]++;
            ht.bitscore[d] = r.bs; ht.align_len[d] = r.aln; ht.tax_desc_row[d] = r.tax; ht.acc_rank[d] = c.amap[r.la];
            ht.pident[d] = r.pid;
        }
    });
    tr.lap("scatter (parallel)");
    ht.n_hits = nh;
    ht.n_queries = ht.query_names.size();
    return BLU_OK;
}

// The ingest half under a selection, into malloc'd copies of the host columns.
static int ingest_columns_selected(const char* blast_output_file, const char* taxonomies_file, int use_taxid, int device,
                            const blu_table_layout* lay, const blu_query_cover* cov, const blu_hit_selection* selection, blu_ingest_columns* out,
                            blu_hit_selection_stats* stats) {
    Selection sel(selection, stats);
    if (int rc = sel.check()) return rc;
    if (int rc = check_query_cover(cov, lay)) return rc;              // (before any file is opened)
    if (int rc = check_table_layout(lay, sel.flt, &lay, cov != nullptr)) return rc;
    sel.cov = cov;
    Db db;
    int rc = load_db(taxonomies_file, use_taxid != 0, db);
    if (rc != BLU_OK) return rc;
    if ((rc = sel.resolve(db, worker_threads())) != BLU_OK) return rc;
    HitTable ht;
    rc = load_hits(blast_output_file, db, ht, device, true, sel.flt, sel.taxa.get(), lay, cov);
    if (rc != BLU_OK) return rc;
    ht.wait_strings();
    if (!ht.strings_ok) { set_error("out of memory while building the query / accession strings"); return BLU_ERR_ALLOC; }
    sel.loaded(ht);
    if ((rc = sel.on_host_columns(device, ht)) != BLU_OK) return rc;
    const size_t nh = ht.n_hits, nq = ht.n_queries;
    auto dup = [](const void* src, size_t bytes) -> void* { void* p = malloc(bytes ? bytes : 1); if (p && bytes) memcpy(p, src, bytes); return p; };
    auto pack = [](const std::vector<std::string>& v, uint64_t* bytes) -> char* {
        size_t n = 0;
        for (auto& s : v) n += s.size() + 1;
        char* p = (char*)malloc(n ? n : 1);
        if (!p) return nullptr;
        size_t at = 0;
        for (auto& s : v) { memcpy(p + at, s.data(), s.size()); at += s.size(); p[at++] = 0; }
        *bytes = n;
        return p;
    };
    out->n_hits = nh; out->n_queries = nq; out->n_accessions = ht.accessions.size();
    out->seg_off = (uint64_t*)dup(ht.seg_off.data(), (nq + 1) * 8);
    out->bitscore = (int32_t*)dup(ht.bitscore.data(), nh * 4);
    out->align_len = (int32_t*)dup(ht.align_len.data(), nh * 4);
    out->tax_desc_row = (uint32_t*)dup(ht.tax_desc_row.data(), nh * 4);
    out->acc_rank = (uint32_t*)dup(ht.acc_rank.data(), nh * 4);
    out->pident = (double*)dup(ht.pident.data(), nh * 8);
    out->query_names = pack(ht.query_names, &out->query_names_bytes);
    out->accessions = pack(ht.accessions, &out->accessions_bytes);
    if (!out->seg_off || !out->bitscore || !out->align_len || !out->tax_desc_row || !out->acc_rank || !out->pident || !out->query_names || !out->accessions) {
        blu_ingest_columns_free(out);
        set_error("out of memory");
        return BLU_ERR_ALLOC;
    }
    return BLU_OK;
}

}  // namespace blu

using namespace blu;

bool blu::parse_f64_field(const char* p, size_t n, double* out) { return parse_f64(std::string_view(p, n), out); }

extern "C" {

int blu_ingest_only(const char* blast_output_file, const char* taxonomies_file, int use_taxid, blu_pipeline_stats* stats,
                    uint64_t* checksum) {
    return blu_ingest_only_on(blast_output_file, taxonomies_file, use_taxid, -1, stats, checksum);
}

int blu_ingest_only_on(const char* blast_output_file, const char* taxonomies_file, int use_taxid, int device,
                       blu_pipeline_stats* stats, uint64_t* checksum) {
    if (!blast_output_file || !taxonomies_file) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    blu_pipeline_stats st{};
    double t0 = now_s();
    Db db;
    int rc = load_db(taxonomies_file, use_taxid != 0, db);
    if (rc != BLU_OK) return rc;
    st.t_load_db_s = now_s() - t0;
    t0 = now_s();
    HitTable ht;
    rc = load_hits(blast_output_file, db, ht, device);
    if (rc != BLU_OK) return rc;
    st.t_load_hits_s = now_s() - t0;
    st.n_hits = ht.bitscore.size(); st.n_queries = ht.n_queries; st.n_taxids = db.taxid.size(); st.n_unmatched_rows = ht.unmatched;
    if (stats) *stats = st;
    ht.wait_strings();
    if (!ht.strings_ok) { set_error("out of memory while building the query / accession strings"); return BLU_ERR_ALLOC; }
    if (checksum) {
        uint64_t h = 1469598103934665603ull;
        auto mix = [&](const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } };
        mix(ht.seg_off.data(), ht.seg_off.size() * 8); mix(ht.bitscore.data(), ht.bitscore.size() * 4);
        mix(ht.align_len.data(), ht.align_len.size() * 4); mix(ht.tax_desc_row.data(), ht.tax_desc_row.size() * 4);
        mix(ht.acc_rank.data(), ht.acc_rank.size() * 4); mix(ht.pident.data(), ht.pident.size() * 8);
        for (auto& q : ht.query_names) mix(q.data(), q.size() + 1);
        for (auto& a : ht.accessions) mix(a.data(), a.size() + 1);
        *checksum = h;
    }
    return BLU_OK;
}

int blu_ingest_columns_on(const char* blast_output_file, const char* taxonomies_file, int use_taxid, int device,
                          blu_ingest_columns* out) {
    return blu_ingest_columns_selected(blast_output_file, taxonomies_file, use_taxid, device, nullptr, out, nullptr);
}

int blu_ingest_columns_selected(const char* blast_output_file, const char* taxonomies_file, int use_taxid, int device,
                                const blu_hit_selection* selection, blu_ingest_columns* out, blu_hit_selection_stats* stats) {
    return blu_ingest_columns_laid_out(blast_output_file, taxonomies_file, use_taxid, device, nullptr, selection, out, stats);
}

int blu_ingest_columns_laid_out(const char* blast_output_file, const char* taxonomies_file, int use_taxid, int device,
                                const blu_table_layout* layout, const blu_hit_selection* selection, blu_ingest_columns* out,
                                blu_hit_selection_stats* stats) {
    return blu_ingest_columns_covered(blast_output_file, taxonomies_file, use_taxid, device, layout, nullptr, selection, out, stats);
}

int blu_ingest_columns_covered(const char* blast_output_file, const char* taxonomies_file, int use_taxid, int device,
                               const blu_table_layout* layout, const blu_query_cover* cover, const blu_hit_selection* selection,
                               blu_ingest_columns* out, blu_hit_selection_stats* stats) {
    if (!blast_output_file || !taxonomies_file || !out) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    memset(out, 0, sizeof *out);
    try { return ingest_columns_selected(blast_output_file, taxonomies_file, use_taxid, device, layout, cover, selection, out, stats); }
    catch (const std::bad_alloc&) { blu_ingest_columns_free(out); set_error("out of memory"); return BLU_ERR_ALLOC; }
}

void blu_ingest_columns_free(blu_ingest_columns* c) {
    if (!c) return;
    free(c->seg_off); free(c->bitscore); free(c->align_len); free(c->tax_desc_row); free(c->acc_rank); free(c->pident);
    free(c->query_names); free(c->accessions);
    memset(c, 0, sizeof *c);
}

int blu_last_ingest_path(void) { return g_last_ingest_path; }

int blu_table_layout_parse(const char* spec, blu_table_layout* out) {
    if (!spec || !out) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    if (out->struct_size != sizeof(blu_table_layout)) {
        set_error("blu_table_layout_parse: struct_size %u is not a blu_table_layout this library knows (%zu bytes)", out->struct_size, sizeof(blu_table_layout));
        return BLU_ERR_INVALID_ARG;
    }
    try { return parse_layout_spec(spec, out); }
    catch (const std::bad_alloc&) { set_error("out of memory"); return BLU_ERR_ALLOC; }
}

int blu_query_cover_parse(const char* spec, uint32_t source, blu_query_cover* out) {
    if (!spec || !out) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    if (out->struct_size != sizeof(blu_query_cover)) {
        set_error("blu_query_cover_parse: struct_size %u is not a blu_query_cover this library knows (%zu bytes)", out->struct_size, sizeof(blu_query_cover));
        return BLU_ERR_INVALID_ARG;
    }
    try { return parse_cover_spec(spec, source, out); }
    catch (const std::bad_alloc&) { set_error("out of memory"); return BLU_ERR_ALLOC; }
}

}  // extern "C"
