// The text the pipeline writes (include/blu_pipeline.h): the result document and the three tables.  Reference files followed:
//   domain/dtos/consensus_result.rs:47-88, build_blast_consensus_identity.rs:43-63   consensus beans
//   use_cases/write_blutils_output.rs:87-111,126-232   flattening, sort by query, JSON / JSONL
// Third-party edge not pinned by any reference test: serde_json's float printing (shortest round-trip digits
// here, ".0" appended to integral values).
#include "pipeline_internal.h"

namespace blu {
namespace {

template <class O>
void json_f64(O& o, double v) {   // serde_json: shortest digits that round-trip, integral values keep ".0"
    if (!std::isfinite(v)) { o += "null"; return; }
    char b[64];
    auto r = std::to_chars(b, b + sizeof b, v);
    const size_t n = (size_t)(r.ptr - b);
    o.append(b, n);
    bool integral = true;
    for (size_t i = 0; i < n; ++i) if (b[i] == '.' || b[i] == 'e' || b[i] == 'E') { integral = false; break; }
    if (integral) o += ".0";
}

// serde_yaml 0.9 scalar style (third-party emitter, approximated): plain when the text cannot be read back as
// anything but that string, single quotes otherwise, double quotes when it holds control characters.
void yaml_str(std::string& o, const std::string& s) {
    static const char* reserved[] = {"null", "Null", "NULL", "~", "true", "True", "TRUE", "false", "False", "FALSE",
                                     "y", "Y", "yes", "Yes", "YES", "n", "N", "no", "No", "NO", "on", "On", "ON", "off", "Off", "OFF"};
    bool plain = !s.empty();
    bool control = false;
    for (unsigned char c : s) if (c < 0x20 || c == 0x7F) control = true;
    if (plain) {
        const unsigned char f = (unsigned char)s[0];
        if (!(isalpha(f) || f == '_' || f == '/')) plain = false;               // digits, '-', '.', indicators, spaces
        for (const char* r : reserved) if (s == r) plain = false;
        if (s.back() == ' ' || s.back() == ':') plain = false;
        if (s.find(": ") != std::string::npos || s.find(" #") != std::string::npos) plain = false;
        for (unsigned char c : s) if (c >= 0x80 || c == '"' || c == '\'' || c == '\\' || c == '`') { /* allowed in plain */ }
    }
    if (control) {
        o.push_back('"');
        for (unsigned char c : s) {
            if (c == '"' || c == '\\') { o.push_back('\\'); o.push_back((char)c); }
            else if (c == '\n') o += "\\n";
            else if (c == '\t') o += "\\t";
            else if (c < 0x20 || c == 0x7F) { char b[8]; snprintf(b, sizeof b, "\\x%02x", c); o += b; }
            else o.push_back((char)c);
        }
        o.push_back('"');
    } else if (plain) {
        o += s;
    } else {
        o.push_back('\'');
        for (char c : s) { if (c == '\'') o.push_back('\''); o.push_back(c); }
        o.push_back('\'');
    }
}

// The writer's view of one query's result: everything the reference's TaxonomyBean carries, as indices into the
// taxonomy / accession tables (no strings are built until the text is emitted).  The scratch vectors are reused from
// record to record by the worker that owns them.
struct Renderer {
    const Db& db;
    const std::vector<std::string>& accessions;
    const TopTable& top;
    const blu_taxonomy* tax;
    struct Bean { uint32_t node, desc_row; int32_t occurrences; const char* rank_serde; };
    struct Scratch {
        std::vector<uint32_t> S, bean_of, order;   // S: the top rows (indices into top.rows) in the reference's sorted order
        std::vector<Bean> beans;                   // first-seen order; `order` = the order they are written in
        std::string tmp;
    };
    struct View {
        const TopRow* ref = nullptr;
        uint32_t drow = 0;
        bool single = false, has_mar = false;
        const char* reached = nullptr;
        const char* mar = nullptr;
    };
    uint32_t len_of(uint32_t d) const { return (uint32_t)(db.lin_off[d + 1] - db.lin_off[d]); }
    const char* rank_serde_of(uint32_t desc_row, uint32_t level) const {
        uint16_t codes[BLU_MAX_DEPTH];
        blu_taxonomy_row_cutoffs(tax, desc_row, BLU_MAX_DEPTH, nullptr, nullptr, codes);
        return blu_taxonomy_rank_name(tax, codes[level], 1);
    }
    // taxonomy_beans_to_string (taxonomy_bean.rs:38-45) of the levels in `mask`; json: escaped for a JSON string body
    template <class O>
    void lineage(O& o, uint32_t desc_row, uint64_t mask, bool json) const {
        bool first = true;
        uint32_t jl = 0;
        for (uint64_t i = db.lin_off[desc_row]; i < db.lin_off[desc_row + 1]; ++i, ++jl) {
            if (!((mask >> jl) & 1)) continue;
            if (!first) o.push_back(';');
            first = false;
            const std::string& rk = db.rank_display[db.lin_rank[i]];
            const std::string& id = db.node_ident[db.lin_node[i]];
            if (json) { json_esc(o, rk.data(), rk.size()); o += "__"; json_esc(o, id.data(), id.size()); }
            else { o += rk; o += "__"; o += id; }
        }
    }
    void compute(uint64_t q, const blu_result& r, Scratch& sc, View& v) const {
        const uint64_t b = top.off[q], e = top.off[q + 1];
        const TopRow* rows = top.rows.data();
        v.ref = rows + b;
        for (uint64_t i = b; i < e; ++i) if (rows[i].row == r.ref_row) { v.ref = rows + i; break; }
        v.drow = v.ref->desc_row;
        v.single = r.status == BLU_ST_CONSENSUS_SINGLE;
        v.reached = blu_taxonomy_rank_name(tax, r.reached_rank, 1);
        v.has_mar = r.max_allowed_level != BLU_NONE_U8;
        if (v.has_mar) {
            uint8_t isdef[BLU_MAX_DEPTH]; uint16_t codes[BLU_MAX_DEPTH];
            blu_taxonomy_row_cutoffs(tax, v.drow, BLU_MAX_DEPTH, nullptr, isdef, codes);
            // DefaultRank(rank) -> rank (serde name); NonDefaultRank(name) -> Other(name) (build_blast_consensus_identity.rs:22-30)
            v.mar = blu_taxonomy_rank_name(tax, codes[r.max_allowed_level], isdef[r.max_allowed_level] ? 1 : 0);
        }
        sc.S.clear(); sc.bean_of.clear(); sc.beans.clear(); sc.order.clear();
        if (v.single) {   // find_single_query_consensus.rs:123-145
            sc.S.push_back((uint32_t)(v.ref - rows));
            sc.bean_of.push_back(0);
            sc.beans.push_back(Bean{r.identifier_node, v.drow, 1, v.reached});
            sc.order.push_back(0);
            return;
        }
        for (uint64_t i = b; i < e; ++i) sc.S.push_back((uint32_t)i);
        std::stable_sort(sc.S.begin(), sc.S.end(), [&](uint32_t x, uint32_t y) {   // find_multi_taxa_consensus.rs:39-54
            const TopRow &a = rows[x], &c = rows[y];
            const uint32_t la = len_of(a.desc_row), lc = len_of(c.desc_row);
            if (la != lc) return la < lc;
            if (a.pident < c.pident) return true;
            if (a.pident > c.pident) return false;
            if (a.align_len != c.align_len) return a.align_len < c.align_len;
            return a.acc_rank < c.acc_rank;
        });
        const uint32_t lvl = (r.flags & BLU_FLAG_AGREE) ? r.bean_index : (uint32_t)r.bean_index + 1;   // level the scan stopped at
        for (uint32_t i : sc.S) {   // consensus_result.rs:65-88 fold, first-seen order
            const uint32_t d = rows[i].desc_row;
            // Every top row has level `lvl`: the reference's scan takes, per level, the rows of the length-ascending sort
            // while they still have that level (find_multi_taxa_consensus.rs:142-145), so from the shortest lineage's length
            // on it takes none and sets nothing; the level it stopped at — and the engine's bean_index, which follows it —
            // lies inside the shortest lineage of the group.  tests/document_edges.py, family "ragged": two- and three-level
            // lineages among four-level ones, the short one the last row of lin_off included.
            const uint32_t node = db.lin_node[db.lin_off[d] + lvl];
            uint32_t bi = 0;
            while (bi < sc.beans.size() && sc.beans[bi].node != node) ++bi;
            if (bi == sc.beans.size()) sc.beans.push_back(Bean{node, d, 0, rank_serde_of(d, lvl)});
            sc.bean_of.push_back(bi);
            sc.beans[bi].occurrences += 1;
        }
        for (uint32_t bi = 0; bi < sc.beans.size(); ++bi) sc.order.push_back(bi);
        std::stable_sort(sc.order.begin(), sc.order.end(), [&](uint32_t x, uint32_t y) {   // build_blast_consensus_identity.rs:49-60
            const Bean &a = sc.beans[x], &c = sc.beans[y];
            if (a.occurrences != c.occurrences) return a.occurrences > c.occurrences;
            return db.node_ident[a.node] < db.node_ident[c.node];
        });
    }
    // the accessions of bean `bi` in the order they were pushed, consecutive repeats dropped (extend + dedup())
    template <class F>
    void bean_accessions(const Scratch& sc, uint32_t bi, F&& f) const {
        uint32_t last = 0;
        bool any = false;
        for (size_t k = 0; k < sc.S.size(); ++k) {
            if (sc.bean_of[k] != bi) continue;
            const uint32_t a = top.rows[sc.S[k]].acc_rank;
            if (any && a == last) continue;
            any = true; last = a;
            f(accessions[a]);
        }
    }
    void taxon_yaml(std::string& o, uint64_t q, const blu_result& r, Scratch& sc) const {
        View v;
        compute(q, r, sc, v);
        auto kv = [&](const char* k) { o += "    "; o += k; o += ": "; };
        auto lin = [&](uint32_t d, uint64_t mask) { sc.tmp.clear(); lineage(sc.tmp, d, mask, false); yaml_str(o, sc.tmp); };
        kv("reachedRank"); yaml_str(o, v.reached); o.push_back('\n');
        kv("maxAllowedRank"); if (v.has_mar) yaml_str(o, v.mar); else o += "null"; o.push_back('\n');
        kv("identifier"); yaml_str(o, db.node_ident[r.identifier_node]); o.push_back('\n');
        kv("percIdentity"); json_f64(o, v.ref->pident); o.push_back('\n');
        kv("bitScore"); json_f64(o, (double)top.score[q]); o.push_back('\n');
        kv("taxonomy"); lin(v.drow, r.level_mask); o.push_back('\n');
        kv("mutated"); o += (r.flags & BLU_FLAG_MUTATED) ? "true" : "false"; o.push_back('\n');
        kv("singleMatch"); o += v.single ? "true" : "false"; o.push_back('\n');
        if (sc.beans.empty()) { kv("consensusBeans"); o += "[]\n"; return; }
        o += "    consensusBeans:\n";
        for (uint32_t bi : sc.order) {
            const Bean& b = sc.beans[bi];
            o += "    - rank: "; yaml_str(o, b.rank_serde); o.push_back('\n');
            o += "      identifier: "; yaml_str(o, db.node_ident[b.node]); o.push_back('\n');
            o += "      occurrences: " + std::to_string(b.occurrences) + "\n";
            o += "      taxonomy: "; lin(b.desc_row, ~0ull); o.push_back('\n');
            bool any = false;
            bean_accessions(sc, bi, [&](const std::string& a) {
                if (!any) o += "      accessions:\n";
                any = true;
                o += "      - "; yaml_str(o, a); o.push_back('\n');
            });
            if (!any) o += "      accessions: []\n";
        }
    }
    // pretty = serde_json::to_string_pretty layout (2-space indent); ind = indentation of the object's own line
    template <class O>
    void taxon(O& o, uint64_t q, const blu_result& r, bool pretty, int ind, Scratch& sc) const {
        View v;
        compute(q, r, sc, v);
        auto nl = [&](int extra) { if (pretty) { o.push_back('\n'); o.append((size_t)(ind + extra) * 2, ' '); } };
        const char* colon = pretty ? ": " : ":";
        auto key = [&](int extra, const char* k, bool comma = true) { if (comma) o.push_back(','); nl(extra); o += k; o += colon; };
        o.push_back('{');
        key(1, "\"reachedRank\"", false); json_str(o, v.reached);
        key(1, "\"maxAllowedRank\"");
        if (v.has_mar) json_str(o, v.mar); else o += "null";
        key(1, "\"identifier\""); json_str(o, db.node_ident[r.identifier_node]);
        key(1, "\"percIdentity\""); json_f64(o, v.ref->pident);
        key(1, "\"bitScore\""); json_f64(o, (double)top.score[q]);
        key(1, "\"taxonomy\""); o.push_back('"'); lineage(o, v.drow, r.level_mask, true); o.push_back('"');
        key(1, "\"mutated\""); o += (r.flags & BLU_FLAG_MUTATED) ? "true" : "false";
        key(1, "\"singleMatch\""); o += v.single ? "true" : "false";
        key(1, "\"consensusBeans\""); o.push_back('[');
        bool first_bean = true;
        for (uint32_t bi : sc.order) {
            const Bean& b = sc.beans[bi];
            if (!first_bean) o.push_back(',');
            first_bean = false;
            nl(2); o.push_back('{');
            key(3, "\"rank\"", false); json_str(o, b.rank_serde);
            key(3, "\"identifier\""); json_str(o, db.node_ident[b.node]);
            key(3, "\"occurrences\""); { char nb[16]; auto rr = std::to_chars(nb, nb + sizeof nb, b.occurrences); o.append(nb, (size_t)(rr.ptr - nb)); }
            key(3, "\"taxonomy\""); o.push_back('"'); lineage(o, b.desc_row, ~0ull, true); o.push_back('"');
            key(3, "\"accessions\""); o.push_back('[');
            bool any = false;
            bean_accessions(sc, bi, [&](const std::string& a) { if (any) o.push_back(','); any = true; nl(4); json_str(o, a); });
            if (any) nl(3);
            o.push_back(']');
            nl(2); o.push_back('}');
        }
        if (!first_bean) nl(1);
        o.push_back(']');
        nl(0); o.push_back('}');
    }
};

}  // namespace

// TopTable from host columns (the CPU ingest, or the staging path of the engine): same content as the device-side
// compaction in ingest_gpu.hip
void top_rows_from_columns(const HitTable& ht, const Column<blu_result>& recs, unsigned nthreads, TopTable& top) {
    const size_t nq = recs.size();
    top.off.resize(nq + 1);
    top.score.resize(nq);
    std::vector<uint64_t> cnt(nq, 0);
    auto slice = [&](unsigned t, unsigned nt, auto&& f) { for (size_t q = nq * t / nt; q < nq * (t + 1) / nt; ++q) f(q); };
    const unsigned nt = nq < 65536 ? 1 : nthreads;
    parallel_for(nt, nt, [&](unsigned t) {
        slice(t, nt, [&](size_t q) {
            const blu_result& r = recs[q];
            top.score[q] = 0;
            if (r.status >= 2 || r.ref_row == 0xFFFFFFFFu) return;
            const int32_t M = ht.bitscore[r.ref_row];
            top.score[q] = M;
            uint64_t c = 0;
            for (uint64_t i = ht.seg_off[q]; i < ht.seg_off[q + 1]; ++i) c += ht.bitscore[i] == M;
            cnt[q] = c;
        });
    });
    top.off[0] = 0;
    for (size_t q = 0; q < nq; ++q) top.off[q + 1] = top.off[q] + cnt[q];
    top.rows.resize(top.off[nq]);
    parallel_for(nt, nt, [&](unsigned t) {
        slice(t, nt, [&](size_t q) {
            if (!cnt[q]) return;
            uint64_t at = top.off[q];
            const int32_t M = top.score[q];
            for (uint64_t i = ht.seg_off[q]; i < ht.seg_off[q + 1]; ++i)
                if (ht.bitscore[i] == M) top.rows[at++] = TopRow{(uint32_t)i, ht.tax_desc_row[i], ht.acc_rank[i], ht.align_len[i], ht.pident[i]};
        });
    });
}

std::string uuid_v4() {
    unsigned char b[16];
    FILE* f = fopen("/dev/urandom", "rb");
    if (!f || fread(b, 1, 16, f) != 16) for (auto& x : b) x = (unsigned char)rand();
    if (f) fclose(f);
    b[6] = (unsigned char)((b[6] & 0x0F) | 0x40);
    b[8] = (unsigned char)((b[8] & 0x3F) | 0x80);
    char s[40];
    snprintf(s, sizeof s, "%02x%02x%02x%02x-%02x%02x-%02x%02x-%02x%02x-%02x%02x%02x%02x%02x%02x", b[0], b[1], b[2], b[3], b[4], b[5],
             b[6], b[7], b[8], b[9], b[10], b[11], b[12], b[13], b[14], b[15]);
    return s;
}

const char* status_site(uint8_t st) {
    switch (st) {
        case BLU_ST_ERR_UNMATCHED_TAXID: return "taxid of a top-score hit is not in the taxonomies file: lineage `null` fails parse_taxonomy (find_single_query_consensus.rs:58-60)";
        case BLU_ST_ERR_BAD_LINEAGE: return "lineage of a top-score hit fails parse_taxonomy (blast_result.rs:109-114)";
        case BLU_ST_ERR_ROOT_DISAGREE: return "top-score hits disagree at the first lineage level: `index - 1` underflow (find_multi_taxa_consensus.rs:181)";
        case BLU_ST_ERR_SINGLE_BELOW_CUTOFFS: return "single top-score hit below every identity cutoff (find_single_query_consensus.rs:113-119)";
        case BLU_ST_ERR_BAD_PIDENT: return "NaN perc_identity among the top-score hits";
        default: return "unknown";
    }
}

// ---- taxon abundance report ---------------------------------------------------------------------------
// Weight of a query under `size` weighting: the first ';'-separated field that is exactly `size=` + decimal digits, else a
// name ending in `_size_` + digits, else 1.  false: the value does not fit 32 bits.
bool size_weight(std::string_view name, uint32_t* w) {
    auto digits = [](std::string_view v) { if (v.empty()) return false; for (char c : v) if (c < '0' || c > '9') return false; return true; };
    auto value = [&](std::string_view v) {
        uint64_t x = 0;
        for (char c : v) { x = x * 10 + (uint64_t)(c - '0'); if (x > 0xFFFFFFFFull) return false; }
        *w = (uint32_t)x;
        return true;
    };
    for (size_t pos = 0;;) {
        const size_t semi = name.find(';', pos);
        const std::string_view f = name.substr(pos, semi == std::string_view::npos ? std::string_view::npos : semi - pos);
        if (f.size() > 5 && f.compare(0, 5, "size=") == 0 && digits(f.substr(5))) return value(f.substr(5));
        if (semi == std::string_view::npos) break;
        pos = semi + 1;
    }
    const size_t at = name.rfind("_size_");
    if (at != std::string_view::npos && digits(name.substr(at + 6))) return value(name.substr(at + 6));
    *w = 1;
    return true;
}

// The report's row order: the paths depth first, siblings by clade descending and element text `rank__identifier`
// ascending (bytewise).  P has parents before children (blu_consensus_report, blu_consensus_sample_table).
// row(i, rank, identifier, taxonomy) for every path in that order.
template <class Row>
void report_rows(const Db& db, const blu_report_path* P, uint64_t n, Row&& row) {
    // children of path i at kids[off[i + 1] .. off[i + 2]); the first-level paths at kids[off[0] .. off[1])
    std::vector<uint64_t> off(n + 2, 0);
    for (uint64_t i = 0; i < n; ++i) ++off[(P[i].parent == BLU_REPORT_NO_PARENT ? 0 : (uint64_t)P[i].parent + 1) + 1];
    for (uint64_t i = 0; i + 1 < off.size(); ++i) off[i + 1] += off[i];
    std::vector<uint32_t> kids(n);
    {
        std::vector<uint64_t> at(off.begin(), off.end() - 1);
        for (uint64_t i = 0; i < n; ++i) kids[at[P[i].parent == BLU_REPORT_NO_PARENT ? 0 : (uint64_t)P[i].parent + 1]++] = (uint32_t)i;
    }
    auto rank_of = [&](uint32_t node) -> const std::string& { return db.rank_display[db.node_rank[node]]; };
    std::string ea, eb;   // (element texts of a comparison: buffers reused)
    auto less = [&](uint32_t a, uint32_t b) {
        if (P[a].clade != P[b].clade) return P[a].clade > P[b].clade;
        ea.assign(rank_of(P[a].node)); ea += "__"; ea += db.node_ident[P[a].node];
        eb.assign(rank_of(P[b].node)); eb += "__"; eb += db.node_ident[P[b].node];
        return ea < eb;
    };
    for (uint64_t g = 0; g + 1 < off.size(); ++g)
        if (off[g + 1] - off[g] > 1) std::sort(kids.begin() + off[g], kids.begin() + off[g + 1], less);
    std::string path;
    std::vector<size_t> len_at;                       // path text length after the element at each depth
    std::vector<std::pair<uint32_t, uint32_t>> stack;  // (path, depth)
    for (uint64_t k = off[1]; k-- > off[0];) stack.emplace_back(kids[k], 0u);
    while (!stack.empty()) {
        const auto [i, d] = stack.back();
        stack.pop_back();
        path.resize(d ? len_at[d - 1] : 0);
        if (d) path.push_back(';');
        const std::string& rk = rank_of(P[i].node);
        const std::string& id = db.node_ident[P[i].node];
        path += rk; path += "__"; path += id;
        if (len_at.size() <= d) len_at.resize(d + 1);
        len_at[d] = path.size();
        row(i, rk, id, path);
        for (uint64_t k = off[(uint64_t)i + 2]; k-- > off[(uint64_t)i + 1];) stack.emplace_back(kids[k], d + 1);
    }
}

// The report's text: header, unclassified, unplaced (when any), then the paths in report_rows' order.
std::string render_report(const Db& db, const blu_report& rep) {
    std::string o = "#percent\tclade\tdirect\trank\tidentifier\ttaxonomy\n";
    const double total = (double)rep.total;
    auto num = [&](uint64_t v) { char b[24]; auto r = std::to_chars(b, b + sizeof b, v); o.append(b, (size_t)(r.ptr - b)); };
    auto pct = [&](uint64_t c) { char b[64]; const int n = snprintf(b, sizeof b, "%.2f", rep.total ? 100.0 * (double)c / total : 0.0); o.append(b, (size_t)n); };
    auto fixed_row = [&](uint64_t c, const char* what) { pct(c); o.push_back('\t'); num(c); o.push_back('\t'); num(c); o += "\t-\t"; o += what; o += "\t\n"; };
    fixed_row(rep.unclassified, "unclassified");
    if (rep.unplaced) fixed_row(rep.unplaced, "unplaced");
    const blu_report_path* P = rep.paths;
    report_rows(db, P, rep.n_paths, [&](uint32_t i, const std::string& rk, const std::string& id, const std::string& path) {
        pct(P[i].clade); o.push_back('\t'); num(P[i].clade); o.push_back('\t'); num(P[i].direct); o.push_back('\t');
        o += rk; o.push_back('\t'); o += id; o.push_back('\t'); o += path; o.push_back('\n');
    });
    return o;
}

// ---- per-sample table ---------------------------------------------------------------------------------
// The sample a query name names: the first ';'-field `sample=` + at least one byte; else, in the label (the name up to its
// first ';', a trailing `_size_` + digits removed), the part left of the last '.' when it is non-empty and the part right
// of that '.' is one or more ASCII digits.  false: no sample.
bool sample_of(std::string_view name, std::string_view* out) {
    auto digits = [](std::string_view v) { if (v.empty()) return false; for (char c : v) if (c < '0' || c > '9') return false; return true; };
    for (size_t pos = 0;;) {
        const size_t semi = name.find(';', pos);
        const std::string_view f = name.substr(pos, semi == std::string_view::npos ? std::string_view::npos : semi - pos);
        if (f.size() > 7 && f.compare(0, 7, "sample=") == 0) { *out = f.substr(7); return true; }
        if (semi == std::string_view::npos) break;
        pos = semi + 1;
    }
    std::string_view label = name.substr(0, name.find(';'));
    const size_t at = label.rfind("_size_");
    if (at != std::string_view::npos && digits(label.substr(at + 6))) label = label.substr(0, at);
    const size_t dot = label.rfind('.');
    if (dot == std::string_view::npos || dot == 0 || !digits(label.substr(dot + 1))) return false;
    *out = label.substr(0, dot);
    return true;
}

// The table's text: header with the sample names, unclassified, unplaced (when any), then one line per path in the
// report's order; a path's cells are tab.cells[cell_at[i] .. cell_at[i + 1]) (sorted by sample).
std::string render_sample_table(const Db& db, const blu_sample_table& tab, const std::vector<std::string_view>& names) {
    std::string o = "#rank\tidentifier\ttaxonomy\ttotal";
    for (std::string_view s : names) { o.push_back('\t'); o.append(s.data(), s.size()); }
    o.push_back('\n');
    const uint32_t ns = tab.n_samples;
    auto num = [&](uint64_t v) { char b[24]; auto r = std::to_chars(b, b + sizeof b, v); o.append(b, (size_t)(r.ptr - b)); };
    auto fixed_row = [&](const uint64_t* per, const char* what) {
        uint64_t t = 0;
        for (uint32_t s = 0; s < ns; ++s) t += per[s];
        if (!t && per == tab.unplaced) return;
        o += "-\t"; o += what; o += "\t\t"; num(t);
        for (uint32_t s = 0; s < ns; ++s) { o.push_back('\t'); num(per[s]); }
        o.push_back('\n');
    };
    fixed_row(tab.unclassified, "unclassified");
    fixed_row(tab.unplaced, "unplaced");
    std::vector<uint64_t> cell_at(tab.n_paths + 1, 0);
    for (uint64_t k = 0; k < tab.n_cells; ++k) ++cell_at[tab.cells[k].path + 1];
    for (uint64_t i = 0; i < tab.n_paths; ++i) cell_at[i + 1] += cell_at[i];
    report_rows(db, tab.paths, tab.n_paths, [&](uint32_t i, const std::string& rk, const std::string& id, const std::string& path) {
        o += rk; o.push_back('\t'); o += id; o.push_back('\t'); o += path; o.push_back('\t'); num(tab.paths[i].clade);
        uint64_t k = cell_at[i];
        for (uint32_t s = 0; s < ns; ++s) {
            o.push_back('\t');
            if (k < cell_at[i + 1] && tab.cells[k].sample == s) num(tab.cells[k++].clade);
            else o.push_back('0');
        }
        o.push_back('\n');
    });
    return o;
}

// ---- support table ----------------------------------------------------------------------------------------
std::string render_support(const Run& r, const std::vector<blu_support>& sup) {
    const Db& db = *r.db;
    const TopTable& top = r.top;
    std::string o = "#query\trank\tidentifier\thits\tmatched\ttop_hits\ttop_support\tsupport\tbit_score\tbits\tsupport_bits\tconfidence\n";
    o.reserve(o.size() + r.items.size() * 96);
    auto num = [&](int64_t v) { char b[24]; auto rr = std::to_chars(b, b + sizeof b, v); o.append(b, (size_t)(rr.ptr - b)); o.push_back('\t'); };
    const blu_support none{};
    for (const Item& it : r.items) {
        o += *it.name; o.push_back('\t');
        const blu_support& c = it.q < 0 ? none : sup[(size_t)it.q];
        const blu_result* rec = it.q < 0 ? nullptr : &r.recs[(size_t)it.q];
        if (!rec || rec->status >= 2) o += "-\tunclassified\t";
        else {
            // the last element of the result's `taxonomy` (Renderer::lineage): the highest level of level_mask the lineage has
            uint32_t drow = 0;
            for (uint64_t i = top.off[(size_t)it.q], e = top.off[(size_t)it.q + 1]; i < e; ++i) {
                if (i == top.off[(size_t)it.q]) drow = top.rows[i].desc_row;
                if (top.rows[i].row == rec->ref_row) { drow = top.rows[i].desc_row; break; }
            }
            const uint64_t len = db.lin_off[drow + 1] - db.lin_off[drow];
            const uint64_t m = len >= 64 ? rec->level_mask : rec->level_mask & ((1ull << len) - 1ull);
            if (m == 0) o += "-\tunplaced\t";
            else {
                const uint64_t at = db.lin_off[drow] + (63u - (uint32_t)__builtin_clzll(m));
                o += db.rank_display[db.lin_rank[at]]; o.push_back('\t'); o += db.node_ident[db.lin_node[at]]; o.push_back('\t');
            }
        }
        num(c.n_hits); num(c.n_matched); num(c.n_top); num(c.n_top_support); num(c.n_support); num(c.top_score); num(c.bits); num(c.support_bits);
        char b[64];
        const int n = snprintf(b, sizeof b, "%.4f\n", c.n_hits ? (double)c.n_support / (double)c.n_hits : 0.0);
        o.append(b, (size_t)n);
    }
    return o;
}

// ---- the document's records ---------------------------------------------------------------------------------------------------
std::string render_yaml(const Run& r, const std::string& run_id, const std::string& cfg) {
    const Renderer R{*r.db, r.ht->accessions, r.top, r.tax};
    Renderer::Scratch sc;
    std::string o = r.items.empty() ? "results: []\n" : "results:\n";
    for (const Item& it : r.items) {
        o += "- runId: "; yaml_str(o, run_id); o.push_back('\n');
        o += "  query: "; yaml_str(o, *it.name); o.push_back('\n');
        if (it.q < 0 || r.recs[(size_t)it.q].status >= 2) { o += "  taxon: null\n"; continue; }
        o += "  taxon:\n";
        R.taxon_yaml(o, (uint64_t)it.q, r.recs[(size_t)it.q], sc);
    }
    if (cfg.empty()) o += "config: null\n";
    else { o += "config:\n"; o += cfg; if (o.back() != '\n') o.push_back('\n'); }
    return o;
}

void render_head(int32_t format, const std::string& cfg, Out& head) {
    if (format == BLU_OUT_JSON) head += "{\n  \"results\": [";
    else if (format == BLU_OUT_JSON_COMPACT) head += "{\"results\":[";
    else { if (cfg.empty()) head += "null"; else head += cfg; head.push_back('\n'); }     // JSONL: the config line comes first
}

void render_block(const Run& r, const std::string& run_id_json, size_t i0, size_t i1, Out& po) {
    thread_local Renderer::Scratch sc;
    const Renderer R{*r.db, r.ht->accessions, r.top, r.tax};
    const bool pretty = r.params->out_format == BLU_OUT_JSON;
    const bool doc = pretty || r.params->out_format == BLU_OUT_JSON_COMPACT;   // one {results, config} document
    po.reserve((i1 - i0) * (pretty ? 1100 : 520));
    const int ind = pretty ? 2 : 0;
    auto nl = [&](int extra) { if (pretty) { po.push_back('\n'); po.append((size_t)(ind + extra) * 2, ' '); } };
    const char* colon = pretty ? ": " : ":";
    for (size_t ii = i0; ii < i1; ++ii) {
        const Item& it = r.items[ii];
        if (pretty) { if (ii) po.push_back(','); nl(0); }
        else if (doc && ii) po.push_back(',');
        po.push_back('{');
        nl(1); po += "\"runId\""; po += colon; po.append(run_id_json.data(), run_id_json.size());
        po.push_back(','); nl(1); po += "\"query\""; po += colon; json_str(po, *it.name);
        po.push_back(','); nl(1); po += "\"taxon\""; po += colon;
        if (it.q < 0 || r.recs[(size_t)it.q].status >= 2) po += "null";
        else R.taxon(po, (uint64_t)it.q, r.recs[(size_t)it.q], pretty, ind + 1, sc);
        nl(0); po.push_back('}');
        if (!doc) po.push_back('\n');
    }
}

void render_tail(int32_t format, const std::string& cfg, bool any_items, Out& tail) {
    const std::string cfg_or_null = cfg.empty() ? std::string("null") : cfg;
    if (format == BLU_OUT_JSON) { if (any_items) tail += "\n  "; tail += "],\n  \"config\": "; tail += cfg_or_null; tail += "\n}"; }
    else if (format == BLU_OUT_JSON_COMPACT) { tail += "],\"config\":"; tail += cfg_or_null; tail.push_back('}'); }
}

}  // namespace blu
