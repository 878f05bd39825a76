// The taxonomies file of the pipeline (include/blu_pipeline.h).  Reference files followed:
//   core/src/use_cases/build_consensus_identities/mod.rs:246-327   blutils DB JSON -> {taxid, numericLineage | textLineage}
//   domain/dtos/blast_result.rs:38-120   lineage grammar `rank__identifier(;rank__identifier)*`
#include "pipeline_internal.h"
#include "seqdb_labels.h"

namespace blu {
namespace {

// ---------------------------------------------------------------------------------------------------------
// minimal JSON reader (enough for the blutils DB and the custom-cutoff file)
// ---------------------------------------------------------------------------------------------------------
struct Json {
    const char* p;
    const char* end;
    bool ok = true;
    void ws() { while (p < end && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) ++p; }
    bool eat(char c) { ws(); if (p < end && *p == c) { ++p; return true; } return false; }
    bool peek(char c) { ws(); return p < end && *p == c; }
    bool string(std::string* out) {
        ws();
        if (p >= end || *p != '"') { ok = false; return false; }
        ++p;
        if (out) out->clear();
        while (p < end && *p != '"') {
            if (*p == '\\' && p + 1 < end) {
                ++p;
                char c = *p++;
                char r = c;
                switch (c) {
                    case 'n': r = '\n'; break; case 't': r = '\t'; break; case 'r': r = '\r'; break;
                    case 'b': r = '\b'; break; case 'f': r = '\f'; break;
                    case 'u': {
                        unsigned v = 0;
                        for (int i = 0; i < 4 && p < end; ++i, ++p) v = v * 16 + (unsigned)(isdigit((unsigned char)*p) ? *p - '0' : (tolower(*p) - 'a' + 10));
                        if (out) {  // UTF-8 encode the BMP code point (surrogate pairs are not expected in lineages)
                            if (v < 0x80) out->push_back((char)v);
                            else if (v < 0x800) { out->push_back((char)(0xC0 | (v >> 6))); out->push_back((char)(0x80 | (v & 0x3F))); }
                            else { out->push_back((char)(0xE0 | (v >> 12))); out->push_back((char)(0x80 | ((v >> 6) & 0x3F))); out->push_back((char)(0x80 | (v & 0x3F))); }
                        }
                        continue;
                    }
                    default: break;
                }
                if (out) out->push_back(r);
            } else {
                if (out) out->push_back(*p);
                ++p;
            }
        }
        if (p >= end) { ok = false; return false; }
        ++p;
        return true;
    }
    bool number(double* out) {
        ws();
        // the token is copied first: the mapped file is not NUL-terminated, and a number may be its last bytes
        char tok[64];
        size_t n = 0;
        while (p + n < end && n < sizeof tok - 1 && (((unsigned)(p[n] - '0') < 10u) || p[n] == '-' || p[n] == '+' || p[n] == '.' || p[n] == 'e' || p[n] == 'E')) {
            tok[n] = p[n];
            ++n;
        }
        tok[n] = 0;
        char* e = nullptr;
        double v = strtod(tok, &e);
        if (e == tok) { ok = false; return false; }
        p += e - tok;
        if (out) *out = v;
        return true;
    }
    void skip() {
        ws();
        if (p >= end) { ok = false; return; }
        if (*p == '"') { string(nullptr); return; }
        if (*p == '{') {
            ++p;
            if (eat('}')) return;
            do { string(nullptr); if (!eat(':')) { ok = false; return; } skip(); } while (ok && eat(','));
            if (!eat('}')) ok = false;
            return;
        }
        if (*p == '[') {
            ++p;
            if (eat(']')) return;
            do { skip(); } while (ok && eat(','));
            if (!eat(']')) ok = false;
            return;
        }
        while (p < end && *p != ',' && *p != '}' && *p != ']' && *p != ' ' && *p != '\n' && *p != '\r' && *p != '\t') ++p;  // number / literal
    }
};

}  // namespace

std::string canonical_display(const std::string& raw) {
    static const char* letters[9] = {"u", "d", "k", "p", "c", "o", "f", "g", "s"};
    std::string other;
    uint16_t k = parse_rank(raw.c_str(), &other);
    return k < K_FIRST_OTHER ? std::string(letters[k]) : other;
}

namespace {

// blast_result.rs:38-120: split on ';' then on "__", every element must give exactly two parts
void add_lineage(Db& db, int64_t taxid, const std::string& lineage) {
    const size_t first = db.lin_node.size();
    bool bad = false;
    size_t pos = 0;
    for (;;) {
        size_t semi = lineage.find(';', pos);
        std::string_view el(lineage.data() + pos, (semi == std::string::npos ? lineage.size() : semi) - pos);
        size_t sep = el.find("__");
        if (sep == std::string_view::npos || el.find("__", sep + 2) != std::string_view::npos) bad = true;   // != 2 parts
        if (!bad) {
            std::string rank(el.substr(0, sep)), ident(el.substr(sep + 2));
            auto rit = db.rank_ids.find(rank);
            if (rit == db.rank_ids.end()) {
                rit = db.rank_ids.emplace(rank, (uint16_t)db.rank_raw.size()).first;
                db.rank_raw.push_back(rank);
                db.rank_display.push_back(canonical_display(rank));
            }
            std::string key = db.rank_display[rit->second];
            key.push_back('\x1f');
            key += ident;
            auto nit = db.node_ids.find(key);
            if (nit == db.node_ids.end()) {
                nit = db.node_ids.emplace(std::move(key), (uint32_t)db.node_ident.size()).first;
                db.node_ident.push_back(ident);
                db.node_rank.push_back(rit->second);
            }
            db.lin_node.push_back(nit->second);
            db.lin_rank.push_back(rit->second);
        }
        if (semi == std::string::npos) break;
        pos = semi + 1;
    }
    if (bad) { db.lin_node.resize(first); db.lin_rank.resize(first); }
    db.bad.push_back(bad ? 1 : 0);
    db.note_row(taxid, (uint32_t)db.taxid.size());
    db.taxid.push_back(taxid);
    db.lin_off.push_back(db.lin_node.size());
}

// ---- binary cache of the parsed taxonomies file ---------------------------------------------
// What load_db produces from the `*.blutils.json` (mod.rs:246-327: only {taxid, numericLineage | textLineage} of each
// entry is used), stored flat so a later run maps it instead of parsing ~100 MB of JSON per 300 k taxids:
//   header | taxid i64[n] | lin_off u64[n+1] | lin_node u32[m] | lin_rank u16[m] | bad u8[n] |
//   rank_off u32[r+1] | rank bytes | node_off u64[k+1] | node bytes      (sections padded to 8 bytes)
// The header records which lineage flavour was interned (use_taxid) and an FNV-1a hash of everything after it.
struct CacheHeader {
    char magic[8];            // "BLUDBC01"
    uint32_t version, use_taxid;
    uint64_t n_tax, n_lin, n_ranks, n_nodes, rank_bytes, node_bytes, payload_bytes, payload_hash;
};
const char kCacheMagic[8] = {'B', 'L', 'U', 'D', 'B', 'C', '0', '1'};

uint64_t fnv1a(const void* data, size_t n, uint64_t h = 1469598103934665603ull) {
    // 8 bytes per step (a hash of 64-bit words, tail bytewise): this guards against truncation / bit rot, not malice
    const unsigned char* p = (const unsigned char*)data;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) { uint64_t w; memcpy(&w, p + i, 8); h = (h ^ w) * 1099511628211ull; }
    for (; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

size_t pad8(size_t n) { return (n + 7) & ~(size_t)7; }

bool is_cache(const MappedFile& f) { return f.size >= sizeof(CacheHeader) && memcmp(f.data, kCacheMagic, 8) == 0; }

int load_db_cache(const MappedFile& f, bool use_taxid, Db& db) {
    CacheHeader h;
    memcpy(&h, f.data, sizeof(h));
    if (h.version != 1) { set_error("taxonomy cache: unsupported version %u", h.version); return BLU_ERR_PARSE; }
    if ((h.use_taxid != 0) != use_taxid) {
        set_error("taxonomy cache was built for %s lineages but the run asks for %s", h.use_taxid ? "numeric (-u)" : "text",
                  use_taxid ? "numeric (-u)" : "text");
        return BLU_ERR_INVALID_ARG;
    }
    const size_t sizes[9] = {h.n_tax * 8, (h.n_tax + 1) * 8, h.n_lin * 4, h.n_lin * 2, h.n_tax, (h.n_ranks + 1) * 4, h.rank_bytes,
                             (h.n_nodes + 1) * 8, h.node_bytes};
    size_t total = 0;
    for (size_t x : sizes) total += pad8(x);
    if (h.n_tax >= (1ull << BLU_ROW_BITS) || total != h.payload_bytes || sizeof(h) + total != f.size) {
        set_error("taxonomy cache: size mismatch (truncated or not a cache file)");
        return BLU_ERR_PARSE;
    }
    const char* p = f.data + sizeof(h);
    if (fnv1a(p, total) != h.payload_hash) { set_error("taxonomy cache: checksum mismatch"); return BLU_ERR_PARSE; }
    auto take = [&](void* dst, size_t bytes) { memcpy(dst, p, bytes); p += pad8(bytes); };
    db.taxid.resize(h.n_tax); take(db.taxid.data(), sizes[0]);
    db.lin_off.resize(h.n_tax + 1); take(db.lin_off.data(), sizes[1]);
    db.lin_node.resize(h.n_lin); take(db.lin_node.data(), sizes[2]);
    db.lin_rank.resize(h.n_lin); take(db.lin_rank.data(), sizes[3]);
    db.bad.resize(h.n_tax); take(db.bad.data(), sizes[4]);
    std::vector<uint32_t> roff(h.n_ranks + 1); take(roff.data(), sizes[5]);
    const char* rbytes = p; p += pad8(sizes[6]);
    std::vector<uint64_t> noff(h.n_nodes + 1); take(noff.data(), sizes[7]);
    const char* nbytes = p;
    // offsets are data: check them before they index anything
    bool ok = db.lin_off[0] == 0 && db.lin_off[h.n_tax] == h.n_lin && roff[0] == 0 && roff[h.n_ranks] == h.rank_bytes &&
              noff[0] == 0 && noff[h.n_nodes] == h.node_bytes;
    for (uint64_t i = 0; ok && i < h.n_tax; ++i) ok = db.lin_off[i] <= db.lin_off[i + 1];
    for (uint64_t i = 0; ok && i < h.n_ranks; ++i) ok = roff[i] <= roff[i + 1];
    for (uint64_t i = 0; ok && i < h.n_nodes; ++i) ok = noff[i] <= noff[i + 1];
    for (uint64_t i = 0; ok && i < h.n_lin; ++i) ok = db.lin_node[i] < h.n_nodes && db.lin_rank[i] < h.n_ranks;
    if (!ok) { set_error("taxonomy cache: inconsistent offsets"); return BLU_ERR_PARSE; }
    db.rank_raw.resize(h.n_ranks); db.rank_display.resize(h.n_ranks);
    for (uint64_t i = 0; i < h.n_ranks; ++i) {
        db.rank_raw[i].assign(rbytes + roff[i], roff[i + 1] - roff[i]);
        db.rank_display[i] = canonical_display(db.rank_raw[i]);
    }
    db.node_ident.resize(h.n_nodes);
    for (uint64_t i = 0; i < h.n_nodes; ++i) db.node_ident[i].assign(nbytes + noff[i], noff[i + 1] - noff[i]);
    db.node_rank.assign(h.n_nodes, 0);
    for (uint64_t i = 0; i < h.n_lin; ++i) db.node_rank[db.lin_node[i]] = db.lin_rank[i];
    db.row_of.reserve(h.n_tax);
    for (uint64_t i = 0; i < h.n_tax; ++i) db.note_row(db.taxid[i], (uint32_t)i);
    return BLU_OK;
}

int write_db_cache(const Db& db, bool use_taxid, const char* path) {
    CacheHeader h{};
    memcpy(h.magic, kCacheMagic, 8);
    h.version = 1; h.use_taxid = use_taxid ? 1 : 0;
    h.n_tax = db.taxid.size(); h.n_lin = db.lin_node.size(); h.n_ranks = db.rank_raw.size(); h.n_nodes = db.node_ident.size();
    std::vector<uint32_t> roff{0};
    std::string rbytes, nbytes;
    for (auto& r : db.rank_raw) { rbytes += r; roff.push_back((uint32_t)rbytes.size()); }
    std::vector<uint64_t> noff{0};
    for (auto& n : db.node_ident) { nbytes += n; noff.push_back(nbytes.size()); }
    h.rank_bytes = rbytes.size(); h.node_bytes = nbytes.size();
    std::string out;
    auto put = [&](const void* src, size_t bytes) { out.append((const char*)src, bytes); out.append(pad8(bytes) - bytes, '\0'); };
    put(db.taxid.data(), db.taxid.size() * 8);
    put(db.lin_off.data(), db.lin_off.size() * 8);
    put(db.lin_node.data(), db.lin_node.size() * 4);
    put(db.lin_rank.data(), db.lin_rank.size() * 2);
    put(db.bad.data(), db.bad.size());
    put(roff.data(), roff.size() * 4);
    put(rbytes.data(), rbytes.size());
    put(noff.data(), noff.size() * 8);
    put(nbytes.data(), nbytes.size());
    h.payload_bytes = out.size();
    h.payload_hash = fnv1a(out.data(), out.size());
    std::string tmp = std::string(path) + ".tmp";
    FILE* fp = fopen(tmp.c_str(), "wb");
    if (!fp) { set_error("cannot write %s", tmp.c_str()); return BLU_ERR_IO; }
    bool ok = fwrite(&h, sizeof(h), 1, fp) == 1 && (out.empty() || fwrite(out.data(), out.size(), 1, fp) == 1);
    ok = (fclose(fp) == 0) && ok;
    if (!ok || rename(tmp.c_str(), path) != 0) { remove(tmp.c_str()); set_error("cannot write %s", path); return BLU_ERR_IO; }
    return BLU_OK;
}

}  // namespace

// mod.rs:246-327 + domain/dtos/taxonomies_map.rs:6-32 (or the binary cache of the same content, see above)
int load_db(const char* path, bool use_taxid, Db& db) {
    MappedFile f;
    if (!f.open(path)) { set_error("Taxonomies file not found: %s", path); return BLU_ERR_IO; }
    if (is_cache(f)) return load_db_cache(f, use_taxid, db);
    Json j{f.data, f.data + f.size};
    if (!j.eat('{')) { set_error("taxonomies file is not a JSON object"); return BLU_ERR_PARSE; }
    bool found = false;
    std::string key, numeric, text;
    if (!j.peek('}')) {
        do {
            if (!j.string(&key) || !j.eat(':')) { j.ok = false; break; }
            if (key != "taxonomies") { j.skip(); continue; }
            found = true;
            if (!j.eat('[')) { j.ok = false; break; }
            if (j.eat(']')) continue;
            do {
                if (!j.eat('{')) { j.ok = false; break; }
                double taxid = 0;
                bool has_taxid = false, has_n = false, has_t = false;
                if (!j.peek('}')) {
                    do {
                        if (!j.string(&key) || !j.eat(':')) { j.ok = false; break; }
                        if (key == "taxid") has_taxid = j.number(&taxid);
                        else if (key == "numericLineage") has_n = j.string(&numeric);
                        else if (key == "textLineage") has_t = j.string(&text);
                        else j.skip();
                    } while (j.ok && j.eat(','));
                }
                if (!j.eat('}')) j.ok = false;
                if (!j.ok) break;
                if (!has_taxid || !has_n || !has_t) { set_error("taxonomy entry %zu lacks taxid/numericLineage/textLineage", db.taxid.size()); return BLU_ERR_PARSE; }
                // mod.rs:278 (u64 -> f64 -> i64), :287-291; a value no i64 holds cannot equal any subject_taxid of the Int64 column
                const int64_t taxid_i = taxid >= 9223372036854775808.0 ? INT64_MAX : (taxid <= -9223372036854775808.0 ? INT64_MIN : (int64_t)taxid);
                add_lineage(db, taxid_i, use_taxid ? numeric : text);
            } while (j.ok && j.eat(','));
            if (!j.eat(']')) j.ok = false;
        } while (j.ok && j.eat(','));
    }
    if (!j.ok || !found) { set_error("Unexpected error detected on parse `taxonomies` as json (offset %zu)", (size_t)(j.p - f.data)); return BLU_ERR_PARSE; }
    return BLU_OK;
}

// the taxonomies file through load_db, then one label per row: the elements come back from the interned lineage (the raw rank
// and the identifier of every element are kept as written; a lineage the loader marked `bad` has none and gets no label)
int load_label_set(const char* taxonomies_file, bool use_taxid, int format, LabelSet& out) {
    Db db;
    if (const int rc = load_db(taxonomies_file, use_taxid, db); rc != BLU_OK) return rc;
    std::vector<uint32_t> kind(db.rank_raw.size());
    std::string other;
    for (size_t r = 0; r < kind.size(); ++r) {
        const uint16_t k = parse_rank(db.rank_raw[r].c_str(), &other);
        kind[r] = k >= K_DOMAIN && k <= K_SPECIES ? k : 0;
    }
    const size_t n = db.taxid.size();
    out.taxid = std::move(db.taxid);
    out.off.resize(n);
    out.len.resize(n);
    out.blob.clear();
    std::vector<LabelElement> el;
    for (size_t i = 0; i < n; ++i) {
        el.clear();
        for (uint64_t j = db.lin_off[i]; j < db.lin_off[i + 1]; ++j)
            el.push_back(LabelElement{kind[db.lin_rank[j]], db.rank_raw[db.lin_rank[j]].empty(), db.node_ident[db.lin_node[j]]});
        out.off[i] = out.blob.size();
        if (!db.bad[i]) (void)render_label(el.data(), el.size(), format, &out.blob);
        const size_t len = out.blob.size() - out.off[i];
        if (len >= (1ull << 32)) { set_error("seqdb: the label of taxid %lld is 4 GiB or longer", (long long)out.taxid[i]); return BLU_ERR_INVALID_ARG; }
        out.len[i] = (uint32_t)len;
    }
    out.row_of = std::move(db.row_of);
    return BLU_OK;
}

}  // namespace blu

using namespace blu;

extern "C" {

int blu_db_cache_build(const char* taxonomies_file, int use_taxid, const char* cache_file) {
    if (!taxonomies_file || !cache_file) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    Db db;
    int rc = load_db(taxonomies_file, use_taxid != 0, db);
    if (rc != BLU_OK) return rc;
    return write_db_cache(db, use_taxid != 0, cache_file);
}

int blu_seqdb_render_labels(const char* taxonomies_file, int use_taxid, int format, const char* out_path) {
    if (!taxonomies_file || !out_path || (format != BLU_SEQDB_SINTAX && format != BLU_SEQDB_DADA2)) {
        set_error("blu_seqdb_render_labels: null or invalid argument");
        return BLU_ERR_INVALID_ARG;
    }
    LabelSet labels;
    if (const int rc = load_label_set(taxonomies_file, use_taxid != 0, format, labels); rc != BLU_OK) return rc;
    std::string text;
    text.reserve(labels.blob.size() + 24 * labels.taxid.size());
    for (size_t i = 0; i < labels.taxid.size(); ++i) {
        text += std::to_string((long long)labels.taxid[i]);
        text += '\t';
        text.append(labels.blob, labels.off[i], labels.len[i]);
        text += '\n';
    }
    if (!write_text_file(out_path, text)) { set_error("seqdb: cannot write %s", out_path); return BLU_ERR_IO; }
    return BLU_OK;
}

// domain/dtos/taxon.rs:28-66: YAML (flat `key: value` lines) or JSON object with the eight fields
int blu_custom_taxon_from_file(const char* path, blu_cutoff_config* cfg) {
    if (!path || !cfg) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    const char* dot = strrchr(path, '.');
    if (!dot || (strcmp(dot, ".yaml") != 0 && strcmp(dot, ".json") != 0)) { set_error("Custom taxon file must be a YAML or JSON file"); return BLU_ERR_INVALID_ARG; }
    MappedFile f;
    if (!f.open(path)) { set_error("Could not open custom taxon file: %s", path); return BLU_ERR_IO; }
    static const char* fields[8] = {"domain", "kingdom", "phylum", "class", "order", "family", "genus", "species"};
    memset(cfg, 0, sizeof *cfg);
    cfg->taxon = BLU_TAXON_CUSTOM;
    cfg->has_custom = 1;
    auto set = [&](const std::string& k, double v) { for (int i = 0; i < 8; ++i) if (k == fields[i]) { cfg->custom[i] = (int16_t)v; cfg->custom_has[i] = 1; } };
    if (strcmp(dot, ".json") == 0) {
        Json j{f.data, f.data + f.size};
        std::string key;
        if (!j.eat('{')) { set_error("Could not parse custom taxon file from JSON"); return BLU_ERR_PARSE; }
        if (!j.peek('}')) do {
            double v;
            if (!j.string(&key) || !j.eat(':')) { j.ok = false; break; }
            if (j.peek('n')) { j.skip(); continue; }
            if (!j.number(&v)) break;
            set(key, v);
        } while (j.ok && j.eat(','));
        if (!j.ok) { set_error("Could not parse custom taxon file from JSON"); return BLU_ERR_PARSE; }
    } else {
        std::string text(f.data, f.size);
        size_t pos = 0;
        while (pos < text.size()) {
            size_t nl = text.find('\n', pos);
            std::string line = text.substr(pos, nl == std::string::npos ? std::string::npos : nl - pos);
            pos = nl == std::string::npos ? text.size() : nl + 1;
            size_t hash = line.find('#');
            if (hash != std::string::npos) line.resize(hash);
            size_t colon = line.find(':');
            if (colon == std::string::npos) continue;
            std::string k = line.substr(0, colon), v = line.substr(colon + 1);
            auto trim = [](std::string& s) { size_t a = s.find_first_not_of(" \t\r"), b = s.find_last_not_of(" \t\r"); s = a == std::string::npos ? "" : s.substr(a, b - a + 1); };
            trim(k); trim(v);
            if (v.empty() || v == "null" || v == "~") continue;
            set(k, atof(v.c_str()));
        }
    }
    if (!cfg->custom_has[0] || !cfg->custom_has[7]) { set_error("custom taxon file lacks the mandatory `domain`/`species` fields (taxon.rs:16-25)"); return BLU_ERR_PARSE; }
    return BLU_OK;
}

}  // extern "C"
