// The taxonomies half of `blu build-db qiime2` (core/src/use_cases/build_qiime_db_from_blutils_db/mod.rs:24-84): the
// `*.blutils.json` read as serde_json::from_str::<TaxonomiesMap> reads it (domain/dtos/taxonomies_map.rs), then one TSV line per
// accession in document order.  It runs on the host in one pass over the mapped document: the TSV is written beside the
// output and renamed into place only once the whole document has been accepted, so a document serde rejects leaves no file
// (the reference removes the old file, then fails before it writes one).
//
// What serde_json rejects and this rejects too: bytes that are not UTF-8 (read_to_string), JSON syntax errors, raw control
// characters and invalid escapes in strings, lone surrogates in \u escapes, nesting deeper than 128, trailing characters, a
// missing required field, a known field given twice, and a value of the wrong type (taxid: an integer in [0, 2^64) written
// without fraction or exponent; optionals: null or their type).  Unknown fields are skipped.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "blu_consensus.h"
#include "blu_internal.h"
#include "blu_pipeline.h"

namespace blu {
namespace {

constexpr int MAX_DEPTH = 128;                   // serde_json's recursion limit

struct Strict {
    const unsigned char* b;
    const unsigned char* p;
    const unsigned char* end;
    std::string err;                             // first error; parsing stops at it
    int depth = 0;

    bool fail(const char* what) {
        if (err.empty()) {
            uint64_t line = 1, col = 1;
            for (const unsigned char* q = b; q < p && q < end; ++q) { if (*q == '\n') { ++line; col = 1; } else ++col; }
            char buf[64];
            snprintf(buf, sizeof buf, " at line %llu column %llu", (unsigned long long)line, (unsigned long long)col);
            err = std::string(what) + buf;
        }
        return false;
    }
    void ws() { while (p < end && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) ++p; }
    bool peek(unsigned char c) { ws(); return p < end && *p == c; }
    bool expect(unsigned char c, const char* what) { ws(); if (p < end && *p == c) { ++p; return true; } return fail(what); }
    bool enter() { return ++depth <= MAX_DEPTH || fail("recursion limit exceeded"); }

    static int hex(unsigned char c) {
        return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1;
    }
    bool hex4(uint32_t* v) {
        if (end - p < 4) { p = end; return fail("EOF while parsing a string"); }
        uint32_t x = 0;
        for (int k = 0; k < 4; ++k) { const int h = hex(p[k]); if (h < 0) { p += k; return fail("invalid escape"); } x = x * 16 + (uint32_t)h; }
        p += 4;
        *v = x;
        return true;
    }
    static void utf8(std::string* o, uint32_t v) {
        if (v < 0x80) o->push_back((char)v);
        else if (v < 0x800) { o->push_back((char)(0xC0 | (v >> 6))); o->push_back((char)(0x80 | (v & 0x3F))); }
        else if (v < 0x10000) { o->push_back((char)(0xE0 | (v >> 12))); o->push_back((char)(0x80 | ((v >> 6) & 0x3F))); o->push_back((char)(0x80 | (v & 0x3F))); }
        else { o->push_back((char)(0xF0 | (v >> 18))); o->push_back((char)(0x80 | ((v >> 12) & 0x3F))); o->push_back((char)(0x80 | ((v >> 6) & 0x3F)));
               o->push_back((char)(0x80 | (v & 0x3F))); }
    }
    // one UTF-8 sequence starting at p (str::from_utf8's rules); its length, 0 if invalid
    size_t utf8_len() const {
        const unsigned char c = *p;
        size_t need; unsigned char lo = 0x80, hi = 0xBF;
        if (c >= 0xC2 && c <= 0xDF) need = 1;
        else if (c == 0xE0) { need = 2; lo = 0xA0; }
        else if ((c >= 0xE1 && c <= 0xEC) || c == 0xEE || c == 0xEF) need = 2;
        else if (c == 0xED) { need = 2; hi = 0x9F; }
        else if (c == 0xF0) { need = 3; lo = 0x90; }
        else if (c >= 0xF1 && c <= 0xF3) need = 3;
        else if (c == 0xF4) { need = 3; hi = 0x8F; }
        else return 0;
        if ((size_t)(end - p) <= need || p[1] < lo || p[1] > hi) return 0;
        for (size_t k = 2; k <= need; ++k) if ((p[k] & 0xC0) != 0x80) return 0;
        return need + 1;
    }
    // a JSON string, decoded into *out (nullptr: validated and skipped)
    bool string(std::string* out) {
        if (!expect('"', "expected a string")) return false;
        if (out) out->clear();
        for (;;) {
            const unsigned char* s = p;
            while (p < end && *p != '"' && *p != '\\' && *p >= 0x20 && *p < 0x80) ++p;
            if (out) out->append((const char*)s, (size_t)(p - s));
            if (p >= end) return fail("EOF while parsing a string");
            const unsigned char c = *p;
            if (c == '"') { ++p; return true; }
            if (c < 0x20) return fail("control character (\\u0000-\\u001F) found while parsing a string");
            if (c >= 0x80) {
                const size_t n = utf8_len();
                if (!n) return fail("invalid UTF-8");
                if (out) out->append((const char*)p, n);
                p += n;
                continue;
            }
            ++p;                                   // backslash
            if (p >= end) return fail("EOF while parsing a string");
            const unsigned char e = *p++;
            char r;
            switch (e) {
                case '"': r = '"'; break; case '\\': r = '\\'; break; case '/': r = '/'; break;
                case 'b': r = '\b'; break; case 'f': r = '\f'; break; case 'n': r = '\n'; break;
                case 'r': r = '\r'; break; case 't': r = '\t'; break;
                case 'u': {
                    uint32_t v;
                    if (!hex4(&v)) return false;
                    if (v >= 0xDC00 && v <= 0xDFFF) return fail("lone leading surrogate in hex escape");
                    if (v >= 0xD800 && v <= 0xDBFF) {
                        if (end - p < 2 || p[0] != '\\' || p[1] != 'u') return fail("unexpected end of hex escape");
                        p += 2;
                        uint32_t lo;
                        if (!hex4(&lo)) return false;
                        if (lo < 0xDC00 || lo > 0xDFFF) return fail("lone leading surrogate in hex escape");
                        v = 0x10000 + ((v - 0xD800) << 10) + (lo - 0xDC00);
                    }
                    if (out) utf8(out, v);
                    continue;
                }
                default: --p; return fail("invalid escape");
            }
            if (out) out->push_back(r);
        }
    }
    // a JSON number; *is_uint: written as a non-negative integer without fraction or exponent, *v its value if it fits u64
    bool number(bool* is_uint, uint64_t* v, bool* fits) {
        ws();
        const unsigned char* s = p;
        bool neg = false, frac = false;
        if (p < end && *p == '-') { neg = true; ++p; }
        if (p >= end || *p < '0' || *p > '9') return fail(neg ? "invalid number" : "expected value");
        uint64_t x = 0; bool ok = true;
        if (*p == '0') { ++p; if (p < end && *p >= '0' && *p <= '9') return fail("invalid number"); }
        else while (p < end && *p >= '0' && *p <= '9') { const uint64_t d = *p - '0'; ok = ok && x <= (~0ull - d) / 10; x = x * 10 + d; ++p; }
        if (p < end && *p == '.') {
            frac = true; ++p;
            if (p >= end || *p < '0' || *p > '9') return fail("invalid number");
            while (p < end && *p >= '0' && *p <= '9') ++p;
        }
        if (p < end && (*p == 'e' || *p == 'E')) {
            frac = true; ++p;
            if (p < end && (*p == '+' || *p == '-')) ++p;
            if (p >= end || *p < '0' || *p > '9') return fail("invalid number");
            while (p < end && *p >= '0' && *p <= '9') ++p;
        }
        (void)s;
        *is_uint = !neg && !frac;
        *v = x;
        *fits = ok;
        return true;
    }
    bool literal(const char* w) {
        const size_t n = strlen(w);
        if ((size_t)(end - p) < n || memcmp(p, w, n) != 0) return fail("expected value");
        p += n;
        return true;
    }
    bool null() { ws(); if (p < end && *p == 'n') return literal("null"); return false; }
    bool skip() {
        ws();
        if (p >= end) return fail("EOF while parsing a value");
        switch (*p) {
            case '"': return string(nullptr);
            case 't': return literal("true");
            case 'f': return literal("false");
            case 'n': return literal("null");
            case '{': {
                ++p;
                if (!enter()) return false;
                if (peek('}')) { ++p; --depth; return true; }
                for (;;) {
                    if (!string(nullptr) || !expect(':', "expected `:`") || !skip()) return false;
                    ws();
                    if (p < end && *p == ',') { ++p; continue; }
                    if (!expect('}', "expected `,` or `}`")) return false;
                    --depth;
                    return true;
                }
            }
            case '[': {
                ++p;
                if (!enter()) return false;
                if (peek(']')) { ++p; --depth; return true; }
                for (;;) {
                    if (!skip()) return false;
                    ws();
                    if (p < end && *p == ',') { ++p; continue; }
                    if (!expect(']', "expected `,` or `]`")) return false;
                    --depth;
                    return true;
                }
            }
            default: { bool u, f; uint64_t v; return number(&u, &v, &f); }
        }
    }
    bool u64(uint64_t* v, const char* field) {
        ws();
        if (p >= end) return fail("EOF while parsing a value");
        if (*p != '-' && (*p < '0' || *p > '9')) { skip(); return fail((std::string("invalid type for `") + field + "`: expected u64").c_str()); }
        bool u, fits;
        const unsigned char* at = p;
        if (!number(&u, v, &fits)) return false;
        if (!u || !fits) { p = at; return fail((std::string("invalid value for `") + field + "`: expected u64").c_str()); }
        return true;
    }
    bool str_field(std::string* out, const char* field) {
        ws();
        if (p < end && *p != '"') return fail((std::string("invalid type for `") + field + "`: expected a string").c_str());
        return string(out);
    }
    // an object: f(key) is called with p at the value and parses it; keys are decoded first
    template <class F>
    bool object(const char* what, F&& f) {
        ws();
        if (p >= end || *p != '{') return fail((std::string("invalid type: expected ") + what).c_str());
        ++p;
        if (!enter()) return false;
        if (peek('}')) { ++p; --depth; return true; }
        std::string key;
        for (;;) {
            if (!string(&key) || !expect(':', "expected `:`") || !f(key)) return false;
            ws();
            if (p < end && *p == ',') { ++p; continue; }
            if (!expect('}', "expected `,` or `}`")) return false;
            --depth;
            return true;
        }
    }
    template <class F>
    bool array(const char* what, F&& f) {
        ws();
        if (p >= end || *p != '[') return fail((std::string("invalid type: expected ") + what).c_str());
        ++p;
        if (!enter()) return false;
        if (peek(']')) { ++p; --depth; return true; }
        for (;;) {
            if (!f()) return false;
            ws();
            if (p < end && *p == ',') { ++p; continue; }
            if (!expect(']', "expected `,` or `]`")) return false;
            --depth;
            return true;
        }
    }
    bool dup(bool& seen, const std::string& key) {
        if (seen) return fail(("duplicate field `" + key + "`").c_str());
        seen = true;
        return true;
    }
};

struct Out {
    int fd;
    std::string buf;
    bool ok = true;
    void flush() {
        size_t o = 0;
        while (ok && o < buf.size()) {
            const ssize_t w = write(fd, buf.data() + o, buf.size() - o);
            if (w < 0 && errno == EINTR) continue;
            if (w <= 0) ok = false; else o += (size_t)w;
        }
        buf.clear();
    }
    void maybe_flush() { if (buf.size() >= (8u << 20)) flush(); }
};

// TaxonomiesMap (taxonomies_map.rs:4-12) -> the TSV lines of mod.rs:59-84
bool document(Strict& J, bool use_taxid, Out& O) {
    bool s_ver = false, s_ign = false, s_rep = false, s_drop = false, s_src = false, s_tax = false;
    std::string str, rank, num_lin, txt_lin, acc, oid;
    std::vector<std::pair<std::string, std::string>> accs;
    const bool ok = J.object("struct TaxonomiesMap", [&](const std::string& k) -> bool {
        if (k == "blutilsVersion") return J.dup(s_ver, k) && J.str_field(&str, "blutilsVersion");
        if (k == "sourceDatabase") return J.dup(s_src, k) && J.str_field(&str, "sourceDatabase");
        if (k == "ignoreTaxids") {
            if (!J.dup(s_ign, k)) return false;
            if (J.null()) return true;
            if (!J.err.empty()) return false;
            return J.array("a sequence (ignoreTaxids)", [&] { uint64_t v; return J.u64(&v, "ignoreTaxids"); });
        }
        if (k == "replaceRank") {
            if (!J.dup(s_rep, k)) return false;
            if (J.null()) return true;
            if (!J.err.empty()) return false;
            return J.object("a map (replaceRank)", [&](const std::string&) { return J.str_field(nullptr, "replaceRank"); });
        }
        if (k == "dropNonLinnaeanTaxonomies") {
            if (!J.dup(s_drop, k)) return false;
            J.ws();
            if (J.p < J.end && *J.p == 'n') return J.literal("null");
            if (J.p < J.end && *J.p == 't') return J.literal("true");
            if (J.p < J.end && *J.p == 'f') return J.literal("false");
            return J.fail("invalid type for `dropNonLinnaeanTaxonomies`: expected a boolean");
        }
        if (k == "taxonomies") {
            if (!J.dup(s_tax, k)) return false;
            return J.array("a sequence (taxonomies)", [&] {
                bool t_id = false, t_rank = false, t_num = false, t_txt = false, t_acc = false;
                uint64_t taxid = 0;
                accs.clear();
                const bool unit_ok = J.object("struct TaxonomyMapUnit", [&](const std::string& f) -> bool {
                    if (f == "taxid") return J.dup(t_id, f) && J.u64(&taxid, "taxid");
                    if (f == "rank") return J.dup(t_rank, f) && J.str_field(&rank, "rank");
                    if (f == "numericLineage") return J.dup(t_num, f) && J.str_field(&num_lin, "numericLineage");
                    if (f == "textLineage") return J.dup(t_txt, f) && J.str_field(&txt_lin, "textLineage");
                    if (f == "accessions") {
                        if (!J.dup(t_acc, f)) return false;
                        accs.clear();
                        return J.array("a sequence (accessions)", [&] {
                            bool a_acc = false, a_oid = false;
                            const bool acc_ok = J.object("struct Accession", [&](const std::string& g) -> bool {
                                if (g == "accession") return J.dup(a_acc, g) && J.str_field(&acc, "accession");
                                if (g == "oid") return J.dup(a_oid, g) && J.str_field(&oid, "oid");
                                return J.skip();
                            });
                            if (!acc_ok) return false;
                            if (!a_acc) return J.fail("missing field `accession`");
                            if (!a_oid) return J.fail("missing field `oid`");
                            accs.emplace_back(acc, oid);
                            return true;
                        });
                    }
                    return J.skip();
                });
                if (!unit_ok) return false;
                for (auto [seen, name] : {std::pair<bool, const char*>{t_id, "taxid"}, {t_rank, "rank"}, {t_num, "numericLineage"},
                                          {t_txt, "textLineage"}, {t_acc, "accessions"}})
                    if (!seen) return J.fail((std::string("missing field `") + name + "`").c_str());
                const std::string& lin = use_taxid ? num_lin : txt_lin;
                const std::string id = std::to_string(taxid);
                for (const auto& a : accs) {                     // mod.rs:64-74: "{taxid}-{oid}-{accession}\t{lineage}\n"
                    O.buf += id; O.buf += '-'; O.buf += a.second; O.buf += '-'; O.buf += a.first;
                    O.buf += '\t'; O.buf += lin; O.buf += '\n';
                }
                O.maybe_flush();
                return O.ok || J.fail("write failed");
            });
        }
        return J.skip();
    });
    if (!ok) return false;
    for (auto [seen, name] : {std::pair<bool, const char*>{s_ver, "blutilsVersion"}, {s_src, "sourceDatabase"}, {s_tax, "taxonomies"}})
        if (!seen) return J.fail((std::string("missing field `") + name + "`").c_str());
    J.ws();
    if (J.p != J.end) return J.fail("trailing characters");
    return true;
}

}  // namespace
}  // namespace blu

extern "C" int blu_qiime_taxonomy_tsv(const char* json_path, int use_taxid, const char* out_path) {
    if (!json_path || !out_path) { blu::set_error("blu_qiime_taxonomy_tsv: null argument"); return BLU_ERR_INVALID_ARG; }
    const int fd = open(json_path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) { blu::set_error("qiime2: cannot read %s: %s", json_path, strerror(errno)); return BLU_ERR_IO; }
    struct stat sb;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { close(fd); blu::set_error("qiime2: %s is not a regular file", json_path); return BLU_ERR_IO; }
    const size_t size = (size_t)sb.st_size;
    const unsigned char* data = nullptr;
    if (size) {
        void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
        if (m == MAP_FAILED) { close(fd); blu::set_error("qiime2: cannot map %s: %s", json_path, strerror(errno)); return BLU_ERR_IO; }
        (void)madvise(m, size, MADV_SEQUENTIAL);
        data = (const unsigned char*)m;
    }
    close(fd);
    struct Unmap { const unsigned char* d; size_t n; ~Unmap() { if (d) munmap((void*)d, n); } } unmap{data, size};
    if (size >= 8 && memcmp(data, "BLUDBC01", 8) == 0) {
        blu::set_error("qiime2: %s is a binary cache written by cache-db; it keeps no accessions, so pass the *.blutils.json it was "
                       "built from", json_path);
        return BLU_ERR_INVALID_ARG;
    }
    const std::string tmp = std::string(out_path) + ".partial";
    const int ofd = open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (ofd < 0) { blu::set_error("qiime2: cannot create %s: %s", tmp.c_str(), strerror(errno)); return BLU_ERR_IO; }
    blu::Out O{ofd};
    O.buf = "Feature ID\tTaxon\n";                                  // mod.rs:49-54
    blu::Strict J{data, data, data + size};
    bool ok = blu::document(J, use_taxid != 0, O);
    if (ok) O.flush();
    const bool wrote = O.ok;
    close(ofd);
    if (!ok || !wrote) {
        unlink(tmp.c_str());
        if (!ok) { blu::set_error("qiime2: %s: Unexpected error occurred on load table: %s", json_path, J.err.c_str()); return BLU_ERR_PARSE; }
        blu::set_error("qiime2: writing %s failed: %s", out_path, strerror(errno));
        return BLU_ERR_IO;
    }
    if (rename(tmp.c_str(), out_path) != 0) {
        unlink(tmp.c_str());
        blu::set_error("qiime2: cannot create %s: %s", out_path, strerror(errno));
        return BLU_ERR_IO;
    }
    return BLU_OK;
}
