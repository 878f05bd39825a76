// `blu build-db blu` on the GPU: NCBI taxdump + the `blastdbcmd -outfmt "%a  %T  %o"` listing -> *.blutils.json and
// *.non-mapped.tsv (reference: core/src/use_cases/build_blutils_db_from_ncbi_files/, build_taxonomy_database.rs:49-498;
// DESIGN.md "Taxonomies database builder" lists every rule with its rs: line and the test that covers it).
//
// Stages (all on the null stream of the call's device):
//   upload    the five dump files and the accession listing: pread into pinned staging -> HBM (the ingest's upload_file)
//   parse     line index (the ingest's newline count + scan), then one thread per dump line: `|` fields over aligned 16-byte
//             loads, trimmed spans, numeric ids, UTF-8 check with an all-ASCII fast path
//   tables    direct-addressed arrays over [0, max id]: winning line of nodes / lineage / names / merged (atomicMax of the
//             line: last line wins, one word per taxid), deleted flags, skip bitmap; the distinct rank strings (about 50)
//             interned through a small hash table that each node reads before it writes, then checked byte for byte
//   group     one thread per accession line (pieces on two spaces, taxid, escaped lengths), stable radix sort of
//             (taxid, line) with as many 8-bit passes as the largest taxid needs, segment starts
//   assemble  one thread per distinct taxid: resolution (node, deleted, merged, unknown), then both lineage strings by a
//             length pass, an exclusive scan and a write pass that walk the lineage text in place
//   render    the `taxonomies` array in document order: one length per accession row (the entry's header on its first row,
//             the footer on its last), one scan, one write thread per row; downloaded in pieces and written with write()
// The host keeps the document head and tail, the rank strings and the TSV (one line per unmapped taxid).  No device
// library is called; byte work bound by memory, no MFMA.
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "blu_consensus.h"
#include "blu_internal.h"
#include "blu_pipeline.h"
#include "ingest.h"
#include "ingest_prims.h"
#include "taxmap_entry_dev.h"
#include "text_dev.h"

namespace blu {
namespace {

constexpr int TPB = 256;
constexpr uint32_t NONE32 = 0xFFFFFFFFu;
constexpr uint16_t NO_RANK = 0xFFFF;
constexpr uint32_t ID_LIMIT = 0x80000000u;        // dump ids must lie in [0, 2^31) (rs:193-197 parse::<i32>)
constexpr uint32_t RANK_SLOTS = 4096;             // rank interning table (NCBI has about 50 ranks)
constexpr uint32_t MAX_RANKS = 2048;

// dump files, in the order the reference loads them (mod.rs:70-80 -> rs:101-118) and the order errors are reported
enum Dump : int { D_NODES = 0, D_LINEAGE = 1, D_NAMES = 2, D_MERGED = 3, D_DELNODES = 4, N_DUMPS = 5 };
__host__ __device__ constexpr int dump_cols(int m) { return m == D_NODES ? 3 : m == D_NAMES ? 4 : m == D_DELNODES ? 1 : 2; }

// error codes (the word is (line << 3) | code, atomicMin: the first bad line wins)
enum : uint32_t { E_FIELDS = 1, E_NUMBER = 2, E_RANGE = 3, E_PIECES = 4, E_TAXID = 5, E_ANCESTOR = 6, E_ANC_RANGE = 7 };

// per-segment status
enum : uint8_t { S_MAPPED = 0, S_MERGED_MAPPED = 1, S_DELETED = 2, S_MERGED_MISSING = 3, S_UNKNOWN = 4, S_DROPPED = 5, S_BEYOND = 6 };

constexpr uint32_t NULL4 = 'n' | ('u' << 8) | ('l' << 16) | ('l' << 24);   // "null" as a little-endian word

// signed decimal of a field (tabs inside removed first, load_dump_file.rs:52); false if not a number or beyond i64
__device__ __forceinline__ bool parse_i64(const unsigned char* __restrict__ text, uint64_t a, uint64_t b, bool skip_tabs, long long* out) {
    bool neg = false, any = false, first = true, ok = true;
    unsigned long long v = 0;
    for_bytes(text, a, b, [&](uint32_t c, uint64_t) {     // (selects, not branches: see taxdb_parse_dump)
        const bool tab = skip_tabs && c == '\t';
        const bool sign = !tab && first && (c == '+' || c == '-');
        const bool digit = !tab && !sign && c >= '0' && c <= '9';
        const unsigned long long nv = v * 10 + (c - '0');
        const bool bad = !tab && !sign && (!digit || v > (~0ull - 9) / 10 || nv > (neg ? (1ull << 63) : (1ull << 63) - 1));
        neg = sign ? c == '-' : neg;
        first = first && tab;
        v = digit && !bad ? nv : v;
        any = any || (digit && !bad);
        ok = ok && !bad;
        return !bad;
    });
    if (!ok || !any) return false;
    *out = neg ? (long long)(0ull - v) : (long long)v;
    return true;
}

__device__ __forceinline__ void block_reduce_add(unsigned long long v, unsigned long long* dst) {
    __shared__ unsigned long long part[TPB / 64];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < TPB / 64; ++w) s += part[w];
        if (s) atomicAdd(dst, s);
    }
    __syncthreads();
}
__device__ __forceinline__ void block_reduce_max(uint32_t v, uint32_t* dst) {
    __shared__ uint32_t part[TPB / 64];
    for (int d = 32; d > 0; d >>= 1) v = max(v, (uint32_t)__shfl_down(v, d));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < TPB / 64; ++w) s = max(s, part[w]);
        atomicMax(dst, s);
    }
    __syncthreads();
}

struct DumpOut {
    uint32_t* id;          // [n] the line's taxid, NONE32 = line skipped (not UTF-8)
    uint64_t* span_a;      // [n] trimmed field: rank (nodes), lineage (taxidlineage), name (names)
    uint32_t* span_len;    // [n]
    uint32_t* aux;         // [n] new taxid (merged), 1 = scientific name (names)
    unsigned long long* err;        // (line << 3) | code, atomicMin
    unsigned long long* counters;   // [0] valid lines [1] scientific names [2] lineage tokens [3] names with non-ASCII bytes
    uint32_t* max_id;
};

// ---- parse: one thread per dump line (load_dump_file.rs:37-57) --------------------------------------------------------
__global__ __launch_bounds__(TPB) void taxdb_parse_dump(const unsigned char* __restrict__ text, const uint64_t* __restrict__ line_start,
                                                        uint32_t n, int mode, DumpOut o) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    unsigned long long c_valid = 0, c_sci = 0, c_tok = 0, c_nonascii = 0;
    uint32_t my_max = 0;
    if (i < n) {
        const uint64_t s = line_start[i], e = line_start[i + 1] - 1;
        const int ncols = dump_cols(mode);
        uint64_t p0 = e, p1 = e, p2 = e, p3 = e;      // the first four '|' of the line
        int np = 0;
        bool high = false;
        for_bytes(text, s, e, [&](uint32_t c, uint64_t p) {
            high |= c >= 0x80;
            // selects, not branches: a conditional store to a by-reference capture ends up in scratch
            const bool bar = c == '|';
            p0 = (bar && np == 0) ? p : p0; p1 = (bar && np == 1) ? p : p1;
            p2 = (bar && np == 2) ? p : p2; p3 = (bar && np == 3) ? p : p3;
            np += bar ? 1 : 0;
            return true;
        });
        const unsigned long long fail = (unsigned long long)i << 3;
        uint32_t id = NONE32;
        if (high && !utf8_valid(text, s, e)) {
            // BufRead::lines + flat_map(Result::ok): the line is dropped
        } else if (np + 1 < ncols) {
            atomicMin(o.err, fail | E_FIELDS);
        } else {
            auto field = [&](int k, uint64_t& a, uint64_t& b) {
                a = k == 0 ? s : (k == 1 ? p0 : k == 2 ? p1 : p2) + 1;
                b = k == 0 ? p0 : k == 1 ? p1 : k == 2 ? p2 : p3;
                trim(text, a, b);
            };
            uint64_t a, b;
            field(0, a, b);
            long long v = 0;
            if (!parse_i64(text, a, b, true, &v)) atomicMin(o.err, fail | E_NUMBER);
            else if (v < 0 || v >= (long long)ID_LIMIT) atomicMin(o.err, fail | E_RANGE);
            else {
                id = (uint32_t)v;
                c_valid = 1;
                my_max = id;
                if (mode == D_MERGED) {
                    field(1, a, b);
                    if (!parse_i64(text, a, b, true, &v)) { atomicMin(o.err, fail | E_NUMBER); id = NONE32; }
                    else if (v < 0 || v >= (long long)ID_LIMIT) { atomicMin(o.err, fail | E_RANGE); id = NONE32; }
                    else { o.aux[i] = (uint32_t)v; my_max = max(my_max, (uint32_t)v); }
                } else if (mode != D_DELNODES) {
                    field(mode == D_NODES ? 2 : 1, a, b);
                    o.span_a[i] = a;
                    o.span_len[i] = (uint32_t)(b - a);
                    if (mode == D_NAMES) {
                        uint64_t ca, cb;
                        field(3, ca, cb);
                        const char* want = "scientific name";
                        int k = 0;
                        bool eq = true;
                        for_bytes(text, ca, cb, [&](uint32_t c, uint64_t) {
                            if (c == '\t') return true;
                            if (k >= 15 || c != (uint32_t)(unsigned char)want[k]) { eq = false; return false; }
                            ++k;
                            return true;
                        });
                        eq = eq && k == 15;
                        o.aux[i] = eq;
                        if (eq) {
                            c_sci = 1;
                            bool hi = false;
                            if (high) for_bytes(text, a, b, [&](uint32_t c, uint64_t) { hi |= c >= 0x80; return !hi; });
                            c_nonascii = hi;
                        }
                    } else if (mode == D_LINEAGE) {
                        // tokens of the lineage once quotes and tabs are gone, split on ' ': not empty and not "null"
                        uint32_t len = 0, h = 0;
                        auto end_tok = [&]() { if (len && !(len == 4 && h == NULL4)) ++c_tok; len = 0; h = 0; };
                        for_bytes(text, a, b, [&](uint32_t c, uint64_t) {
                            if (c == '"' || c == '\t') return true;
                            if (c == ' ') { end_tok(); return true; }
                            if (len < 4) h |= c << (8 * len);
                            ++len;
                            return true;
                        });
                        end_tok();
                    }
                }
            }
        }
        o.id[i] = id;
    }
    block_reduce_add(c_valid, &o.counters[0]);
    block_reduce_add(c_sci, &o.counters[1]);
    block_reduce_add(c_tok, &o.counters[2]);
    block_reduce_add(c_nonascii, &o.counters[3]);
    block_reduce_max(my_max, o.max_id);
}

// ---- tables: the winning line of each taxid (last line wins: HashMap inserts in file order) ------------------------
__global__ __launch_bounds__(TPB) void taxdb_last_line(const uint32_t* __restrict__ id, const uint32_t* __restrict__ only, uint32_t n,
                                                       uint32_t* __restrict__ row) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n || id[i] == NONE32 || (only && !only[i])) return;
    atomicMax(&row[id[i]], i + 1);
}
__global__ __launch_bounds__(TPB) void taxdb_mark(const uint32_t* __restrict__ id, uint32_t n, uint8_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i < n && id[i] != NONE32) flag[id[i]] = 1;
}
__global__ __launch_bounds__(TPB) void taxdb_mark_bits(const uint32_t* __restrict__ ids, uint32_t n, uint32_t* __restrict__ bits) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) atomicOr(&bits[ids[i] >> 5], 1u << (ids[i] & 31));
}

// the rank of a nodes line as the reference folds it: quotes and tabs removed, ASCII lower case (rs:199-206)
__device__ __forceinline__ uint32_t rank_byte(uint32_t c) { return (c >= 'A' && c <= 'Z') ? c + 32 : c; }
__device__ __forceinline__ unsigned long long rank_hash(const unsigned char* __restrict__ text, uint64_t a, uint32_t len) {
    unsigned long long h = 0xcbf29ce484222325ull;
    for_bytes(text, a, a + len, [&](uint32_t c, uint64_t) {
        if (c == '"' || c == '\t') return true;
        h = (h ^ rank_byte(c)) * 0x100000001b3ull;
        return true;
    });
    return h | 1ull;                       // 0 = empty slot
}

struct NodeTabs {
    const uint32_t* node_row; const uint32_t* lin_row; const uint32_t* name_row; const uint32_t* merged_row;
    const uint8_t* deleted; const uint32_t* skip_bits; uint32_t skip_limit;
    uint16_t* node_rank; uint32_t n_ids;
};

// every taxid of nodes ⋈ taxidlineage (inner join, rs:120-135): hash its rank and make sure the rank has a slot.  Each
// thread reads the slot first and writes only when its rank is not there yet: ~50 slots, ~50 CAS that succeed.
__global__ __launch_bounds__(TPB) void taxdb_rank_slots(const unsigned char* __restrict__ text, const uint64_t* __restrict__ span_a,
                                                        const uint32_t* __restrict__ span_len, const uint32_t* __restrict__ node_row,
                                                        const uint32_t* __restrict__ lin_row, uint32_t n_ids,
                                                        unsigned long long* __restrict__ node_hash, unsigned long long* __restrict__ slot_hash,
                                                        uint32_t* __restrict__ slot_line, uint32_t* __restrict__ full) {
    const uint32_t t = blockIdx.x * TPB + threadIdx.x;
    if (t >= n_ids) return;
    if (!node_row[t] || !lin_row[t]) { node_hash[t] = 0; return; }
    const uint32_t line = node_row[t] - 1;
    const unsigned long long h = rank_hash(text, span_a[line], span_len[line]);
    node_hash[t] = h;
    uint32_t k = (uint32_t)(h ^ (h >> 29)) & (RANK_SLOTS - 1);
    for (uint32_t probe = 0; probe < RANK_SLOTS; ++probe, k = (k + 1) & (RANK_SLOTS - 1)) {
        unsigned long long cur = __atomic_load_n(&slot_hash[k], __ATOMIC_RELAXED);
        if (cur == h) return;
        if (cur == 0) {
            cur = atomicCAS(&slot_hash[k], 0ull, h);
            if (cur == 0) { slot_line[k] = line; return; }
            if (cur == h) return;
        }
    }
    atomicOr(full, 1u);
}

// rank id of every node through its slot, checked against the slot's string byte for byte (two ranks with one hash -> error)
__global__ __launch_bounds__(TPB) void taxdb_rank_assign(const unsigned char* __restrict__ text, const uint64_t* __restrict__ span_a,
                                                         const uint32_t* __restrict__ span_len, const uint32_t* __restrict__ node_row,
                                                         uint32_t n_ids, const unsigned long long* __restrict__ node_hash,
                                                         const unsigned long long* __restrict__ slot_hash, const uint16_t* __restrict__ slot_rank,
                                                         const unsigned char* __restrict__ rank_text, const uint32_t* __restrict__ rank_off,
                                                         uint16_t* __restrict__ node_rank, uint32_t* __restrict__ collision) {
    const uint32_t t = blockIdx.x * TPB + threadIdx.x;
    if (t >= n_ids) return;
    const unsigned long long h = node_hash[t];
    if (!h) { node_rank[t] = NO_RANK; return; }
    uint32_t k = (uint32_t)(h ^ (h >> 29)) & (RANK_SLOTS - 1);
    while (slot_hash[k] != h) k = (k + 1) & (RANK_SLOTS - 1);
    const uint16_t r = slot_rank[k];
    const uint32_t line = node_row[t] - 1;
    uint32_t j = rank_off[r];
    const uint32_t end = rank_off[r + 1];
    bool eq = true;
    for_bytes(text, span_a[line], span_a[line] + span_len[line], [&](uint32_t c, uint64_t) {
        if (c == '"' || c == '\t') return true;
        if (j >= end || rank_text[j] != rank_byte(c)) { eq = false; return false; }
        ++j;
        return true;
    });
    if (!eq || j != end) atomicOr(collision, 1u);
    node_rank[t] = r;
}

// ---- group: one thread per accession line (build_accessions_map.rs:49-74) --------------------------------------------
struct AccOut {
    uint32_t* key;         // [n] taxid, or n_ids for a taxid beyond the tables (>= 2^31 or negative: unknown)
    uint32_t* val;         // [n] line
    unsigned long long* tax64;   // [n] the taxid as u64 (i64 cast)
    uint64_t* acc_a; uint32_t* acc_len;
    uint64_t* oid_a; uint32_t* oid_len;
    uint32_t* esc_len;     // [n] escaped accession + escaped oid
    unsigned long long* err;
    uint32_t* first_bad;   // first line that is not UTF-8: read_line fails there and the reference's loop ends
};

__global__ __launch_bounds__(TPB) void taxdb_parse_acc(const unsigned char* __restrict__ text, const uint64_t* __restrict__ line_start,
                                                       uint32_t n, uint32_t n_ids, AccOut o) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const uint64_t s = line_start[i], e = line_start[i + 1] - 1;
    uint64_t sep0 = e, sep1 = e;              // the first two "  " separators (str::split: leftmost, non-overlapping)
    int ns = 0;
    bool prev_sp = false, high = false;
    for_bytes(text, s, e, [&](uint32_t c, uint64_t p) {
        high |= c >= 0x80;
        const bool cut = c == ' ' && prev_sp;         // (selects, as in taxdb_parse_dump)
        sep0 = (cut && ns == 0) ? p - 1 : sep0;
        sep1 = (cut && ns == 1) ? p - 1 : sep1;
        ns += cut ? 1 : 0;
        prev_sp = c == ' ' && !cut;
        return true;
    });
    o.key[i] = n_ids;
    o.val[i] = i;
    if (high && !utf8_valid(text, s, e)) { atomicMin(o.first_bad, i); return; }
    const unsigned long long fail = (unsigned long long)i << 3;
    if (ns < 2) { atomicMin(o.err, fail | E_PIECES); return; }
    uint64_t a0 = s, b0 = sep0, a1 = sep0 + 2, b1 = sep1, a2 = sep1 + 2, b2 = e;
    if (ns > 2) {   // a third separator ends the oid piece: find it again (rare)
        bool pv = false;
        uint64_t cut = e;
        for_bytes(text, a2, e, [&](uint32_t c, uint64_t p) {
            if (c == ' ' && pv) { cut = p - 1; return false; }
            pv = c == ' ';
            return true;
        });
        b2 = cut;
    }
    trim(text, a0, b0); trim(text, a1, b1); trim(text, a2, b2);
    long long v = 0;
    if (!parse_i64(text, a1, b1, false, &v)) { atomicMin(o.err, fail | E_TAXID); return; }
    const unsigned long long u = (unsigned long long)v;
    o.tax64[i] = u;
    o.key[i] = u < n_ids ? (uint32_t)u : n_ids;
    o.acc_a[i] = a0; o.acc_len[i] = (uint32_t)(b0 - a0);
    o.oid_a[i] = a2; o.oid_len[i] = (uint32_t)(b2 - a2);
    o.esc_len[i] = esc_len(text, a0, b0) + esc_len(text, a2, b2);
}

__global__ __launch_bounds__(TPB) void taxdb_heads(const uint32_t* __restrict__ key, uint32_t n, uint32_t* __restrict__ head) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) head[i] = (i == 0 || key[i] != key[i - 1]) ? 1u : 0u;
}
__global__ __launch_bounds__(TPB) void taxdb_seg_ids(const uint32_t* __restrict__ head, const uint32_t* __restrict__ excl, const uint32_t* __restrict__ key,
                                                     uint32_t n, uint32_t* __restrict__ seg_of, uint32_t* __restrict__ seg_start,
                                                     uint32_t* __restrict__ seg_key) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = excl[i] + head[i] - 1;
    seg_of[i] = s;
    if (head[i]) { seg_start[s] = i; seg_key[s] = key[i]; }
}

// ---- assemble ------------------------------------------------------------------------------------------------------
struct Names {   // what a lineage level needs of its taxon
    const unsigned char* text; const uint64_t* a; const uint32_t* len;    // names.dmp text and the name span of each line
};
struct RankTabs {
    const unsigned char* tok; const uint32_t* lin_off; const uint32_t* leaf_off;   // lineage tokens (replaced), leaf tokens
    const uint8_t* lin_drop; const uint8_t* leaf_drop;
};
struct LinText { const unsigned char* text; const uint64_t* a; const uint32_t* len; };   // taxidlineage.dmp lineage spans

__device__ __forceinline__ bool exists(const NodeTabs& T, uint32_t t) { return t < T.n_ids && T.node_rank[t] != NO_RANK; }

// slug of a taxon's name (rs:226-231: quotes removed; empty or "null" -> taxid-<id>; then slugify_ascii); out may be null
__device__ __forceinline__ uint32_t name_slug(const NodeTabs& T, const Names& N, uint32_t t, unsigned char* out) {
    uint64_t a = 0;
    uint32_t len = 0;
    if (T.name_row[t]) { a = N.a[T.name_row[t] - 1]; len = N.len[T.name_row[t] - 1]; }
    uint32_t kept = 0, h = 0;
    for_bytes(N.text, a, a + len, [&](uint32_t c, uint64_t) {
        if (c == '"' || c == '\t') return true;
        if (kept < 4) h |= c << (8 * kept);
        ++kept;
        return kept <= 4;
    });
    if (kept == 0 || (kept == 4 && h == NULL4)) {
        const uint32_t d = n_digits(t);
        if (out) { const char* p = "taxid-"; for (int k = 0; k < 6; ++k) out[k] = (unsigned char)p[k]; put_digits(out + 6, t, d); }
        return 6 + d;
    }
    uint32_t n = 0;
    bool pending = false;
    for_bytes(N.text, a, a + len, [&](uint32_t c, uint64_t) {
        if (c == '"' || c == '\t') return true;        // removed before the slug (a tab inside a name joins its sides)
        if (c >= 'A' && c <= 'Z') c += 32;
        if ((c >= 'a' && c <= 'z') || (c >= '0' && c <= '9')) {
            if (pending && n) { if (out) out[n] = '-'; ++n; }
            pending = false;
            if (out) out[n] = (unsigned char)c;
            ++n;
        } else {
            pending = true;
        }
        return true;
    });
    return n;
}

struct Ctx { NodeTabs T; LinText L; Names N; RankTabs R; int drop; const uint32_t* merged_to; };

// Walk the lineage of node m (rs:345-424) and build both strings for output taxid t (rs:440-466): length only when num /
// txt are null.  Levels: tokens of the lineage text once quotes and tabs are gone, split on ' '; empty and "null" skipped,
// then the skip list, then ancestors without a node (counted in *warn), then -d on the replaced rank.  false: a token
// that is not an id (err set).
__device__ __forceinline__ bool assemble(const Ctx& C, uint32_t m, uint32_t t, uint32_t* warn, unsigned long long* err, unsigned char* num,
                         unsigned char* txt, unsigned long long* nl_out, unsigned long long* tl_out) {
    const NodeTabs& T = C.T;
    const uint32_t line = T.lin_row[m] - 1;
    const uint64_t a = C.L.a[line], b = a + C.L.len[line];
    unsigned long long nl = 0, tl = 0;
    uint32_t levels = 0;
    uint32_t raw = 0, phase = 0;          // 0 leading white space, 4 after '+', 1 digits, 2 trailing white space, 3 not an id
    unsigned long long v = 0;
    bool big = false, ok = true;
    uint32_t h = 0;
    auto level = [&](uint32_t anc, uint32_t rk) {
        const unsigned char* tok = C.R.tok + C.R.lin_off[rk];
        const uint32_t tn = C.R.lin_off[rk + 1] - C.R.lin_off[rk], d = n_digits(anc);
        if (num) {
            unsigned char* o = num + nl;
            for (uint32_t k = 0; k < tn; ++k) o[k] = tok[k];
            o[tn] = '_'; o[tn + 1] = '_';
            put_digits(o + tn + 2, anc, d);
            o[tn + 2 + d] = ';';
        }
        nl += tn + 3 + d;
        if (txt) {
            unsigned char* o = txt + tl;
            for (uint32_t k = 0; k < tn; ++k) o[k] = tok[k];
            o[tn] = '_'; o[tn + 1] = '_';
        }
        const uint32_t sl = name_slug(T, C.N, anc, txt ? txt + tl + tn + 2 : nullptr);
        if (txt) txt[tl + tn + 2 + sl] = ';';
        tl += tn + 3 + sl;
        ++levels;
    };
    auto end_tok = [&]() -> bool {
        const bool skip = raw == 0 || (raw == 4 && h == NULL4);
        const unsigned long long val = v;
        const uint32_t ph = phase;
        const bool bg = big;
        raw = 0; v = 0; phase = 0; big = false; h = 0;
        if (skip) return true;
        if (ph != 1 && ph != 2) { atomicMin(err, ((unsigned long long)line << 3) | E_ANCESTOR); return false; }
        if (bg || val >= ID_LIMIT) { atomicMin(err, ((unsigned long long)line << 3) | E_ANC_RANGE); return false; }
        const uint32_t anc = (uint32_t)val;
        if (anc < T.skip_limit && ((T.skip_bits[anc >> 5] >> (anc & 31)) & 1u)) return true;
        if (!exists(T, anc)) { ++*warn; return true; }
        const uint16_t rk = T.node_rank[anc];
        if (C.drop && C.R.lin_drop[rk]) return true;
        level(anc, rk);
        return true;
    };
    for_bytes(C.L.text, a, b, [&](uint32_t c, uint64_t) {
        if (c == '"' || c == '\t') return true;
        if (c == ' ') { ok = end_tok(); return ok; }
        if (raw < 4) h |= c << (8 * raw);
        ++raw;
        // str::trim then parse::<u64>: white space only around, one optional '+', digits
        if (is_ws(c)) phase = phase == 0 ? 0 : phase == 1 || phase == 2 ? 2 : 3;
        else if (c >= '0' && c <= '9') {
            if (phase == 0 || phase == 4 || phase == 1) { phase = 1; if (v > 0x0FFFFFFFFFFFFFFFull) big = true; else v = v * 10 + (c - '0'); }
            else phase = 3;
        } else phase = (c == '+' && phase == 0) ? 4 : 3;
        return true;
    });
    if (ok) ok = end_tok();
    if (!ok) return false;
    // join(";") + ";" + leaf: each level already carries its ';', an empty lineage gives the leading one
    if (levels == 0) { if (num) num[nl] = ';'; if (txt) txt[tl] = ';'; ++nl; ++tl; }
    const uint32_t rk = T.node_rank[m];
    const unsigned char* tok = C.R.tok + C.R.leaf_off[rk];
    const uint32_t tn = C.R.leaf_off[rk + 1] - C.R.leaf_off[rk], d = n_digits(t);
    if (num) { unsigned char* o = num + nl; for (uint32_t k = 0; k < tn; ++k) o[k] = tok[k]; o[tn] = '_'; o[tn + 1] = '_'; put_digits(o + tn + 2, t, d); }
    nl += tn + 2 + d;
    if (txt) { unsigned char* o = txt + tl; for (uint32_t k = 0; k < tn; ++k) o[k] = tok[k]; o[tn] = '_'; o[tn + 1] = '_'; }
    tl += tn + 2 + name_slug(T, C.N, m, txt ? txt + tl + tn + 2 : nullptr);
    *nl_out = nl;
    *tl_out = tl;
    return true;
}

struct SegOut {
    uint8_t* status; uint32_t* node; uint32_t* warn;
    unsigned long long* num_len; unsigned long long* txt_len;
    unsigned long long* err;
};

// one thread per distinct taxid: resolution (rs:283-343, in this order) and the lengths of both lineages
__global__ __launch_bounds__(TPB) void taxdb_resolve(const uint32_t* __restrict__ seg_key, uint32_t n_seg, Ctx C, SegOut o) {
    const uint32_t s = blockIdx.x * TPB + threadIdx.x;
    if (s >= n_seg) return;
    const NodeTabs& T = C.T;
    const uint32_t t = seg_key[s];
    uint32_t warn = 0, m = t;
    unsigned long long nl = 0, tl = 0;
    uint8_t st;
    if (t >= T.n_ids) st = S_BEYOND;                                    // beyond every table: unknown (host side)
    else if (exists(T, t)) st = S_MAPPED;                               // 1. the node
    else if (T.deleted[t]) st = S_DELETED;                              // 2. deleted
    else if (T.merged_row[t]) {                                         // 3./4. merged into a node / into nothing
        m = C.merged_to[T.merged_row[t] - 1];
        st = exists(T, m) ? S_MERGED_MAPPED : S_MERGED_MISSING;
    } else st = S_UNKNOWN;                                              // 5.
    if (st == S_MAPPED || st == S_MERGED_MAPPED) {
        if (!assemble(C, m, t, &warn, o.err, nullptr, nullptr, &nl, &tl)) { nl = tl = 0; }
        if (C.drop && C.R.leaf_drop[T.node_rank[m]]) { st = S_DROPPED; nl = tl = 0; }   // rs:426-438: the whole taxid
    }
    o.status[s] = st;
    o.node[s] = m;
    o.warn[s] = warn;
    o.num_len[s] = nl;
    o.txt_len[s] = tl;
}

__global__ __launch_bounds__(TPB) void taxdb_lineages(const uint32_t* __restrict__ seg_key, uint32_t n_seg, Ctx C, const uint8_t* __restrict__ status,
                                                      const uint32_t* __restrict__ node, const unsigned long long* __restrict__ num_off,
                                                      const unsigned long long* __restrict__ txt_off, unsigned char* __restrict__ num,
                                                      unsigned char* __restrict__ txt) {
    const uint32_t s = blockIdx.x * TPB + threadIdx.x;
    if (s >= n_seg || (status[s] != S_MAPPED && status[s] != S_MERGED_MAPPED)) return;
    uint32_t warn = 0;
    unsigned long long nl, tl, err = ~0ull;
    assemble(C, node[s], seg_key[s], &warn, &err, num + num_off[s], txt + txt_off[s], &nl, &tl);
}

// ---- render ----------------------------------------------------------------------------------------------------------
// (the pieces of one entry, the escapes and the byte writers: taxmap_entry_dev.h)
struct RowIn {
    const uint32_t* seg_of; const uint32_t* seg_start; const uint32_t* seg_key; const uint8_t* status; const uint32_t* node;
    const unsigned long long* num_off; const unsigned long long* num_len; const unsigned long long* txt_off;
    const unsigned long long* txt_len; const unsigned char* num; const unsigned char* txt;
    const uint32_t* line;                  // sorted position -> accession line
    const uint32_t* esc_len; const uint64_t* acc_a; const uint32_t* acc_len; const uint64_t* oid_a; const uint32_t* oid_len;
    const unsigned char* acc_text;
    const unsigned char* leaf_tok; const uint32_t* leaf_off; const uint16_t* node_rank;
};

__device__ __forceinline__ bool row_emitted(const RowIn& R, uint32_t s) { return R.status[s] == S_MAPPED || R.status[s] == S_MERGED_MAPPED; }

__global__ __launch_bounds__(TPB) void taxdb_row_len(RowIn R, uint32_t n, unsigned long long* __restrict__ len) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i > n) return;
    if (i == n) { len[i] = 0; return; }
    const uint32_t s = R.seg_of[i];
    if (!row_emitted(R, s)) { len[i] = 0; return; }
    unsigned long long l = cl(A0) + cl(A1) + cl(A2) + R.esc_len[R.line[i]];
    l += (i + 1 == R.seg_start[s + 1]) ? cl(A_LAST) : cl(A_NEXT);
    if (i == R.seg_start[s]) {
        const uint16_t rk = R.node_rank[R.node[s]];
        l += cl(H0) + n_digits(R.seg_key[s]) + cl(H1) + (R.leaf_off[rk + 1] - R.leaf_off[rk]) + cl(H2) + R.num_len[s] + cl(H3) +
             R.txt_len[s] + cl(H4);
    }
    len[i] = l;
}

__global__ __launch_bounds__(TPB) void taxdb_row_write(RowIn R, uint32_t n, const unsigned long long* __restrict__ off, unsigned char* __restrict__ doc) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = R.seg_of[i];
    if (!row_emitted(R, s)) return;
    unsigned char* o = doc + off[i];
    if (i == R.seg_start[s]) {
        const uint32_t t = R.seg_key[s];
        const uint16_t rk = R.node_rank[R.node[s]];
        o = put(o, H0);
        const uint32_t d = n_digits(t);
        put_digits(o, t, d);
        o = put(o + d, H1);
        o = put_bytes(o, R.leaf_tok + R.leaf_off[rk], R.leaf_off[rk + 1] - R.leaf_off[rk]);
        o = put(o, H2);
        o = put_bytes(o, R.num + R.num_off[s], R.num_len[s]);
        o = put(o, H3);
        o = put_bytes(o, R.txt + R.txt_off[s], R.txt_len[s]);
        o = put(o, H4);
    }
    const uint32_t ln = R.line[i];
    o = put(o, A0);
    o = put_escaped(o, R.acc_text, R.acc_a[ln], R.acc_len[ln]);
    o = put(o, A1);
    o = put_escaped(o, R.acc_text, R.oid_a[ln], R.oid_len[ln]);
    o = put(o, A2);
    put(o, (i + 1 == R.seg_start[s + 1]) ? A_LAST : A_NEXT);
}

__global__ __launch_bounds__(TPB) void taxdb_gather_u64(const unsigned long long* __restrict__ src, const uint32_t* __restrict__ idx, uint32_t n,
                                                        unsigned long long* __restrict__ dst) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

}  // namespace

namespace {

struct Parsed {
    uint32_t* id = nullptr; uint64_t* span_a = nullptr; uint32_t* span_len = nullptr; uint32_t* aux = nullptr;
    unsigned long long counters[4] = {0, 0, 0, 0};
    uint32_t max_id = 0;
};

// LinnaeanRank::from_str + Display (linnaean_ranks.rs:55-90): the letter, or the slug of an Other rank
std::string rank_token(const std::string& r, bool* other) {
    // parse_rank reads a C string and a rank may hold a NUL: to both of its rules (trim + letter match, slug) NUL is what 0x01
    // is, a byte that is neither white space nor [a-z0-9]
    std::string s = r, slug;
    std::replace(s.begin(), s.end(), '\0', '\x01');
    const uint16_t k = parse_rank(s.c_str(), &slug);
    *other = k == K_FIRST_OTHER;
    return *other ? slug : std::string(1, "udkpcofgs"[k]);
}

int build(const blu_taxdb_desc& D, blu_taxdb_stats& S) {
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) {
        (void)hipGetLastError();
        set_error("build-db: no HIP device (the builder runs on the GPU only)");
        return BLU_ERR_NO_DEVICE;
    }
    if (D.device < 0 || D.device >= n_dev || hipSetDevice(D.device) != hipSuccess) { set_error("build-db: no HIP device %d", D.device); return BLU_ERR_NO_DEVICE; }
    HipPolicy pol{"build-db", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    double t0 = now_s();
    auto lap = [&](double* field) { (void)hipDeviceSynchronize(); const double t = now_s(); *field += 1e3 * (t - t0); t0 = t; };

    // ---- upload + line index of every input (the line index is part of the parse stage's time)
    const char* paths[N_DUMPS] = {D.nodes_path, D.lineage_path, D.names_path, D.merged_path, D.delnodes_path};
    DeviceText txt[N_DUMPS], acc;
    for (int m = 0; m < N_DUMPS; ++m)
        if (const int rc = load_text(paths[m], D.device, mem, txt[m]); rc != BLU_OK) return rc;
    if (const int rc = load_text(D.accessions_path, D.device, mem, acc); rc != BLU_OK) return rc;
    lap(&S.t_upload_ms);

    // ---- parse the dumps
    Parsed P[N_DUMPS];
    unsigned long long* d_err = nullptr;
    unsigned long long* d_cnt = nullptr;
    uint32_t* d_max = nullptr;
    HIP_CHECK(pol, mem.alloc(&d_err, 8 * N_DUMPS, "counters"));
    HIP_CHECK(pol, mem.alloc(&d_cnt, 32 * N_DUMPS, "counters"));
    HIP_CHECK(pol, mem.alloc(&d_max, 4 * N_DUMPS, "counters"));
    HIP_CHECK(pol, hipMemset(d_err, 0xFF, 8 * N_DUMPS));
    HIP_CHECK(pol, hipMemset(d_cnt, 0, 32 * N_DUMPS));
    HIP_CHECK(pol, hipMemset(d_max, 0, 4 * N_DUMPS));
    for (int m = 0; m < N_DUMPS; ++m) {
        const uint32_t n = txt[m].n_lines;
        Parsed& p = P[m];
        HIP_CHECK(pol, mem.alloc(&p.id, (size_t)n * 4, "parsed dump"));
        HIP_CHECK(pol, mem.alloc(&p.span_a, (size_t)n * 8, "parsed dump"));
        HIP_CHECK(pol, mem.alloc(&p.span_len, (size_t)n * 4, "parsed dump"));
        HIP_CHECK(pol, mem.alloc(&p.aux, (size_t)n * 4, "parsed dump"));
        DumpOut o{p.id, p.span_a, p.span_len, p.aux, d_err + m, d_cnt + 4 * m, d_max + m};
        if (n) hipLaunchKernelGGL(taxdb_parse_dump, dim3(grid(n)), dim3(TPB), 0, 0, (const unsigned char*)txt[m].d, (const uint64_t*)txt[m].line, n, m, o);
    }
    HIP_CHECK(pol, hipGetLastError());
    {
        unsigned long long err[N_DUMPS], cnt[4 * N_DUMPS];
        uint32_t mx[N_DUMPS];
        HIP_CHECK(pol, hipMemcpy(err, d_err, sizeof err, hipMemcpyDeviceToHost));
        HIP_CHECK(pol, hipMemcpy(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost));
        HIP_CHECK(pol, hipMemcpy(mx, d_max, sizeof mx, hipMemcpyDeviceToHost));
        for (int m = 0; m < N_DUMPS; ++m) {
            if (err[m] != ~0ull) {
                const uint32_t code = (uint32_t)(err[m] & 7);
                const char* what = code == E_FIELDS ? "fewer `|`-separated fields than the file needs"
                                 : code == E_NUMBER ? "a taxid that is not a number" : "a taxid outside 0..2147483647";
                set_error("%s:%llu: %s", paths[m], (err[m] >> 3) + 1, what);
                return BLU_ERR_PARSE;
            }
            memcpy(P[m].counters, cnt + 4 * m, 32);
            P[m].max_id = mx[m];
        }
    }
    S.n_nodes = P[D_NODES].counters[0];
    S.n_names = P[D_NAMES].counters[1];
    S.n_lineage_tokens = P[D_LINEAGE].counters[2];
    S.n_nonascii_names = P[D_NAMES].counters[3];
    lap(&S.t_parse_ms);

    // ---- tables over [0, n_ids)
    uint32_t max_id = 0;
    for (int m = 0; m < N_DUMPS; ++m) max_id = std::max(max_id, P[m].max_id);
    const uint32_t n_ids = max_id + 1;
    uint32_t *node_row, *lin_row, *name_row, *merged_row, *skip_bits;
    uint8_t* deleted;
    unsigned long long* node_hash;
    uint16_t* node_rank;
    HIP_CHECK(pol, mem.alloc(&node_row, (size_t)n_ids * 4, "taxid tables"));
    HIP_CHECK(pol, mem.alloc(&lin_row, (size_t)n_ids * 4, "taxid tables"));
    HIP_CHECK(pol, mem.alloc(&name_row, (size_t)n_ids * 4, "taxid tables"));
    HIP_CHECK(pol, mem.alloc(&merged_row, (size_t)n_ids * 4, "taxid tables"));
    HIP_CHECK(pol, mem.alloc(&deleted, (size_t)n_ids, "taxid tables"));
    HIP_CHECK(pol, mem.alloc(&node_hash, (size_t)n_ids * 8, "taxid tables"));
    HIP_CHECK(pol, mem.alloc(&node_rank, (size_t)n_ids * 2, "taxid tables"));
    HIP_CHECK(pol, hipMemset(node_row, 0, (size_t)n_ids * 4)); HIP_CHECK(pol, hipMemset(lin_row, 0, (size_t)n_ids * 4));
    HIP_CHECK(pol, hipMemset(name_row, 0, (size_t)n_ids * 4)); HIP_CHECK(pol, hipMemset(merged_row, 0, (size_t)n_ids * 4));
    HIP_CHECK(pol, hipMemset(deleted, 0, n_ids));
    auto last_line = [&](int m, const uint32_t* only, uint32_t* row) {
        if (txt[m].n_lines) hipLaunchKernelGGL(taxdb_last_line, dim3(grid(txt[m].n_lines)), dim3(TPB), 0, 0, (const uint32_t*)P[m].id, only, txt[m].n_lines, row);
    };
    last_line(D_NODES, nullptr, node_row);
    last_line(D_LINEAGE, nullptr, lin_row);
    last_line(D_NAMES, P[D_NAMES].aux, name_row);     // scientific names only (load_names_dataframe.rs:20-32)
    last_line(D_MERGED, nullptr, merged_row);
    if (txt[D_DELNODES].n_lines) hipLaunchKernelGGL(taxdb_mark, dim3(grid(txt[D_DELNODES].n_lines)), dim3(TPB), 0, 0, (const uint32_t*)P[D_DELNODES].id, txt[D_DELNODES].n_lines, deleted);
    // skip bitmap: over the tables, widened to the largest -s id that an ancestor can carry (< 2^31)
    std::vector<uint32_t> skip_ids;
    uint32_t skip_limit = n_ids;
    if (D.has_skip) for (uint64_t k = 0; k < D.n_skip; ++k) if (D.skip_taxids[k] < ID_LIMIT) {
        skip_ids.push_back((uint32_t)D.skip_taxids[k]);
        skip_limit = std::max(skip_limit, (uint32_t)D.skip_taxids[k] + 1);
    }
    const size_t skip_words = ((size_t)skip_limit + 31) / 32;
    HIP_CHECK(pol, mem.alloc(&skip_bits, skip_words * 4, "skip bitmap"));
    HIP_CHECK(pol, hipMemset(skip_bits, 0, skip_words * 4));
    if (!skip_ids.empty()) {
        uint32_t* d_ids;
        HIP_CHECK(pol, mem.alloc(&d_ids, skip_ids.size() * 4, "skip list"));
        HIP_CHECK(pol, hipMemcpy(d_ids, skip_ids.data(), skip_ids.size() * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(taxdb_mark_bits, dim3(grid(skip_ids.size())), dim3(TPB), 0, 0, (const uint32_t*)d_ids, (uint32_t)skip_ids.size(), skip_bits);
    }
    // ranks: slots on the device, strings and tokens on the host
    unsigned long long* slot_hash;
    uint32_t *slot_line, *flags;
    HIP_CHECK(pol, mem.alloc(&slot_hash, RANK_SLOTS * 8, "rank slots"));
    HIP_CHECK(pol, mem.alloc(&slot_line, RANK_SLOTS * 4, "rank slots"));
    HIP_CHECK(pol, mem.alloc(&flags, 8, "rank slots"));
    HIP_CHECK(pol, hipMemset(slot_hash, 0, RANK_SLOTS * 8));
    HIP_CHECK(pol, hipMemset(flags, 0, 8));
    hipLaunchKernelGGL(taxdb_rank_slots, dim3(grid(n_ids)), dim3(TPB), 0, 0, (const unsigned char*)txt[D_NODES].d, (const uint64_t*)P[D_NODES].span_a,
                       (const uint32_t*)P[D_NODES].span_len, (const uint32_t*)node_row, (const uint32_t*)lin_row, n_ids, node_hash, slot_hash, slot_line, flags);
    HIP_CHECK(pol, hipGetLastError());
    std::vector<unsigned long long> h_slot_hash(RANK_SLOTS);
    std::vector<uint32_t> h_slot_line(RANK_SLOTS);
    uint32_t h_flags[2];
    HIP_CHECK(pol, hipMemcpy(h_flags, flags, 8, hipMemcpyDeviceToHost));
    if (h_flags[0]) { set_error("build-db: %s has more distinct ranks than the rank table holds (%u)", D.nodes_path, RANK_SLOTS); return BLU_ERR_INVALID_ARG; }
    HIP_CHECK(pol, hipMemcpy(h_slot_hash.data(), slot_hash, RANK_SLOTS * 8, hipMemcpyDeviceToHost));
    HIP_CHECK(pol, hipMemcpy(h_slot_line.data(), slot_line, RANK_SLOTS * 4, hipMemcpyDeviceToHost));
    std::vector<uint16_t> slot_rank(RANK_SLOTS, 0);
    std::string rank_text, tok;
    std::vector<uint32_t> rank_off{0}, lin_off, leaf_off;
    std::vector<uint8_t> lin_drop, leaf_drop;
    std::vector<std::string> ranks;
    // -r pairs: HashMap semantics (a repeated key keeps its last value)
    std::vector<std::pair<std::string, std::string>> rep;
    if (D.has_replace) for (uint64_t k = 0; k < D.n_replace; ++k) {
        auto it = std::find_if(rep.begin(), rep.end(), [&](const auto& p) { return p.first == D.replace_from[k]; });
        if (it != rep.end()) it->second = D.replace_to[k];
        else rep.emplace_back(D.replace_from[k], D.replace_to[k]);
    }
    for (uint32_t k = 0; k < RANK_SLOTS; ++k) {
        if (!h_slot_hash[k]) continue;
        if (ranks.size() >= MAX_RANKS) { set_error("build-db: %s has more than %u distinct ranks", D.nodes_path, MAX_RANKS); return BLU_ERR_INVALID_ARG; }
        uint64_t a = 0;
        uint32_t len = 0;
        HIP_CHECK(pol, hipMemcpy(&a, P[D_NODES].span_a + h_slot_line[k], 8, hipMemcpyDeviceToHost));
        HIP_CHECK(pol, hipMemcpy(&len, P[D_NODES].span_len + h_slot_line[k], 4, hipMemcpyDeviceToHost));
        std::string raw(len, '\0'), r;
        if (len) HIP_CHECK(pol, hipMemcpy(&raw[0], txt[D_NODES].d + a, len, hipMemcpyDeviceToHost));
        for (char c : raw) if (c != '"' && c != '\t') r.push_back((c >= 'A' && c <= 'Z') ? (char)(c + 32) : c);   // rs:199-206
        slot_rank[k] = (uint16_t)ranks.size();
        ranks.push_back(r);
        rank_text += r;
        rank_off.push_back((uint32_t)rank_text.size());
    }
    const uint32_t n_ranks = (uint32_t)ranks.size();
    for (const std::string& r : ranks) {               // lineage levels: replaced, then parsed (rs:377-398)
        std::string target = r;
        for (const auto& p : rep) if (p.first == r) target = p.second;
        bool other = false;
        lin_off.push_back((uint32_t)tok.size());
        tok += rank_token(target, &other);
        lin_drop.push_back(other && D.drop_non_linnaean);
    }
    lin_off.push_back((uint32_t)tok.size());
    for (const std::string& r : ranks) {               // the leaf: not replaced (rs:426-438)
        bool other = false;
        leaf_off.push_back((uint32_t)tok.size());
        tok += rank_token(r, &other);
        leaf_drop.push_back(other && D.drop_non_linnaean);
    }
    leaf_off.push_back((uint32_t)tok.size());
    uint16_t* d_slot_rank;
    unsigned char *d_rank_text, *d_tok;
    uint32_t *d_rank_off, *d_lin_off, *d_leaf_off;
    uint8_t *d_lin_drop, *d_leaf_drop;
    auto up = [&](auto** dst, const void* src, size_t bytes) -> hipError_t {
        hipError_t e = mem.alloc(dst, bytes, "rank tables");
        if (e == hipSuccess && bytes) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
        return e;
    };
    HIP_CHECK(pol, up(&d_slot_rank, slot_rank.data(), RANK_SLOTS * 2));
    HIP_CHECK(pol, up(&d_rank_text, rank_text.data(), rank_text.size()));
    HIP_CHECK(pol, up(&d_rank_off, rank_off.data(), rank_off.size() * 4));
    HIP_CHECK(pol, up(&d_tok, tok.data(), tok.size()));
    HIP_CHECK(pol, up(&d_lin_off, lin_off.data(), lin_off.size() * 4));
    HIP_CHECK(pol, up(&d_leaf_off, leaf_off.data(), leaf_off.size() * 4));
    HIP_CHECK(pol, up(&d_lin_drop, lin_drop.data(), n_ranks));
    HIP_CHECK(pol, up(&d_leaf_drop, leaf_drop.data(), n_ranks));
    hipLaunchKernelGGL(taxdb_rank_assign, dim3(grid(n_ids)), dim3(TPB), 0, 0, (const unsigned char*)txt[D_NODES].d, (const uint64_t*)P[D_NODES].span_a,
                       (const uint32_t*)P[D_NODES].span_len, (const uint32_t*)node_row, n_ids, (const unsigned long long*)node_hash,
                       (const unsigned long long*)slot_hash, (const uint16_t*)d_slot_rank, (const unsigned char*)d_rank_text, (const uint32_t*)d_rank_off,
                       node_rank, flags + 1);
    HIP_CHECK(pol, hipGetLastError());
    HIP_CHECK(pol, hipMemcpy(h_flags, flags, 8, hipMemcpyDeviceToHost));
    if (h_flags[1]) { set_error("build-db: two rank strings of %s share one 64-bit hash", D.nodes_path); return BLU_ERR_INVALID_ARG; }
    lap(&S.t_tables_ms);

    // ---- group the accession lines by taxid
    uint32_t n = acc.n_lines;
    AccOut ao{};
    uint32_t *keys_alt, *vals_alt, *first_bad;
    HIP_CHECK(pol, mem.alloc(&ao.key, (size_t)n * 4, "accession rows")); HIP_CHECK(pol, mem.alloc(&ao.val, (size_t)n * 4, "accession rows"));
    HIP_CHECK(pol, mem.alloc(&ao.tax64, (size_t)n * 8, "accession rows"));
    HIP_CHECK(pol, mem.alloc(&ao.acc_a, (size_t)n * 8, "accession rows")); HIP_CHECK(pol, mem.alloc(&ao.acc_len, (size_t)n * 4, "accession rows"));
    HIP_CHECK(pol, mem.alloc(&ao.oid_a, (size_t)n * 8, "accession rows")); HIP_CHECK(pol, mem.alloc(&ao.oid_len, (size_t)n * 4, "accession rows"));
    HIP_CHECK(pol, mem.alloc(&ao.esc_len, (size_t)n * 4, "accession rows"));
    HIP_CHECK(pol, mem.alloc(&keys_alt, (size_t)n * 4, "accession rows")); HIP_CHECK(pol, mem.alloc(&vals_alt, (size_t)n * 4, "accession rows"));
    HIP_CHECK(pol, mem.alloc(&first_bad, 4, "accession rows"));
    HIP_CHECK(pol, hipMemset(first_bad, 0xFF, 4));
    HIP_CHECK(pol, hipMemset(d_err, 0xFF, 8));
    ao.err = d_err;
    ao.first_bad = first_bad;
    if (n) hipLaunchKernelGGL(taxdb_parse_acc, dim3(grid(n)), dim3(TPB), 0, 0, (const unsigned char*)acc.d, (const uint64_t*)acc.line, n, n_ids, ao);
    HIP_CHECK(pol, hipGetLastError());
    {
        uint32_t fb = NONE32;
        unsigned long long err = ~0ull;
        HIP_CHECK(pol, hipMemcpy(&fb, first_bad, 4, hipMemcpyDeviceToHost));
        HIP_CHECK(pol, hipMemcpy(&err, d_err, 8, hipMemcpyDeviceToHost));
        if (fb < n) n = fb;                         // the reference's read loop ends at the first line that is not UTF-8
        if (err != ~0ull && (err >> 3) < n) {
            set_error("%s:%llu: %s", D.accessions_path, (err >> 3) + 1,
                      (err & 7) == E_PIECES ? "fewer than three fields separated by two spaces" : "a taxid that is not an i64");
            return BLU_ERR_PARSE;
        }
    }
    S.n_accession_lines = n;
    uint32_t *keys = ao.key, *vals = ao.val;
    int bits = 0;
    while (bits < 32 && (n_ids >> bits) != 0) ++bits;   // keys <= n_ids
    {
        uint32_t* table;
        void* tmp;
        HIP_CHECK(pol, mem.alloc(&table, radix_table_words(n) * 4, "radix sort"));
        HIP_CHECK(pol, mem.alloc(&tmp, radix_scan_tmp_bytes(n), "radix sort"));
        HIP_CHECK(pol, radix_sort_pairs(&keys, &keys_alt, &vals, &vals_alt, n, bits, table, tmp));
    }
    uint32_t *head, *excl, *seg_of, *seg_start, *seg_key;
    void* stmp;
    HIP_CHECK(pol, mem.alloc(&head, ((size_t)n + 1) * 4, "segments")); HIP_CHECK(pol, mem.alloc(&excl, ((size_t)n + 1) * 4, "segments"));
    HIP_CHECK(pol, mem.alloc(&seg_of, (size_t)n * 4, "segments")); HIP_CHECK(pol, mem.alloc(&seg_start, ((size_t)n + 1) * 4, "segments"));
    HIP_CHECK(pol, mem.alloc(&seg_key, (size_t)n * 4, "segments"));
    HIP_CHECK(pol, mem.alloc(&stmp, std::max(scan_tmp_bytes_u32((size_t)n + 1), scan_tmp_bytes_u64((size_t)n + 1)), "scan"));
    HIP_CHECK(pol, hipMemset(head + n, 0, 4));
    if (n) hipLaunchKernelGGL(taxdb_heads, dim3(grid(n)), dim3(TPB), 0, 0, (const uint32_t*)keys, n, head);
    HIP_CHECK(pol, exclusive_scan_u32(head, excl, (size_t)n + 1, stmp));
    if (n) hipLaunchKernelGGL(taxdb_seg_ids, dim3(grid(n)), dim3(TPB), 0, 0, (const uint32_t*)head, (const uint32_t*)excl, (const uint32_t*)keys, n,
                              seg_of, seg_start, seg_key);
    uint32_t n_seg = 0;
    HIP_CHECK(pol, hipMemcpy(&n_seg, excl + n, 4, hipMemcpyDeviceToHost));
    HIP_CHECK(pol, hipMemcpy(seg_start + n_seg, &n, 4, hipMemcpyHostToDevice));
    lap(&S.t_group_ms);

    // ---- resolve + assemble the lineages
    SegOut so{};
    unsigned long long *num_off, *txt_off;
    HIP_CHECK(pol, mem.alloc(&so.status, n_seg, "segments")); HIP_CHECK(pol, mem.alloc(&so.node, (size_t)n_seg * 4, "segments"));
    HIP_CHECK(pol, mem.alloc(&so.warn, (size_t)n_seg * 4, "segments"));
    HIP_CHECK(pol, mem.alloc(&so.num_len, ((size_t)n_seg + 1) * 8, "segments")); HIP_CHECK(pol, mem.alloc(&so.txt_len, ((size_t)n_seg + 1) * 8, "segments"));
    HIP_CHECK(pol, mem.alloc(&num_off, ((size_t)n_seg + 1) * 8, "segments")); HIP_CHECK(pol, mem.alloc(&txt_off, ((size_t)n_seg + 1) * 8, "segments"));
    HIP_CHECK(pol, hipMemset(so.num_len + n_seg, 0, 8)); HIP_CHECK(pol, hipMemset(so.txt_len + n_seg, 0, 8));
    HIP_CHECK(pol, hipMemset(d_err, 0xFF, 8));
    so.err = d_err;
    Ctx C{};
    C.T = NodeTabs{node_row, lin_row, name_row, merged_row, deleted, skip_bits, skip_limit, node_rank, n_ids};
    C.L = LinText{txt[D_LINEAGE].d, P[D_LINEAGE].span_a, P[D_LINEAGE].span_len};
    C.N = Names{txt[D_NAMES].d, P[D_NAMES].span_a, P[D_NAMES].span_len};
    C.R = RankTabs{d_tok, d_lin_off, d_leaf_off, d_lin_drop, d_leaf_drop};
    C.drop = D.drop_non_linnaean ? 1 : 0;
    C.merged_to = P[D_MERGED].aux;
    if (n_seg) hipLaunchKernelGGL(taxdb_resolve, dim3(grid(n_seg)), dim3(TPB), 0, 0, (const uint32_t*)seg_key, n_seg, C, so);
    HIP_CHECK(pol, hipGetLastError());
    {
        unsigned long long err = ~0ull;
        HIP_CHECK(pol, hipMemcpy(&err, d_err, 8, hipMemcpyDeviceToHost));
        if (err != ~0ull) {
            set_error("%s:%llu: %s", D.lineage_path, (err >> 3) + 1,
                      (err & 7) == E_ANCESTOR ? "an ancestor that is not a taxid" : "an ancestor outside 0..2147483647");
            return BLU_ERR_PARSE;
        }
    }
    HIP_CHECK(pol, exclusive_scan_u64(so.num_len, num_off, (size_t)n_seg + 1, stmp));
    HIP_CHECK(pol, exclusive_scan_u64(so.txt_len, txt_off, (size_t)n_seg + 1, stmp));
    unsigned long long num_total = 0, txt_total = 0;
    HIP_CHECK(pol, hipMemcpy(&num_total, num_off + n_seg, 8, hipMemcpyDeviceToHost));
    HIP_CHECK(pol, hipMemcpy(&txt_total, txt_off + n_seg, 8, hipMemcpyDeviceToHost));
    unsigned char *num, *txtb;
    HIP_CHECK(pol, mem.alloc(&num, num_total + 16, "numeric lineages"));
    HIP_CHECK(pol, mem.alloc(&txtb, txt_total + 16, "text lineages"));
    if (n_seg) hipLaunchKernelGGL(taxdb_lineages, dim3(grid(n_seg)), dim3(TPB), 0, 0, (const uint32_t*)seg_key, n_seg, C, (const uint8_t*)so.status,
                                  (const uint32_t*)so.node, (const unsigned long long*)num_off, (const unsigned long long*)txt_off, num, txtb);
    HIP_CHECK(pol, hipGetLastError());
    lap(&S.t_assemble_ms);

    // ---- render the taxonomies array
    RowIn R{seg_of, seg_start, seg_key, so.status, so.node, num_off, so.num_len, txt_off, so.txt_len, num, txtb, vals,
            ao.esc_len, ao.acc_a, ao.acc_len, ao.oid_a, ao.oid_len, acc.d, d_tok, d_leaf_off, node_rank};
    unsigned long long *row_len, *row_off;
    HIP_CHECK(pol, mem.alloc(&row_len, ((size_t)n + 1) * 8, "render"));
    HIP_CHECK(pol, mem.alloc(&row_off, ((size_t)n + 1) * 8, "render"));
    hipLaunchKernelGGL(taxdb_row_len, dim3(grid((uint64_t)n + 1)), dim3(TPB), 0, 0, R, n, row_len);
    HIP_CHECK(pol, exclusive_scan_u64(row_len, row_off, (size_t)n + 1, stmp));
    unsigned long long body = 0;
    HIP_CHECK(pol, hipMemcpy(&body, row_off + n, 8, hipMemcpyDeviceToHost));
    unsigned char* d_doc;
    HIP_CHECK(pol, mem.alloc(&d_doc, body + 16, "document"));
    if (n) hipLaunchKernelGGL(taxdb_row_write, dim3(grid(n)), dim3(TPB), 0, 0, R, n, (const unsigned long long*)row_off, d_doc);
    HIP_CHECK(pol, hipGetLastError());
    Column<char> h_doc;
    h_doc.resize(body);
    {
        std::vector<D2HPiece> pieces;
        d2h_add(pieces, h_doc.data(), d_doc, body);
        HIP_CHECK(pol, d2h_parallel(pieces, D.device));
    }
    // per-taxid outcome -> stats and the TSV (ascending taxid: the segments are in key order, the taxids beyond the
    // tables come last and are sorted here)
    std::vector<uint8_t> st(n_seg);
    std::vector<uint32_t> skey(n_seg), warn(n_seg);
    if (n_seg) {
        HIP_CHECK(pol, hipMemcpy(st.data(), so.status, n_seg, hipMemcpyDeviceToHost));
        HIP_CHECK(pol, hipMemcpy(skey.data(), seg_key, (size_t)n_seg * 4, hipMemcpyDeviceToHost));
        HIP_CHECK(pol, hipMemcpy(warn.data(), so.warn, (size_t)n_seg * 4, hipMemcpyDeviceToHost));
    }
    std::string tsv;
    uint64_t distinct = 0;
    for (uint32_t s = 0; s < n_seg; ++s) {
        S.n_unmapped_ancestors += warn[s];
        const char* why = nullptr;
        switch (st[s]) {
            case S_MAPPED: ++S.n_mapped; break;
            case S_MERGED_MAPPED: ++S.n_mapped_merged; break;
            case S_DROPPED: ++S.n_dropped; break;
            case S_DELETED: ++S.n_deleted; why = "deleted"; break;
            case S_MERGED_MISSING: ++S.n_merged_missing; why = "merged"; break;
            case S_UNKNOWN: ++S.n_unknown; why = "unknown"; break;
            default: break;
        }
        if (st[s] != S_BEYOND) ++distinct;
        if (why) { tsv += std::to_string(skey[s]); tsv += '\t'; tsv += why; tsv += '\n'; }
    }
    if (n_seg && st[n_seg - 1] == S_BEYOND) {
        uint32_t first = 0;
        HIP_CHECK(pol, hipMemcpy(&first, seg_start + n_seg - 1, 4, hipMemcpyDeviceToHost));
        const uint32_t nb = n - first;
        unsigned long long* d_big;
        HIP_CHECK(pol, mem.alloc(&d_big, (size_t)nb * 8, "taxids beyond the tables"));
        hipLaunchKernelGGL(taxdb_gather_u64, dim3(grid(nb)), dim3(TPB), 0, 0, (const unsigned long long*)ao.tax64, (const uint32_t*)(vals + first), nb, d_big);
        std::vector<unsigned long long> big(nb);
        HIP_CHECK(pol, hipMemcpy(big.data(), d_big, (size_t)nb * 8, hipMemcpyDeviceToHost));
        std::sort(big.begin(), big.end());
        big.erase(std::unique(big.begin(), big.end()), big.end());
        for (unsigned long long v : big) { tsv += std::to_string(v); tsv += "\tunknown\n"; ++S.n_unknown; ++distinct; }
    }
    S.n_distinct_taxids = distinct;
    lap(&S.t_render_ms);

    // ---- write: the head and tail around the rendered array (serde_json::to_string_pretty of TaxonomiesMap)
    std::string headtxt = "{\n  \"blutilsVersion\": ";
    json_str(headtxt, D.blutils_version ? D.blutils_version : BLU_TAXDB_DEFAULT_VERSION);
    headtxt += ",\n";
    if (!D.has_skip) headtxt += "  \"ignoreTaxids\": null,\n";
    else if (D.n_skip == 0) headtxt += "  \"ignoreTaxids\": [],\n";
    else {
        headtxt += "  \"ignoreTaxids\": [";
        for (uint64_t k = 0; k < D.n_skip; ++k) headtxt += (k ? ",\n    " : "\n    ") + std::to_string(D.skip_taxids[k]);
        headtxt += "\n  ],\n";
    }
    if (!D.has_replace) headtxt += "  \"replaceRank\": null,\n";
    else if (rep.empty()) headtxt += "  \"replaceRank\": {},\n";
    else {
        headtxt += "  \"replaceRank\": {";
        for (size_t k = 0; k < rep.size(); ++k) {
            headtxt += k ? ",\n    " : "\n    ";
            json_str(headtxt, rep[k].first);
            headtxt += ": ";
            json_str(headtxt, rep[k].second);
        }
        headtxt += "\n  },\n";
    }
    headtxt += std::string("  \"dropNonLinnaeanTaxonomies\": ") + (D.drop_non_linnaean ? "true" : "false") + ",\n";
    headtxt += "  \"sourceDatabase\": ";
    json_str(headtxt, D.source_database ? D.source_database : "");
    headtxt += ",\n";
    const std::string stem = D.output_stem;
    const std::string json_path = stem + ".blutils.json", tsv_path = stem + ".non-mapped.tsv";
    {   // rs:256-262: the TSV is removed and created again on every run
        if (unlink(tsv_path.c_str()) != 0 && errno != ENOENT) { set_error("build-db: cannot remove %s: %s", tsv_path.c_str(), strerror(errno)); return BLU_ERR_IO; }
        const int fd = open(tsv_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
        if (fd < 0) { set_error("build-db: cannot create %s: %s", tsv_path.c_str(), strerror(errno)); return BLU_ERR_IO; }
        const bool ok = write_all(fd, tsv.data(), tsv.size());
        if (close(fd) != 0 || !ok) { set_error("build-db: writing %s failed", tsv_path.c_str()); return BLU_ERR_IO; }
    }
    {
        const int fd = open(json_path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
        if (fd < 0) { set_error("build-db: cannot create %s: %s", json_path.c_str(), strerror(errno)); return BLU_ERR_IO; }
        bool ok;
        if (body == 0) {
            headtxt += "  \"taxonomies\": []\n}";
            ok = write_all(fd, headtxt.data(), headtxt.size());
        } else {
            headtxt += "  \"taxonomies\": [\n";
            static const char tail[] = "\n  ]\n}";
            ok = write_all(fd, headtxt.data(), headtxt.size()) && write_all(fd, h_doc.data() + 2, body - 2) && write_all(fd, tail, sizeof tail - 1);
        }
        if (close(fd) != 0 || !ok) { set_error("build-db: writing %s failed", json_path.c_str()); return BLU_ERR_IO; }
        S.doc_bytes = headtxt.size() + (body ? body - 2 + 6 : 0);
    }
    S.tsv_bytes = tsv.size();
    for (int m = 0; m < N_DUMPS; ++m) S.input_bytes += txt[m].size;
    S.input_bytes += acc.size;
    lap(&S.t_write_ms);
    return BLU_OK;
}

}  // namespace
}  // namespace blu

extern "C" int blu_taxdb_build(const blu_taxdb_desc* desc, blu_taxdb_stats* stats) {
    if (!desc || !desc->nodes_path || !desc->names_path || !desc->lineage_path || !desc->merged_path || !desc->delnodes_path ||
        !desc->accessions_path || !desc->output_stem || (desc->has_skip && desc->n_skip && !desc->skip_taxids) ||
        (desc->has_replace && desc->n_replace && (!desc->replace_from || !desc->replace_to))) {
        blu::set_error("blu_taxdb_build: null argument");
        return BLU_ERR_INVALID_ARG;
    }
    blu_taxdb_stats local;
    blu_taxdb_stats& S = stats ? *stats : local;
    memset(&S, 0, sizeof S);
    return blu::build(*desc, S);
}
