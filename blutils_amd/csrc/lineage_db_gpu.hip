// `build-db lineages` on the GPU: a two-column lineage table (`ID<TAB>d__Bacteria; p__Proteobacteria; ...`) -> *.blutils.json,
// *.non-mapped.tsv and the `ID taxid` map of `makeblastdb -taxid_map` (include/blu_pipeline.h: blu_lineage_db_build; DESIGN.md
// §25 lists every rule with the test that covers it).
//
// Stages (all on the null stream of the call's device):
//   upload    the table: pread into pinned staging -> HBM, and its line index
//   parse     one thread per line: blank / comment / header, then fields, UTF-8 and a walk over the lineage that counts its
//             surviving levels and the bytes of its normalised text `rank__identifier;...`; two scans; the same walk writes the
//             text and one item per (line, level): the length of that prefix and its running 64-bit hash.  Items lie in
//             (line, level) order, so an item's index is its first-appearance key
//   intern    the exact path dictionary: open addressing over item indices.  A slot is claimed by one CAS of an item index (the
//             key is text that the kernel before wrote, so one word publishes it); a thread that finds a slot taken compares its
//             prefix with the slot's byte for byte and probes on when they differ; equal paths lower the slot to their smallest
//             index with atomicMin.  No thread waits for another: every probe loop is bounded by the table size, a table more
//             than half full is doubled by the host and built again.  Items that are their slot's minimum are the taxa: a scan
//             over that mark numbers them
//   group     stable radix sort of the lines by the taxid of their last level, segment starts
//   render    the `taxonomies` array, one thread per accession row (taxmap_entry_dev.h: the entry bytes of `build-db blu`), the
//             numeric lineage of an entry written from its items' ids; the taxid map and the TSV by length, scan and write over
//             the lines; downloaded in pieces
// The host keeps the document head and tail and the -r table.  No device library is called; byte work, no MFMA.
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstring>
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
constexpr uint64_t MAX_ITEMS = 1ull << 30;         // item indices and twice as many slots stay below 2^32

// error codes (the word is (line << 3) | code, atomicMin: the first bad line wins; one code per line, in this order)
enum : uint32_t { E_UTF8 = 1, E_NO_TAB = 2, E_EMPTY_ID = 3, E_NO_RANK = 4, E_EMPTY_RANK = 5, E_DEPTH = 6 };
enum : uint8_t { L_SKIP = 0, L_MAPPED = 1, L_EMPTY = 2 };
enum : int { LIST_MAP = 0, LIST_TSV = 1 };

// the -r table: pair k replaces the token bytes[off[2k], off[2k + 1]) by bytes[off[2k + 1], off[2k + 2]) (already parsed)
struct RankRules { const unsigned char* bytes; const uint32_t* off; uint32_t n; };

__device__ __forceinline__ uint32_t lower(uint32_t c) { return (c >= 'A' && c <= 'Z') ? c + 32 : c; }
__device__ __forceinline__ bool alnum(uint32_t c) { return (c >= 'a' && c <= 'z') || (c >= '0' && c <= '9'); }

__device__ __forceinline__ bool has_alnum(const unsigned char* __restrict__ text, uint64_t a, uint64_t b) {
    for (; a < b; ++a) if (alnum(lower(text[a]))) return true;
    return false;
}

// slugify_ascii (taxonomy.cpp) of text[a, b) into sink; returns its bytes
template <class S>
__device__ __forceinline__ uint32_t emit_slug(const unsigned char* __restrict__ text, uint64_t a, uint64_t b, S&& sink) {
    uint32_t n = 0;
    bool pending = false;
    for (; a < b; ++a) {
        const uint32_t c = lower(text[a]);
        if (alnum(c)) {
            if (pending && n) { sink('-'); ++n; }
            pending = false;
            sink(c);
            ++n;
        } else {
            pending = true;
        }
    }
    return n;
}

// the rank of a level from its token text[a, b): trimmed, lower case, -r (exact), then parse_rank (taxonomy.cpp): the letter of
// d/domain ... s/species and u/undefined, else the slug.  Returns the bytes given to sink, 0 = the rank is empty
template <class S>
__device__ __forceinline__ uint32_t emit_rank(const unsigned char* __restrict__ text, uint64_t a, uint64_t b, const RankRules& R, S&& sink) {
    trim(text, a, b);
    for (uint32_t k = 0; k < R.n; ++k) {
        const uint32_t fa = R.off[2 * k], fb = R.off[2 * k + 1], te = R.off[2 * k + 2];
        if (fb - fa != b - a) continue;
        bool eq = true;
        for (uint64_t j = 0; j < b - a && eq; ++j) eq = lower(text[a + j]) == R.bytes[fa + j];
        if (!eq) continue;
        for (uint32_t j = fb; j < te; ++j) sink(R.bytes[j]);
        return te - fb;
    }
    const char* names = "undefined|domain|kingdom|phylum|class|order|family|genus|species|";   // the letter is the first byte
    for (uint32_t p = 0; names[p];) {
        uint32_t q = p;
        while (names[q] != '|') ++q;
        bool eq = b - a == q - p;
        for (uint32_t j = 0; eq && j < q - p; ++j) eq = lower(text[a + j]) == (uint32_t)names[p + j];
        if (eq || (b - a == 1 && lower(text[a]) == (uint32_t)names[p])) { sink((uint32_t)names[p]); return 1; }
        p = q + 1;
    }
    return emit_slug(text, a, b, sink);
}

// The levels of the lineage text[a, b): pieces at every ';', trimmed, empty ones skipped; a piece is RANK__NAME at its first
// "__".  The lineage ends before the first level whose identifier (the slug of NAME) is empty: *truncated.  The normalised
// text `rank__identifier` of the levels, joined with ';', goes to sink byte by byte; end_level(k) follows level k.  Returns
// the surviving levels; *err: a piece without "__", an empty rank, more than BLU_MAX_DEPTH levels
template <class S, class L>
__device__ __forceinline__ uint32_t walk_lineage(const unsigned char* __restrict__ text, uint64_t a, uint64_t b, const RankRules& R, S&& sink,
                                                 L&& end_level, bool* truncated, uint32_t* err) {
    uint32_t levels = 0;
    for (uint64_t p = a;;) {
        uint64_t q = p;
        while (q < b && text[q] != ';') ++q;
        uint64_t pa = p, pb = q;
        trim(text, pa, pb);
        p = q + 1;
        if (pa < pb) {
            uint64_t u = pa;
            while (u + 1 < pb && !(text[u] == '_' && text[u + 1] == '_')) ++u;
            if (u + 1 >= pb) { *err = E_NO_RANK; break; }
            if (!has_alnum(text, u + 2, pb)) { *truncated = true; break; }
            if (levels == BLU_MAX_DEPTH) { *err = E_DEPTH; break; }
            if (levels) sink(';');
            if (emit_rank(text, pa, u, R, sink) == 0) { *err = E_EMPTY_RANK; break; }
            sink('_'); sink('_');
            emit_slug(text, u + 2, pb, sink);
            end_level(levels);
            ++levels;
        }
        if (q >= b) break;
    }
    return levels;
}

struct Lines {
    const unsigned char* text; uint64_t size;      // the table, padded
    const uint64_t* start; uint32_t n;             // line k is [start[k], start[k + 1] - 1)
};
__device__ __forceinline__ void line_span(const Lines& T, uint32_t i, uint64_t& s, uint64_t& e) {
    s = min(T.start[i], T.size);
    e = min(max(T.start[i + 1], s + 1) - 1, T.size);
}

// ---- parse 1: blank and comment lines, and the first line that is neither: (line << 1) | (its first field is not `Feature ID`)
__global__ __launch_bounds__(TPB) void lindb_scan_lines(Lines T, uint8_t* __restrict__ kind, uint32_t* __restrict__ first) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= T.n) return;
    uint64_t s, e;
    line_span(T, i, s, e);
    uint64_t f = s;
    while (f < e && is_ws(T.text[f])) ++f;
    if (f == e || T.text[f] == '#') { kind[i] = L_SKIP; return; }
    kind[i] = L_MAPPED;
    uint64_t t = f;
    while (t < e && T.text[t] != '\t') ++t;
    trim(T.text, f, t);
    const char* want = "Feature ID";
    bool header = t - f == 10;
    for (uint32_t k = 0; header && k < 10; ++k) header = T.text[f + k] == (unsigned char)want[k];
    atomicMin(first, (i << 1) | (header ? 0u : 1u));
}

struct LineOut {
    uint8_t* kind;                     // [n] in: L_SKIP or not; out: L_SKIP, L_MAPPED, L_EMPTY
    unsigned long long* levels;        // [n + 1] surviving levels
    unsigned long long* norm_len;      // [n + 1] bytes of the normalised lineage
    uint32_t* is_data;                 // [n + 1] 1 = data line (its exclusive scan is the oid)
    uint64_t* id_a; uint32_t* id_len; uint32_t* id_esc;      // [n] the trimmed ID and its escaped length
    uint64_t* lin_a; uint32_t* lin_len;                      // [n] the lineage field
    unsigned long long* err;           // (line << 3) | code, atomicMin
    unsigned long long* counters;      // [0] data lines [1] without a level [2] truncated
    uint32_t* max_depth;
};

// ---- parse 2: one thread per line: fields, UTF-8, the lineage walk as a count
__global__ __launch_bounds__(TPB) void lindb_classify(Lines T, uint32_t header, RankRules R, LineOut o) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= T.n) return;
    o.levels[i] = 0; o.norm_len[i] = 0; o.is_data[i] = 0;
    o.id_a[i] = 0; o.id_len[i] = 0; o.id_esc[i] = 0; o.lin_a[i] = 0; o.lin_len[i] = 0;
    if (o.kind[i] == L_SKIP || i == header) { o.kind[i] = L_SKIP; return; }
    o.is_data[i] = 1;
    o.kind[i] = L_EMPTY;
    atomicAdd(&o.counters[0], 1ull);
    uint64_t s, e;
    line_span(T, i, s, e);
    uint64_t t1 = e, t2 = e;               // the first two tabs
    int nt = 0;
    bool high = false;
    for_bytes(T.text, s, e, [&](uint32_t c, uint64_t p) {
        high |= c >= 0x80;
        const bool tab = c == '\t';        // (selects, not branches: a conditional store to a by-reference capture ends up in scratch)
        t1 = (tab && nt == 0) ? p : t1;
        t2 = (tab && nt == 1) ? p : t2;
        nt += tab ? 1 : 0;
        return true;
    });
    const unsigned long long fail = (unsigned long long)i << 3;
    if (high && !utf8_valid(T.text, s, e)) { atomicMin(o.err, fail | E_UTF8); return; }
    if (nt == 0) { atomicMin(o.err, fail | E_NO_TAB); return; }
    uint64_t ia = s, ib = t1;
    trim(T.text, ia, ib);
    if (ia == ib) { atomicMin(o.err, fail | E_EMPTY_ID); return; }
    unsigned long long bytes = 0;
    bool truncated = false;
    uint32_t err = 0;
    const uint32_t levels = walk_lineage(T.text, t1 + 1, t2, R, [&](uint32_t) { ++bytes; }, [](uint32_t) {}, &truncated, &err);
    if (err) { atomicMin(o.err, fail | err); return; }
    o.kind[i] = levels ? L_MAPPED : L_EMPTY;
    o.levels[i] = levels;
    o.norm_len[i] = bytes;
    o.id_a[i] = ia; o.id_len[i] = (uint32_t)(ib - ia); o.id_esc[i] = esc_len(T.text, ia, ib);
    o.lin_a[i] = t1 + 1; o.lin_len[i] = (uint32_t)(t2 - t1 - 1);
    if (!levels) atomicAdd(&o.counters[1], 1ull);
    if (truncated) atomicAdd(&o.counters[2], 1ull);
    atomicMax(o.max_depth, levels);
}

// what the dictionary and the renderer read of the parsed table
struct Paths {
    const unsigned char* norm; unsigned long long norm_total;     // the normalised lineages back to back
    const unsigned long long* norm_off;    // [n + 1] per line
    const unsigned long long* item_off;    // [n + 1] per line: its first item
    const uint32_t* item_line;             // [n_items]
    const uint32_t* item_len;              // [n_items] bytes of the prefix that ends with the item's level
    const unsigned long long* item_hash;   // [n_items] hash of that prefix
    uint32_t n_items, n_lines;
};

// ---- parse 3: the same walk writes the normalised text and the items of the line
__global__ __launch_bounds__(TPB) void lindb_write_paths(Lines T, RankRules R, const uint8_t* __restrict__ kind, const uint64_t* __restrict__ lin_a,
                                                         const uint32_t* __restrict__ lin_len, Paths P, unsigned long long hash_mask,
                                                         unsigned char* __restrict__ norm, uint32_t* __restrict__ item_line,
                                                         uint32_t* __restrict__ item_len, unsigned long long* __restrict__ item_hash) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= T.n || kind[i] != L_MAPPED) return;
    // both ranges were measured by lindb_classify with this walk; the stores stay inside them whatever the arrays hold
    const unsigned long long n0 = min(P.norm_off[i], P.norm_total), n1 = min(max(P.norm_off[i + 1], n0), P.norm_total);
    const unsigned long long j0 = min(P.item_off[i], (unsigned long long)P.n_items);
    const unsigned long long j1 = min(max(P.item_off[i + 1], j0), (unsigned long long)P.n_items);
    const uint64_t a = min(lin_a[i], T.size), b = min(a + lin_len[i], T.size);
    unsigned long long w = 0, h = 0xcbf29ce484222325ull;
    bool truncated = false;
    uint32_t err = 0;
    walk_lineage(T.text, a, b, R,
                 [&](uint32_t c) { if (n0 + w < n1) norm[n0 + w] = (unsigned char)c; ++w; h = (h ^ c) * 0x100000001b3ull; },
                 [&](uint32_t k) {
                     if (j0 + k >= j1) return;
                     item_line[j0 + k] = i; item_len[j0 + k] = (uint32_t)w; item_hash[j0 + k] = h & hash_mask;
                 },
                 &truncated, &err);
}

// the prefix of item j: its first byte, and its length cut to what the buffer holds behind it
__device__ __forceinline__ const unsigned char* item_text(const Paths& P, uint32_t j, uint32_t* len) {
    const unsigned long long a = min(P.norm_off[min(P.item_line[j], P.n_lines)], P.norm_total);
    *len = (uint32_t)min((unsigned long long)P.item_len[j], P.norm_total - a);
    return P.norm + a;
}
// two items are one taxon when their prefixes are the same bytes (compared from the end: paths share their heads)
__device__ __forceinline__ bool same_path(const Paths& P, uint32_t x, uint32_t y) {
    if (x == y) return true;
    if (P.item_hash[x] != P.item_hash[y]) return false;
    uint32_t lx, ly;
    const unsigned char *tx = item_text(P, x, &lx), *ty = item_text(P, y, &ly);
    if (lx != ly) return false;
    for (uint32_t k = lx; k > 0; --k) if (tx[k - 1] != ty[k - 1]) return false;
    return true;
}
__device__ __forceinline__ uint32_t first_slot(unsigned long long h, uint32_t mask) {
    h *= 0x9E3779B97F4A7C15ull;
    return (uint32_t)(h >> 32) & mask;
}

// ---- intern: every item finds or claims the slot of its path; flags: [0] an item found no slot, [1] slots claimed
__global__ __launch_bounds__(TPB) void lindb_intern(Paths P, uint32_t* __restrict__ slot, uint32_t n_slots, uint32_t* __restrict__ item_slot,
                                                    uint32_t* __restrict__ flags) {
    const uint32_t j = blockIdx.x * TPB + threadIdx.x;
    if (j >= P.n_items) return;
    const uint32_t mask = n_slots - 1;
    uint32_t k = first_slot(P.item_hash[j], mask);
    for (uint32_t probe = 0; probe < n_slots; ++probe, k = (k + 1) & mask) {
        uint32_t cur = __hip_atomic_load(&slot[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == NONE32) {
            cur = atomicCAS(&slot[k], NONE32, j);
            if (cur == NONE32) { atomicAdd(&flags[1], 1u); item_slot[j] = k; return; }
        }
        cur = min(cur, P.n_items - 1);
        if (same_path(P, cur, j)) {
            if (j < cur) atomicMin(&slot[k], j);          // every item of a slot is the same path: the slot ends on their minimum
            item_slot[j] = k;
            return;
        }
    }
    item_slot[j] = 0;
    atomicOr(&flags[0], 1u);
}

// the items that are the first appearance of their path
__global__ __launch_bounds__(TPB) void lindb_mark_first(const uint32_t* __restrict__ slot, uint32_t n_slots, const uint32_t* __restrict__ item_slot,
                                                        uint32_t n_items, uint32_t* __restrict__ first) {
    const uint32_t j = blockIdx.x * TPB + threadIdx.x;
    if (j > n_items) return;
    first[j] = (j < n_items && slot[min(item_slot[j], n_slots - 1)] == j) ? 1u : 0u;
}
// the taxid of every item: 1 + the first appearances before its path's
__global__ __launch_bounds__(TPB) void lindb_item_ids(const uint32_t* __restrict__ slot, uint32_t n_slots, const uint32_t* __restrict__ item_slot,
                                                      const uint32_t* __restrict__ first_excl, uint32_t n_items, uint32_t* __restrict__ item_id) {
    const uint32_t j = blockIdx.x * TPB + threadIdx.x;
    if (j >= n_items) return;
    const uint32_t rep = min(slot[min(item_slot[j], n_slots - 1)], n_items - 1);
    item_id[j] = first_excl[rep] + 1;
}

// ---- group: the sort key of a line is the taxid of its last level; other lines go behind every taxon
__global__ __launch_bounds__(TPB) void lindb_leaf_keys(const uint8_t* __restrict__ kind, const unsigned long long* __restrict__ item_off,
                                                       const uint32_t* __restrict__ item_id, uint32_t n_items, uint32_t n, uint32_t n_taxa,
                                                       uint32_t* __restrict__ leaf, uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    uint32_t t = n_taxa + 1;
    if (kind[i] == L_MAPPED && item_off[i + 1] > item_off[i] && item_off[i + 1] <= n_items) t = min(item_id[item_off[i + 1] - 1], n_taxa);
    leaf[i] = t;
    key[i] = t;
    val[i] = i;
}
__global__ __launch_bounds__(TPB) void lindb_heads(const uint32_t* __restrict__ key, uint32_t n, uint32_t* __restrict__ head) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i <= n) head[i] = (i < n && (i == 0 || key[i] != key[i - 1])) ? 1u : 0u;
}
__global__ __launch_bounds__(TPB) void lindb_segments(const uint32_t* __restrict__ head, const uint32_t* __restrict__ excl, uint32_t n,
                                                      uint32_t* __restrict__ seg_of, uint32_t* __restrict__ seg_start) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = excl[i] + head[i] - 1;
    seg_of[i] = s;
    if (head[i]) seg_start[s] = i;
}

// ---- render ----------------------------------------------------------------------------------------------------------
// numericLineage of a line from its normalised text t[0, len) and the ids of its levels: each `rank__identifier` becomes
// `rank__<id>`; out may be null.  Returns its bytes; *rank_a, *rank_len: the rank of the last level, inside t
__device__ __forceinline__ uint32_t numeric_lineage(const unsigned char* __restrict__ t, uint32_t len, const uint32_t* __restrict__ ids,
                                                    uint32_t n_levels, unsigned char* out, uint32_t* rank_a, uint32_t* rank_len) {
    uint32_t n = 0, p = 0;
    *rank_a = 0; *rank_len = 0;
    for (uint32_t k = 0; k < n_levels && p < len; ++k) {
        uint32_t u = p;
        while (u < len && t[u] != '_') ++u;            // a rank holds no '_'
        const uint32_t d = n_digits(ids[k]);
        if (out) {
            if (k) out[n] = ';';
            unsigned char* o = out + n + (k ? 1 : 0);
            for (uint32_t j = p; j < u; ++j) *o++ = t[j];
            *o++ = '_'; *o++ = '_';
            put_digits(o, ids[k], d);
        }
        n += (k ? 1 : 0) + (u - p) + 2 + d;
        *rank_a = p; *rank_len = u - p;
        while (u < len && t[u] != ';') ++u;
        p = u + 1;
    }
    return n;
}

struct RowIn {
    const uint32_t* seg_of; const uint32_t* seg_start;     // [n_rows], [n_seg + 1]
    const uint32_t* line;                  // sorted position -> line
    const uint32_t* key;                   // sorted position -> taxid
    const uint32_t* oid;                   // [n] data-line ordinal
    const uint32_t* item_id;
    const uint64_t* id_a; const uint32_t* id_len; const uint32_t* id_esc;
    const unsigned char* text;
    Paths P;
    uint32_t n_lines;
};

struct RowLine { const unsigned char* norm; uint32_t norm_len; const uint32_t* ids; uint32_t n_levels; };
__device__ __forceinline__ RowLine row_line(const RowIn& R, uint32_t ln) {
    const unsigned long long n0 = min(R.P.norm_off[ln], R.P.norm_total), n1 = min(max(R.P.norm_off[ln + 1], n0), R.P.norm_total);
    const unsigned long long j0 = min(R.P.item_off[ln], (unsigned long long)R.P.n_items);
    const unsigned long long j1 = min(max(R.P.item_off[ln + 1], j0), (unsigned long long)R.P.n_items);
    return RowLine{R.P.norm + n0, (uint32_t)(n1 - n0), R.item_id + j0, (uint32_t)(j1 - j0)};
}

__global__ __launch_bounds__(TPB) void lindb_row_len(RowIn R, uint32_t n, unsigned long long* __restrict__ len) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i > n) return;
    if (i == n) { len[i] = 0; return; }
    const uint32_t s = R.seg_of[i], ln = min(R.line[i], R.n_lines - 1);
    unsigned long long l = cl(A0) + cl(A1) + cl(A2) + R.id_esc[ln] + n_digits(R.oid[ln]);
    l += (i + 1 == R.seg_start[s + 1]) ? cl(A_LAST) : cl(A_NEXT);
    if (i == R.seg_start[s]) {
        const RowLine L = row_line(R, ln);
        uint32_t ra, rl;
        const uint32_t num = numeric_lineage(L.norm, L.norm_len, L.ids, L.n_levels, nullptr, &ra, &rl);
        l += cl(H0) + n_digits(R.key[i]) + cl(H1) + rl + cl(H2) + num + cl(H3) + L.norm_len + cl(H4);
    }
    len[i] = l;
}

__global__ __launch_bounds__(TPB) void lindb_row_write(RowIn R, uint32_t n, const unsigned long long* __restrict__ off, unsigned char* __restrict__ doc) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = R.seg_of[i], ln = min(R.line[i], R.n_lines - 1);
    unsigned char* o = doc + off[i];
    if (i == R.seg_start[s]) {
        const RowLine L = row_line(R, ln);
        uint32_t ra, rl;
        o = put(o, H0);
        const uint32_t d = n_digits(R.key[i]);
        put_digits(o, R.key[i], d);
        o = put(o + d, H1);
        unsigned char* rank_at = o;
        numeric_lineage(L.norm, L.norm_len, L.ids, L.n_levels, nullptr, &ra, &rl);
        o = put_bytes(rank_at, L.norm + ra, rl);
        o = put(o, H2);
        o += numeric_lineage(L.norm, L.norm_len, L.ids, L.n_levels, o, &ra, &rl);
        o = put(o, H3);
        o = put_bytes(o, L.norm, L.norm_len);
        o = put(o, H4);
    }
    o = put(o, A0);
    o = put_escaped(o, R.text, R.id_a[ln], R.id_len[ln]);
    o = put(o, A1);
    const uint32_t d = n_digits(R.oid[ln]);
    put_digits(o, R.oid[ln], d);
    o = put(o + d, A2);
    put(o, (i + 1 == R.seg_start[s + 1]) ? A_LAST : A_NEXT);
}

// the line lists: LIST_MAP `ID taxid\n` of every mapped line, LIST_TSV `ID\tLINE\tempty-lineage\n` of every line without a level
#define EMPTY_LINEAGE "\tempty-lineage\n"
__global__ __launch_bounds__(TPB) void lindb_list_len(int mode, const uint8_t* __restrict__ kind, const uint32_t* __restrict__ id_len,
                                                      const uint32_t* __restrict__ leaf, uint32_t n, unsigned long long* __restrict__ len) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i > n) return;
    unsigned long long l = 0;
    if (i < n && mode == LIST_MAP && kind[i] == L_MAPPED) l = id_len[i] + 1 + n_digits(leaf[i]) + 1;
    if (i < n && mode == LIST_TSV && kind[i] == L_EMPTY) l = id_len[i] + 1 + n_digits(i + 1) + cl(EMPTY_LINEAGE);
    len[i] = l;
}
__global__ __launch_bounds__(TPB) void lindb_list_write(int mode, const uint8_t* __restrict__ kind, const unsigned char* __restrict__ text,
                                                        const uint64_t* __restrict__ id_a, const uint32_t* __restrict__ id_len,
                                                        const uint32_t* __restrict__ leaf, uint32_t n, const unsigned long long* __restrict__ off,
                                                        unsigned char* __restrict__ out) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n || kind[i] != (mode == LIST_MAP ? L_MAPPED : L_EMPTY)) return;
    unsigned char* o = put_bytes(out + off[i], text + id_a[i], id_len[i]);
    const uint32_t v = mode == LIST_MAP ? leaf[i] : i + 1, d = n_digits(v);
    *o++ = mode == LIST_MAP ? ' ' : '\t';
    put_digits(o, v, d);
    o += d;
    if (mode == LIST_MAP) *o = '\n';
    else put(o, EMPTY_LINEAGE);
}

}  // namespace

namespace {

// LinnaeanRank::from_str + Display of a -r target: the letter, or the slug of an Other rank
std::string rank_token(const std::string& r) {
    std::string slug;
    const uint16_t k = parse_rank(r.c_str(), &slug);
    return k == K_FIRST_OTHER ? slug : std::string(1, "udkpcofgs"[k]);
}

int write_file(const std::string& path, const void* a, size_t na, const void* b = nullptr, size_t nb = 0, const void* c = nullptr, size_t nc = 0) {
    const int fd = open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd < 0) { set_error("build-db: cannot create %s: %s", path.c_str(), strerror(errno)); return BLU_ERR_IO; }
    const bool ok = write_all(fd, a, na) && write_all(fd, b, nb) && write_all(fd, c, nc);
    if (close(fd) != 0 || !ok) { set_error("build-db: writing %s failed", path.c_str()); unlink(path.c_str()); return BLU_ERR_IO; }
    return BLU_OK;
}

int build(const blu_lineage_db_desc& D, blu_lineage_db_stats& S) {
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

    // ---- the -r table: HashMap semantics (a repeated key keeps its last value, at its first place)
    std::vector<std::pair<std::string, std::string>> rep;
    if (D.has_replace) for (uint64_t k = 0; k < D.n_replace; ++k) {
        auto it = std::find_if(rep.begin(), rep.end(), [&](const auto& p) { return p.first == D.replace_from[k]; });
        if (it != rep.end()) it->second = D.replace_to[k];
        else rep.emplace_back(D.replace_from[k], D.replace_to[k]);
    }
    std::string rule_bytes;
    std::vector<uint32_t> rule_off{0};
    for (const auto& p : rep) {
        rule_bytes += p.first; rule_off.push_back((uint32_t)rule_bytes.size());
        rule_bytes += rank_token(p.second); rule_off.push_back((uint32_t)rule_bytes.size());
    }
    RankRules R{nullptr, nullptr, (uint32_t)rep.size()};
    {
        unsigned char* d_bytes; uint32_t* d_off;
        HIP_CHECK(pol, mem.upload(&d_bytes, rule_bytes.data(), rule_bytes.size(), "rank rules"));
        HIP_CHECK(pol, mem.upload(&d_off, rule_off.data(), rule_off.size(), "rank rules"));
        R.bytes = d_bytes; R.off = d_off;
    }

    // ---- upload + line index
    DeviceText txt;
    if (const int rc = load_text(D.table_path, D.device, mem, txt); rc != BLU_OK) return rc;
    const uint32_t n = txt.n_lines;
    const Lines T{txt.d, txt.size, txt.line, n};
    S.n_lines = n;
    S.input_bytes = txt.size;
    lap(&S.t_upload_ms);

    // ---- parse
    LineOut lo{};
    unsigned long long* d_words;           // [0] err [1..3] counters
    uint32_t* d_small;                     // [0] first line [1] max depth [2..3] dictionary flags
    HIP_CHECK(pol, mem.alloc(&lo.kind, (size_t)n, "lines"));
    HIP_CHECK(pol, mem.alloc(&lo.levels, ((size_t)n + 1) * 8, "lines")); HIP_CHECK(pol, mem.alloc(&lo.norm_len, ((size_t)n + 1) * 8, "lines"));
    HIP_CHECK(pol, mem.alloc(&lo.is_data, ((size_t)n + 1) * 4, "lines"));
    HIP_CHECK(pol, mem.alloc(&lo.id_a, (size_t)n * 8, "lines")); HIP_CHECK(pol, mem.alloc(&lo.id_len, (size_t)n * 4, "lines"));
    HIP_CHECK(pol, mem.alloc(&lo.id_esc, (size_t)n * 4, "lines"));
    HIP_CHECK(pol, mem.alloc(&lo.lin_a, (size_t)n * 8, "lines")); HIP_CHECK(pol, mem.alloc(&lo.lin_len, (size_t)n * 4, "lines"));
    HIP_CHECK(pol, mem.alloc(&d_words, 32, "counters"));
    HIP_CHECK(pol, mem.alloc(&d_small, 16, "counters"));
    HIP_CHECK(pol, hipMemset(d_words, 0, 32)); HIP_CHECK(pol, hipMemset(d_words, 0xFF, 8));
    HIP_CHECK(pol, hipMemset(d_small, 0, 16)); HIP_CHECK(pol, hipMemset(d_small, 0xFF, 4));
    HIP_CHECK(pol, hipMemset(lo.levels + n, 0, 8)); HIP_CHECK(pol, hipMemset(lo.norm_len + n, 0, 8)); HIP_CHECK(pol, hipMemset(lo.is_data + n, 0, 4));
    lo.err = d_words; lo.counters = d_words + 1; lo.max_depth = d_small + 1;
    uint32_t first = NONE32;
    if (n) {
        hipLaunchKernelGGL(lindb_scan_lines, dim3(grid(n)), dim3(TPB), 0, 0, T, lo.kind, d_small);
        HIP_CHECK(pol, hipGetLastError());
        HIP_CHECK(pol, hipMemcpy(&first, d_small, 4, hipMemcpyDeviceToHost));
        const uint32_t header = (first != NONE32 && !(first & 1u)) ? first >> 1 : NONE32;
        hipLaunchKernelGGL(lindb_classify, dim3(grid(n)), dim3(TPB), 0, 0, T, header, R, lo);
        HIP_CHECK(pol, hipGetLastError());
    }
    {
        unsigned long long w[4];
        uint32_t depth = 0;
        HIP_CHECK(pol, hipMemcpy(w, d_words, 32, hipMemcpyDeviceToHost));
        HIP_CHECK(pol, hipMemcpy(&depth, d_small + 1, 4, hipMemcpyDeviceToHost));
        if (w[0] != ~0ull) {
            const uint32_t code = (uint32_t)(w[0] & 7);
            const char* what = code == E_UTF8 ? "the line is not UTF-8"
                             : code == E_NO_TAB ? "no tab between the ID and the lineage"
                             : code == E_EMPTY_ID ? "an empty ID"
                             : code == E_NO_RANK ? "a level without `__` (every level must be RANK__NAME; rank-less lineages such as "
                                                   "`Bacteria;Proteobacteria` are not supported)"
                             : code == E_EMPTY_RANK ? "a level whose rank is empty" : "more than 64 levels";
            set_error("%s:%llu: %s", D.table_path, (w[0] >> 3) + 1, what);
            return code == E_DEPTH ? BLU_ERR_DEPTH : BLU_ERR_PARSE;
        }
        S.n_data_lines = w[1]; S.n_empty = w[2]; S.n_truncated = w[3]; S.max_depth = depth;
    }
    unsigned long long *item_off, *norm_off;
    uint32_t* oid;
    void* stmp;
    HIP_CHECK(pol, mem.alloc(&item_off, ((size_t)n + 1) * 8, "lines")); HIP_CHECK(pol, mem.alloc(&norm_off, ((size_t)n + 1) * 8, "lines"));
    HIP_CHECK(pol, mem.alloc(&oid, ((size_t)n + 1) * 4, "lines"));
    HIP_CHECK(pol, mem.alloc(&stmp, std::max(scan_tmp_bytes_u32((size_t)n + 1), scan_tmp_bytes_u64((size_t)n + 1)), "scan"));
    HIP_CHECK(pol, exclusive_scan_u64(lo.levels, item_off, (size_t)n + 1, stmp));
    HIP_CHECK(pol, exclusive_scan_u64(lo.norm_len, norm_off, (size_t)n + 1, stmp));
    HIP_CHECK(pol, exclusive_scan_u32(lo.is_data, oid, (size_t)n + 1, stmp));
    unsigned long long items64 = 0, norm_total = 0;
    HIP_CHECK(pol, hipMemcpy(&items64, item_off + n, 8, hipMemcpyDeviceToHost));
    HIP_CHECK(pol, hipMemcpy(&norm_total, norm_off + n, 8, hipMemcpyDeviceToHost));
    if (items64 > MAX_ITEMS) { set_error("build-db: %s has more than 2^30 lineage levels in all", D.table_path); return BLU_ERR_INVALID_ARG; }
    const uint32_t n_items = (uint32_t)items64;
    S.n_levels = n_items;
    unsigned char* norm;
    uint32_t *item_line, *item_len;
    unsigned long long* item_hash;
    HIP_CHECK(pol, mem.alloc(&norm, norm_total + 16, "normalised lineages"));
    HIP_CHECK(pol, mem.alloc(&item_line, (size_t)n_items * 4, "items")); HIP_CHECK(pol, mem.alloc(&item_len, (size_t)n_items * 4, "items"));
    HIP_CHECK(pol, mem.alloc(&item_hash, (size_t)n_items * 8, "items"));
    const Paths P{norm, norm_total, norm_off, item_off, item_line, item_len, item_hash, n_items, n};
    const unsigned long long hash_mask = (D.hash_bits == 0 || D.hash_bits >= 64) ? ~0ull : (1ull << D.hash_bits) - 1;
    if (n_items) hipLaunchKernelGGL(lindb_write_paths, dim3(grid(n)), dim3(TPB), 0, 0, T, R, (const uint8_t*)lo.kind, (const uint64_t*)lo.lin_a,
                                    (const uint32_t*)lo.lin_len, P, hash_mask, norm, item_line, item_len, item_hash);
    HIP_CHECK(pol, hipGetLastError());
    lap(&S.t_parse_ms);

    // ---- intern: the dictionary, doubled while more than half full
    uint32_t *slot = nullptr, *item_slot, *first_mark, *first_excl, *item_id, n_slots = 16, n_taxa = 0;
    const uint64_t want = D.initial_slots ? D.initial_slots : 2ull * n_items;
    while (n_slots < want && n_slots < (1u << 31)) n_slots <<= 1;
    HIP_CHECK(pol, mem.alloc(&item_slot, (size_t)n_items * 4, "items")); HIP_CHECK(pol, mem.alloc(&item_id, (size_t)n_items * 4, "items"));
    HIP_CHECK(pol, mem.alloc(&first_mark, ((size_t)n_items + 1) * 4, "items")); HIP_CHECK(pol, mem.alloc(&first_excl, ((size_t)n_items + 1) * 4, "items"));
    for (;;) {
        ++S.n_dictionary_builds;
        HIP_CHECK(pol, mem.alloc(&slot, (size_t)n_slots * 4, "path dictionary"));
        HIP_CHECK(pol, hipMemset(slot, 0xFF, (size_t)n_slots * 4));
        HIP_CHECK(pol, hipMemset(d_small + 2, 0, 8));
        if (n_items) hipLaunchKernelGGL(lindb_intern, dim3(grid(n_items)), dim3(TPB), 0, 0, P, slot, n_slots, item_slot, d_small + 2);
        HIP_CHECK(pol, hipGetLastError());
        uint32_t flags[2];
        HIP_CHECK(pol, hipMemcpy(flags, d_small + 2, 8, hipMemcpyDeviceToHost));
        if (!flags[0] && flags[1] <= n_slots / 2) break;
        if (n_slots >= (1u << 31)) { set_error("build-db: the path dictionary of %s cannot grow further", D.table_path); return BLU_ERR_INVALID_ARG; }
        mem.free(slot);
        n_slots <<= 1;
    }
    {
        void* itmp;
        HIP_CHECK(pol, mem.alloc(&itmp, scan_tmp_bytes_u32((size_t)n_items + 1), "scan"));
        hipLaunchKernelGGL(lindb_mark_first, dim3(grid((uint64_t)n_items + 1)), dim3(TPB), 0, 0, (const uint32_t*)slot, n_slots, (const uint32_t*)item_slot,
                           n_items, first_mark);
        HIP_CHECK(pol, exclusive_scan_u32(first_mark, first_excl, (size_t)n_items + 1, itmp));
        HIP_CHECK(pol, hipMemcpy(&n_taxa, first_excl + n_items, 4, hipMemcpyDeviceToHost));
        if (n_items) hipLaunchKernelGGL(lindb_item_ids, dim3(grid(n_items)), dim3(TPB), 0, 0, (const uint32_t*)slot, n_slots, (const uint32_t*)item_slot,
                                        (const uint32_t*)first_excl, n_items, item_id);
        HIP_CHECK(pol, hipGetLastError());
    }
    S.n_taxa = n_taxa;
    lap(&S.t_intern_ms);

    // ---- group the lines by the taxid of their last level
    uint32_t *leaf, *keys, *vals, *keys_alt, *vals_alt;
    HIP_CHECK(pol, mem.alloc(&leaf, (size_t)n * 4, "rows"));
    HIP_CHECK(pol, mem.alloc(&keys, (size_t)n * 4, "rows")); HIP_CHECK(pol, mem.alloc(&vals, (size_t)n * 4, "rows"));
    HIP_CHECK(pol, mem.alloc(&keys_alt, (size_t)n * 4, "rows")); HIP_CHECK(pol, mem.alloc(&vals_alt, (size_t)n * 4, "rows"));
    if (n) hipLaunchKernelGGL(lindb_leaf_keys, dim3(grid(n)), dim3(TPB), 0, 0, (const uint8_t*)lo.kind, (const unsigned long long*)item_off,
                              (const uint32_t*)item_id, n_items, n, n_taxa, leaf, keys, vals);
    HIP_CHECK(pol, hipGetLastError());
    int bits = 0;
    while (bits < 32 && (((uint64_t)n_taxa + 1) >> bits) != 0) ++bits;   // keys <= n_taxa + 1
    {
        uint32_t* table;
        void* tmp;
        HIP_CHECK(pol, mem.alloc(&table, radix_table_words(n) * 4, "radix sort"));
        HIP_CHECK(pol, mem.alloc(&tmp, radix_scan_tmp_bytes(n), "radix sort"));
        HIP_CHECK(pol, radix_sort_pairs(&keys, &keys_alt, &vals, &vals_alt, n, bits, table, tmp));
    }
    const uint32_t n_rows = (uint32_t)(S.n_data_lines - S.n_empty);      // the mapped lines come first
    uint32_t *head, *excl, *seg_of, *seg_start, n_seg = 0;
    HIP_CHECK(pol, mem.alloc(&head, ((size_t)n_rows + 1) * 4, "segments")); HIP_CHECK(pol, mem.alloc(&excl, ((size_t)n_rows + 1) * 4, "segments"));
    HIP_CHECK(pol, mem.alloc(&seg_of, (size_t)n_rows * 4, "segments")); HIP_CHECK(pol, mem.alloc(&seg_start, ((size_t)n_rows + 1) * 4, "segments"));
    hipLaunchKernelGGL(lindb_heads, dim3(grid((uint64_t)n_rows + 1)), dim3(TPB), 0, 0, (const uint32_t*)keys, n_rows, head);
    HIP_CHECK(pol, exclusive_scan_u32(head, excl, (size_t)n_rows + 1, stmp));
    if (n_rows) hipLaunchKernelGGL(lindb_segments, dim3(grid(n_rows)), dim3(TPB), 0, 0, (const uint32_t*)head, (const uint32_t*)excl, n_rows, seg_of, seg_start);
    HIP_CHECK(pol, hipGetLastError());
    HIP_CHECK(pol, hipMemcpy(&n_seg, excl + n_rows, 4, hipMemcpyDeviceToHost));
    HIP_CHECK(pol, hipMemcpy(seg_start + n_seg, &n_rows, 4, hipMemcpyHostToDevice));
    S.n_taxonomies = n_seg;
    lap(&S.t_group_ms);

    // ---- render the taxonomies array and the two line lists
    const RowIn RI{seg_of, seg_start, vals, keys, oid, item_id, lo.id_a, lo.id_len, lo.id_esc, txt.d, P, n};
    unsigned long long *row_len, *row_off, body = 0;
    const size_t n_len = (size_t)std::max(n, n_rows) + 1;
    HIP_CHECK(pol, mem.alloc(&row_len, n_len * 8, "render"));
    HIP_CHECK(pol, mem.alloc(&row_off, n_len * 8, "render"));
    hipLaunchKernelGGL(lindb_row_len, dim3(grid((uint64_t)n_rows + 1)), dim3(TPB), 0, 0, RI, n_rows, row_len);
    HIP_CHECK(pol, exclusive_scan_u64(row_len, row_off, (size_t)n_rows + 1, stmp));
    HIP_CHECK(pol, hipMemcpy(&body, row_off + n_rows, 8, hipMemcpyDeviceToHost));
    unsigned char* d_doc;
    HIP_CHECK(pol, mem.alloc(&d_doc, body + 16, "document"));
    if (n_rows) hipLaunchKernelGGL(lindb_row_write, dim3(grid(n_rows)), dim3(TPB), 0, 0, RI, n_rows, (const unsigned long long*)row_off, d_doc);
    HIP_CHECK(pol, hipGetLastError());
    Column<char> h_doc, h_list[2];
    h_doc.resize(body);
    std::vector<D2HPiece> pieces;
    d2h_add(pieces, h_doc.data(), d_doc, body);
    for (int mode : {LIST_MAP, LIST_TSV}) {
        if (mode == LIST_MAP && !D.taxid_map_path) continue;
        unsigned long long total = 0;
        hipLaunchKernelGGL(lindb_list_len, dim3(grid((uint64_t)n + 1)), dim3(TPB), 0, 0, mode, (const uint8_t*)lo.kind, (const uint32_t*)lo.id_len,
                           (const uint32_t*)leaf, n, row_len);
        HIP_CHECK(pol, exclusive_scan_u64(row_len, row_off, (size_t)n + 1, stmp));
        HIP_CHECK(pol, hipMemcpy(&total, row_off + n, 8, hipMemcpyDeviceToHost));
        unsigned char* d_list;
        HIP_CHECK(pol, mem.alloc(&d_list, total + 16, "line list"));
        if (n) hipLaunchKernelGGL(lindb_list_write, dim3(grid(n)), dim3(TPB), 0, 0, mode, (const uint8_t*)lo.kind, (const unsigned char*)txt.d,
                                  (const uint64_t*)lo.id_a, (const uint32_t*)lo.id_len, (const uint32_t*)leaf, n, (const unsigned long long*)row_off, d_list);
        HIP_CHECK(pol, hipGetLastError());
        h_list[mode].resize(total);
        d2h_add(pieces, h_list[mode].data(), d_list, total);
    }
    HIP_CHECK(pol, hipDeviceSynchronize());
    HIP_CHECK(pol, d2h_parallel(pieces, D.device));
    lap(&S.t_render_ms);

    // ---- write: the head and tail around the rendered array (serde_json::to_string_pretty of TaxonomiesMap)
    std::string headtxt = "{\n  \"blutilsVersion\": ";
    json_str(headtxt, D.blutils_version ? D.blutils_version : BLU_TAXDB_DEFAULT_VERSION);
    headtxt += ",\n  \"ignoreTaxids\": null,\n";
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
    headtxt += "  \"dropNonLinnaeanTaxonomies\": null,\n  \"sourceDatabase\": ";
    json_str(headtxt, D.source_database ? D.source_database : "");
    headtxt += ",\n";
    const std::string stem = D.output_stem;
    const std::string json_path = stem + ".blutils.json", tsv_path = stem + ".non-mapped.tsv";
    if (unlink(tsv_path.c_str()) != 0 && errno != ENOENT) { set_error("build-db: cannot remove %s: %s", tsv_path.c_str(), strerror(errno)); return BLU_ERR_IO; }
    if (const int rc = write_file(tsv_path, h_list[LIST_TSV].data(), h_list[LIST_TSV].size()); rc != BLU_OK) return rc;
    if (body == 0) {
        headtxt += "  \"taxonomies\": []\n}";
        if (const int rc = write_file(json_path, headtxt.data(), headtxt.size()); rc != BLU_OK) return rc;
    } else {
        headtxt += "  \"taxonomies\": [\n";
        static const char tail[] = "\n  ]\n}";
        if (const int rc = write_file(json_path, headtxt.data(), headtxt.size(), h_doc.data() + 2, body - 2, tail, sizeof tail - 1); rc != BLU_OK) return rc;
    }
    S.doc_bytes = headtxt.size() + (body ? body - 2 + 6 : 0);
    S.tsv_bytes = h_list[LIST_TSV].size();
    if (D.taxid_map_path) {
        const std::string map_path = D.taxid_map_path, partial = map_path + ".partial";
        if (const int rc = write_file(partial, h_list[LIST_MAP].data(), h_list[LIST_MAP].size()); rc != BLU_OK) return rc;
        if (rename(partial.c_str(), map_path.c_str()) != 0) {
            set_error("build-db: cannot rename %s to %s: %s", partial.c_str(), map_path.c_str(), strerror(errno));
            unlink(partial.c_str());
            return BLU_ERR_IO;
        }
        S.map_bytes = h_list[LIST_MAP].size();
    }
    lap(&S.t_write_ms);
    return BLU_OK;
}

}  // namespace
}  // namespace blu

extern "C" int blu_lineage_db_build(const blu_lineage_db_desc* desc, blu_lineage_db_stats* stats) {
    if (!desc || !desc->table_path || !desc->output_stem || (desc->has_replace && desc->n_replace && (!desc->replace_from || !desc->replace_to))) {
        blu::set_error("blu_lineage_db_build: null argument");
        return BLU_ERR_INVALID_ARG;
    }
    blu_lineage_db_stats local;
    blu_lineage_db_stats& S = stats ? *stats : local;
    memset(&S, 0, sizeof S);
    return blu::build(*desc, S);
}
