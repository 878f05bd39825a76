// GPU ingest of BLAST outfmt-6 text ("GPU-side parser"): the whole file goes to HBM once and comes back as
// the grouped SoA columns the engine reads.  It produces exactly what the CPU ingest in pipeline_ingest.cpp produces
// (reference: build_consensus_identities/mod.rs:134-244,329-373 — 13 tab-separated columns, rows regrouped by query
// in first-appearance order with file order kept inside a query, bit_score truncated toward zero, left join on the
// taxid), for files in the plain form BLAST writes; any other file (quotes, empty lines, odd numbers) is handed back
// to the CPU path untouched (BLU_INGEST_FALLBACK).
//
// This file holds the parser, the hit and taxon filters, the dictionaries, the grouping, and the host code that runs them:
// GpuIngest, whose steps are the stages below.  The upload and the threaded download are dev_io.cpp; the line index, the
// prefix sums, the radix sort and the column compaction are dev_prims.hip (both behind ingest_prims.h); the engine on the
// columns left here is engine_dev.hip.  All on the handle's device, the kernels on the default stream:
//   0. upload          pread() into pinned staging slots -> HBM (dev_io.cpp: the file is never mapped into the process)
//   1. line index      newline count per 4 KiB tile -> exclusive scan -> line starts (dev_prims.hip)
//   2. parse           one thread per line: tab scan over aligned 16-byte loads, decimal fast path for the four numeric
//                      columns (mantissa <= 15 digits and |exp10| <= 22: one IEEE operation, so the value is strtod's),
//                      taxid -> taxonomy row through the uploaded open-addressing map, two 64-bit hashes of the query
//                      and accession fields; under a hit or taxon filter a keep word per line, and the kept rows compacted.
//                      One staged form (parse_rows_body), one general form (parse_row_general) and one tail (finish_row)
//                      serve all eight kernels: a build is a MODE (no filter, thresholds, taxon filter) and a layout type
//                      (the reference's columns, a column layout, a layout with a query cover).  Only how a thread of
//                      the staged form learns where a field begins and ends differs by layout: RefFields, LayoutFields
//   3. dictionaries    open-addressing tables keyed by hash (insert = CAS on the hash + atomicMin of the row), finalised
//                      with length + first 12 key bytes; every row then verifies its own text against its slot (a
//                      mismatch = two strings with one 64-bit hash -> fallback), so ids are exact, not probabilistic
//   4. ids             queries numbered by first row (the first rows marked in a row-indexed array, a prefix sum over it);
//                      accessions ranked in byte order on the host (only the distinct strings travel; the sort runs on a
//                      thread of its own while the device builds the query dictionary) and the ranks uploaded
//   5. grouping        stable radix sort by query id unless the file is grouped already; gathers; segment offsets
//   6. hand-over       the grouped columns stay on the device for the engine (host copies only on request); the distinct
//                      query / accession strings come back packed and a background thread turns them into the host tables
// HBM-bound byte work: no MFMA.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <string_view>
#include <thread>
#include <type_traits>
#include <vector>

#include "blu_consensus.h"
#include "hit_pass.h"
#include "ingest.h"
#include "taxid_probe.h"
#include "wave_scan.h"

namespace blu {
namespace {

enum : uint32_t {
    FB_EMPTY_LINE = 1, FB_COLUMNS = 2, FB_QUOTE = 4, FB_NUMBER = 8, FB_RANGE = 16, FB_HASH_COLLISION = 32, FB_TABLE_FULL = 64,
};

struct Slot {            // 32 bytes
    unsigned long long hash;   // 0 = empty
    uint32_t first_row;        // smallest row index holding this key
    uint32_t id;               // query id / accession rank
    uint32_t len;
    unsigned char head[12];
};
// ---- 2. parse (the taxid join: taxid_probe.h) ------------------------------------------------------------------
__device__ const double P10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

struct NumState {
    unsigned long long mant;
    int digits, frac, exp10, exp_digits;
    bool neg, exp_neg, exp_sign, seen_dot, seen_exp, bad, any;
    __device__ void reset() { mant = 0; digits = frac = exp10 = exp_digits = 0; neg = exp_neg = exp_sign = seen_dot = seen_exp = bad = any = false; }
    __device__ void feed(uint32_t c, bool first) {
        if (c - '0' < 10u) {
            if (seen_exp) { exp10 = exp10 * 10 + (int)(c - '0'); if (++exp_digits > 3) bad = true; }
            else { mant = mant * 10 + (c - '0'); if (mant != 0 || seen_dot) ++digits; if (seen_dot) ++frac; any = true; }
        } else if (c == '-' && first) neg = true;
        else if (c == '.' && !seen_dot && !seen_exp) seen_dot = true;
        else if ((c == 'e' || c == 'E') && any && !seen_exp) seen_exp = true;
        else if ((c == '-' || c == '+') && seen_exp && exp_digits == 0 && !exp_sign) { exp_sign = true; exp_neg = c == '-'; }
        else bad = true;
    }
    // the value strtod gives, or bad: mantissa and 10^k exact, one correctly rounded operation (Clinger's fast path)
    __device__ bool value(double* out) const {
        if (bad || !any || digits > 15 || frac > 300 || (seen_exp && exp_digits == 0)) return false;
        const int e = (exp_neg ? -exp10 : exp10) - frac;
        if (e < -22 || e > 22) return false;
        const double m = (double)mant;
        const double x = e < 0 ? m / P10[-e] : m * P10[e];
        *out = neg ? -x : x;
        return true;
    }
    // the grammar value() takes, whatever the exponent: the e-value column of a filtered parse (its decision: e_value_verdict)
    __device__ bool plain() const { return !(bad || !any || digits > 15 || frac > 300 || (seen_exp && exp_digits == 0)); }
    __device__ int exponent() const { return (exp_neg ? -exp10 : exp10) - frac; }
};

// ---- hit filter.  The parse kernels' filtered builds evaluate the thresholds of include/blu_pipeline.h's
// blu_hit_filter on the values they parsed and leave one word per line: 0 dropped, 1 kept, 2 = e-value left to the host.
struct DevFilter {
    uint32_t mask;               // BLU_FILTER_* bits
    uint32_t e_band;             // 1: an e-value within a few decades of max_e may be computed here (max_e in [1e-280, 1e280])
    double min_pid, min_bs, max_e;
    long long min_aln;
    int k_keep, k_drop;          // decimal magnitude tests: digits + exponent <= k_keep -> below max_e; digits - 1 + exponent >= k_drop -> above
    double e_lo, e_hi;           // max_e (1 -+ 2^-46): a computed value at or below e_lo is kept, at or above e_hi dropped
    uint32_t* keep;              // [n_rows]
    unsigned long long* counts;  // [0 .. HIT_SPREAD) kept lines (hit_pass.h: spread over blocks), [HIT_SPREAD] lines left to the host
};
enum : uint32_t { KEEP_NO = 0, KEEP_YES = 1, KEEP_ASK_HOST = 2 };

// `strtod(field) <= max_e` for a field of the plain grammar (NumState::plain), value = mant x 10^e with mant < 10^15.
//   1. mant == 0: the value is zero.  A minus sign: left to the host (BLAST writes none).
//   2. d = decimal digits of mant: 10^(d - 1 + e) <= value < 10^(d + e); the host derived k_keep / k_drop from max_e with two
//      decades of slack, so these two tests are safe whatever strtod rounds to (overflow to inf and underflow to 0 included).
//   3. |e| <= 22: one correctly rounded operation on exact operands gives strtod's value (as NumState::value): compared as is.
//   4. otherwise mant is scaled by exact powers of ten, 22 decades per step: at most 14 steps inside the band, each within
//      2^-53 relative, so the result x is within 2^-49 of the decimal value v.  x <= max_e (1 - 2^-46) gives v < max_e, hence
//      strtod(v) <= max_e (rounding is monotonic); x >= max_e (1 + 2^-46) gives v > max_e (1 + 2^-47), beyond the double
//      above max_e, hence strtod(v) > max_e.  In between — in practice a field spelled like the threshold — the host decides
//      from the field's bytes.
__device__ __noinline__ uint32_t e_value_verdict(unsigned long long mant, int e, bool neg, const DevFilter& f) {
    if (mant == 0) return f.max_e >= 0.0 ? KEEP_YES : KEEP_NO;
    if (neg) return KEEP_ASK_HOST;
    const double m = (double)mant;
    int d = 1;
    while (d < 15 && m >= P10[d]) ++d;
    if (d + e <= f.k_keep) return KEEP_YES;
    if (d - 1 + e >= f.k_drop) return KEEP_NO;
    if (e >= -22 && e <= 22) return (e < 0 ? m / P10[-e] : m * P10[e]) <= f.max_e ? KEEP_YES : KEEP_NO;
    if (!f.e_band) return KEEP_ASK_HOST;
    double x = m;
    for (int r = e; r > 0; r -= 22) x *= P10[r < 22 ? r : 22];
    for (int r = -e; r > 0; r -= 22) x /= P10[r < 22 ? r : 22];
    return x <= f.e_lo ? KEEP_YES : (x >= f.e_hi ? KEEP_NO : KEEP_ASK_HOST);
}

// the four thresholds on one validated line -> its keep word, and the two counts (one atomic per wave and count)
__device__ __forceinline__ void filter_row(const DevFilter& f, uint32_t i, double v_pid, double v_aln, double v_bs,
                                           unsigned long long e_mant, int e_exp, bool e_neg) {
    bool pass = true;
    if ((f.mask & BLU_FILTER_MIN_PERC_IDENTITY) && !(v_pid >= f.min_pid)) pass = false;
    if ((f.mask & BLU_FILTER_MIN_ALIGN_LENGTH) && !((long long)v_aln >= f.min_aln)) pass = false;   // (v_aln passed the 32-bit range check)
    if ((f.mask & BLU_FILTER_MIN_BIT_SCORE) && !(v_bs >= f.min_bs)) pass = false;                   // as written: before the truncation
    uint32_t k = pass ? KEEP_YES : KEEP_NO;
    if (pass && (f.mask & BLU_FILTER_MAX_E_VALUE)) k = e_value_verdict(e_mant, e_exp, e_neg, f);
    f.keep[i] = k;
    const uint32_t lane = threadIdx.x & 63u;
    spread_add_ballot(f.counts, 0, k == KEEP_YES);
    const unsigned long long ask = __ballot(k == KEEP_ASK_HOST);     // (rare: one word takes them all)
    if (k == KEEP_ASK_HOST && (ask & ((1ull << lane) - 1ull)) == 0) atomicAdd(&f.counts[HIT_SPREAD], (unsigned long long)__popcll(ask));
}

// ---- taxon filter.  The host made one 16-bit code per taxonomy row from the lineages (ingest.h: TaxonCodes);
// the PARSE_TAXA builds of the parse kernels read the code of the row a line joined to — 2 bytes beside the 16-byte map entry the
// join just read — and takes the line's verdict from it before the thresholds: a failing line's keep word is 0 at once and
// its e-value is never looked at.
struct DevTaxa {
    const uint16_t* code;                  // [n_tax]
    uint32_t n_tax;
    uint32_t unmatched;                    // the verdict of a line whose taxid is not in the taxonomy
    unsigned long long* excluded_by;       // [n_exclude] lines whose first matching exclude element it is
    unsigned long long* not_only;          // [HIT_SPREAD] lines failing only the only list (spread over blocks)
};
struct DevFilterTaxa { DevFilter f; DevTaxa t; };

// The counts are per wave, not per line.  Excluded lanes: the code of the first one left is broadcast, the lanes that share it
// are found with one ballot, one lane adds their number to that element's count, and they retire — one round per distinct
// code in the wave (one or two as a rule, since neighbouring lines hit neighbouring taxa), so an element that removes most
// of a table costs one atomic per wave.  `left` is the same in every lane: the loop is uniform over the wave's active lanes.
__device__ __forceinline__ uint32_t taxon_verdict(const DevTaxa& t, uint32_t row) {
    const uint32_t code = row < t.n_tax ? (uint32_t)t.code[row] : t.unmatched;   // (BLU_UNMATCHED_TAXID is no row)
    const uint32_t lane = threadIdx.x & 63u;
    const bool excl = code != 0 && code != TAXON_NOT_ONLY;
    unsigned long long left = __ballot(excl);
    while (left) {
        const int first = __builtin_amdgcn_readfirstlane(__ffsll(left) - 1);
        const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)code, first);
        const unsigned long long same = __ballot(excl && code == c);
        if (lane == (uint32_t)first) atomicAdd(&t.excluded_by[c - 1], (unsigned long long)__popcll(same));
        left &= ~same;
    }
    spread_add_ballot(t.not_only, 0, code == TAXON_NOT_ONLY);
    return code;
}

__device__ __forceinline__ unsigned long long hash_step(unsigned long long h, uint32_t c) { return (h ^ c) * 1099511628211ull; }
__device__ __forceinline__ unsigned long long hash_finish(unsigned long long h, uint32_t len) {
    h ^= (unsigned long long)len * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
    return h ? h : 1ull;   // 0 marks an empty slot
}

struct RowOut {
    unsigned long long* qh; unsigned long long* ah;     // hashes of the query / accession fields
    unsigned long long* qpos; unsigned long long* apos;  // field offset | length << 44
    uint32_t* tax; double* pid; int32_t* aln; int32_t* bs;
};

// ---- where a line's fields are.  The parse reads seven fields of a line, the roles.  In the reference's thirteen columns their
// places are constants: RefLayout, an empty type, so every test against it folds at compile time.  In a table written with another
// `-outfmt "6 ..."` list they sit where include/blu_pipeline.h's blu_table_layout says: DevLayout, a kernel
// argument, the same for every thread — it lives in scalar registers, and every test against it is a vector compare with a
// scalar operand.  The parser below reads either through lay_n_cols / lay_col / lay_tax_list and is otherwise one text.
enum : int { ROLE_QUERY = 0, ROLE_ACC = 1, ROLE_TAX = 2, ROLE_PID = 3, ROLE_ALN = 4, ROLE_BS = 5, ROLE_E = 6, N_ROLES = 7 };
struct DevLayout {               // 48 bytes
    uint32_t n_cols;             // fields a line must have (1 .. 64)
    uint32_t col[N_ROLES];       // column of each role; ROLE_E: 0xFFFFFFFF without an e-value column (the threshold is refused then)
    uint32_t tax_list;           // the taxid field is `staxids`: the number ends at its first ';'
    uint32_t reserved;
    unsigned long long wanted;   // bit t: tab t — the one behind column t — bounds a role field (column t or t + 1 holds a role)
};
struct RefLayout {};             // mod.rs:134-244: 13 columns, the roles in columns 0 .. 4, the e-value in 11, the bit score in 12
__device__ constexpr uint32_t lay_n_cols(const RefLayout&) { return 13; }
__device__ constexpr uint32_t lay_n_cols(const DevLayout& L) { return L.n_cols; }
__device__ constexpr uint32_t lay_col(const RefLayout&, int r) { return r == ROLE_BS ? 12u : r == ROLE_E ? 11u : (uint32_t)r; }
__device__ constexpr uint32_t lay_col(const DevLayout& L, int r) { return L.col[r]; }
__device__ constexpr bool lay_tax_list(const RefLayout&) { return false; }
__device__ constexpr bool lay_tax_list(const DevLayout& L) { return L.tax_list != 0; }

// ---- the query cover: a fifth threshold of the keep word, on fields the seven roles do not include — one
// column (`qcovhsp` or `qcovs`: BLAST's integer percent) or three (`qstart`, `qend`, `qlen`: the exact ratio).  A cover build
// takes the layout with the cover behind it, DevLayoutCover: the layout's type says whether a build has a cover (HAS_COVER).
// `wanted` also names the tab in front of every cover field.
enum : int { COVER_FIELDS = 3 };
struct DevCover {
    uint32_t by_len;             // 0: col[0] holds the percent c, kept iff c * 1000 >= p_milli; 1: col = {qstart, qend, qlen},
    uint32_t n_fields;           //    kept iff (|qend - qstart| + 1) * 100000 >= p_milli * qlen.  n_fields: 1 or 3
    uint32_t col[COVER_FIELDS];  // (unused: 0xFFFFFFFF, which no tab count reaches)
    uint32_t reserved;
    double p_milli;              // the threshold times 1000: an integer 0 .. 100000
    unsigned long long* below;   // [HIT_SPREAD] lines below the cover, whatever the other filters say (spread over blocks)
};
struct DevLayoutCover : DevLayout { DevCover cov; };
template <class LAY> constexpr bool HAS_COVER = std::is_same<LAY, DevLayoutCover>::value;

// One cover field, already read: an Int64 field (no fraction, no exponent — else FB_NUMBER and the host parser's error) in
// 0 .. 2^31 - 1 (else FB_RANGE, likewise).  NumState::value has the integer exactly: at most 15 digits.
__device__ __forceinline__ uint32_t cover_field(const NumState& num, double* v) {
    if (!num.value(v) || num.seen_dot || num.seen_exp) return FB_NUMBER;
    return *v >= 0.0 && *v <= 2147483647.0 ? 0u : FB_RANGE;
}
// The line's verdict on its three values (v[1], v[2] unused for a percent column) and the count.  Every operand is an integer
// below 2^31 and every product below 2^48: the doubles compare as the host's 64-bit integers do.  Every lane that validated
// its line calls it, before the taxon verdict: the count does not depend on the other filters.  false: qlen = 0 (FB_RANGE).
__device__ __forceinline__ bool cover_verdict(const DevCover& c, const double v[COVER_FIELDS], bool* below) {
    if (c.by_len) {
        if (v[2] == 0.0) return false;
        *below = !((fabs(v[1] - v[0]) + 1.0) * 100000.0 >= c.p_milli * v[2]);
    } else *below = !(v[0] * 1000.0 >= c.p_milli);
    spread_add_ballot(c.below, 0, *below);
    return true;
}

// ---- the parser: two forms (general, staged) over one tail, each a template on MODE and on the layout's type.
// PARSE_PLAIN: every unfiltered call; flt is null and unmatched rows are counted here.  PARSE_FILTER: the e-value field is read
// when its threshold is on, the thresholds are evaluated on the parsed values and every line gets a keep word (filter_row);
// unmatched rows are counted over the kept rows, after the compaction.  PARSE_TAXA: as PARSE_FILTER with the taxon verdict
// (taxon_verdict) taken first; the thresholds may all be off, as they may under a cover alone.
enum : int { PARSE_PLAIN = 0, PARSE_FILTER = 1, PARSE_TAXA = 2 };

struct RowValues {               // what a line's fields read as, before finish_row's checks
    double tax = 0, pid = 0, aln = 0, bs = 0, cov[COVER_FIELDS] = {0, 0, 0};
    unsigned long long e_mant = 0;   // the e-value field, read only under its threshold: e_value_verdict's operands
    int e_exp = 0;
    bool e_neg = false;
};

// The tail of both forms, on a line whose fields all read well: the 32-bit range checks, the truncation of the bit score, the
// cover's verdict and count (ahead of the taxon verdict's early-out: it is counted whatever the other filters say), the taxid
// join, the line's keep word — a line the taxon filter or the cover removes never has its e-value looked at — or, in the
// unfiltered builds, the unmatched count; then the four value columns.  false: the line set FB_RANGE and nothing was stored.
template <int MODE, class LAY>
__device__ __forceinline__ bool finish_row(const LAY& L, uint32_t i, const RowValues& v, const DevTaxidMap& taxmap, const RowOut& o,
                                           uint32_t* __restrict__ flags, unsigned long long* __restrict__ n_unmatched, const DevFilterTaxa* flt) {
    static_assert(MODE != PARSE_PLAIN || !HAS_COVER<LAY>, "a cover leaves a keep word: it needs a filtered build");
    // mod.rs:184 AnyValue::Float64 -> try_extract::<i64> (truncation); the engine columns are 32-bit
    const double bs_t = trunc(v.bs);
    if (!(bs_t >= -2147483648.0 && bs_t <= 2147483647.0) || !(v.aln >= -2147483648.0 && v.aln <= 2147483647.0) ||
        !(v.tax >= -9.2e18 && v.tax <= 9.2e18)) { atomicOr(flags, FB_RANGE); return false; }
    bool below = false;
    if constexpr (HAS_COVER<LAY>) if (!cover_verdict(L.cov, v.cov, &below)) { atomicOr(flags, FB_RANGE); return false; }
    const uint32_t row = taxid_lookup(taxmap, (long long)v.tax);   // left join (mod.rs:72-76)
    if constexpr (MODE == PARSE_PLAIN) { if (row == BLU_UNMATCHED_TAXID) atomicAdd(n_unmatched, 1ull); }
    else {
        bool drop = below;
        if constexpr (MODE == PARSE_TAXA) drop = taxon_verdict(flt->t, row) || below;
        if (drop) flt->f.keep[i] = KEEP_NO;
        else filter_row(flt->f, i, v.pid, v.aln, v.bs, v.e_mant, v.e_exp, v.e_neg);
    }
    o.tax[i] = row; o.pid[i] = v.pid; o.aln[i] = (int32_t)v.aln; o.bs[i] = (int32_t)bs_t;
    return true;
}

// The general form: one line, read from global memory a byte at a time through one state machine for all its columns, up to the
// end of column n_cols - 1.  It takes any line length: the staged form below hands it the blocks whose 256 lines do not fit the
// LDS stage.  A `staxids` field is fed to the number reader up to its first ';' only.
template <int MODE, class LAY>
__device__ __noinline__ void parse_row_general(const unsigned char* __restrict__ text, const uint64_t* __restrict__ line_start, uint32_t i,
                                               const DevTaxidMap& taxmap, const RowOut& o, uint32_t* __restrict__ flags,
                                               unsigned long long* __restrict__ n_unmatched, const DevFilterTaxa* flt, const LAY L) {
    constexpr bool FILTER = MODE != PARSE_PLAIN, COVER = HAS_COVER<LAY>;
    const uint64_t p = line_start[i];
    uint64_t e = line_start[i + 1] - 1;                 // the newline (or one past the end of a last line without one)
    if (e > p && text[e - 1] == '\r') --e;
    if (e <= p) { atomicOr(flags, FB_EMPTY_LINE); return; }
    const uint32_t n_cols = lay_n_cols(L), c_q = lay_col(L, ROLE_QUERY), c_a = lay_col(L, ROLE_ACC), c_tax = lay_col(L, ROLE_TAX),
                   c_pid = lay_col(L, ROLE_PID), c_aln = lay_col(L, ROLE_ALN), c_bs = lay_col(L, ROLE_BS);
    uint32_t c_e = 0xFFFFFFFFu;                         // (the e-value column, when its threshold is on)
    if constexpr (FILTER) if ((flt->f.mask & BLU_FILTER_MAX_E_VALUE) && lay_col(L, ROLE_E) < n_cols) c_e = lay_col(L, ROLE_E);
    uint32_t col = 0;
    uint64_t fstart = p;                                // start of the current field
    unsigned long long h = 1469598103934665603ull;
    NumState num;
    num.reset();
    bool cut = false;                                   // behind the first ';' of a `staxids` field
    RowValues v;
    uint32_t fb = 0;
    auto cover_col = [&](uint32_t c) {                  // which cover field column c holds, or -1
        if constexpr (COVER) {
#pragma unroll
            for (int k = 0; k < COVER_FIELDS; ++k) if (c == L.cov.col[k]) return k;
        }
        return -1;
    };
    auto end_field = [&](uint64_t fend) {
        const uint64_t len = fend - fstart;
        if (col == c_q) { o.qh[i] = hash_finish(h, (uint32_t)len); o.qpos[i] = fstart | (len << 44); if (len >= (1u << 20)) fb |= FB_COLUMNS; }
        else if (col == c_a) { o.ah[i] = hash_finish(h, (uint32_t)len); o.apos[i] = fstart | (len << 44); if (len >= (1u << 20)) fb |= FB_COLUMNS; }
        // (subject_taxid and align_length are Int64 columns, mod.rs:226-244: a fraction or an exponent is left to the CPU
        // parser, which refuses the file as the reference would)
        else if (col == c_tax) { if (!num.value(&v.tax) || num.seen_dot || num.seen_exp) fb |= FB_NUMBER; }
        else if (col == c_pid) { if (!num.value(&v.pid)) fb |= FB_NUMBER; }
        else if (col == c_aln) { if (!num.value(&v.aln) || num.seen_dot || num.seen_exp) fb |= FB_NUMBER; }
        else if (col == c_bs) { if (!num.value(&v.bs)) fb |= FB_NUMBER; }
        else if (FILTER && col == c_e) { if (!num.plain()) fb |= FB_NUMBER; v.e_mant = num.mant; v.e_exp = num.exponent(); v.e_neg = num.neg; }
        else if (COVER) {
            const int k = cover_col(col);
            if (k >= 0) { double x = 0; fb |= cover_field(num, &x); v.cov[0] = k == 0 ? x : v.cov[0]; v.cov[1] = k == 1 ? x : v.cov[1]; v.cov[2] = k == 2 ? x : v.cov[2]; }
        }
        ++col;
        fstart = fend + 1;
        h = 1469598103934665603ull;
        num.reset();
        cut = false;
    };
    // aligned 16-byte loads; bytes outside [p, e) are skipped
    for (uint64_t a = p & ~15ull; a < e && col < n_cols; a += 16) {
        const uint4 w16 = *reinterpret_cast<const uint4*>(text + a);
        const uint32_t w[4] = {w16.x, w16.y, w16.z, w16.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint64_t q = a + k;
            if (q < p || q >= e || col >= n_cols) continue;
            const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xFF;
            if (c == '\t') { end_field(q); continue; }
            if (col == c_q || col == c_a) { h = hash_step(h, c); if (c == '"') fb |= FB_QUOTE; }
            else if (col == c_tax || col == c_pid || col == c_aln || col == c_bs || (FILTER && col == c_e) || (COVER && cover_col(col) >= 0)) {
                if (lay_tax_list(L) && col == c_tax && c == ';') cut = true;
                if (!cut) num.feed(c, q == fstart);     // (one feed for every numeric column: the 16 unrolled copies of this body are the form's size)
            }
        }
    }
    if (col < n_cols) end_field(e);                     // the last field ends with the line
    if (col < n_cols) fb |= FB_COLUMNS;
    if (fb) { atomicOr(flags, fb); return; }
    finish_row<MODE>(L, i, v, taxmap, o, flags, n_unmatched, flt);
}

// ---- the staged form's field providers.  After the stage a thread finds the tabs of its line and leaves in LDS what tells it
// where a role's field begins and ends; this is the one part that differs between the reference's columns and a layout, and
// everything behind it is written against begin(role) / end(role).  A thread reads back only what it wrote: no barrier.
constexpr uint32_t STAGE_BYTES = 32768;
constexpr int PARSE_THREADS = 256;

// bit 7 of every byte of the staged word at a (a multiple of 4) that is a tab inside [p, e): four bytes per compare, the exact
// zero-byte test on word ^ 0x09090909, bytes outside the line masked off
__device__ __forceinline__ uint32_t tab_mask(const uint32_t* sw, uint32_t a, uint32_t p, uint32_t e) {
    const uint32_t x = sw[a >> 2] ^ 0x09090909u;
    uint32_t m = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
    if (a < p) m &= 0xFFFFFFFFu << (8 * (p - a));
    if (e - a < 4) m &= (1u << (8 * (e - a))) - 1u;
    return m;
}

// The reference's columns: the positions of the line's first 13 tabs, [column][thread], 13 x 256 x 2 = 6.5 KB; a role's bounds
// are the tabs around its constant column.  It keeps a scan of its own because this one has no test inside its loop — every tab
// is stored where its count says — while the layout's asks `wanted` and seven columns at every tab: 11 ms against 12 ms on the
// same 100 M lines (profiles/outfmt_bench.json), and this is the kernel of every call without --blast-outfmt.
struct RefFields {
    static constexpr int LDS_WORDS = 13 * PARSE_THREADS;
    const uint16_t* mine;
    uint32_t p, e, n_tabs;
    __device__ __forceinline__ bool scan(const RefLayout&, const uint32_t* sw, uint32_t p_, uint32_t e_, uint16_t* lds) {
        mine = lds; p = p_; e = e_; n_tabs = 0;
        for (uint32_t a = p & ~3u; a < e && n_tabs < 13; a += 4) {
            uint32_t m = tab_mask(sw, a, p, e);
            while (m && n_tabs < 13) {
                lds[n_tabs * PARSE_THREADS] = (uint16_t)(a + ((uint32_t)__builtin_ctz(m) >> 3));
                ++n_tabs;
                m &= m - 1;
            }
        }
        return n_tabs >= 12;                                         // (false: fewer than 13 columns)
    }
    __device__ __forceinline__ uint32_t tab(uint32_t c) const { return (uint32_t)mine[c * PARSE_THREADS]; }
    __device__ __forceinline__ uint32_t begin(int r) const { const uint32_t c = lay_col(RefLayout{}, r); return c == 0 ? p : tab(c - 1) + 1; }
    // (the bit score ends at the 13th tab, or with the line when there is none)
    __device__ __forceinline__ uint32_t end(int r) const { const uint32_t c = lay_col(RefLayout{}, r); return c == 12 && n_tabs < 13 ? e : tab(c); }
};

// A layout: the scan walks the line's tabs up to the end of column n_cols - 1 — the field count has to be checked — but acts only
// at a tab `wanted` names, and leaves in LDS only the bounds of the role fields, begin and end per role and thread: 2 x 7 x 256 x
// 2 = 7 KB beside the 32 KB stage whatever the column count (one word per column would be 64 x 256 x 2 = 32 KB more).
// Of a cover field it keeps only the begin, and in a register, not in LDS: the three 16-bit positions share one
// 64-bit word; the field ends at the next tab or with the line, which the short walk over its digits finds for itself.  LDS
// stays at 39 936 B with or without a cover.
template <class LAY>
struct LayoutFields {
    static constexpr int LDS_WORDS = 2 * N_ROLES * PARSE_THREADS;    // [role][begin, end][thread]
    uint16_t* mine;
    unsigned long long cov_at;                                       // begin of cover field k: bits 16 k .. 16 k + 15
    __device__ __forceinline__ void set_begin(int r, uint32_t at) { mine[(2 * r) * PARSE_THREADS] = (uint16_t)at; }
    __device__ __forceinline__ void set_end(int r, uint32_t at) { mine[(2 * r + 1) * PARSE_THREADS] = (uint16_t)at; }
    __device__ __forceinline__ uint32_t begin(int r) const { return (uint32_t)mine[(2 * r) * PARSE_THREADS]; }
    __device__ __forceinline__ uint32_t end(int r) const { return (uint32_t)mine[(2 * r + 1) * PARSE_THREADS]; }
    __device__ __forceinline__ uint32_t cover_begin(int k) const { return (uint32_t)(cov_at >> (16 * k)) & 0xFFFFu; }
    // tab t ends column t and column t + 1 begins behind it
    __device__ __forceinline__ bool scan(const LAY& L, const uint32_t* sw, uint32_t p, uint32_t e, uint16_t* lds) {
        mine = lds; cov_at = 0;
        const uint32_t n_cols = L.n_cols;
#pragma unroll
        for (int r = 0; r < N_ROLES; ++r) if (L.col[r] == 0) set_begin(r, p);
        if constexpr (HAS_COVER<LAY>) {
#pragma unroll
            for (int k = 0; k < COVER_FIELDS; ++k) if (L.cov.col[k] == 0) cov_at |= (unsigned long long)p << (16 * k);
        }
        uint32_t n_tabs = 0;
        for (uint32_t a = p & ~3u; a < e && n_tabs < n_cols; a += 4) {
            uint32_t m = tab_mask(sw, a, p, e);
            while (m && n_tabs < n_cols) {
                if ((L.wanted >> n_tabs) & 1ull) {
                    const uint32_t at = a + ((uint32_t)__builtin_ctz(m) >> 3);
#pragma unroll
                    for (int r = 0; r < N_ROLES; ++r) {
                        if (L.col[r] == n_tabs) set_end(r, at);
                        if (L.col[r] == n_tabs + 1) set_begin(r, at + 1);
                    }
                    if constexpr (HAS_COVER<LAY>) {
#pragma unroll
                        for (int k = 0; k < COVER_FIELDS; ++k) if (L.cov.col[k] == n_tabs + 1) cov_at |= (unsigned long long)(at + 1) << (16 * k);
                    }
                }
                ++n_tabs;
                m &= m - 1;
            }
        }
        if (n_tabs + 1 < n_cols) return false;                       // fewer columns than the layout names
        if (n_tabs + 1 == n_cols) {                                  // the layout's last column ends with the line
#pragma unroll
            for (int r = 0; r < N_ROLES; ++r) if (L.col[r] == n_cols - 1) set_end(r, e);
        }
        return true;
    }
};

// The staged form, the parse kernel proper: a block takes 256 consecutive lines, whose text is one contiguous span of the file
// (17 KB for BLAST's usual 67-byte lines).  The span is staged in LDS with coalesced 16-byte loads; every lane then (1) finds the
// tabs of its line with word-wide compares (the field provider), (2) walks the fields the engine reads ONE FIELD AT A TIME, so
// that the 64 lanes of a wave are in the same field and the same branch of the same small loop: the general form spends its
// time in divergence (a wave has lanes in every column at once and runs the end-of-field code of all of them at nearly every
// byte) and in instruction fetch (its 16-byte unrolled body does not fit the instruction cache).  Same grammar, same hashes,
// same flags as the general form; a block whose span exceeds the stage (lines of 128 bytes and more on average) is parsed by it.
template <int MODE, class LAY>
__device__ __forceinline__ void parse_rows_body(const unsigned char* __restrict__ text, const uint64_t* __restrict__ line_start, uint32_t n_rows,
                                                const DevTaxidMap& taxmap, const RowOut& o, uint32_t* __restrict__ flags,
                                                unsigned long long* __restrict__ n_unmatched, const DevFilterTaxa* flt, const LAY& L) {
    using Fields = std::conditional_t<std::is_same<LAY, RefLayout>::value, RefFields, LayoutFields<LAY>>;
    __shared__ uint4 stage16[STAGE_BYTES / 16];
    __shared__ uint16_t field_at[Fields::LDS_WORDS];
    const uint32_t r0 = blockIdx.x * PARSE_THREADS, r1 = min(r0 + (uint32_t)PARSE_THREADS, n_rows), i = r0 + threadIdx.x;
    // (the four line starts travel together: two round trips to memory per block — these, then the text — and no more)
    const uint64_t ls0 = line_start[r0], s1 = line_start[r1];       // (line_start[n_rows] = one past the last newline, or size + 1)
    const uint64_t my_p = line_start[min(i, r1 - 1)], my_e = line_start[min(i, r1 - 1) + 1];
    const uint64_t s0 = ls0 & ~15ull;
    if (s1 - s0 > STAGE_BYTES) {                                     // uniform over the block
        if (i < r1) parse_row_general<MODE>(text, line_start, i, taxmap, o, flags, n_unmatched, flt, L);
        return;
    }
    {
        const uint32_t n16 = (uint32_t)((s1 - s0 + 15) >> 4);        // (reads at most 15 bytes past s1 <= size + 1: inside the 64 bytes of padding)
        const uint4* src = reinterpret_cast<const uint4*>(text + s0);
        constexpr int PER_THREAD = STAGE_BYTES / 16 / PARSE_THREADS; // all of a thread's loads are in flight before the first is stored
        uint4 w[PER_THREAD];
#pragma unroll
        for (int j = 0; j < PER_THREAD; ++j) { const uint32_t k = threadIdx.x + (uint32_t)j * PARSE_THREADS; w[j] = src[min(k, n16 - 1)]; }
#pragma unroll
        for (int j = 0; j < PER_THREAD; ++j) { const uint32_t k = threadIdx.x + (uint32_t)j * PARSE_THREADS; if (k < n16) stage16[k] = w[j]; }
    }
    __syncthreads();
    if (i >= r1) return;
    const unsigned char* sb = reinterpret_cast<const unsigned char*>(stage16);
    const uint32_t p = (uint32_t)(my_p - s0);
    uint32_t e = (uint32_t)(my_e - 1 - s0);                          // the newline (or one past the end of a last line without one)
    if (e > p && sb[e - 1] == '\r') --e;
    if (e <= p) { atomicOr(flags, FB_EMPTY_LINE); return; }
    // ---- (1) the tabs
    Fields f;
    if (!f.scan(L, reinterpret_cast<const uint32_t*>(stage16), p, e, field_at + threadIdx.x)) { atomicOr(flags, FB_COLUMNS); return; }
    uint32_t fb = 0;
    // ---- (2) query and accession: FNV-1a over the field, as in the general form
    auto hash_field = [&](uint32_t s, uint32_t t) {
        unsigned long long h = 1469598103934665603ull;
        for (uint32_t q = s; q < t; ++q) { const uint32_t c = sb[q]; h = hash_step(h, c); if (c == '"') fb |= FB_QUOTE; }
        return hash_finish(h, t - s);
    };
    const uint32_t q0 = f.begin(ROLE_QUERY), q1 = f.end(ROLE_QUERY), a0 = f.begin(ROLE_ACC), a1 = f.end(ROLE_ACC);
    const unsigned long long qh = hash_field(q0, q1), ah = hash_field(a0, a1);
    // ---- the four numbers; list: the field is `staxids`, the number ends at its first ';'
    auto number = [&](int r, bool integer, bool list, double* x) {
        NumState num;
        num.reset();
        const uint32_t s = f.begin(r), t = f.end(r);
        for (uint32_t q = s; q < t; ++q) { const uint32_t c = sb[q]; if (list && c == ';') break; num.feed(c, q == s); }
        if (!num.value(x) || (integer && (num.seen_dot || num.seen_exp))) fb |= FB_NUMBER;
    };
    RowValues v;
    number(ROLE_TAX, true, lay_tax_list(L), &v.tax);                 // (subject_taxid and align_length are Int64 columns, mod.rs:226-244)
    number(ROLE_PID, false, false, &v.pid);
    number(ROLE_ALN, true, false, &v.aln);
    number(ROLE_BS, false, false, &v.bs);
    if constexpr (MODE != PARSE_PLAIN) {
        if ((flt->f.mask & BLU_FILTER_MAX_E_VALUE) && lay_col(L, ROLE_E) < lay_n_cols(L)) {   // the e-value column, read only under its threshold
            NumState num;
            num.reset();
            const uint32_t s = f.begin(ROLE_E), t = f.end(ROLE_E);
            for (uint32_t q = s; q < t; ++q) num.feed(sb[q], q == s);
            if (!num.plain()) fb |= FB_NUMBER;
            v.e_mant = num.mant; v.e_exp = num.exponent(); v.e_neg = num.neg;
        }
    }
    if constexpr (HAS_COVER<LAY>) {                                  // the cover fields: from their begin to the next tab or the line's end
#pragma unroll
        for (int k = 0; k < COVER_FIELDS; ++k) {
            if (k >= (int)L.cov.n_fields) continue;
            NumState num;
            num.reset();
            const uint32_t s = f.cover_begin(k);
            for (uint32_t q = s; q < e; ++q) { const uint32_t c = sb[q]; if (c == '\t') break; num.feed(c, q == s); }
            fb |= cover_field(num, &v.cov[k]);
        }
    }
    if (fb) { atomicOr(flags, fb); return; }
    if (!finish_row<MODE>(L, i, v, taxmap, o, flags, n_unmatched, flt)) return;
    o.qh[i] = qh; o.qpos[i] = (s0 + q0) | ((unsigned long long)(q1 - q0) << 44);
    o.ah[i] = ah; o.apos[i] = (s0 + a0) | ((unsigned long long)(a1 - a0) << 44);
}

// The eight builds.  Every one takes the same arguments, then its layout if it has one: n_unmatched is read by the unfiltered
// builds only, and flt (in device memory: read with scalar loads) is null in them.
#define PARSE_ARGS const unsigned char* __restrict__ text, const uint64_t* __restrict__ line_start, uint32_t n_rows, DevTaxidMap taxmap, RowOut o, \
                   uint32_t* __restrict__ flags, unsigned long long* __restrict__ n_unmatched, const DevFilterTaxa* __restrict__ flt
__global__ __launch_bounds__(PARSE_THREADS) void parse_rows(PARSE_ARGS) {
    parse_rows_body<PARSE_PLAIN>(text, line_start, n_rows, taxmap, o, flags, n_unmatched, flt, RefLayout{});
}
__global__ __launch_bounds__(PARSE_THREADS, 4) void parse_rows_filtered(PARSE_ARGS) {
    parse_rows_body<PARSE_FILTER>(text, line_start, n_rows, taxmap, o, flags, n_unmatched, flt, RefLayout{});
}
__global__ __launch_bounds__(PARSE_THREADS, 4) void parse_rows_taxa(PARSE_ARGS) {
    parse_rows_body<PARSE_TAXA>(text, line_start, n_rows, taxmap, o, flags, n_unmatched, flt, RefLayout{});
}
__global__ __launch_bounds__(PARSE_THREADS, 4) void parse_rows_layout(PARSE_ARGS, DevLayout lay) {
    parse_rows_body<PARSE_PLAIN>(text, line_start, n_rows, taxmap, o, flags, n_unmatched, flt, lay);
}
__global__ __launch_bounds__(PARSE_THREADS, 4) void parse_rows_layout_filtered(PARSE_ARGS, DevLayout lay) {
    parse_rows_body<PARSE_FILTER>(text, line_start, n_rows, taxmap, o, flags, n_unmatched, flt, lay);
}
__global__ __launch_bounds__(PARSE_THREADS, 4) void parse_rows_layout_taxa(PARSE_ARGS, DevLayout lay) {
    parse_rows_body<PARSE_TAXA>(text, line_start, n_rows, taxmap, o, flags, n_unmatched, flt, lay);
}
__global__ __launch_bounds__(PARSE_THREADS, 4) void parse_rows_layout_qcov(PARSE_ARGS, DevLayoutCover lay) {
    parse_rows_body<PARSE_FILTER>(text, line_start, n_rows, taxmap, o, flags, n_unmatched, flt, lay);
}
__global__ __launch_bounds__(PARSE_THREADS, 4) void parse_rows_layout_qcov_taxa(PARSE_ARGS, DevLayoutCover lay) {
    parse_rows_body<PARSE_TAXA>(text, line_start, n_rows, taxmap, o, flags, n_unmatched, flt, lay);
}
#undef PARSE_ARGS

// ---- 2b. hit filter: the e-values left to the host, and the stable compaction of the parsed rows ---------------------------
// rows whose keep word is KEEP_ASK_HOST, in any order, each with the place of its e-value field (field offset | length << 44);
// e_col: the 0-based column that holds it — 11 in the reference's columns, the layout's otherwise
__global__ void list_undecided(const uint32_t* __restrict__ keep, uint32_t n, const unsigned char* __restrict__ text,
                               const uint64_t* __restrict__ line_start, uint32_t cap, uint32_t* __restrict__ rows,
                               unsigned long long* __restrict__ pos, uint32_t* __restrict__ cursor, uint32_t e_col) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || keep[i] != KEEP_ASK_HOST) return;
    const uint64_t p = line_start[i];
    uint64_t e = line_start[i + 1] - 1;
    if (e > p && text[e - 1] == '\r') --e;
    uint64_t q = p;
    for (uint32_t tabs = 0; q < e && tabs < e_col; ++q) if (text[q] == '\t') ++tabs;
    const uint64_t s = q;
    while (q < e && text[q] != '\t') ++q;
    const uint32_t at = atomicAdd(cursor, 1u);
    if (at < cap) { rows[at] = i; pos[at] = s | ((q - s) << 44); }
}
__global__ void apply_decisions(const uint32_t* __restrict__ rows, const uint32_t* __restrict__ decision, uint32_t n, uint32_t n_rows,
                                uint32_t* __restrict__ keep) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n && rows[k] < n_rows) keep[rows[k]] = decision[k] ? KEEP_YES : KEEP_NO;
}
__global__ __launch_bounds__(1024) void count_unmatched(const uint32_t* __restrict__ tax, uint32_t n, unsigned long long* __restrict__ count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    __shared__ uint32_t wave_sums[1024 / 64];
    const uint32_t total = block_sum<1024>(i < n && tax[i] == BLU_UNMATCHED_TAXID, wave_sums);
    if (threadIdx.x == 0 && total) atomicAdd(count, (unsigned long long)total);
}

// ---- 3. dictionaries ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void count_run_heads(const unsigned long long* __restrict__ h, uint32_t n, unsigned long long* __restrict__ count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t head = i < n && (i == 0 || h[i] != h[i - 1]);
    __shared__ uint32_t wave_sums[1024 / 64];
    const uint32_t total = block_sum<1024>(head, wave_sums);
    if (threadIdx.x == 0 && total) atomicAdd(count, (unsigned long long)total);   // one atomic per 1024 rows
}

__global__ void dict_init(Slot* __restrict__ tab, uint64_t n_slots) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < n_slots) { Slot e; memset(&e, 0, sizeof e); e.first_row = 0xFFFFFFFFu; tab[s] = e; }
}

// insert = CAS on the hash, atomicMin on the row; only_heads: rows whose hash equals the previous row's are skipped
__global__ void dict_insert(const unsigned long long* __restrict__ h, uint32_t n, Slot* __restrict__ tab, uint64_t mask, bool only_heads,
                            uint32_t* __restrict__ n_keys, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool active = i < n;
    unsigned long long key = 0;
    if (active) {
        key = h[i];
        if (only_heads && i > 0 && h[i - 1] == key) active = false;
    }
    bool claimed = false, full = false;
    if (active) {
        uint64_t s = key & mask;
        full = true;
        for (uint32_t probes = 0; probes < 8192; ++probes) {
            unsigned long long cur = __hip_atomic_load(&tab[s].hash, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == 0) {
                cur = atomicCAS(&tab[s].hash, 0ull, key);
                if (cur == 0) { claimed = true; cur = key; }
            }
            if (cur == key) {
                // (first_row only ever decreases: a value read here is an upper bound of the current one, so a row that is not
                // below it has nothing to store — 100 M rows, 300 k accessions: all but a few of the atomics go)
                if (__hip_atomic_load(&tab[s].first_row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > i) atomicMin(&tab[s].first_row, i);
                full = false;
                break;
            }
            s = (s + 1) & mask;
        }
    }
    (void)claimed; (void)n_keys;   // (the keys are counted by dict_count afterwards: one atomic per new key on one word — 2 M
                                   // of them for a query dictionary — took 18 of this kernel's 19.6 ms)
    if (full) atomicOr(flags, FB_TABLE_FULL);
}

// number of occupied slots -> *n_keys (zeroed by the caller): a block reduction, one atomic per block
__global__ __launch_bounds__(1024) void dict_count(const Slot* __restrict__ tab, uint64_t n_slots, uint32_t* __restrict__ n_keys) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t used = s < n_slots && tab[s].hash != 0ull;
    __shared__ uint32_t wave_sums[1024 / 64];
    const uint32_t c = block_sum<1024>(used, wave_sums);
    if (threadIdx.x == 0 && c) atomicAdd(n_keys, c);
}

// occupied slots: key length and first bytes from the text of their first row; list of (first_row, slot)
__global__ void dict_finalize(Slot* __restrict__ tab, uint64_t n_slots, const unsigned char* __restrict__ text,
                              const unsigned long long* __restrict__ pos, uint32_t* __restrict__ list_row, uint32_t* __restrict__ list_slot,
                              uint32_t* __restrict__ cursor) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots || tab[s].hash == 0) return;
    const unsigned long long fp = pos[tab[s].first_row];
    const uint64_t off = fp & ((1ull << 44) - 1);
    const uint32_t len = (uint32_t)(fp >> 44);
    tab[s].len = len;
    for (uint32_t k = 0; k < 12; ++k) tab[s].head[k] = k < len ? text[off + k] : 0;
    const uint32_t at = atomicAdd(cursor, 1u);
    list_row[at] = tab[s].first_row;
    list_slot[at] = (uint32_t)s;
}

// queries are numbered in the order of their first rows (mod.rs:192-208) without sorting anything: the first rows are marked in a
// row-indexed array, an exclusive prefix sum over it gives every marked row the number of marked rows before it — the id
__global__ void mark_first_rows(const uint32_t* __restrict__ list_row, uint32_t n, uint32_t* __restrict__ mark) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) mark[list_row[k]] = 1u;
}
__global__ void number_queries(Slot* __restrict__ tab, const uint32_t* __restrict__ list_row, const uint32_t* __restrict__ list_slot, uint32_t n,
                               const uint32_t* __restrict__ rank_of_row, const unsigned long long* __restrict__ pos,
                               unsigned long long* __restrict__ pos_by_id) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t row = list_row[k], id = rank_of_row[row];
    tab[list_slot[k]].id = id;
    pos_by_id[id] = pos[row];          // the query's name: the text of its first row
}

__global__ void dict_assign_ids(Slot* __restrict__ tab, const uint32_t* __restrict__ slot_of_rank, const uint32_t* __restrict__ id_of_rank, uint32_t n) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) tab[slot_of_rank[r]].id = id_of_rank ? id_of_rank[r] : r;
}

// every row: find its slot, compare its own text with the slot's key (exact ids), write the id
__global__ void dict_lookup(const unsigned long long* __restrict__ h, const unsigned long long* __restrict__ pos, uint32_t n,
                            const Slot* __restrict__ tab, uint64_t mask, const unsigned char* __restrict__ text,
                            const unsigned long long* __restrict__ pos_all, uint32_t* __restrict__ id_out, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const unsigned long long key = h[i];
    uint64_t s = key & mask;
    for (;;) {                                           // present: it was inserted (or merged into a run) above
        const unsigned long long cur = tab[s].hash;
        if (cur == key) break;
        if (cur == 0) { atomicOr(flags, FB_TABLE_FULL); id_out[i] = 0; return; }
        s = (s + 1) & mask;
    }
    const Slot sl = tab[s];
    const uint64_t off = pos[i] & ((1ull << 44) - 1);
    const uint32_t len = (uint32_t)(pos[i] >> 44);
    bool same = len == sl.len;
    {   // the first min(len, 12) bytes against the slot's: ONE unaligned 12-byte load (the text has 64 bytes of padding behind
        // it; the slot's bytes beyond its length are zero) instead of twelve byte loads with 64 lines each
        uint32_t w[3], hw[3];
        __builtin_memcpy(w, text + off, 12);
        __builtin_memcpy(hw, sl.head, 12);
        const uint32_t n = len < 12u ? len : 12u;
#pragma unroll
        for (uint32_t j = 0; j < 3; ++j) {
            const uint32_t nb = n > 4 * j ? n - 4 * j : 0u;
            const uint32_t m = nb >= 4 ? 0xFFFFFFFFu : (1u << (8 * nb)) - 1u;
            same = same && ((w[j] ^ hw[j]) & m) == 0;
        }
    }
    if (same && len > 12 && sl.first_row != i) {
        const uint64_t roff = pos_all[sl.first_row] & ((1ull << 44) - 1);
        for (uint32_t k = 12; same && k < len; ++k) same = text[off + k] == text[roff + k];
    }
    if (!same) atomicOr(flags, FB_HASH_COLLISION);
    id_out[i] = sl.id;
}

__global__ void gather_pos(const unsigned long long* __restrict__ pos, const uint32_t* __restrict__ rows, uint32_t n, unsigned long long* __restrict__ out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n) out[r] = pos[rows[r]];
}

// first 16 bytes of each listed field as two big-endian words: integer compares order them like memcmp
__global__ void gather_key16(const unsigned long long* __restrict__ pos, uint32_t n, const unsigned char* __restrict__ text,
                             unsigned long long* __restrict__ k0, unsigned long long* __restrict__ k1) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    const uint64_t off = pos[r] & ((1ull << 44) - 1);
    const uint32_t len = (uint32_t)(pos[r] >> 44);
    unsigned long long a = 0, b = 0;
    for (uint32_t k = 0; k < 8; ++k) a = (a << 8) | (k < len ? text[off + k] : 0);
    for (uint32_t k = 8; k < 16; ++k) b = (b << 8) | (k < len ? text[off + k] : 0);
    k0[r] = a; k1[r] = b;
}

// ---- 5. grouping ---------------------------------------------------------------------------------------------------
// the distinct strings themselves, packed back to back: lengths -> (exclusive scan) -> bytes
__global__ void pos_lengths(const unsigned long long* __restrict__ pos, uint32_t n, unsigned long long* __restrict__ len) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= n) len[i] = i < n ? pos[i] >> 44 : 0ull;
}
__global__ void gather_bytes(const unsigned long long* __restrict__ pos, uint32_t n, const unsigned char* __restrict__ text,
                             const unsigned long long* __restrict__ off, unsigned char* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t src = pos[i] & ((1ull << 44) - 1);
    const uint32_t len = (uint32_t)(pos[i] >> 44);
    unsigned char* d = out + off[i];
    for (uint32_t k = 0; k < len; ++k) d[k] = text[src + k];
}
__global__ void check_grouped(const uint32_t* __restrict__ qid, uint32_t n, uint32_t* __restrict__ unsorted) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > 0 && i < n && qid[i] < qid[i - 1]) *unsorted = 1u;
}
__global__ void iota_u32(uint32_t* __restrict__ v, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = i;
}
// segment offsets from the query ids in grouped (non-decreasing) order: the first row of every id, and the row count
// behind the last one.  Every id 0 .. n_queries - 1 occurs (ids are handed out to keys that are in the table).  (A
// histogram with one atomic per row and a scan did the same in 5.7 ms per 100 M rows; this reads the ids once.)
__global__ void segment_starts(const uint32_t* __restrict__ qid_sorted, uint32_t n, uint32_t n_queries, unsigned long long* __restrict__ seg_off) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t q = qid_sorted[i];
    if (i == 0 || qid_sorted[i - 1] != q) seg_off[q] = i;
    if (i == n - 1) seg_off[n_queries] = n;
}
struct Cols { const int32_t* bs; const int32_t* aln; const uint32_t* tax; const uint32_t* arank; const double* pid; };
struct ColsOut { int32_t* bs; int32_t* aln; uint32_t* tax; uint32_t* arank; double* pid; };
__global__ void gather_cols(Cols in, ColsOut out, const uint32_t* __restrict__ perm, uint32_t n) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = perm ? perm[j] : j;
    out.bs[j] = in.bs[i]; out.aln[j] = in.aln[i]; out.tax[j] = in.tax[i]; out.arank[j] = in.arank[i]; out.pid[j] = in.pid[i];
}

const char* fallback_text(uint32_t f) {
    if (f & FB_EMPTY_LINE) return "an empty line";
    if (f & FB_COLUMNS) return "a line with fewer columns than the 13 of outfmt-6 or than the layout names (or an oversized field)";
    if (f & FB_QUOTE) return "a quoted query / accession field";
    if (f & FB_NUMBER) return "a numeric field outside the decimal fast path";
    if (f & FB_RANGE) return "a number outside the engine's 32-bit columns";
    if (f & FB_HASH_COLLISION) return "two strings with one 64-bit hash";
    if (f & FB_TABLE_FULL) return "a dictionary table that filled up";
    return "unknown";
}

uint64_t pow2_at_least(uint64_t x) { uint64_t p = 1024; while (p < x) p <<= 1; return p; }

// stage trace of the GPU ingest (BLU_INGEST_TRACE=1): one stderr line per lap, the device drained first
struct IngestTrace {
    const bool on = getenv("BLU_INGEST_TRACE") != nullptr;
    double tp = now_s();
    void operator()(const char* what) {
        if (!on) return;
        (void)hipDeviceSynchronize();
        const double t = now_s();
        fprintf(stderr, "[ingest-gpu] %-26s %.3f s\n", what, t - tp);
        tp = t;
    }
};
}  // namespace

// (defined in consensus_kernel.hip; named here only so that the warm-up can ask for its attributes, which makes the runtime load
// the code object of that translation unit — the two dozen builds of the consensus kernels — ahead of the engine stage)
__global__ void blu_classify_tasks(const uint64_t* __restrict__ seg_off, uint64_t n_queries, uint64_t n_hits, uint64_t, uint64_t, uint32_t, uint32_t*, uint32_t*);

void warm_up_device(int device) {
    void* p = nullptr;
    if (hipSetDevice(device) == hipSuccess && hipMalloc(&p, 256) == hipSuccess) {
        (void)hipMemsetAsync(p, 0, 256, nullptr);
        // one kernel of this library: its code object (5 MB, two dozen builds of the consensus kernels) is loaded onto the
        // device by the first launch — 8-10 ms that otherwise sit in front of the line index
        hipLaunchKernelGGL(iota_u32, dim3(1), dim3(64), 0, nullptr, (uint32_t*)p, 64u);
        hipFuncAttributes attr;
        (void)hipFuncGetAttributes(&attr, (const void*)blu_classify_tasks);
        // the two other translation units the default path runs kernels of: the line index and the engine's packing
        load_dev_prims();
        load_engine_dev();
        (void)hipStreamSynchronize(nullptr);
        (void)hipFree(p);
    }
    (void)hipGetLastError();
}

namespace {

// the thresholds as the kernels read them; the e-value's decimal magnitude tests and bracket (e_value_verdict) from max_e
DevFilter device_filter(const blu_hit_filter& f) {
    DevFilter d{};
    d.mask = f.mask & 15u;
    d.min_pid = f.min_perc_identity; d.min_bs = f.min_bit_score; d.max_e = f.max_e_value; d.min_aln = f.min_align_length;
    const double E = f.max_e_value;
    constexpr int NEVER = -(1 << 30), ALWAYS = 1 << 30;
    if (!(E >= 0.0)) { d.k_keep = NEVER; d.k_drop = NEVER; }                  // negative or NaN: no value above zero passes
    else if (E == 0.0) { d.k_keep = -325; d.k_drop = -322; }                  // below 10^-325 strtod gives 0; from 10^-322 it does not
    else if (std::isinf(E)) { d.k_keep = ALWAYS; d.k_drop = ALWAYS; }
    else {
        // t = floor(log10 E) give or take one (the library's rounding at a power of ten): value < 10^(t - 2) <= E / 10 is kept,
        // value >= 10^(t + 3) >= 10 E is dropped
        const int t = (int)std::floor(std::log10(E));
        d.k_keep = t - 2; d.k_drop = t + 3;
        d.e_band = E >= 1e-280 && E <= 1e280;
        d.e_lo = E * (1.0 - 0x1p-46); d.e_hi = E * (1.0 + 0x1p-46);
    }
    return d;
}

#define STEP(x) do { if (const int rc_ = (x)) return rc_; } while (0)

// One call of the GPU ingest on the device: the inputs, the arena the caller frees, and what the steps of run() hand from one to
// the next.  Any other device buffer is a step's own: allocated in it, and freed in it or left to the arena.  A step that fails
// returns at once (a HIP error through HIP_CHECK, a file for the CPU parser through fallback()).
struct GpuIngest {
    const int fd;
    const size_t size;
    const TaxidMap& row_of;
    const int device;
    const bool host_columns;
    HitTable& ht;
    DeviceArena& mem;
    HipPolicy& pol;
    IngestTrace& lap;
    const blu_hit_filter* const flt;   // (null: none)
    TaxonCodes* const taxa;            // (null: none)
    const blu_table_layout* const lay; // (null: the reference's columns; else checked, and not the reference's own: DESIGN.md §23)
    const blu_query_cover* const cov;  // (null: none; else checked against lay, which is then not null: DESIGN.md §24)

    unsigned char* d_text = nullptr;   // the padded text: upload_and_index -> accession_dictionary_finish, which frees it
    uint64_t* d_line = nullptr;        // line starts: upload_and_index -> parse, drop_filtered_rows (which frees them)
    uint32_t n_rows = 0;               // lines; from drop_filtered_rows on, the kept ones
    // {flags, -, -, -, counter, -, -, -, big counters}: the fall-back bits, one 32-bit count, [0] unmatched rows [1] run heads;
    // under a filter the parse's counts follow (n_back): upload_and_index -> every step
    uint32_t *d_flags = nullptr, *d_counter = nullptr;
    unsigned long long* d_big = nullptr;
    void* d_tmp = nullptr;             // scan scratch, grown by need_tmp: every step
    size_t tmp_bytes = 0;
    // the eight parsed-row arrays: parse -> the dictionaries (hashes, field places) and group (the four values)
    unsigned long long *d_qh = nullptr, *d_ah = nullptr, *d_qpos = nullptr, *d_apos = nullptr;
    uint32_t* d_tax = nullptr;
    double* d_pid = nullptr;
    int32_t *d_aln = nullptr, *d_bs = nullptr;
    // a filtered parse -> drop_filtered_rows: the keep words, the filter and the row codes as the kernel read them, the counts
    uint32_t* d_keep = nullptr;
    DevFilterTaxa* d_filter = nullptr;                   // (null without a filter; .t unused without a taxon filter)
    uint16_t* d_code = nullptr;
    std::vector<unsigned long long> back;
    // accession_dictionary_begin -> accession_dictionary_finish: the table, its slots, the slot of every distinct accession
    Slot* d_atab = nullptr;
    uint64_t acap = 0;
    uint32_t* d_alist_slot = nullptr;
    uint32_t n_acc = 0;
    // the distinct query / accession strings packed back to back (bytes + n + 1 offsets) and the accessions' byte order:
    // the dictionaries -> hand_over's strings thread
    std::vector<char> q_bytes, a_bytes;
    std::vector<unsigned long long> q_off, a_off;
    std::vector<uint32_t> order;
    std::vector<unsigned long long> k0, k1;      // first 16 bytes of every distinct accession as two big-endian words
    std::thread acc_sort;                        // the host's sort of the distinct accessions, beside the query dictionary
    std::atomic<bool> acc_sort_failed{false};
    uint32_t n_queries = 0;
    uint32_t *d_qid = nullptr, *d_arank = nullptr;   // ids of the rows: the dictionaries -> group
    ColsOut grouped{};                               // group -> hand_over
    unsigned long long* d_seg = nullptr;

    ~GpuIngest() { if (acc_sort.joinable()) acc_sort.join(); }   // (whichever way run() is left)

    int run() {
        STEP(upload_and_index());             lap("line index");
        STEP(parse());
        STEP(drop_filtered_rows());           lap("parse");
        STEP(accession_dictionary_begin());
        STEP(query_dictionary());             lap("query dictionary");
        STEP(accession_dictionary_finish());  lap("accession dictionary");
        STEP(group());                        lap("grouping");
        return hand_over();
    }

    // ---- what the steps share
    int fallback(const char* reason) { *pol.why = reason; return BLU_INGEST_FALLBACK; }
    int fall_back_on(uint32_t h_flags) { return h_flags ? fallback(fallback_text(h_flags)) : BLU_OK; }
    // the flag word the kernels left: a set bit hands the file to the CPU parser
    int check_flags() {
        uint32_t h_flags = 0;
        HIP_CHECK(pol, hipMemcpy(&h_flags, d_flags, 4, hipMemcpyDeviceToHost));
        return fall_back_on(h_flags);
    }
    int zero_counter() { HIP_CHECK(pol, hipMemset(d_counter, 0, 4)); return BLU_OK; }
    size_t n_taxa_back() const { return taxa ? HIT_SPREAD + (size_t)taxa->n_exclude : 0; }
    size_t n_back() const { return 8 + HIT_SPREAD + 1 + n_taxa_back() + (cov ? HIT_SPREAD : 0); }   // (the cover's count comes last)
    hipError_t need_tmp(size_t bytes) {
        if (bytes <= tmp_bytes) return hipSuccess;
        if (d_tmp) mem.free(d_tmp);
        d_tmp = nullptr; tmp_bytes = 0;
        hipError_t e = mem.alloc(&d_tmp, bytes, "scan scratch");
        if (e == hipSuccess) tmp_bytes = bytes;
        return e;
    }
    // distinct strings at d_pos[0 .. n) of the device text -> host
    int download_strings(const unsigned long long* d_pos, uint32_t n, std::vector<char>& bytes, std::vector<unsigned long long>& off) {
        unsigned long long *d_len = nullptr, *d_off = nullptr;
        unsigned char* d_out = nullptr;
        off.assign((size_t)n + 1, 0);
        HIP_CHECK(pol, mem.alloc(&d_len, ((size_t)n + 1) * 8, "string offsets"));
        HIP_CHECK(pol, mem.alloc(&d_off, ((size_t)n + 1) * 8, "string offsets"));
        hipLaunchKernelGGL(pos_lengths, dim3((n + 256) / 256), dim3(256), 0, 0, d_pos, n, d_len);
        HIP_CHECK(pol, need_tmp(scan_tmp_bytes_u64((size_t)n + 1)));
        HIP_CHECK(pol, exclusive_scan_u64(d_len, d_off, (size_t)n + 1, d_tmp));
        HIP_CHECK(pol, hipMemcpy(off.data(), d_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
        bytes.resize(off[n]);
        HIP_CHECK(pol, mem.alloc(&d_out, off[n], "strings"));
        if (n) hipLaunchKernelGGL(gather_bytes, dim3((n + 255) / 256), dim3(256), 0, 0, d_pos, n, d_text, d_off, d_out);
        HIP_CHECK(pol, hipMemcpy(bytes.data(), d_out, off[n], hipMemcpyDeviceToHost));
        mem.free(d_len); mem.free(d_off); mem.free(d_out);
        return BLU_OK;
    }
    // an empty table of cap slots, the hashes h[0, n_rows) inserted (only_heads: dict_insert), the keys counted: their number
    // and the flag word come back
    int build_dictionary(Slot* tab, uint64_t cap, const unsigned long long* h, bool only_heads, bool clear_flags, uint32_t* n_keys,
                         uint32_t* h_flags) {
        hipLaunchKernelGGL(dict_init, grid(cap), dim3(256), 0, 0, tab, cap);   // empty slots, first_row = all ones for atomicMin
        STEP(zero_counter());
        if (clear_flags) HIP_CHECK(pol, hipMemset(d_flags, 0, 4));
        hipLaunchKernelGGL(dict_insert, grid(n_rows), dim3(256), 0, 0, h, n_rows, tab, cap - 1, only_heads, d_counter, d_flags);
        hipLaunchKernelGGL(dict_count, grid(cap, 1024), dim3(1024), 0, 0, tab, cap, d_counter);
        HIP_CHECK(pol, hipMemcpy(n_keys, d_counter, 4, hipMemcpyDeviceToHost));
        HIP_CHECK(pol, hipMemcpy(h_flags, d_flags, 4, hipMemcpyDeviceToHost));
        return BLU_OK;
    }

    // ---- upload + line index
    int upload_and_index() {
        lap("device start-up");
        bool open_tail = false;
        // (the device-buffer lap times the padding only: the readers' pieces end at `size`)
        STEP(upload_text(fd, size, device, "the table", mem, &d_text, &open_tail, [&] { lap("  upload: device buffer"); }));
        lap("upload text");
        const uint64_t n_tiles = line_tiles(size);
        uint32_t *d_tile = nullptr, *d_tile_base = nullptr;
        HIP_CHECK(pol, mem.alloc(&d_tile, (n_tiles + 1) * 4, "line index"));
        HIP_CHECK(pol, mem.alloc(&d_tile_base, (n_tiles + 1) * 4, "line index"));
        // under a hit filter the kept / undecided counts follow the big counters, and under a taxon filter the not-only counts
        // and one count per exclude element after them: all of it comes back in one copy
        const size_t flag_bytes = flt || taxa || cov ? n_back() * 8 : 64;
        HIP_CHECK(pol, mem.alloc(&d_flags, flag_bytes, "flags"));
        HIP_CHECK(pol, hipMemset(d_flags, 0, flag_bytes));
        d_counter = d_flags + 4;
        d_big = reinterpret_cast<unsigned long long*>(d_flags + 8);
        HIP_CHECK(pol, need_tmp(scan_tmp_bytes_u32((size_t)n_tiles + 1)));
        uint32_t n_newlines = 0;
        HIP_CHECK(pol, line_count(d_text, size, d_tile, d_tile_base, d_tmp, &n_newlines));
        const uint64_t rows64 = (uint64_t)n_newlines + (open_tail ? 1 : 0);
        if (rows64 >= 0x7FFFFFF0ull) return fallback("2^31 rows or more");
        n_rows = (uint32_t)rows64;
        if (n_rows == 0) return fallback("no rows");
        HIP_CHECK(pol, mem.alloc(&d_line, ((size_t)n_rows + 2) * 8, "line index"));
        HIP_CHECK(pol, line_write(d_text, size, d_tile_base, d_line, n_rows, open_tail));
        return BLU_OK;
    }

    // the layout as the kernels read it
    DevLayout device_layout() const {
        DevLayout d{};
        d.n_cols = lay->n_columns;
        d.col[ROLE_QUERY] = lay->query; d.col[ROLE_ACC] = lay->accession; d.col[ROLE_TAX] = lay->taxid; d.col[ROLE_PID] = lay->perc_identity;
        d.col[ROLE_ALN] = lay->align_length; d.col[ROLE_BS] = lay->bit_score; d.col[ROLE_E] = lay->e_value;
        d.tax_list = lay->taxid_is_list;
        for (int r = 0; r < N_ROLES; ++r) {
            if (d.col[r] >= d.n_cols) continue;                      // (no e-value column)
            d.wanted |= 1ull << d.col[r];
            if (d.col[r] > 0) d.wanted |= 1ull << (d.col[r] - 1);
        }
        return d;
    }
    // the layout with the cover behind it: the cover's columns, the threshold, where its count goes; the tab in front of each
    // cover field joins `wanted`
    DevLayoutCover device_layout_cover(unsigned long long* d_below) const {
        DevLayoutCover d{};
        static_cast<DevLayout&>(d) = device_layout();
        const bool by_len = cov->source == BLU_QUERY_COVER_QLEN;
        d.cov.by_len = by_len ? 1u : 0u;
        d.cov.n_fields = by_len ? 3u : 1u;
        d.cov.col[0] = by_len ? cov->qstart : cov->cover_column;
        d.cov.col[1] = by_len ? cov->qend : 0xFFFFFFFFu;
        d.cov.col[2] = by_len ? cov->qlen : 0xFFFFFFFFu;
        d.cov.p_milli = (double)cov->min_cover_milli;
        d.cov.below = d_below;
        for (uint32_t k = 0; k < d.cov.n_fields; ++k) if (d.cov.col[k] > 0) d.wanted |= 1ull << (d.cov.col[k] - 1);
        return d;
    }

    // ---- parse: one of the eight builds of the parse kernel, by the table's layout (none, one, one with a cover: DESIGN.md §23,
    // §24) and by the filter (none, thresholds, a taxon filter: DESIGN.md §14, §16).  Under a filter it leaves a keep word per
    // line, and its counts come back with the flags in `back`
    int parse() {
        TaxidMap::E* d_taxmap = nullptr;
        HIP_CHECK(pol, mem.upload(&d_taxmap, row_of.tab.data(), row_of.tab.size(), "taxid map"));
        HIP_CHECK(pol, mem.alloc(&d_qh, (size_t)n_rows * 8, "parsed rows")); HIP_CHECK(pol, mem.alloc(&d_ah, (size_t)n_rows * 8, "parsed rows"));
        HIP_CHECK(pol, mem.alloc(&d_qpos, (size_t)n_rows * 8, "parsed rows")); HIP_CHECK(pol, mem.alloc(&d_apos, (size_t)n_rows * 8, "parsed rows"));
        HIP_CHECK(pol, mem.alloc(&d_tax, (size_t)n_rows * 4, "parsed rows")); HIP_CHECK(pol, mem.alloc(&d_pid, (size_t)n_rows * 8, "parsed rows"));
        HIP_CHECK(pol, mem.alloc(&d_aln, (size_t)n_rows * 4, "parsed rows")); HIP_CHECK(pol, mem.alloc(&d_bs, (size_t)n_rows * 4, "parsed rows"));
        const RowOut o{d_qh, d_ah, d_qpos, d_apos, d_tax, d_pid, d_aln, d_bs};
        const DevTaxidMap tm{d_taxmap, row_of.tab.size() - 1};
        if (lay && flt && (flt->mask & BLU_FILTER_MAX_E_VALUE) && lay->e_value >= lay->n_columns) return fallback("an e-value threshold without an e-value column");
        if (cov && !lay) return fallback("a query cover without a column layout");
        const bool filtered = flt || taxa || cov;
        unsigned long long* const d_fcnt = reinterpret_cast<unsigned long long*>(d_flags + 16);   // (the filters' counts, behind the big counters)
        if (filtered) {
            HIP_CHECK(pol, mem.alloc(&d_keep, (size_t)n_rows * 4, "keep words"));
            HIP_CHECK(pol, mem.alloc(&d_filter, sizeof(DevFilterTaxa), "hit filter"));
            DevFilterTaxa hf{};
            if (flt) hf.f = device_filter(*flt);                     // (no threshold beside a taxon filter or a cover: an empty mask keeps every line)
            hf.f.keep = d_keep; hf.f.counts = d_fcnt;
            if (taxa) {                                              // the row codes go up next to the taxid map; the verdict is taken in the parse
                const size_t n_tax = taxa->code.size();
                HIP_CHECK(pol, mem.upload(&d_code, taxa->code.data(), n_tax, "taxon codes"));
                hf.t.code = d_code; hf.t.n_tax = (uint32_t)n_tax; hf.t.unmatched = taxa->unmatched;
                hf.t.not_only = d_fcnt + HIT_SPREAD + 1; hf.t.excluded_by = hf.t.not_only + HIT_SPREAD;
            }
            HIP_CHECK(pol, hipMemcpy(d_filter, &hf, sizeof hf, hipMemcpyHostToDevice));
        }
        // every build takes the same arguments (d_filter is null without a filter), then its layout if it has one
        auto launch = [&](auto kernel, auto... layout) {
            hipLaunchKernelGGL(kernel, dim3(grid(n_rows, PARSE_THREADS)), dim3(PARSE_THREADS), 0, 0, d_text, d_line, n_rows, tm, o, d_flags, d_big, d_filter, layout...);
        };
        if (cov) launch(taxa ? parse_rows_layout_qcov_taxa : parse_rows_layout_qcov, device_layout_cover(d_fcnt + HIT_SPREAD + 1 + n_taxa_back()));
        else if (lay) launch(taxa ? parse_rows_layout_taxa : filtered ? parse_rows_layout_filtered : parse_rows_layout, device_layout());
        else launch(taxa ? parse_rows_taxa : filtered ? parse_rows_filtered : parse_rows);
        if (!filtered) return check_flags();
        back.resize(n_back());
        HIP_CHECK(pol, hipMemcpy(back.data(), d_flags, n_back() * 8, hipMemcpyDeviceToHost));
        return fall_back_on((uint32_t)back[0]);
    }

    // ---- after a filtered parse: the e-values the device left open are decided, the rows are compacted in file order before
    // anything else sees them, the unmatched rows are counted over what is left
    int drop_filtered_rows() {
        if (!flt && !taxa && !cov) return BLU_OK;
        uint64_t n_kept = spread_sum(back.data() + 8, 0);
        const uint64_t n_ask = back[8 + HIT_SPREAD];
        const unsigned long long* const tb = back.data() + 8 + HIT_SPREAD + 1;   // (under a taxon filter: not-only, then per element)
        uint64_t n_excluded = 0, n_not_only = 0;
        if (taxa) {
            n_not_only = spread_sum(tb, 0);
            for (uint32_t k = 0; k < taxa->n_exclude; ++k) n_excluded += tb[HIT_SPREAD + k];
            if (n_excluded + n_not_only + n_kept + n_ask > n_rows) return fallback("inconsistent taxon-filter counts");
        }
        const uint64_t n_below = cov ? spread_sum(tb + n_taxa_back(), 0) : 0;
        if (n_below > n_rows) return fallback("inconsistent query-cover counts");
        lap("parse (filtered)");
        if (n_ask) STEP(decide_e_values_on_host((uint32_t)n_ask, &n_kept));
        if (n_kept > n_rows) return fallback("inconsistent hit-filter counts");
        const uint64_t n_lines = n_rows;
        if (n_kept == 0) return fallback("no rows kept by the filters");   // (the host parser returns the empty table)
        if (n_kept < n_rows) STEP(compact_rows((uint32_t)n_kept));
        mem.free(d_keep); mem.free(d_filter);
        if (d_code) mem.free(d_code);
        mem.free(d_line); d_line = nullptr;
        hipLaunchKernelGGL(count_unmatched, grid(n_rows, 1024), dim3(1024), 0, 0, (const uint32_t*)d_tax, n_rows, d_big);
        ht.n_lines = n_lines; ht.n_kept = n_kept; ht.n_below = n_below;
        if (taxa) {
            taxa->n_excluded = n_excluded; taxa->n_not_only = n_not_only;
            taxa->excluded_by.assign(tb + HIT_SPREAD, tb + HIT_SPREAD + taxa->n_exclude);
        }
        return BLU_OK;
    }
    // e-values the device left open (as a rule: fields spelled like the threshold): the host decides them from the file's bytes
    // with the host parser's own number reader and sends the decisions back
    int decide_e_values_on_host(uint32_t n_u, uint64_t* n_kept) {
        if (*n_kept + n_u > n_rows) return fallback("inconsistent hit-filter counts");
        uint32_t *d_urow = nullptr, *d_udec = nullptr;
        unsigned long long* d_upos = nullptr;
        HIP_CHECK(pol, mem.alloc(&d_urow, (size_t)n_u * 4, "undecided e-values")); HIP_CHECK(pol, mem.alloc(&d_upos, (size_t)n_u * 8, "undecided e-values"));
        HIP_CHECK(pol, mem.alloc(&d_udec, (size_t)n_u * 4, "undecided e-values"));
        HIP_CHECK(pol, hipMemset(d_urow, 0xFF, (size_t)n_u * 4));
        HIP_CHECK(pol, hipMemset(d_upos, 0, (size_t)n_u * 8));
        STEP(zero_counter());
        hipLaunchKernelGGL(list_undecided, grid(n_rows), dim3(256), 0, 0, (const uint32_t*)d_keep, n_rows, d_text, d_line, n_u, d_urow, d_upos, d_counter,
                           lay ? lay->e_value : 11u);
        std::vector<char> e_bytes;
        std::vector<unsigned long long> e_off;
        STEP(download_strings(d_upos, n_u, e_bytes, e_off));
        std::vector<uint32_t> dec(n_u);
        for (uint32_t k = 0; k < n_u; ++k) {
            double v = 0;
            if (!parse_f64_field(e_bytes.data() + e_off[k], (size_t)(e_off[k + 1] - e_off[k]), &v)) return fallback("an e-value the host parser reads differently");
            dec[k] = flt && v <= flt->max_e_value ? 1u : 0u;
            *n_kept += dec[k];
        }
        HIP_CHECK(pol, hipMemcpy(d_udec, dec.data(), (size_t)n_u * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(apply_decisions, grid(n_u), dim3(256), 0, 0, (const uint32_t*)d_urow, (const uint32_t*)d_udec, n_u, n_rows, d_keep);
        mem.free(d_urow); mem.free(d_upos); mem.free(d_udec);
        lap("  filter: e-values decided on the host");
        return BLU_OK;
    }
    // stable compaction, one column after another through ONE spare buffer (hit_pass.h: Compaction), 8-byte columns first.
    // Peak: the eight arrays (52 B / line) + keep words and their scan (8 B / line) + 8 B / kept line.
    int compact_rows(uint32_t n_out) {
        uint32_t* d_kpos = nullptr;
        HIP_CHECK(pol, mem.alloc(&d_kpos, (size_t)n_rows * 4, "keep positions"));
        HIP_CHECK(pol, need_tmp(scan_tmp_bytes_u32((size_t)n_rows)));
        HIP_CHECK(pol, exclusive_scan_u32(d_keep, d_kpos, (size_t)n_rows, d_tmp));
        Compaction cp{d_keep, d_kpos, n_rows, n_out, nullptr};
        HIP_CHECK(pol, mem.alloc(&cp.spare, (size_t)n_out * 8, "compaction spare"));
        HIP_CHECK(pol, cp.rotate(d_qh, d_ah, d_qpos, d_apos, d_pid, d_tax, d_aln, d_bs));
        mem.free(cp.spare); mem.free(d_kpos);
        n_rows = n_out;
        lap("  filter: compaction");
        return BLU_OK;
    }

    // ---- accession dictionary, first half: distinct count unknown; the table grows until the load stays under one half.
    // (It comes before the query dictionary so that the host's sort of the distinct accessions — 12 ms for 300 k — runs on a
    // thread of its own while the device builds the query dictionary.)
    int accession_dictionary_begin() {
        uint64_t cap = pow2_at_least(std::min<uint64_t>((uint64_t)n_rows * 2 + 16, 1ull << 20));   // (32 MB: stays in the caches while 100 M rows probe it; x4 when more than half full)
        for (;;) {
            HIP_CHECK(pol, mem.alloc(&d_atab, cap * sizeof(Slot), "accession table"));
            lap("  acc: table allocation");
            uint32_t h_flags = 0;
            STEP(build_dictionary(d_atab, cap, d_ah, /* only_heads */ false, /* clear_flags */ true, &n_acc, &h_flags));
            if (!(h_flags & FB_TABLE_FULL) && (uint64_t)n_acc * 2 <= cap) break;
            mem.free(d_atab); d_atab = nullptr;
            if (cap >= pow2_at_least((uint64_t)n_rows * 2 + 16)) return fallback(fallback_text(FB_TABLE_FULL));
            cap *= 4;
        }
        acap = cap;
        lap("  acc: insert");
        uint32_t* d_alist_row = nullptr;
        unsigned long long* d_aposlist = nullptr;
        HIP_CHECK(pol, hipMemset(d_flags, 0, 4));
        HIP_CHECK(pol, mem.alloc(&d_alist_row, (size_t)n_acc * 4, "accession list")); HIP_CHECK(pol, mem.alloc(&d_alist_slot, (size_t)n_acc * 4, "accession list"));
        STEP(zero_counter());
        hipLaunchKernelGGL(dict_finalize, grid(cap), dim3(256), 0, 0, d_atab, cap, d_text, d_apos, d_alist_row, d_alist_slot, d_counter);
        HIP_CHECK(pol, mem.alloc(&d_aposlist, (size_t)n_acc * 8, "accession list"));
        hipLaunchKernelGGL(gather_pos, grid(n_acc), dim3(256), 0, 0, d_apos, d_alist_row, n_acc, d_aposlist);
        STEP(download_strings(d_aposlist, n_acc, a_bytes, a_off));
        lap("  acc: distinct to host");
        // byte order of the distinct accessions (String::cmp), on the host: only the distinct strings are touched, and
        // mostly not even those — the GPU hands over their first 16 bytes as two big-endian integers; the text is read
        // only to order keys that agree on all 16
        k0.resize(n_acc); k1.resize(n_acc);
        unsigned long long *d_k0 = nullptr, *d_k1 = nullptr;
        HIP_CHECK(pol, mem.alloc(&d_k0, (size_t)n_acc * 8 + 8, "accession keys"));
        HIP_CHECK(pol, mem.alloc(&d_k1, (size_t)n_acc * 8 + 8, "accession keys"));
        hipLaunchKernelGGL(gather_key16, grid(n_acc), dim3(256), 0, 0, d_aposlist, n_acc, d_text, d_k0, d_k1);
        HIP_CHECK(pol, hipMemcpy(k0.data(), d_k0, (size_t)n_acc * 8, hipMemcpyDeviceToHost));
        HIP_CHECK(pol, hipMemcpy(k1.data(), d_k1, (size_t)n_acc * 8, hipMemcpyDeviceToHost));
        mem.free(d_k0);
        mem.free(d_k1);
        order.resize(n_acc);
        for (uint32_t k = 0; k < n_acc; ++k) order[k] = k;
        acc_sort = std::thread([this] { sort_accessions(); });
        return BLU_OK;
    }
    // (the body of acc_sort) `order` into the accessions' byte order: chunk sorts by a pool of threads, then a tree of merges
    void sort_accessions() {
        try {
            auto view = [&](uint32_t k) { return std::string_view(a_bytes.data() + a_off[k], (size_t)(a_off[k + 1] - a_off[k])); };
            auto less = [&](uint32_t a, uint32_t b) {
                if (k0[a] != k0[b]) return k0[a] < k0[b];
                if (k1[a] != k1[b]) return k1[a] < k1[b];
                const size_t la = (size_t)(a_off[a + 1] - a_off[a]), lb = (size_t)(a_off[b + 1] - a_off[b]);
                if (la <= 16 && lb <= 16) return la < lb;          // equal padded prefixes: the shorter string sorts first
                return view(a) < view(b);
            };
            const unsigned nt = n_acc < 65536 ? 1 : ingest_threads(32);
            std::vector<std::thread> pool;
            for (unsigned t = 0; t < nt; ++t)
                pool.emplace_back([&, t]() { std::sort(order.begin() + (size_t)n_acc * t / nt, order.begin() + (size_t)n_acc * (t + 1) / nt, less); });
            for (auto& th : pool) th.join();
            for (unsigned w = 1; w < nt; w *= 2)
                for (unsigned t = 0; t + w < nt; t += 2 * w)
                    std::inplace_merge(order.begin() + (size_t)n_acc * t / nt, order.begin() + (size_t)n_acc * (t + w) / nt,
                                       order.begin() + (size_t)n_acc * std::min(t + 2 * w, nt) / nt, less);
        } catch (...) { acc_sort_failed = true; }   // (no exception leaves a std::thread)
    }

    // ---- query dictionary: sized by the number of runs of equal hashes (an upper bound of the distinct count)
    int query_dictionary() {
        Slot* d_qtab = nullptr;
        uint32_t *d_list_row = nullptr, *d_list_slot = nullptr, *d_mark = nullptr, *d_rank_of_row = nullptr;
        unsigned long long* d_poslist = nullptr;
        hipLaunchKernelGGL(count_run_heads, grid(n_rows, 1024), dim3(1024), 0, 0, d_qh, n_rows, d_big + 1);
        unsigned long long runs = 0;
        HIP_CHECK(pol, hipMemcpy(&runs, d_big + 1, 8, hipMemcpyDeviceToHost));
        const uint64_t cap = pow2_at_least(runs * 2 + 16);
        HIP_CHECK(pol, mem.alloc(&d_qtab, cap * sizeof(Slot), "query table"));
        uint32_t h_flags = 0;
        STEP(build_dictionary(d_qtab, cap, d_qh, /* only_heads */ true, /* clear_flags */ false, &n_queries, &h_flags));
        STEP(fall_back_on(h_flags));
        lap("  query: insert");
        HIP_CHECK(pol, mem.alloc(&d_list_row, (size_t)n_queries * 4, "query list")); HIP_CHECK(pol, mem.alloc(&d_list_slot, (size_t)n_queries * 4, "query list"));
        STEP(zero_counter());
        hipLaunchKernelGGL(dict_finalize, grid(cap), dim3(256), 0, 0, d_qtab, cap, d_text, d_qpos, d_list_row, d_list_slot, d_counter);
        // ids in first-appearance order, and the names' positions in id order
        HIP_CHECK(pol, mem.alloc(&d_mark, ((size_t)n_rows + 1) * 4, "query ids")); HIP_CHECK(pol, mem.alloc(&d_rank_of_row, ((size_t)n_rows + 1) * 4, "query ids"));
        HIP_CHECK(pol, hipMemset(d_mark, 0, ((size_t)n_rows + 1) * 4));
        hipLaunchKernelGGL(mark_first_rows, grid(n_queries), dim3(256), 0, 0, (const uint32_t*)d_list_row, n_queries, d_mark);
        HIP_CHECK(pol, need_tmp(scan_tmp_bytes_u32((size_t)n_rows + 1)));
        HIP_CHECK(pol, exclusive_scan_u32(d_mark, d_rank_of_row, (size_t)n_rows + 1, d_tmp));
        HIP_CHECK(pol, mem.alloc(&d_poslist, (size_t)n_queries * 8, "query list"));
        hipLaunchKernelGGL(number_queries, grid(n_queries), dim3(256), 0, 0, d_qtab, (const uint32_t*)d_list_row, (const uint32_t*)d_list_slot, n_queries,
                           (const uint32_t*)d_rank_of_row, (const unsigned long long*)d_qpos, d_poslist);
        HIP_CHECK(pol, mem.alloc(&d_qid, (size_t)n_rows * 4, "query ids"));
        hipLaunchKernelGGL(dict_lookup, grid(n_rows), dim3(256), 0, 0, d_qh, d_qpos, n_rows, d_qtab, cap - 1, d_text, d_qpos, d_qid, d_flags);
        STEP(check_flags());
        lap("  query: ids of the rows");
        // query names: the text of each query's first row, in id order
        STEP(download_strings(d_poslist, n_queries, q_bytes, q_off));
        lap("  query: names");
        mem.free(d_poslist);
        mem.free(d_list_row); mem.free(d_list_slot); mem.free(d_mark); mem.free(d_rank_of_row);
        mem.free(d_qtab);
        mem.free(d_qh); d_qh = nullptr;
        mem.free(d_qpos); d_qpos = nullptr;
        return BLU_OK;
    }

    // ---- accession dictionary, second half: the ranks go up, every row gets its accession's
    int accession_dictionary_finish() {
        acc_sort.join();
        if (acc_sort_failed) return fallback("the host could not sort the accessions");
        lap("  acc: wait for the host sort");
        uint32_t* d_ranks = nullptr;
        std::vector<uint32_t> rank_of(n_acc);
        for (uint32_t r = 0; r < n_acc; ++r) rank_of[order[r]] = r;
        HIP_CHECK(pol, mem.alloc(&d_ranks, (size_t)n_acc * 4, "accession ranks"));
        HIP_CHECK(pol, hipMemcpy(d_ranks, rank_of.data(), (size_t)n_acc * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(dict_assign_ids, grid(n_acc), dim3(256), 0, 0, d_atab, d_alist_slot, (const uint32_t*)d_ranks, n_acc);
        HIP_CHECK(pol, mem.alloc(&d_arank, (size_t)n_rows * 4, "accession ranks"));
        hipLaunchKernelGGL(dict_lookup, grid(n_rows), dim3(256), 0, 0, d_ah, d_apos, n_rows, d_atab, acap - 1, d_text, d_apos, d_arank, d_flags);
        STEP(check_flags());
        lap("  acc: ranks of the rows");
        mem.free(d_atab); d_atab = nullptr;
        mem.free(d_ah); d_ah = nullptr;
        mem.free(d_apos); d_apos = nullptr;
        mem.free(d_text); d_text = nullptr;
        return BLU_OK;
    }

    // ---- grouping: queries in first-appearance order, file order inside a query (mod.rs:192-208)
    int group() {
        STEP(zero_counter());
        hipLaunchKernelGGL(check_grouped, grid(n_rows), dim3(256), 0, 0, d_qid, n_rows, d_counter);
        uint32_t unsorted = 0;
        HIP_CHECK(pol, hipMemcpy(&unsorted, d_counter, 4, hipMemcpyDeviceToHost));
        lap(unsorted ? "  grouping: check (unsorted)" : "  grouping: check (sorted)");
        uint32_t *d_perm = nullptr, *d_perm2 = nullptr, *d_qid2 = nullptr;
        if (unsorted) {
            HIP_CHECK(pol, mem.alloc(&d_perm, (size_t)n_rows * 4, "regrouping")); HIP_CHECK(pol, mem.alloc(&d_perm2, (size_t)n_rows * 4, "regrouping"));
            HIP_CHECK(pol, mem.alloc(&d_qid2, (size_t)n_rows * 4, "regrouping"));
            hipLaunchKernelGGL(iota_u32, grid(n_rows), dim3(256), 0, 0, d_perm, n_rows);
            int bits = 1;
            while ((1ull << bits) < n_queries) ++bits;
            uint32_t* d_table = nullptr;
            HIP_CHECK(pol, mem.alloc(&d_table, radix_table_words(n_rows) * 4, "regrouping"));
            HIP_CHECK(pol, need_tmp(radix_scan_tmp_bytes(n_rows)));
            // (stable: file order survives inside a query; afterwards d_qid2 / d_perm2 name the sorted arrays whichever buffer they are)
            uint32_t *k0 = d_qid, *k1 = d_qid2, *v0 = d_perm, *v1 = d_perm2;
            HIP_CHECK(pol, radix_sort_pairs(&k0, &k1, &v0, &v1, n_rows, bits, d_table, d_tmp));
            d_qid2 = k0; d_qid = k1; d_perm2 = v0; d_perm = v1;
            mem.free(d_table);
        }
        HIP_CHECK(pol, mem.alloc(&d_seg, ((size_t)n_queries + 1) * 8 * 2, "segment offsets"));
        HIP_CHECK(pol, hipMemset(d_seg, 0, ((size_t)n_queries + 1) * 8 * 2));
        hipLaunchKernelGGL(segment_starts, grid(n_rows), dim3(256), 0, 0, (const uint32_t*)(unsorted ? d_qid2 : d_qid), n_rows, n_queries,
                           d_seg + n_queries + 1);
        HIP_CHECK(pol, mem.alloc(&grouped.bs, (size_t)n_rows * 4, "grouped columns")); HIP_CHECK(pol, mem.alloc(&grouped.aln, (size_t)n_rows * 4, "grouped columns"));
        HIP_CHECK(pol, mem.alloc(&grouped.tax, (size_t)n_rows * 4, "grouped columns")); HIP_CHECK(pol, mem.alloc(&grouped.arank, (size_t)n_rows * 4, "grouped columns"));
        HIP_CHECK(pol, mem.alloc(&grouped.pid, (size_t)n_rows * 8, "grouped columns"));
        lap("  grouping: offsets + allocations");
        const Cols in{d_bs, d_aln, d_tax, d_arank, d_pid};
        hipLaunchKernelGGL(gather_cols, grid(n_rows), dim3(256), 0, 0, in, grouped, (const uint32_t*)(unsorted ? d_perm2 : nullptr), n_rows);
        return BLU_OK;
    }

    // ---- the grouped columns stay on the device for the engine; the host copies are made only on request
    int hand_over() {
        unsigned long long unmatched = 0;
        HIP_CHECK(pol, hipMemcpy(&unmatched, d_big, 8, hipMemcpyDeviceToHost));
        ht.unmatched = unmatched;
        ht.n_hits = n_rows;
        ht.host_columns = false;
        ht.dev.reset(new DeviceHits());
        ht.dev->device = device; ht.dev->n_hits = n_rows; ht.dev->n_queries = n_queries;
        ht.dev->bitscore = grouped.bs; ht.dev->align_len = grouped.aln; ht.dev->tax_desc_row = grouped.tax; ht.dev->acc_rank = grouped.arank;
        ht.dev->pident = grouped.pid;
        ht.dev->seg_off = d_seg + n_queries + 1; ht.dev->seg_block = d_seg;
        for (void* q : {(void*)grouped.bs, (void*)grouped.aln, (void*)grouped.tax, (void*)grouped.arank, (void*)grouped.pid, (void*)d_seg}) mem.release(q);
        if (host_columns) {
            STEP(download_columns(ht));
            lap("download columns");
        }
        ht.n_queries = n_queries;
        start_strings_thread();
        return BLU_OK;
    }
    // the host strings (query names in id order, accessions in byte order) are built from the packed bytes by a
    // background thread while the caller goes on to the engine: nothing on the device waits for them
    void start_strings_thread() {
        const unsigned nt = (uint64_t)n_queries + n_acc < 65536 ? 1 : ingest_threads(16);
        HitTable* const hp = &ht;
        ht.strings_thread = std::thread([hp, nt, q_bytes = std::move(q_bytes), q_off = std::move(q_off), a_bytes = std::move(a_bytes),
                                         a_off = std::move(a_off), order = std::move(order)]() {
            std::atomic<bool> oom{false};            // (an exception must not leave a std::thread: the caller checks strings_ok)
            // (sizing 2 M strings is 64 MB of fresh pages: 10 ms that need not stand between the ingest and the engine)
            try { hp->query_names.resize(q_off.size() - 1); hp->accessions.resize(a_off.size() - 1); }
            catch (const std::bad_alloc&) { hp->strings_ok = false; return; }
            auto work = [&](unsigned t) {
                try {
                    const size_t nq = q_off.size() - 1, na = a_off.size() - 1;
                    for (size_t q = nq * t / nt; q < nq * (t + 1) / nt; ++q)
                        hp->query_names[q].assign(q_bytes.data() + q_off[q], (size_t)(q_off[q + 1] - q_off[q]));
                    for (size_t r = na * t / nt; r < na * (t + 1) / nt; ++r) {
                        const uint32_t k = order[r];
                        hp->accessions[r].assign(a_bytes.data() + a_off[k], (size_t)(a_off[k + 1] - a_off[k]));
                    }
                } catch (const std::bad_alloc&) { oom = true; }
            };
            try {
                std::vector<std::thread> pool;
                struct JoinAll { std::vector<std::thread>& p; ~JoinAll() { for (auto& th : p) if (th.joinable()) th.join(); } } join_all{pool};
                for (unsigned t = 1; t < nt; ++t) pool.emplace_back(work, t);
                work(0);
            } catch (...) { oom = true; }
            if (oom) hp->strings_ok = false;
        });
    }
};
#undef STEP

}  // namespace

int load_hits_gpu(int fd, size_t size, const TaxidMap& row_of, int device, bool host_columns, HitTable& ht, std::string* why,
                  const blu_hit_filter* flt, TaxonCodes* taxa, const blu_table_layout* lay, const blu_query_cover* cov) {
    if (flt && !(flt->mask & 15u)) flt = nullptr;
    IngestTrace lap;
    std::string why_unread;
    if (!why) why = &why_unread;
    if (size == 0) { *why = "an empty file"; return BLU_INGEST_FALLBACK; }
    if (size >= (1ull << 44)) { *why = "a file of 16 TiB or more"; return BLU_INGEST_FALLBACK; }
    if (hipSetDevice(device) != hipSuccess) { set_error("hipSetDevice(%d) failed", device); return BLU_ERR_NO_DEVICE; }
    // out of device memory is no error of the call: the CPU parser takes the file
    HipPolicy pol{"GPU ingest", BLU_INGEST_FALLBACK, why};
    DeviceArena mem(pol);
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (double)size * 2.8 + (1ull << 30) > (double)free_b) {
            *why = "a file too large for this device's free memory";
            return BLU_INGEST_FALLBACK;
        }
        mem.keep = (double)size * 4.0 + (4ull << 30) < (double)free_b;
    }
    // (in a block of its own: the sort thread is joined and the host strings are let go before the arena's buffers are)
    int rc;
    { GpuIngest ingest{fd, size, row_of, device, host_columns, ht, mem, mem.pol, lap, flt, taxa, lay, cov}; rc = ingest.run(); }
    if (rc != BLU_OK) ht.clear();
    lap("hand-over");
    // with room on the card (mem.keep) the work buffers — the text, the hashes, the dictionaries: 10 GB for a 2 M-query table —
    // are freed with the columns, off the caller's path (5-7 ms of hipFree); otherwise here
    if (rc == BLU_OK && mem.keep && ht.dev) mem.hand_over(ht.dev->trash);
    mem.free_all();
    lap("free the work buffers");
    return rc;
}

// The columns come back in 64 MiB pieces copied by a pool of host threads: the first touch of the fresh host pages
// costs more than the transfer, and it parallelises (the vectors are resized without initialisation).
int download_columns(HitTable& ht) {
    if (ht.host_columns) return BLU_OK;
    if (!ht.dev) { set_error("download_columns: no device columns"); return BLU_ERR_INVALID_ARG; }
    const DeviceHits& d = *ht.dev;
    const size_t n_rows = d.n_hits, n_queries = d.n_queries;
    ht.seg_off.resize(n_queries + 1);
    ht.bitscore.resize(n_rows); ht.align_len.resize(n_rows); ht.tax_desc_row.resize(n_rows); ht.acc_rank.resize(n_rows); ht.pident.resize(n_rows);
    std::vector<D2HPiece> pieces;
    auto add = [&](void* dst, const void* src, size_t bytes) { d2h_add(pieces, dst, src, bytes, 64u << 20); };
    add(ht.seg_off.data(), d.seg_off, (n_queries + 1) * 8);
    add(ht.bitscore.data(), d.bitscore, n_rows * 4); add(ht.align_len.data(), d.align_len, n_rows * 4);
    add(ht.tax_desc_row.data(), d.tax_desc_row, n_rows * 4); add(ht.acc_rank.data(), d.acc_rank, n_rows * 4);
    add(ht.pident.data(), d.pident, n_rows * 8);
    // (pinning the destination pieces first — hipHostRegister — made it slower: 0.33 s instead of 0.21 s for 2 GB)
    const hipError_t e = d2h_parallel(pieces, d.device);
    if (e != hipSuccess) { set_error("GPU ingest: column download failed: %s", hipGetErrorString(e)); return BLU_ERR_HIP; }
    ht.host_columns = true;
    return BLU_OK;
}
}  // namespace blu
