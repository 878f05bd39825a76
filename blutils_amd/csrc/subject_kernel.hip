// Best hit per subject (include/blu_consensus.h: blu_hits_subject_keep, blu_hits_subject_best): of the rows of one
// (query, acc_rank) pair the one with the highest truncated bit-score is kept, the first of the segment among equals, and the
// others are dropped.  One pass over the grouped columns, between the parser and the band.
//
// The rows of a pair are ordered by pack = (uint64)((uint32)bitscore ^ 0x80000000) << 32 | (0xFFFFFFFF - i), i the row's index in
// its segment: larger for a better score, among equal scores larger for an earlier row, unique inside a segment.  A row is kept iff
// no row of its segment has its acc_rank and a larger pack.
//
// Short segments (<= 64 rows): a wave takes SUBJ_QPW consecutive queries, one after the other.  Each lane loads its row; the wave
// loops over the segment's rows and reads row k's acc_rank and biased score with a readlane (k is wave-uniform, and so is the
// trip count: every lane takes part in every read); the low half of row k's pack is known from k.  One store per lane, counts by
// ballot and popcount.  No LDS.
//
// Long segments (> 64 rows): the short kernel leaves them alone and writes their length to a word per query.  A scan of the lengths
// and long_query_list (hit_pass.h) turn these words into the list of long queries and the start of each among the R long rows.  A thread per long
// row finds its query by a binary search in that list.  One open-addressing table of 16-byte slots {key, val}, a power-of-two
// capacity >= 2 R, home slot = mix(key) & (capacity - 1), linear probing that wraps: kernel 1 claims the slot of
// key = query << 32 | acc_rank with a CAS and raises val to its pack with a 64-bit atomicMax; kernel 2 looks the pair up and keeps the
// row iff val is its own pack.  pack being unique inside a segment, the outcome does not depend on scheduling.  A probe gives up
// after `capacity` steps (it never does on a table that holds at most R <= capacity / 2 keys) and raises the error word.
//
// Segments, counters, the long-query list, the compaction and the staging of host columns are hit_pass.h's.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "hit_pass.h"
#include "ingest.h"

namespace blu {
namespace {

constexpr uint32_t SUBJ_BLOCK = 256;                 // threads per block: four waves
constexpr uint32_t SUBJ_QPW = BLU_SUBJECT_QUERIES_PER_WAVE;
// spread counters: kept rows, thinned queries, long queries, long rows; then the error word
constexpr uint32_t CNT_KEPT = 0, CNT_THINNED = 1, CNT_LONG = 2, CNT_LONG_ROWS = 3, CNT_ERROR = 4 * HIT_SPREAD, CNT_WORDS = 4 * HIT_SPREAD + 1;
constexpr unsigned long long EMPTY_KEY = ~0ull;

struct Slot { unsigned long long key, val; };        // 16 bytes

struct SubjDev {
    const int32_t* __restrict__ bitscore;
    const uint32_t* __restrict__ acc_rank;
    const unsigned long long* __restrict__ seg_off;
    uint64_t n_hits, n_queries;
    uint32_t* __restrict__ keep;                     // [n_hits]
    uint32_t* __restrict__ long_len;                 // [n_queries + 1]: the length of a long segment, else 0
    uint32_t* __restrict__ long_flag;                // [n_queries + 1]: 1 for a long segment, else 0
    unsigned long long* __restrict__ counts;         // [CNT_WORDS]
};

__device__ __forceinline__ uint32_t biased(int32_t bs) { return (uint32_t)bs ^ 0x80000000u; }

__global__ __launch_bounds__(SUBJ_BLOCK) void subject_short_kernel(SubjDev d) {
    const uint32_t lane = threadIdx.x & 63u;
    // (the wave's number as a scalar: the offsets, the trip counts and the readlane indices below are then wave-uniform to the compiler too)
    const uint64_t wave = (uint64_t)blockIdx.x * (SUBJ_BLOCK / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned long long n_kept = 0, n_thinned = 0, n_long = 0, n_long_rows = 0;   // (wave-uniform)
    for (uint32_t k = 0; k < SUBJ_QPW; ++k) {
        const uint64_t q = wave * SUBJ_QPW + k;
        if (q >= d.n_queries) break;                 // (wave-uniform)
        uint64_t s0, s1;
        segment_of(d.seg_off, q, d.n_hits, &s0, &s1);
        const uint64_t len = s1 - s0;
        const bool is_long = len > 64u;
        if (lane == 0) { d.long_len[q] = is_long ? (uint32_t)len : 0u; d.long_flag[q] = is_long ? 1u : 0u; }
        if (is_long) { n_long += 1; n_long_rows += len; continue; }
        if (len == 0) continue;
        const uint32_t n = (uint32_t)len;            // (wave-uniform)
        const bool has = lane < n;
        const uint64_t i = s0 + lane;
        const uint32_t acc = has ? d.acc_rank[i] : 0u;
        const uint32_t hi = has ? biased(d.bitscore[i]) : 0u;
        bool keep = has;
        for (uint32_t r = 0; r < n; ++r) {           // (row r's pack is hi_r << 32 | 0xFFFFFFFF - r: larger than this lane's iff ...)
            const uint32_t acc_r = (uint32_t)__builtin_amdgcn_readlane((int)acc, (int)r);
            const uint32_t hi_r = (uint32_t)__builtin_amdgcn_readlane((int)hi, (int)r);
            if (acc_r == acc && (hi_r > hi || (hi_r == hi && r < lane))) keep = false;
        }
        if (has) d.keep[i] = keep ? 1u : 0u;
        const unsigned long long kept = (unsigned long long)__popcll(__ballot(keep));
        n_kept += kept;
        n_thinned += kept < n ? 1ull : 0ull;
    }
    if (lane == 0) {
        spread_add(d.counts, CNT_KEPT, n_kept); spread_add(d.counts, CNT_THINNED, n_thinned);
        spread_add(d.counts, CNT_LONG, n_long); spread_add(d.counts, CNT_LONG_ROWS, n_long_rows);
    }
}

__global__ void subject_table_init(Slot* __restrict__ tab, uint64_t n_slots) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_slots) tab[i] = Slot{EMPTY_KEY, 0ull};
}

struct LongDev {
    const int32_t* __restrict__ bitscore;
    const uint32_t* __restrict__ acc_rank;
    const unsigned long long* __restrict__ seg_off;
    uint64_t n_hits;
    const uint32_t* __restrict__ list_q;             // [n_long]
    const uint32_t* __restrict__ list_start;         // [n_long + 1], the last entry = n_rows
    uint32_t n_long, n_rows;
    Slot* tab;
    uint64_t mask;                                   // capacity - 1
    uint32_t* __restrict__ keep;
    uint32_t* thinned;                               // [n_long]: 0, set to 1 by the first dropped row of the query
    unsigned long long* counts;
};

__device__ __forceinline__ uint64_t subject_home(unsigned long long key, uint64_t mask) {
    uint64_t x = key * 0x9E3779B97F4A7C15ull;
    return (x ^ (x >> 32)) & mask;
}

// long row t -> its query's place j in the list, its row and its pair's key and pack; false: no such row
__device__ __forceinline__ bool long_row(const LongDev& d, uint32_t t, uint32_t* j_out, uint64_t* row, unsigned long long* key,
                                         unsigned long long* pack) {
    if (t >= d.n_rows) return false;
    uint32_t lo = 0, hi = d.n_long;                  // the last j with list_start[j] <= t
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (d.list_start[mid] <= t) lo = mid; else hi = mid; }
    const uint32_t q = d.list_q[lo], i = t - d.list_start[lo];
    uint64_t s0, s1;
    segment_of(d.seg_off, q, d.n_hits, &s0, &s1);
    if (s0 + i >= s1) return false;                  // (the lengths were taken from the same offsets: never)
    *j_out = lo; *row = s0 + i;
    *key = (unsigned long long)q << 32 | d.acc_rank[s0 + i];
    *pack = (unsigned long long)biased(d.bitscore[s0 + i]) << 32 | (0xFFFFFFFFu - i);
    return true;
}

__global__ __launch_bounds__(SUBJ_BLOCK) void subject_insert_kernel(LongDev d) {
    const uint32_t t = blockIdx.x * SUBJ_BLOCK + threadIdx.x;
    uint32_t j; uint64_t row; unsigned long long key, pack;
    if (!long_row(d, t, &j, &row, &key, &pack)) return;
    uint64_t s = subject_home(key, d.mask);
    for (uint64_t step = 0; step <= d.mask; ++step, s = (s + 1) & d.mask) {
        const unsigned long long prev = atomicCAS(&d.tab[s].key, EMPTY_KEY, key);
        if (prev == EMPTY_KEY || prev == key) { atomicMax(&d.tab[s].val, pack); return; }
    }
    atomicOr(&d.counts[CNT_ERROR], 1ull);            // (a full table: the capacity rule rules it out)
}

__global__ __launch_bounds__(SUBJ_BLOCK) void subject_lookup_kernel(LongDev d) {
    const uint32_t t = blockIdx.x * SUBJ_BLOCK + threadIdx.x;
    uint32_t j = 0; uint64_t row = 0; unsigned long long key = 0, pack = 0;
    const bool has = long_row(d, t, &j, &row, &key, &pack);
    bool keep = false;
    if (has) {
        bool found = false;
        uint64_t s = subject_home(key, d.mask);
        for (uint64_t step = 0; step <= d.mask; ++step, s = (s + 1) & d.mask) {
            const unsigned long long k = d.tab[s].key;
            if (k == key) { keep = d.tab[s].val == pack; found = true; break; }
            if (k == EMPTY_KEY) break;
        }
        if (!found) atomicOr(&d.counts[CNT_ERROR], 1ull);
        d.keep[row] = keep ? 1u : 0u;
        if (found && !keep && __hip_atomic_load(&d.thinned[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u && atomicExch(&d.thinned[j], 1u) == 0u)
            spread_add(d.counts, CNT_THINNED, 1ull);
    }
    spread_add_ballot(d.counts, CNT_KEPT, keep);
}

uint64_t table_capacity(uint64_t long_rows) { uint64_t c = 2; while (c < 2 * long_rows) c <<= 1; return c; }

}  // namespace

int check_subject_best(const blu_subject_best* sel) {
    if (sel && (sel->mask & ~BLU_SUBJECT_BEST_PER_QUERY)) { set_error("best hit per subject: unknown bits in the mask"); return BLU_ERR_INVALID_ARG; }
    return BLU_OK;
}

int subject_keep_device(const int32_t* d_bitscore, const uint32_t* d_acc_rank, const uint64_t* d_seg_off, uint64_t n_hits, uint64_t n_queries,
                        uint32_t* d_keep, uint64_t* n_kept, uint64_t* n_thinned) {
    HipPolicy pol{"best hit per subject", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    *n_kept = *n_thinned = 0;
    if (n_hits == 0) return BLU_OK;
    HIP_CHECK(pol, hipMemsetAsync(d_keep, 0, n_hits * 4, nullptr));   // (a row that no segment names is dropped)
    if (n_queries == 0) { HIP_CHECK(pol, hipStreamSynchronize(nullptr)); return BLU_OK; }
    const uint64_t waves = (n_queries + SUBJ_QPW - 1) / SUBJ_QPW;
    const uint64_t blocks = (waves + SUBJ_BLOCK / 64 - 1) / (SUBJ_BLOCK / 64);
    unsigned long long* d_counts = nullptr;
    uint32_t *d_len = nullptr, *d_flag = nullptr;             // [n_queries + 1]: a pad word for the scans
    unsigned long long counts[CNT_WORDS];
    HIP_CHECK(pol, mem.alloc(&d_counts, sizeof counts, "counts"));
    HIP_CHECK(pol, mem.alloc(&d_len, (n_queries + 1) * 4, "long lengths"));
    HIP_CHECK(pol, mem.alloc(&d_flag, (n_queries + 1) * 4, "long flags"));
    HIP_CHECK(pol, hipMemsetAsync(d_counts, 0, sizeof counts, nullptr));
    HIP_CHECK(pol, hipMemsetAsync(d_len + n_queries, 0, 4, nullptr));
    SubjDev d{};
    d.bitscore = d_bitscore; d.acc_rank = d_acc_rank; d.seg_off = (const unsigned long long*)d_seg_off; d.n_hits = n_hits; d.n_queries = n_queries;
    d.keep = d_keep; d.long_len = d_len; d.long_flag = d_flag; d.counts = d_counts;
    hipLaunchKernelGGL(subject_short_kernel, dim3((unsigned)blocks), dim3(SUBJ_BLOCK), 0, nullptr, d);
    HIP_CHECK(pol, hipGetLastError());
    HIP_CHECK(pol, hipMemcpy(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost));
    const uint64_t n_long = spread_sum(counts, CNT_LONG), long_rows = spread_sum(counts, CNT_LONG_ROWS);
    if (n_long) {
        if (long_rows > n_hits) { set_error("best hit per subject: the segments overlap (their rows sum to more than n_hits)"); return BLU_ERR_INVALID_ARG; }
        const uint64_t cap = table_capacity(long_rows);
        uint32_t *d_rstart = nullptr, *d_list_q = nullptr, *d_list_start = nullptr, *d_thinned = nullptr;
        void* d_tmp = nullptr;
        Slot* d_tab = nullptr;
        HIP_CHECK(pol, mem.alloc(&d_rstart, (n_queries + 1) * 4, "long row starts"));
        HIP_CHECK(pol, mem.alloc(&d_tmp, scan_tmp_bytes_u32(n_queries + 1), "scan work"));
        HIP_CHECK(pol, mem.alloc(&d_thinned, n_long * 4, "thinned flags"));
        HIP_CHECK(pol, mem.alloc(&d_tab, cap * sizeof(Slot), "pair table"));
        HIP_CHECK(pol, exclusive_scan_u32(d_len, d_rstart, n_queries + 1, d_tmp));
        if (const int rc = long_query_list(pol, mem, d_flag, n_queries, n_long, d_rstart, d_tmp, &d_list_q, &d_list_start)) return rc;
        HIP_CHECK(pol, hipMemsetAsync(d_thinned, 0, n_long * 4, nullptr));
        const uint32_t rows32 = (uint32_t)long_rows;
        HIP_CHECK(pol, hipMemcpyAsync(d_list_start + n_long, &rows32, 4, hipMemcpyHostToDevice, nullptr));
        hipLaunchKernelGGL(subject_table_init, grid(cap), dim3(256), 0, nullptr, d_tab, cap);
        LongDev l{};
        l.bitscore = d_bitscore; l.acc_rank = d_acc_rank; l.seg_off = (const unsigned long long*)d_seg_off; l.n_hits = n_hits;
        l.list_q = d_list_q; l.list_start = d_list_start; l.n_long = (uint32_t)n_long; l.n_rows = rows32;
        l.tab = d_tab; l.mask = cap - 1; l.keep = d_keep; l.thinned = d_thinned; l.counts = d_counts;
        hipLaunchKernelGGL(subject_insert_kernel, grid(long_rows, SUBJ_BLOCK), dim3(SUBJ_BLOCK), 0, nullptr, l);
        hipLaunchKernelGGL(subject_lookup_kernel, grid(long_rows, SUBJ_BLOCK), dim3(SUBJ_BLOCK), 0, nullptr, l);
        HIP_CHECK(pol, hipGetLastError());
        HIP_CHECK(pol, hipMemcpy(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost));
        if (counts[CNT_ERROR]) { set_error("best hit per subject: the pair table failed (overlapping segments?)"); return BLU_ERR_INVALID_ARG; }
    }
    *n_kept = spread_sum(counts, CNT_KEPT); *n_thinned = spread_sum(counts, CNT_THINNED);
    return BLU_OK;
}

int subject_best_device(HitColumns& c, uint64_t n_hits, uint64_t n_queries, bool rotate, uint32_t unmatched_marker,
                        uint64_t* n_hits_out, uint64_t* n_unmatched, uint64_t* n_thinned, std::vector<void*>* retired, bool count_only) {
    HipPolicy pol{"best hit per subject", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    *n_hits_out = n_hits; *n_thinned = 0;
    if (n_hits == 0 || count_only)
        return compact_kept_device(pol.who, c, n_hits, n_queries, nullptr, true, rotate, unmatched_marker, n_hits_out, n_unmatched, retired);
    uint32_t* d_keep = nullptr;
    HIP_CHECK(pol, mem.alloc(&d_keep, (n_hits + 1) * 4, "keep words"));
    HIP_CHECK(pol, hipMemsetAsync(d_keep + n_hits, 0, 4, nullptr));
    uint64_t n_kept = 0;
    int rc = subject_keep_device(*c.bitscore, *c.acc_rank, (const uint64_t*)c.seg_off, n_hits, n_queries, d_keep, &n_kept, n_thinned);
    if (rc != BLU_OK) return rc;
    return compact_kept_device(pol.who, c, n_hits, n_queries, d_keep, n_kept == n_hits, rotate, unmatched_marker, n_hits_out, n_unmatched, retired);
}

int subject_best_hits(DeviceHits& dev, blu_subject_best_stats* stats, uint64_t* unmatched) {
    *stats = blu_subject_best_stats{dev.n_hits, dev.n_hits, dev.n_queries, 0};
    if (int rc = check_hit_counts("best hit per subject", dev.n_hits, dev.n_queries)) return rc;
    if (int rc = use_device("best hit per subject", dev.device)) return rc;
    HitColumns c = columns_of(dev);
    uint64_t n_out = dev.n_hits, n_thinned = 0;
    const int rc = subject_best_device(c, dev.n_hits, dev.n_queries, true, BLU_UNMATCHED_TAXID, &n_out, unmatched, &n_thinned, &dev.trash, false);
    if (rc != BLU_OK) return rc;
    dev.n_hits = n_out;
    stats->n_kept = n_out; stats->n_thinned = n_thinned;
    return BLU_OK;
}

}  // namespace blu

using namespace blu;

extern "C" {

int blu_hits_subject_keep(int device, const int32_t* bitscore, const uint32_t* acc_rank, const uint64_t* seg_off, uint64_t n_hits,
                          uint64_t n_queries, int on_device, void* stream, uint32_t* keep_out, blu_subject_best_stats* stats) {
    if (stats) *stats = blu_subject_best_stats{n_hits, 0, n_queries, 0};
    if ((n_hits && (!bitscore || !acc_rank || !keep_out)) || (n_queries && !seg_off)) return refuse_null_array("blu_hits_subject_keep");
    int rc = check_hit_counts("best hit per subject", n_hits, n_queries);
    if (rc != BLU_OK) return rc;
    if (n_hits == 0) return BLU_OK;
    if ((rc = use_device("blu_hits_subject_keep", device)) != BLU_OK) return rc;
    HipPolicy pol{"blu_hits_subject_keep", BLU_ERR_ALLOC};
    uint64_t n_kept = 0, n_thinned = 0;
    if (on_device) {
        HIP_CHECK(pol, hipStreamSynchronize((hipStream_t)stream));
        rc = subject_keep_device(bitscore, acc_rank, seg_off, n_hits, n_queries, keep_out, &n_kept, &n_thinned);
    } else {
        // host pointers: the two columns and the offsets go up, the same kernels run, the verdicts come back
        DeviceArena mem(pol);
        int32_t* d_bs = nullptr;
        uint32_t *d_acc = nullptr, *d_keep = nullptr;
        uint64_t* d_seg = nullptr;
        HIP_CHECK(pol, mem.upload(&d_bs, bitscore, n_hits, "bit-scores"));
        HIP_CHECK(pol, mem.upload(&d_acc, acc_rank, n_hits, "accession ranks"));
        HIP_CHECK(pol, mem.alloc(&d_keep, n_hits * 4, "keep words"));
        HIP_CHECK(pol, mem.upload(&d_seg, seg_off, n_queries ? n_queries + 1 : 0, "offsets"));
        rc = subject_keep_device(d_bs, d_acc, d_seg, n_hits, n_queries, d_keep, &n_kept, &n_thinned);
        if (rc == BLU_OK) HIP_CHECK(pol, mem.download(keep_out, d_keep, n_hits));
    }
    if (rc != BLU_OK) return rc;
    if (stats) { stats->n_kept = n_kept; stats->n_thinned = n_thinned; }
    return BLU_OK;
}

int blu_hits_subject_best(int device, int32_t* bitscore, int32_t* align_len, uint32_t* tax_desc_row, uint32_t* acc_rank, double* pident,
                          uint64_t* seg_off, uint64_t n_hits, uint64_t n_queries, int on_device, const blu_subject_best* sel, void* stream,
                          uint32_t unmatched_marker, uint64_t* n_hits_out, uint64_t* n_unmatched_out, blu_subject_best_stats* stats) {
    if (stats) *stats = blu_subject_best_stats{n_hits, n_hits, n_queries, 0};
    if (n_hits_out) *n_hits_out = n_hits;
    int rc = check_subject_best(sel);
    if (rc != BLU_OK) return rc;
    if ((n_hits && (!bitscore || !align_len || !tax_desc_row || !acc_rank || !pident)) || (n_queries && !seg_off)) return refuse_null_array("blu_hits_subject_best");
    if ((rc = check_hit_counts("best hit per subject", n_hits, n_queries)) != BLU_OK) return rc;
    const bool active = sel && sel->mask != 0;
    if (!active && !on_device) {                     // no selection: the table as it is (no device needed)
        if (n_unmatched_out) { *n_unmatched_out = 0; for (uint64_t i = 0; i < n_hits; ++i) *n_unmatched_out += tax_desc_row[i] == unmatched_marker; }
        return BLU_OK;
    }
    HitColumns c{&bitscore, &align_len, &tax_desc_row, &acc_rank, &pident, (unsigned long long*)seg_off};
    if (on_device && (rc = check_aligned16("blu_hits_subject_best", c)) != BLU_OK) return rc;
    if ((rc = use_device("blu_hits_subject_best", device)) != BLU_OK) return rc;
    HipPolicy pol{"blu_hits_subject_best", BLU_ERR_ALLOC};
    uint64_t n_out = n_hits, n_unmatched = 0, n_thinned = 0;
    if (on_device) {
        HIP_CHECK(pol, hipStreamSynchronize((hipStream_t)stream));
        rc = subject_best_device(c, n_hits, n_queries, false, unmatched_marker, &n_out, &n_unmatched, &n_thinned, nullptr, !active);
    } else {
        rc = with_staged_columns(pol, c, n_hits, n_queries, nullptr, 0, &n_out, [&](HitColumns& d, const uint32_t*, uint64_t* n) {
            return subject_best_device(d, n_hits, n_queries, false, unmatched_marker, n, &n_unmatched, &n_thinned, nullptr, false);
        });
    }
    if (rc != BLU_OK) return rc;
    if (n_hits_out) *n_hits_out = n_out;
    if (n_unmatched_out) *n_unmatched_out = n_unmatched;
    if (stats) { stats->n_kept = n_out; stats->n_thinned = n_thinned; }
    return BLU_OK;
}

}  // extern "C"
