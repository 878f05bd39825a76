// Minimum cover (include/blu_consensus.h: blu_hits_cover_keep, blu_hits_cover_apply): of the rows that tie on a
// query's top truncated bit-score, the ones outside the deepest taxon that still holds `need` of them are dropped, need the
// smallest integer with need * 100000 >= n * min_cover_milli.  One pass over the grouped columns, after the band and before the
// engine.
//
// The taxonomy rows sit in lexicographic lineage order, so a clade is a range of sorted positions, and a clade that holds more
// than half of the top group T holds the row m at index floor(n / 2) of T sorted by position.  The levels a row a shares with m
// are share(a, m) = min lcp8[min(pos_a, pos_m) .. max(pos_a, pos_m)) (the lineage length when the positions are equal), the
// covering depth d* is the need-th largest share, and a row of T is dropped iff share < d*.  No lineage row is read: the
// engine row ids (position | length << BLU_ROW_BITS) and the lcp8 / rmq tables of the taxonomy are all there is.
//
// Short segments (<= 64 rows): a wave takes COVER_QPW consecutive queries, one after the other, one row per lane.  The maximum
// is a wave reduction, T a ballot, m comes from rank counting over the lanes of T (a readlane per lane of T: the mask is a
// scalar, and so is the trip count), share is one range minimum per lane and d* a bisection over d with a ballot and a popcount
// per step (count(d) falls as d grows).  No LDS.
//
// Long segments (> 64 rows): the short kernel flags them; long_query_list (hit_pass.h) turns the flags into the list of long
// queries and a block takes one query of the list.  Sweeps of the segment, 256 rows at a time: the maximum; the size of T and
// the rows that leave the query alone; four digit histograms in LDS that select the position of m among the 25 position bits
// (7 + 6 + 6 + 6); a 65-bin histogram of share and its suffix sum for d*; the keep words.  Integer LDS atomics only: sums,
// maxima and ors of integers, so the outcome does not depend on scheduling.
//
// Counts: summed per wave (short) or per block (long), then added to the spread counters of hit_pass.h, whose segments,
// compaction and staging of host columns this pass uses too.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "hit_pass.h"
#include "ingest.h"

namespace blu {
namespace {

constexpr uint32_t COVER_BLOCK = 256;                // threads per block: four waves
constexpr uint32_t COVER_QPW = BLU_COVER_QUERIES_PER_WAVE;
constexpr uint32_t CNT_KEPT = 0, CNT_NARROWED = 1, CNT_UNRESOLVED = 2, CNT_LONG = 3, CNT_WORDS = 4 * HIT_SPREAD;   // spread counters
constexpr unsigned long long MILLI_ONE = 100000ull;  // 100 % in milli-percent
constexpr uint32_t POS_MASK = (1u << BLU_ROW_BITS) - 1u;
constexpr uint32_t SHARE_BINS = BLU_MAX_DEPTH + 1u;  // a share is 0 .. 64

struct CoverDev {
    const int32_t* __restrict__ bitscore;
    const uint32_t* __restrict__ tax_row;            // engine row ids, or desc rows when row_map is set
    const uint32_t* __restrict__ row_map;            // [n_tax] desc row -> engine row id, or null
    const unsigned long long* __restrict__ seg_off;
    uint64_t n_hits, n_queries;
    const uint8_t* __restrict__ lcp8;                // TaxDev::lcp8
    const uint8_t* __restrict__ rmq;                 // TaxDev::rmq
    uint32_t rmq_nb, n_tax, max_depth;
    uint32_t milli;                                  // min_cover_milli
    uint32_t* __restrict__ keep;                     // [n_hits]
    uint8_t* __restrict__ depth;                     // [n_queries] or null
    uint32_t* __restrict__ long_flag;                // [n_queries + 1]: 1 for a long segment, else 0
    const uint32_t* __restrict__ list_q;             // [n_long] the long queries (long kernel)
    uint32_t n_long;
    unsigned long long* __restrict__ counts;         // [CNT_WORDS]
};

// the engine row id of row i; *ok false: the row leaves its query alone when it is in the top group (unmatched, a desc row the
// map does not have, a bad or empty lineage, a position the taxonomy does not have, a length no lineage has)
__device__ __forceinline__ uint32_t row_id(const CoverDev& d, uint64_t i, bool* ok) {
    uint32_t id = d.tax_row[i];
    if (d.row_map && id != BLU_UNMATCHED_TAXID) {
        if (id >= d.n_tax) { *ok = false; return BLU_UNMATCHED_TAXID; }
        id = d.row_map[id];
    }
    const uint32_t pos = id & POS_MASK, len = id >> BLU_ROW_BITS;
    *ok = id != BLU_UNMATCHED_TAXID && pos < d.n_tax && len != 0u && len <= d.max_depth;
    return id;
}

// min lcp8[lo .. hi) for lo < hi < n_tax: the sparse table over 16-entry blocks for the whole blocks in between (level k entry j =
// the minimum of blocks j .. j + 2^k - 1: two overlapping entries cover any run of blocks), the entries one by one at the two
// edges.  Nothing at or beyond lcp8[n_tax - 1] — the 0xFF padding — is read.
__device__ __forceinline__ uint32_t range_min(const CoverDev& d, uint32_t lo, uint32_t hi) {
    const uint32_t b0 = (lo + 15u) >> 4, b1 = hi >> 4;   // whole blocks: b0 .. b1 - 1
    uint32_t m = 0xFFu;
    if (b0 > b1) {                                    // inside one block
        for (uint32_t i = lo; i < hi; ++i) m = min(m, (uint32_t)d.lcp8[i]);
        return m;
    }
    for (uint32_t i = lo; i < (b0 << 4); ++i) m = min(m, (uint32_t)d.lcp8[i]);
    for (uint32_t i = b1 << 4; i < hi; ++i) m = min(m, (uint32_t)d.lcp8[i]);
    if (b0 < b1) {
        const uint32_t k = 31u - (uint32_t)__clz((int)(b1 - b0));   // 2^k <= b1 - b0 < 2^(k + 1)
        m = min(m, (uint32_t)d.rmq[(uint64_t)k * d.rmq_nb + b0]);
        m = min(m, (uint32_t)d.rmq[(uint64_t)k * d.rmq_nb + b1 - (1u << k)]);
    }
    return m;
}

// the levels row `id` shares with the row at pos_m (both valid)
__device__ __forceinline__ uint32_t share_with(const CoverDev& d, uint32_t id, uint32_t pos_m) {
    const uint32_t pos = id & POS_MASK;
    const uint32_t s = pos == pos_m ? id >> BLU_ROW_BITS : range_min(d, min(pos, pos_m), max(pos, pos_m));
    return min(s, (uint32_t)BLU_MAX_DEPTH);
}

__device__ __forceinline__ uint32_t rows_needed(uint32_t n, uint32_t milli) {
    return (uint32_t)(((unsigned long long)n * milli + (MILLI_ONE - 1ull)) / MILLI_ONE);
}

__global__ __launch_bounds__(COVER_BLOCK) void cover_short_kernel(CoverDev d) {
    const uint32_t lane = threadIdx.x & 63u;
    // (the wave's number as a scalar: the offsets, the trip counts and the readlane indices below are then wave-uniform to the compiler too)
    const uint64_t wave = (uint64_t)blockIdx.x * (COVER_BLOCK / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    unsigned long long n_kept = 0, n_narrowed = 0, n_unresolved = 0, n_long = 0;   // (wave-uniform)
    for (uint32_t k = 0; k < COVER_QPW; ++k) {
        const uint64_t q = wave * COVER_QPW + k;
        if (q >= d.n_queries) break;                 // (wave-uniform)
        uint64_t s0, s1;
        segment_of(d.seg_off, q, d.n_hits, &s0, &s1);
        const uint64_t len = s1 - s0;
        const bool is_long = len > 64u;
        if (lane == 0) d.long_flag[q] = is_long ? 1u : 0u;
        if (is_long) { n_long += 1; continue; }
        uint32_t depth = BLU_NONE_U8;                // (wave-uniform)
        if (len != 0) {
            const uint32_t n_rows = (uint32_t)len;
            const bool has = lane < n_rows;
            const uint64_t i = s0 + lane;
            const int32_t b = has ? d.bitscore[i] : INT32_MIN;
            const int32_t t = wave_max32(b);
            const bool top = has && b == t;
            const unsigned long long t_mask = __ballot(top);
            const uint32_t n = (uint32_t)__popcll(t_mask);
            bool ok = true;
            const uint32_t id = top ? row_id(d, i, &ok) : 0u;
            const bool alone = __ballot(top && !ok) != 0ull;
            bool keep = has;
            if (n > 1u && alone) n_unresolved += 1;
            if (n > 1u && !alone) {
                // the row of T at index n / 2 in the order (position, lane)
                const uint32_t pos = id & POS_MASK;
                uint32_t rank = 0;
                for (unsigned long long rest = t_mask; rest; rest &= rest - 1ull) {
                    const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane(__ffsll((long long)rest) - 1);
                    const uint32_t pos_r = (uint32_t)__builtin_amdgcn_readlane((int)pos, (int)r);
                    rank += (pos_r < pos || (pos_r == pos && r < lane)) ? 1u : 0u;
                }
                const unsigned long long m_mask = __ballot(top && rank == n / 2u);   // (one lane: the ranks of T are 0 .. n - 1)
                const uint32_t m_lane = (uint32_t)__builtin_amdgcn_readfirstlane(__ffsll((long long)m_mask) - 1);
                const uint32_t pos_m = (uint32_t)__builtin_amdgcn_readlane((int)pos, (int)m_lane);
                const uint32_t share = top ? share_with(d, id, pos_m) : 0u;
                const uint32_t need = rows_needed(n, d.milli);
                uint32_t lo = 0, hi = SHARE_BINS;    // count(lo) >= need > count(hi): count(0) = n, count(65) = 0
                while (hi - lo > 1u) {
                    const uint32_t mid = (lo + hi) / 2u;
                    if ((uint32_t)__popcll(__ballot(top && share >= mid)) >= need) lo = mid; else hi = mid;
                }
                depth = lo;
                keep = has && (!top || share >= lo);
            }
            if (has) d.keep[i] = keep ? 1u : 0u;
            const unsigned long long kept = (unsigned long long)__popcll(__ballot(keep));
            n_kept += kept;
            n_narrowed += kept < n_rows ? 1ull : 0ull;
        }
        if (d.depth && lane == 0) d.depth[q] = (uint8_t)depth;
    }
    if (lane == 0) {
        spread_add(d.counts, CNT_KEPT, n_kept); spread_add(d.counts, CNT_NARROWED, n_narrowed);
        spread_add(d.counts, CNT_UNRESOLVED, n_unresolved); spread_add(d.counts, CNT_LONG, n_long);
    }
}

// digits of the radix selection over the BLU_ROW_BITS position bits, most significant first: 7 + 6 + 6 + 6
constexpr uint32_t SEL_PASSES = 4, SEL_BINS = 128;
__device__ __forceinline__ uint32_t sel_shift(uint32_t p) { return 18u - 6u * p; }
__device__ __forceinline__ uint32_t sel_bins(uint32_t p) { return p == 0 ? 128u : 64u; }

__global__ __launch_bounds__(COVER_BLOCK) void cover_long_kernel(CoverDev d) {
    __shared__ int s_max;
    __shared__ uint32_t s_n, s_alone, s_dropped;
    __shared__ uint32_t s_hist[SEL_BINS];
    __shared__ uint32_t s_prefix, s_target, s_depth;
    const uint32_t tid = threadIdx.x;
    if (blockIdx.x >= d.n_long) return;              // (block-uniform)
    const uint32_t q = d.list_q[blockIdx.x];
    if (q >= d.n_queries) return;                    // (block-uniform; the list was made from these queries: never)
    uint64_t s0, s1;
    segment_of(d.seg_off, q, d.n_hits, &s0, &s1);
    if (tid == 0) { s_max = INT32_MIN; s_n = 0; s_alone = 0; s_dropped = 0; s_prefix = 0; }
    if (tid < SEL_BINS) s_hist[tid] = 0;
    __syncthreads();
    int32_t mx = INT32_MIN;
    for (uint64_t i = s0 + tid; i < s1; i += COVER_BLOCK) mx = max(mx, d.bitscore[i]);
    mx = wave_max32(mx);
    if ((tid & 63u) == 0) atomicMax(&s_max, mx);
    __syncthreads();
    const int32_t t = s_max;
    // the size of T, and whether one of its rows leaves the query alone
    {
        uint32_t n_mine = 0, bad_mine = 0;
        for (uint64_t i = s0 + tid; i < s1; i += COVER_BLOCK) {
            if (d.bitscore[i] != t) continue;
            bool ok;
            (void)row_id(d, i, &ok);
            n_mine += 1; bad_mine |= ok ? 0u : 1u;
        }
        if (n_mine) atomicAdd(&s_n, n_mine);
        if (bad_mine) atomicOr(&s_alone, 1u);
    }
    __syncthreads();
    const uint32_t n = s_n;
    const bool alone = s_alone != 0u;
    const uint64_t n_rows = s1 - s0;
    if (n <= 1u || alone) {                          // (block-uniform) the query stays as it is
        for (uint64_t i = s0 + tid; i < s1; i += COVER_BLOCK) d.keep[i] = 1u;
        if (tid == 0) {
            spread_add(d.counts, CNT_KEPT, (unsigned long long)n_rows);
            spread_add(d.counts, CNT_UNRESOLVED, n > 1u ? 1ull : 0ull);
            if (d.depth) d.depth[q] = (uint8_t)BLU_NONE_U8;
        }
        return;
    }
    // the position of the row of T at index n / 2 by position: one digit a pass, the rows whose higher digits are the chosen ones
    if (tid == 0) s_target = n / 2u;
    __syncthreads();
    for (uint32_t p = 0; p < SEL_PASSES; ++p) {
        const uint32_t shift = sel_shift(p), bins = sel_bins(p), prefix = s_prefix;
        for (uint64_t i = s0 + tid; i < s1; i += COVER_BLOCK) {
            if (d.bitscore[i] != t) continue;
            bool ok;
            const uint32_t pos = row_id(d, i, &ok) & POS_MASK;
            if (p != 0 && (pos >> (shift + 6u)) != (prefix >> (shift + 6u))) continue;
            atomicAdd(&s_hist[(pos >> shift) & (bins - 1u)], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            uint32_t left = s_target, dgt = 0;
            while (dgt + 1u < bins && left >= s_hist[dgt]) { left -= s_hist[dgt]; ++dgt; }
            s_target = left;
            s_prefix = prefix | (dgt << shift);
        }
        __syncthreads();
        if (tid < SEL_BINS) s_hist[tid] = 0;
        __syncthreads();
    }
    const uint32_t pos_m = s_prefix;
    // the histogram of share (s_hist has SEL_BINS >= SHARE_BINS words, all zero here), its suffix sum, d*
    for (uint64_t i = s0 + tid; i < s1; i += COVER_BLOCK) {
        if (d.bitscore[i] != t) continue;
        bool ok;
        const uint32_t id = row_id(d, i, &ok);
        atomicAdd(&s_hist[share_with(d, id, pos_m)], 1u);
    }
    __syncthreads();
    if (tid == 0) {
        const uint32_t need = rows_needed(n, d.milli);
        uint32_t dd = SHARE_BINS, sum = 0;
        while (dd > 0u && sum < need) { --dd; sum += s_hist[dd]; }
        s_depth = dd;
    }
    __syncthreads();
    const uint32_t depth = s_depth;
    uint32_t dropped = 0;
    for (uint64_t i = s0 + tid; i < s1; i += COVER_BLOCK) {
        bool keep = true;
        if (d.bitscore[i] == t) {
            bool ok;
            const uint32_t id = row_id(d, i, &ok);
            keep = share_with(d, id, pos_m) >= depth;
        }
        d.keep[i] = keep ? 1u : 0u;
        dropped += keep ? 0u : 1u;
    }
    if (dropped) atomicAdd(&s_dropped, dropped);
    __syncthreads();
    if (tid == 0) {
        spread_add(d.counts, CNT_KEPT, (unsigned long long)(n_rows - s_dropped));
        spread_add(d.counts, CNT_NARROWED, s_dropped ? 1ull : 0ull);
        if (d.depth) d.depth[q] = (uint8_t)depth;
    }
}

}  // namespace

int check_min_cover(int64_t min_cover_milli) {
    if (min_cover_milli < 50001 || min_cover_milli > 100000) {
        set_error("min cover: min_cover_milli must be 50001 .. 100000 (above 50 %%, at most 100 %%), not %lld", (long long)min_cover_milli);
        return BLU_ERR_INVALID_ARG;
    }
    return BLU_OK;
}

int cover_keep_device(const blu_taxonomy* tax, const int32_t* d_bitscore, const uint32_t* d_tax_row, const uint32_t* d_row_map,
                      const uint64_t* d_seg_off, uint64_t n_hits, uint64_t n_queries, uint32_t min_cover_milli, uint32_t* d_keep,
                      uint8_t* d_depth, blu_min_cover_stats* stats) {
    HipPolicy pol{"min cover", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    *stats = blu_min_cover_stats{n_hits, 0, n_queries, 0, 0};
    if (n_hits) HIP_CHECK(pol, hipMemsetAsync(d_keep, 0, n_hits * 4, nullptr));   // (a row that no segment names is dropped)
    if (d_depth && n_queries) HIP_CHECK(pol, hipMemsetAsync(d_depth, BLU_NONE_U8, n_queries, nullptr));
    if (n_hits == 0 || n_queries == 0) { HIP_CHECK(pol, hipStreamSynchronize(nullptr)); return BLU_OK; }
    const uint64_t waves = (n_queries + COVER_QPW - 1) / COVER_QPW;
    const uint64_t blocks = (waves + COVER_BLOCK / 64 - 1) / (COVER_BLOCK / 64);
    unsigned long long* d_counts = nullptr;
    uint32_t* d_flag = nullptr;
    unsigned long long counts[CNT_WORDS];
    HIP_CHECK(pol, mem.alloc(&d_counts, sizeof counts, "counts"));
    HIP_CHECK(pol, mem.alloc(&d_flag, (n_queries + 1) * 4, "long flags"));
    HIP_CHECK(pol, hipMemsetAsync(d_counts, 0, sizeof counts, nullptr));
    CoverDev d{};
    d.bitscore = d_bitscore; d.tax_row = d_tax_row; d.row_map = d_row_map; d.seg_off = (const unsigned long long*)d_seg_off;
    d.n_hits = n_hits; d.n_queries = n_queries;
    d.lcp8 = tax->d_lcp8; d.rmq = tax->d_rmq; d.rmq_nb = tax->rmq_nb; d.n_tax = (uint32_t)tax->n_tax; d.max_depth = tax->max_depth;
    d.milli = min_cover_milli; d.keep = d_keep; d.depth = d_depth; d.long_flag = d_flag; d.counts = d_counts;
    hipLaunchKernelGGL(cover_short_kernel, dim3((unsigned)blocks), dim3(COVER_BLOCK), 0, nullptr, d);
    HIP_CHECK(pol, hipGetLastError());
    HIP_CHECK(pol, hipMemcpy(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost));
    const uint64_t n_long = spread_sum(counts, CNT_LONG);
    if (n_long) {
        uint32_t* d_list_q = nullptr;
        void* d_tmp = nullptr;
        HIP_CHECK(pol, mem.alloc(&d_tmp, scan_tmp_bytes_u32(n_queries + 1), "scan work"));
        if (const int rc = long_query_list(pol, mem, d_flag, n_queries, n_long, nullptr, d_tmp, &d_list_q, nullptr)) return rc;
        d.list_q = d_list_q; d.n_long = (uint32_t)n_long;
        hipLaunchKernelGGL(cover_long_kernel, dim3((unsigned)n_long), dim3(COVER_BLOCK), 0, nullptr, d);
        HIP_CHECK(pol, hipGetLastError());
        HIP_CHECK(pol, hipMemcpy(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost));
    }
    stats->n_kept = spread_sum(counts, CNT_KEPT); stats->n_narrowed = spread_sum(counts, CNT_NARROWED); stats->n_unresolved = spread_sum(counts, CNT_UNRESOLVED);
    return BLU_OK;
}

int cover_apply_device(const blu_taxonomy* tax, HitColumns& c, const uint32_t* d_row_map, uint64_t n_hits, uint64_t n_queries,
                       uint32_t min_cover_milli, bool rotate, uint32_t unmatched_marker, uint64_t* n_hits_out, uint64_t* n_unmatched,
                       blu_min_cover_stats* stats, std::vector<void*>* retired) {
    HipPolicy pol{"min cover", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    *n_hits_out = n_hits;
    *stats = blu_min_cover_stats{n_hits, n_hits, n_queries, 0, 0};
    if (n_hits == 0) return compact_kept_device("min cover", c, 0, n_queries, nullptr, true, rotate, unmatched_marker, n_hits_out, n_unmatched, retired);
    uint32_t* d_keep = nullptr;
    HIP_CHECK(pol, mem.alloc(&d_keep, (n_hits + 1) * 4, "keep words"));
    HIP_CHECK(pol, hipMemsetAsync(d_keep + n_hits, 0, 4, nullptr));
    int rc = cover_keep_device(tax, *c.bitscore, *c.tax_desc_row, d_row_map, (const uint64_t*)c.seg_off, n_hits, n_queries, min_cover_milli,
                               d_keep, nullptr, stats);
    if (rc != BLU_OK) return rc;
    return compact_kept_device("min cover", c, n_hits, n_queries, d_keep, stats->n_kept == n_hits, rotate, unmatched_marker, n_hits_out,
                               n_unmatched, retired);
}

int cover_hits(const blu_taxonomy* tax, DeviceHits& dev, const uint32_t* fwd, uint64_t n_tax, uint32_t min_cover_milli,
               blu_min_cover_stats* stats, uint64_t* unmatched) {
    *stats = blu_min_cover_stats{dev.n_hits, dev.n_hits, dev.n_queries, 0, 0};
    if (int rc = check_hit_counts("min cover", dev.n_hits, dev.n_queries)) return rc;
    if (n_tax != tax->n_tax) { set_error("min cover: the row map has %llu rows, the taxonomy %llu", (unsigned long long)n_tax, (unsigned long long)tax->n_tax); return BLU_ERR_INVALID_ARG; }
    if (int rc = use_device("min cover", dev.device)) return rc;
    HipPolicy pol{"min cover", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    struct ToTrash { DeviceArena& mem; DeviceHits& dev; ~ToTrash() { mem.hand_over(dev.trash); } } to_trash{mem, dev};
    uint32_t* d_map = nullptr;
    HIP_CHECK(pol, mem.upload(&d_map, fwd, n_tax, "row map"));
    HitColumns c = columns_of(dev);
    uint64_t n_out = dev.n_hits;
    const int rc = cover_apply_device(tax, c, d_map, dev.n_hits, dev.n_queries, min_cover_milli, true, BLU_UNMATCHED_TAXID, &n_out, unmatched,
                                      stats, &dev.trash);
    if (rc != BLU_OK) return rc;
    dev.n_hits = n_out;
    return BLU_OK;
}

}  // namespace blu

using namespace blu;

namespace {

// the refusals both calls share, before any device is asked for
int cover_refusals(const char* who, const blu_taxonomy* tax, bool null_array, uint64_t n_hits, uint64_t n_queries, uint32_t min_cover_milli) {
    if (int rc = check_min_cover((int64_t)min_cover_milli)) return rc;
    if (!tax) { set_error("%s: null taxonomy handle", who); return BLU_ERR_INVALID_ARG; }
    if (null_array) return refuse_null_array(who);
    if (int rc = check_hit_counts("min cover", n_hits, n_queries)) return rc;
    if (tax->device < 0) { set_error("host-only taxonomy handle: %s needs a HIP device (no CPU fallback)", who); return BLU_ERR_NO_DEVICE; }
    return BLU_OK;
}

}  // namespace

extern "C" {

int blu_hits_cover_keep(const blu_taxonomy* tax, const int32_t* bitscore, const uint32_t* tax_row, const uint32_t* row_map,
                        const uint64_t* seg_off, uint64_t n_hits, uint64_t n_queries, int on_device, uint32_t min_cover_milli, void* stream,
                        uint32_t* keep_out, uint8_t* depth_out, blu_min_cover_stats* stats) {
    if (stats) *stats = blu_min_cover_stats{n_hits, 0, n_queries, 0, 0};
    int rc = cover_refusals("blu_hits_cover_keep", tax, (n_hits && (!bitscore || !tax_row || !keep_out)) || (n_queries && !seg_off), n_hits, n_queries,
                            min_cover_milli);
    if (rc != BLU_OK) return rc;
    if ((rc = use_device("blu_hits_cover_keep", tax->device)) != BLU_OK) return rc;
    HipPolicy pol{"blu_hits_cover_keep", BLU_ERR_ALLOC};
    blu_min_cover_stats st{};
    if (on_device) {
        HIP_CHECK(pol, hipStreamSynchronize((hipStream_t)stream));
        rc = cover_keep_device(tax, bitscore, tax_row, row_map, seg_off, n_hits, n_queries, min_cover_milli, keep_out, depth_out, &st);
    } else {
        // host pointers: the two columns, the map and the offsets go up, the same kernels run, the verdicts come back
        DeviceArena mem(pol);
        int32_t* d_bs = nullptr;
        uint32_t *d_tax = nullptr, *d_map = nullptr, *d_keep = nullptr;
        uint64_t* d_seg = nullptr;
        uint8_t* d_depth = nullptr;
        HIP_CHECK(pol, mem.upload(&d_bs, bitscore, n_hits, "bit-scores"));
        HIP_CHECK(pol, mem.upload(&d_tax, tax_row, n_hits, "taxonomy rows"));
        HIP_CHECK(pol, mem.alloc(&d_keep, n_hits * 4, "keep words"));
        HIP_CHECK(pol, mem.upload(&d_seg, seg_off, n_queries ? n_queries + 1 : 0, "offsets"));
        if (row_map) HIP_CHECK(pol, mem.upload(&d_map, row_map, tax->n_tax, "row map"));
        if (depth_out) HIP_CHECK(pol, mem.alloc(&d_depth, n_queries, "depths"));
        rc = cover_keep_device(tax, d_bs, d_tax, d_map, d_seg, n_hits, n_queries, min_cover_milli, d_keep, d_depth, &st);
        if (rc == BLU_OK) HIP_CHECK(pol, mem.download(keep_out, d_keep, n_hits));
        if (rc == BLU_OK && depth_out) HIP_CHECK(pol, mem.download(depth_out, d_depth, n_queries));
    }
    if (rc != BLU_OK) return rc;
    if (stats) *stats = st;
    return BLU_OK;
}

int blu_hits_cover_apply(const blu_taxonomy* tax, int32_t* bitscore, int32_t* align_len, uint32_t* tax_row, uint32_t* acc_rank, double* pident,
                         const uint32_t* row_map, uint64_t* seg_off, uint64_t n_hits, uint64_t n_queries, int on_device,
                         uint32_t min_cover_milli, void* stream, uint32_t unmatched_marker, uint64_t* n_hits_out, uint64_t* n_unmatched_out,
                         blu_min_cover_stats* stats) {
    if (stats) *stats = blu_min_cover_stats{n_hits, n_hits, n_queries, 0, 0};
    if (n_hits_out) *n_hits_out = n_hits;
    int rc = cover_refusals("blu_hits_cover_apply", tax,
                            (n_hits && (!bitscore || !align_len || !tax_row || !acc_rank || !pident)) || (n_queries && !seg_off), n_hits, n_queries,
                            min_cover_milli);
    if (rc != BLU_OK) return rc;
    HitColumns c{&bitscore, &align_len, &tax_row, &acc_rank, &pident, (unsigned long long*)seg_off};
    if (on_device && (rc = check_aligned16("blu_hits_cover_apply", c)) != BLU_OK) return rc;
    if ((rc = use_device("blu_hits_cover_apply", tax->device)) != BLU_OK) return rc;
    HipPolicy pol{"blu_hits_cover_apply", BLU_ERR_ALLOC};
    uint64_t n_out = n_hits, n_unmatched = 0;
    blu_min_cover_stats st{};
    if (on_device) {
        HIP_CHECK(pol, hipStreamSynchronize((hipStream_t)stream));
        rc = cover_apply_device(tax, c, row_map, n_hits, n_queries, min_cover_milli, false, unmatched_marker, &n_out, &n_unmatched, &st, nullptr);
    } else {
        rc = with_staged_columns(pol, c, n_hits, n_queries, row_map, tax->n_tax, &n_out, [&](HitColumns& d, const uint32_t* d_map, uint64_t* n) {
            return cover_apply_device(tax, d, d_map, n_hits, n_queries, min_cover_milli, false, unmatched_marker, n, &n_unmatched, &st, nullptr);
        });
    }
    if (rc != BLU_OK) return rc;
    if (n_hits_out) *n_hits_out = n_out;
    if (n_unmatched_out) *n_unmatched_out = n_unmatched;
    if (stats) { *stats = st; stats->n_kept = n_out; }
    return BLU_OK;
}

}  // extern "C"
