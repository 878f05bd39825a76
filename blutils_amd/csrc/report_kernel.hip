// Taxon abundance report (include/blu_consensus.h: blu_consensus_report): the per-query records of the engine ->
// the distinct taxonomy paths with their direct counts, on the device.
//
// A query's path is exactly what the renderer writes as `taxonomy` (pipeline_render.cpp, Renderer::lineage): the levels j of
// the lineage row of tax_row[ref_row] whose bit is set in level_mask.  Paths are interned in one open-addressing table
// keyed by (parent path id << 32 | node id): the slot a key lands in IS the path id, so a path's parent is named by
// its key and nothing else has to be stored.  Every query walks its own levels; a probe that finds its key is a load
// and no atomic, so the few-species case (millions of queries on ~10 paths) reads a handful of hot lines.
//
// Direct counts are u64 integer sums (deterministic).  They are pre-aggregated per block in an LDS table (Guideline 12):
// a block of 1 024 queries adds each distinct leaf to global memory once, so a hot leaf costs one global atomic per
// block instead of one per query.  Clade sums, sibling order and text are host work over the distinct paths.
//
// Table size: a query reaches at most popcount(level_mask) paths, so P = sum over classified queries of popcount is a
// bound on the distinct paths.  The first attempt sizes the table from min(n_queries * max_depth, 2 n_tax + 4 096) (both
// read off the handle, no pass over the records) at load <= 1/2 and
// gives up (flag) on a probe longer than REPORT_PROBE_FIRST; the table is then rebuilt from zero at 2 P slots, where a
// probe always ends (load <= 1/2).  No count is ever dropped: a table that cannot be allocated is BLU_ERR_ALLOC.
//
// The per-sample table (sample_cells) and the table from count rows (count_cells) are counted here too, and the three share
// what is not their own counting: the two cell kernels decode_record (what a record is) and their LDS cell table; all
// three report_compact, TableRun (the tables, the attempt loop, flag_error), compact_table and parents_first on the way
// back, and entry_begin / stage_records in front of the three C entries.  report_paths spells the decode and the walk out
// (see there).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "blu_internal.h"
#include "ingest_prims.h"

namespace blu {
namespace {

constexpr unsigned long long REPORT_EMPTY = ~0ull;
constexpr uint32_t REPORT_NONE = 0xFFFFFFFFu;   // parent of a first-level path
constexpr uint32_t RB = 256;                    // threads per block
constexpr uint32_t RQ = 4;                      // queries per thread
constexpr uint32_t LDS_SLOTS = 2048;            // block-local leaf table (24 KB)
constexpr uint32_t LDS_PROBE = 8;
constexpr uint32_t REPORT_PROBE_FIRST = 128;
// ctl[2]: OVERFLOW starts the next attempt, the others refuse the call (flag_error).  BAD_SAMPLE is the two cell kernels',
// BAD_ROW count_cells'.
constexpr uint32_t FLAG_OVERFLOW = 1u, FLAG_BAD_RECORD = 2u, FLAG_BAD_SAMPLE = 4u, FLAG_BAD_ROW = 8u, FLAG_BAD_NODE = 16u;
constexpr uint32_t CTL_WORDS = 7, CTL_BAD_NODE = 6;   // ctl[]: what every entry point allocates and clears

struct ReportDev {
    const uint32_t* lin;          // TaxDev rows
    uint64_t n_tax;
    uint32_t stride, node_base, max_depth;
    const blu_result* recs;
    uint64_t n_queries;
    const uint32_t* row_src;      // engine row ids: row_src[idx * row_stride], idx = ref_row (or q when by_query)
    uint64_t n_rows;
    uint32_t row_stride;
    uint32_t by_query;
    const uint32_t* weight;       // [n_queries] or null (= 1)
    unsigned long long* keys;     // [cap]
    unsigned long long* direct;   // [cap]
    uint32_t cap_mask;
    uint32_t max_probe;
    // [CTL_WORDS] {unclassified, unplaced, flags, the query of a bad record, of a bad sample, of a bad row, of a bad node}
    unsigned long long* ctl;
};

__device__ __forceinline__ uint32_t mix_key(unsigned long long k) {   // murmur3 fmix64
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (uint32_t)k;
}

// slot of (parent, node), inserted if new; REPORT_NONE when max_probe slots were all taken by other keys.  The key of a
// first-level node 0xFFFFFFFF would be REPORT_EMPTY itself (an empty slot would read as found): the walks refuse that
// node before they come here (reserved_first).
__device__ __forceinline__ uint32_t intern(const ReportDev& d, uint32_t parent, uint32_t node) {
    const unsigned long long key = ((unsigned long long)parent << 32) | node;
    uint32_t h = mix_key(key) & d.cap_mask;
    for (uint32_t p = 0; p < d.max_probe; ++p, h = (h + 1) & d.cap_mask) {
        // a key goes EMPTY -> key once: a stale read can only be EMPTY, and the CAS then tells the truth
        const unsigned long long cur = d.keys[h];
        if (cur == key) return h;
        if (cur != REPORT_EMPTY) continue;
        const unsigned long long prev = atomicCAS(d.keys + h, REPORT_EMPTY, key);
        if (prev == REPORT_EMPTY || prev == key) return h;
    }
    return REPORT_NONE;
}

__device__ __forceinline__ bool reserved_first(uint32_t parent, uint32_t node) { return (parent & node) == REPORT_NONE; }

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// What record q is.  REC_NO_TAXON: taxon null (status >= 2); REC_BAD: a taxon, but its reference row names no taxonomy row;
// REC_NO_LEVEL: taxonomy "" (no selected level inside the lineage); REC_PATH: lin is the lineage row, len its length cut to
// max_depth, m the level mask cut to len (not 0).  The flag and ctl[] of a bad record are the caller's to write.
enum RecordKind : uint32_t { REC_NO_TAXON, REC_BAD, REC_NO_LEVEL, REC_PATH };
struct Record {
    RecordKind kind;
    const uint32_t* lin;
    uint32_t len;
    unsigned long long m;
};

__device__ __forceinline__ Record decode_record(const ReportDev& d, uint64_t q) {
    const uint4* rp = reinterpret_cast<const uint4*>(d.recs + q);
    const uint4 a = rp[0], b = rp[1];
    const uint32_t status = a.x & 0xFFu;
    const uint32_t ref_row = a.w;
    const unsigned long long mask = (unsigned long long)b.x | ((unsigned long long)b.y << 32);
    if (status >= 2) return {REC_NO_TAXON, nullptr, 0, 0};
    const uint64_t idx = d.by_query ? q : (uint64_t)ref_row;
    uint32_t row = REPORT_NONE;
    if (idx < d.n_rows) row = d.row_src[idx * d.row_stride];
    const uint32_t pos = row & ((1u << BLU_ROW_BITS) - 1u);
    if (row == BLU_UNMATCHED_TAXID || pos >= d.n_tax) return {REC_BAD, nullptr, 0, 0};
    const uint32_t* lin = d.lin + (uint64_t)pos * d.stride;
    const uint32_t len = min(lin[0] & 0xFFu, d.max_depth);
    const unsigned long long m = len >= 64 ? mask : mask & ((1ull << len) - 1ull);
    return {m ? REC_PATH : REC_NO_LEVEL, lin, len, m};
}

// One lane's walk (sample_cells): the selected levels of a REC_PATH record interned in turn, each(path id) called for every
// one reached.
// stopped: 0 and `leaf` is the id of the last level, or the flag that ended the walk (FLAG_BAD_NODE, FLAG_OVERFLOW).
struct Walk { uint32_t leaf, stopped; };

template <class Each>
__device__ __forceinline__ Walk walk_levels(const ReportDev& d, const Record& r, Each&& each) {
    uint32_t path = REPORT_NONE;
    for (uint32_t j = 0; j < r.len; ++j) {
        if (!((r.m >> j) & 1ull)) continue;
        const uint32_t node = r.lin[d.node_base + j];
        if (reserved_first(path, node)) return {REPORT_NONE, FLAG_BAD_NODE};
        path = intern(d, path, node);
        if (path == REPORT_NONE) return {REPORT_NONE, FLAG_OVERFLOW};
        each(path);
    }
    return {path, 0u};
}

// The decode and the walk are written out here, not taken from decode_record / walk_levels: around the helpers the
// compiler lays the four-query loop out with more branches and waits (or does not unroll it), and this kernel, the hottest
// of the file, measured 1 to 9 % slower.  A change to the record layout or the refusal rules is made here and in decode_record.
__global__ __launch_bounds__(RB) void report_paths(ReportDev d) {
    __shared__ uint32_t s_key[LDS_SLOTS];
    __shared__ unsigned long long s_cnt[LDS_SLOTS];
    __shared__ unsigned long long s_un[2];
    for (uint32_t i = threadIdx.x; i < LDS_SLOTS; i += RB) { s_key[i] = REPORT_NONE; s_cnt[i] = 0; }
    if (threadIdx.x < 2) s_un[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long un = 0, np = 0;
    uint32_t flags = 0;
    const uint64_t base = (uint64_t)blockIdx.x * (RB * RQ) + threadIdx.x;
    for (uint32_t k = 0; k < RQ; ++k) {
        const uint64_t q = base + (uint64_t)k * RB;
        if (q >= d.n_queries) break;
        const uint4* rp = reinterpret_cast<const uint4*>(d.recs + q);
        const uint4 a = rp[0], b = rp[1];
        const uint32_t status = a.x & 0xFFu;
        const uint32_t ref_row = a.w;
        const unsigned long long mask = (unsigned long long)b.x | ((unsigned long long)b.y << 32);
        const unsigned long long w = d.weight ? (unsigned long long)d.weight[q] : 1ull;
        if (status >= 2) { un += w; continue; }                       // taxon: null
        const uint64_t idx = d.by_query ? q : (uint64_t)ref_row;
        uint32_t row = REPORT_NONE;
        if (idx < d.n_rows) row = d.row_src[idx * d.row_stride];
        const uint32_t pos = row & ((1u << BLU_ROW_BITS) - 1u);
        if (row == BLU_UNMATCHED_TAXID || pos >= d.n_tax) { flags |= FLAG_BAD_RECORD; d.ctl[3] = q; continue; }
        const uint32_t* lin = d.lin + (uint64_t)pos * d.stride;
        const uint32_t len = min(lin[0] & 0xFFu, d.max_depth);
        const unsigned long long m = len >= 64 ? mask : mask & ((1ull << len) - 1ull);
        if (m == 0) { np += w; continue; }                             // taxonomy: ""
        uint32_t path = REPORT_NONE;
        bool ok = true;
        for (uint32_t j = 0; j < len; ++j) {
            if (!((m >> j) & 1ull)) continue;
            const uint32_t node = lin[d.node_base + j];
            if (reserved_first(path, node)) { flags |= FLAG_BAD_NODE; d.ctl[CTL_BAD_NODE] = q; ok = false; break; }
            path = intern(d, path, node);
            if (path == REPORT_NONE) { flags |= FLAG_OVERFLOW; ok = false; break; }
        }
        if (!ok) continue;
        // direct count of the leaf: block-local table first, global memory when it is crowded
        uint32_t h = (path * 2654435761u) >> 21;                        // 11 bits: LDS_SLOTS
        bool done = false;
        for (uint32_t p = 0; p < LDS_PROBE && !done; ++p, h = (h + 1) & (LDS_SLOTS - 1)) {
            uint32_t cur = s_key[h];
            if (cur == REPORT_NONE) {
                cur = atomicCAS(s_key + h, REPORT_NONE, path);
                if (cur == REPORT_NONE) cur = path;
            }
            if (cur == path) { atomicAdd(s_cnt + h, w); done = true; }
        }
        if (!done) atomicAdd(d.direct + path, w);
    }
    un = wave_sum(un);
    np = wave_sum(np);
    if ((threadIdx.x & 63) == 0 && (un | np)) { atomicAdd(&s_un[0], un); atomicAdd(&s_un[1], np); }
    if (flags) atomicOr(reinterpret_cast<unsigned int*>(d.ctl + 2), flags);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < LDS_SLOTS; i += RB)
        if (s_key[i] != REPORT_NONE && s_cnt[i]) atomicAdd(d.direct + s_key[i], s_cnt[i]);
    if (threadIdx.x == 0) {
        if (s_un[0]) atomicAdd(d.ctl + 0, s_un[0]);
        if (s_un[1]) atomicAdd(d.ctl + 1, s_un[1]);
    }
}

// P: sum of popcount(level_mask) over the classified queries (the retry's table bound)
__global__ __launch_bounds__(RB) void report_bound(const blu_result* __restrict__ recs, uint64_t n_queries,
                                                   unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s;
    if (threadIdx.x == 0) s = 0;
    __syncthreads();
    unsigned long long c = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * RB + threadIdx.x; q < n_queries; q += (uint64_t)gridDim.x * RB) {
        const blu_result& r = recs[q];
        if (r.status < 2) c += (unsigned long long)__popcll(r.level_mask);
    }
    c = wave_sum(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s, c);
    __syncthreads();
    if (threadIdx.x == 0 && s) atomicAdd(out, s);
}

__global__ void report_flags(const unsigned long long* __restrict__ keys, uint64_t cap, uint32_t* __restrict__ used) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cap) used[i] = keys[i] != REPORT_EMPTY ? 1u : 0u;
    else if (i == cap) used[i] = 0;
}

// the occupied path slots in slot order, parents renamed to their index in that order; direct null (the per-sample tables
// count in cells): 0
__global__ void report_compact(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ direct,
                               const uint32_t* __restrict__ at, uint64_t cap, blu_report_path* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    const unsigned long long k = keys[i];
    if (k == REPORT_EMPTY) return;
    const uint32_t parent = (uint32_t)(k >> 32);
    blu_report_path p;
    p.node = (uint32_t)k;
    p.parent = parent == REPORT_NONE ? REPORT_NONE : at[parent];
    p.direct = direct ? direct[i] : 0;
    p.clade = 0;
    out[at[i]] = p;
}

// ---- per-sample table (blu_consensus_sample_table) -------------------------------------------------------
// One walk per query, as report_paths: every prefix path p of the query's path is interned in the report's path table and
// the query's weight goes to the cell (p, sample), so a cell is a clade count with no roll-up.  Cells live in a second
// open-addressing table keyed (path id << 32 | sample id), u64 integer adds.  Each block pre-aggregates its cells in LDS
// first: a pooled file is per-sample files back to back, so a block of consecutive queries mostly shares one sample and
// its upper levels.  The per-sample unclassified / unplaced counts travel through the same LDS table under two path ids
// no path table reaches (the tables are limited to 2^31 slots).
constexpr uint32_t CELL_UNCLASSIFIED = 0xFFFFFFFEu, CELL_UNPLACED = 0xFFFFFFFDu;
constexpr uint32_t CELL_LDS_SLOTS = 2048;       // block-local cell table (32 KB)

struct SampleDev {
    ReportDev r;                    // the report's walk and path table (r.direct is not used)
    const uint32_t* sample_of;      // [n_queries]
    uint32_t n_samples;
    uint32_t cell_mask;
    unsigned long long* cell_keys;  // [cell_mask + 1]
    unsigned long long* cell_val;   // [cell_mask + 1]
    unsigned long long* fixed;      // [2 n_samples]: unclassified per sample, then unplaced per sample
};

// adds w to a cell of the global table; false when max_probe slots were all taken by other keys
__device__ __forceinline__ bool cell_add(const SampleDev& d, unsigned long long key, unsigned long long w) {
    uint32_t h = mix_key(key) & d.cell_mask;
    for (uint32_t p = 0; p < d.r.max_probe; ++p, h = (h + 1) & d.cell_mask) {
        unsigned long long cur = d.cell_keys[h];
        if (cur == REPORT_EMPTY) {
            cur = atomicCAS(d.cell_keys + h, REPORT_EMPTY, key);
            if (cur == REPORT_EMPTY) cur = key;
        }
        if (cur == key) { atomicAdd(d.cell_val + h, w); return true; }
    }
    return false;
}

// a block's sum for one key reaches global memory: the fixed rows' arrays, or the cell table
__device__ __forceinline__ uint32_t cell_flush(const SampleDev& d, unsigned long long key, unsigned long long w) {
    const uint32_t path = (uint32_t)(key >> 32), s = (uint32_t)key;
    if (path == CELL_UNCLASSIFIED) { atomicAdd(d.fixed + s, w); return 0; }
    if (path == CELL_UNPLACED) { atomicAdd(d.fixed + d.n_samples + s, w); return 0; }
    return cell_add(d, key, w) ? 0u : FLAG_OVERFLOW;
}

// adds w to a cell of the block's LDS table, or of global memory when that is crowded; the flags of a global add that failed
__device__ __forceinline__ uint32_t block_cell_add(unsigned long long* s_key, unsigned long long* s_cnt, const SampleDev& d,
                                                   uint32_t path, uint32_t s, unsigned long long w) {
    const unsigned long long key = ((unsigned long long)path << 32) | s;
    uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 53);   // 11 bits: CELL_LDS_SLOTS
    for (uint32_t p = 0; p < LDS_PROBE; ++p, h = (h + 1) & (CELL_LDS_SLOTS - 1)) {
        unsigned long long cur = s_key[h];
        if (cur == REPORT_EMPTY) {
            cur = atomicCAS(s_key + h, REPORT_EMPTY, key);
            if (cur == REPORT_EMPTY) cur = key;
        }
        if (cur == key) { atomicAdd(s_cnt + h, w); return 0; }
    }
    return cell_flush(d, key, w);
}

// a cell kernel begins: the block's LDS table empty
__device__ __forceinline__ void block_cells_clear(unsigned long long* s_key, unsigned long long* s_cnt) {
    for (uint32_t i = threadIdx.x; i < CELL_LDS_SLOTS; i += RB) { s_key[i] = REPORT_EMPTY; s_cnt[i] = 0; }
    __syncthreads();
}

// ... and ends: the block's sums reach global memory, the thread's flags ctl[2]
__device__ __forceinline__ void block_cells_flush(const unsigned long long* s_key, const unsigned long long* s_cnt, const SampleDev& d,
                                                  uint32_t flags) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < CELL_LDS_SLOTS; i += RB)
        if (s_key[i] != REPORT_EMPTY && s_cnt[i]) flags |= cell_flush(d, s_key[i], s_cnt[i]);
    if (flags) atomicOr(reinterpret_cast<unsigned int*>(d.r.ctl + 2), flags);
}

__global__ __launch_bounds__(RB) void sample_cells(SampleDev d) {
    __shared__ unsigned long long s_key[CELL_LDS_SLOTS];
    __shared__ unsigned long long s_cnt[CELL_LDS_SLOTS];
    block_cells_clear(s_key, s_cnt);
    uint32_t flags = 0;
    // block-local table first, global memory when it is crowded (w > 0: a zero weight leaves no cell behind)
    auto add = [&](uint32_t path, uint32_t s, unsigned long long w) { if (w) flags |= block_cell_add(s_key, s_cnt, d, path, s, w); };
    const uint64_t base = (uint64_t)blockIdx.x * (RB * RQ) + threadIdx.x;
    for (uint32_t k = 0; k < RQ; ++k) {
        const uint64_t q = base + (uint64_t)k * RB;
        if (q >= d.r.n_queries) break;
        const uint32_t s = d.sample_of[q];
        const Record rec = decode_record(d.r, q);   // (ahead of the sample's check: its loads go out beside the sample's)
        if (s >= d.n_samples) { flags |= FLAG_BAD_SAMPLE; d.r.ctl[4] = q; continue; }
        const unsigned long long w = d.r.weight ? (unsigned long long)d.r.weight[q] : 1ull;
        if (rec.kind == REC_NO_TAXON) { add(CELL_UNCLASSIFIED, s, w); continue; }
        if (rec.kind == REC_BAD) { flags |= FLAG_BAD_RECORD; d.r.ctl[3] = q; continue; }
        if (rec.kind == REC_NO_LEVEL) { add(CELL_UNPLACED, s, w); continue; }
        const Walk end = walk_levels(d.r, rec, [&](uint32_t path) { add(path, s, w); });
        flags |= end.stopped;
        if (end.stopped == FLAG_BAD_NODE) d.r.ctl[CTL_BAD_NODE] = q;
    }
    block_cells_flush(s_key, s_cnt, d, flags);
}

// the occupied cells in slot order, their path slots renamed to the compacted path index
__global__ void sample_cells_compact(const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ val,
                                     const uint32_t* __restrict__ at, const uint32_t* __restrict__ path_at, uint64_t cap,
                                     blu_sample_cell* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    const unsigned long long k = keys[i];
    if (k == REPORT_EMPTY) return;
    blu_sample_cell c;
    c.path = path_at[(uint32_t)(k >> 32)];
    c.sample = (uint32_t)k;
    c.clade = val[i];
    out[at[i]] = c;
}

// ---- per-sample table from count rows (blu_consensus_sample_table_counts) ------------------------------
// A query carries a CSR row of (sample, count) pairs instead of one sample and one weight: from none to thousands of them,
// so a lane per query does not fit.  A wave takes COUNT_Q consecutive queries in turn (a block: 4 x COUNT_Q consecutive
// queries, whose upper levels meet in the LDS cell table).  Per query the lanes load the lineage row together, lane 0 walks
// the selected levels through `intern` (a level's key holds its parent's slot, so the walk is serial) and lane k keeps the
// k-th path id.  The wave then goes through the row floor(64 / levels) non-zeros a step: a lane is one (non-zero, level)
// pair and adds the count to the cell (path, sample).  The per-sample unclassified / unplaced counts are a one-level row
// under the two reserved path ids.  All adds are u64 integer adds: exact, whatever the order.
constexpr uint32_t COUNT_Q = 32;
constexpr uint32_t COUNT_Q_BLOCK = COUNT_Q * (RB / 64);

struct CountDev {
    SampleDev s;                  // s.sample_of and s.r.weight are not read
    CountRows rows;
};

__global__ __launch_bounds__(RB) void count_cells(CountDev d) {
    __shared__ unsigned long long s_key[CELL_LDS_SLOTS];
    __shared__ unsigned long long s_cnt[CELL_LDS_SLOTS];
    block_cells_clear(s_key, s_cnt);
    const ReportDev& r = d.s.r;
    uint32_t flags = 0;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t q0 = (uint64_t)blockIdx.x * COUNT_Q_BLOCK + (uint64_t)(threadIdx.x >> 6) * COUNT_Q;
    for (uint32_t k = 0; k < COUNT_Q; ++k) {
        // (everything up to the pair loop is the same in all 64 lanes)
        const uint64_t q = q0 + k;
        if (q >= r.n_queries) break;
        const uint64_t lo = d.rows.row_ptr[q], hi = d.rows.row_ptr[q + 1];
        if (lo > hi || hi > d.rows.nnz) { flags |= FLAG_BAD_ROW; if (lane == 0) r.ctl[5] = q; continue; }
        const Record rec = decode_record(r, q);
        if (rec.kind == REC_BAD) { flags |= FLAG_BAD_RECORD; if (lane == 0) r.ctl[3] = q; continue; }
        uint32_t mine = rec.kind == REC_NO_TAXON ? CELL_UNCLASSIFIED : CELL_UNPLACED;   // lane k: the id of the query's k-th path
        uint32_t n_levels = 1;
        if (rec.kind == REC_PATH) {
            const uint32_t node = lane < rec.len ? rec.lin[r.node_base + lane] : 0u;   // lane j: the node of level j
            uint32_t path = REPORT_NONE;
            bool bad_node = false;
            n_levels = 0;
            for (unsigned long long t = rec.m; t; t &= t - 1ull, ++n_levels) {
                const uint32_t nd = __shfl(node, __ffsll(t) - 1, 64);
                if (reserved_first(path, nd)) { bad_node = true; break; }
                uint32_t p = REPORT_NONE;
                if (lane == 0) p = intern(r, path, nd);
                path = __shfl(p, 0, 64);
                if (path == REPORT_NONE) break;
                if (lane == n_levels) mine = path;
            }
            if (bad_node) { flags |= FLAG_BAD_NODE; if (lane == 0) r.ctl[CTL_BAD_NODE] = q; continue; }
            if (path == REPORT_NONE) { flags |= FLAG_OVERFLOW; continue; }
        }
        // lane -> (non-zero `nz` of the step, level `lv`); the lanes past per * n_levels idle
        const uint32_t per = 64u / n_levels;
        const uint32_t nz = lane / n_levels, lv = lane - nz * n_levels;
        const uint32_t path = __shfl(mine, lv, 64);
        if (nz >= per) continue;
        for (uint64_t i = lo + nz; i < hi; i += per) {
            const uint32_t s = d.rows.sample[i];
            const unsigned long long w = d.rows.count[i];
            if (s >= d.s.n_samples) { flags |= FLAG_BAD_SAMPLE; r.ctl[4] = q; continue; }
            if (w) flags |= block_cell_add(s_key, s_cnt, d.s, path, s, w);   // (a zero leaves no cell)
        }
    }
    block_cells_flush(s_key, s_cnt, d.s, flags);
}

// out[0]: P, the bound on the paths (report_bound); out[1]: sum of popcount(level_mask) * non-zeros of the row over the
// classified queries, the bound on the cells.  A row the count kernel would refuse counts as empty.
__global__ __launch_bounds__(RB) void count_bound(const blu_result* __restrict__ recs, CountRows rows, uint64_t n_queries,
                                                  unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s[2];
    if (threadIdx.x < 2) s[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long c = 0, cn = 0;
    for (uint64_t q = (uint64_t)blockIdx.x * RB + threadIdx.x; q < n_queries; q += (uint64_t)gridDim.x * RB) {
        const blu_result& r = recs[q];
        if (r.status >= 2) continue;
        const uint64_t lo = rows.row_ptr[q], hi = rows.row_ptr[q + 1];
        const unsigned long long pc = (unsigned long long)__popcll(r.level_mask);
        c += pc;
        if (lo <= hi && hi <= rows.nnz) cn += pc * (hi - lo);
    }
    c = wave_sum(c);
    cn = wave_sum(cn);
    if ((threadIdx.x & 63) == 0 && (c | cn)) { atomicAdd(&s[0], c); atomicAdd(&s[1], cn); }
    __syncthreads();
    if (threadIdx.x == 0 && (s[0] | s[1])) { atomicAdd(out, s[0]); atomicAdd(out + 1, s[1]); }
}

// ---- host side: the three entries share their tables, their attempts and the way back ------------------------------------

uint64_t next_pow2(uint64_t x) { uint64_t c = 1; while (c < x) c <<= 1; return c; }

// the slots of a table that holds up to n keys at load <= 1/2
uint64_t table_slots(uint64_t n) { return std::max<uint64_t>(next_pow2(2 * n), 1024); }

// the first attempt's guess at the distinct paths: read off the handle, no pass over the records
uint64_t path_guess(const blu_taxonomy* tax, uint64_t nq) {
    return std::min<uint64_t>(nq * std::max<uint32_t>(tax->max_depth, 1), 2 * tax->n_tax + 4096);
}

dim3 bound_grid(uint64_t nq) { return dim3((unsigned)std::min<uint64_t>((nq + RB - 1) / RB, 4096)); }

// everything of ReportDev but the tables of an attempt (TableRun::point)
ReportDev report_dev(const blu_taxonomy* tax, const ReportInput& in, unsigned long long* d_ctl) {
    ReportDev d{};
    d.lin = tax->d_lin; d.n_tax = tax->n_tax; d.stride = tax->dev_stride; d.node_base = tax->node_base;
    d.max_depth = tax->max_depth;
    d.recs = in.recs; d.n_queries = in.n_queries; d.row_src = in.row_src; d.n_rows = in.n_rows; d.row_stride = in.row_stride;
    d.by_query = in.by_query ? 1u : 0u; d.weight = in.weight; d.ctl = d_ctl;
    return d;
}

// ctl[2] -> the refusal, in the one order that is every entry's (an entry never raises a flag it does not have)
int flag_error(const char* who, const unsigned long long* ctl, uint32_t n_samples, uint64_t nnz) {
    const uint32_t flags = (uint32_t)ctl[2];
    if (flags & FLAG_BAD_ROW)
        set_error("%s: query %llu has a row_ptr that decreases or ends past the %llu non-zeros", who, ctl[5], (unsigned long long)nnz);
    else if (flags & FLAG_BAD_SAMPLE)
        set_error("%s: query %llu has a sample id that is not below n_samples = %u", who, ctl[4], n_samples);
    else if (flags & FLAG_BAD_RECORD)
        set_error("%s: record %llu has a taxon (status 0 / 1) but its reference row names no taxonomy row", who, ctl[3]);
    else if (flags & FLAG_BAD_NODE)
        set_error("%s: record %llu has a path that begins with node id 0xFFFFFFFF, which no path may begin with", who, ctl[CTL_BAD_NODE]);
    else return BLU_OK;
    return BLU_ERR_INVALID_ARG;
}

// One entry's device state and the cycle all three run: allocate the tables, clear them, launch, read ctl back, refuse
// (flag_error) or start again from zero at the sizes `resize` sets.  cells: a cell table and per-sample counters beside the
// path table (the two per-sample entries); else the path table carries direct counts (the report).  The first sizes are
// the caller's to set (cap, ccap) between begin() and run().
struct TableRun {
    HipPolicy pol;                // pol.who is the prefix of every message: "report", "sample table", "count table"
    DeviceArena mem{pol};
    const bool cells;
    const uint32_t n_samples;
    const uint64_t nnz;           // (for count_cells' refusal of a row)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the device work: begin() ... stop()
    unsigned long long *d_ctl = nullptr, *keys = nullptr, *direct = nullptr, *ckeys = nullptr, *cval = nullptr, *fixed = nullptr;
    uint64_t cap = 0, ccap = 0;
    uint32_t max_probe = REPORT_PROBE_FIRST, attempts = 0;
    unsigned long long ctl[CTL_WORDS] = {};    // of the last attempt

    TableRun(const char* who, bool cells, uint32_t n_samples = 0, uint64_t nnz = 0)
        : pol{who, BLU_ERR_ALLOC}, cells(cells), n_samples(n_samples), nnz(nnz) {}
    ~TableRun() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); }

    uint64_t fixed_bytes() const { return 2 * (uint64_t)n_samples * 8; }

    int begin() {
        HIP_CHECK(pol, hipEventCreate(&ev0));
        HIP_CHECK(pol, hipEventCreate(&ev1));
        HIP_CHECK(pol, mem.alloc(&d_ctl, sizeof ctl, "counters"));
        if (cells) HIP_CHECK(pol, mem.alloc(&fixed, fixed_bytes(), "per-sample counters"));
        HIP_CHECK(pol, hipEventRecord(ev0, nullptr));
        return BLU_OK;
    }

    // the tables of the attempt at hand
    void point(ReportDev& r) const { r.keys = keys; r.direct = direct; r.cap_mask = (uint32_t)(cap - 1); r.max_probe = max_probe; }
    void point(SampleDev& s) const {
        point(s.r);
        s.cell_keys = ckeys; s.cell_val = cval; s.cell_mask = (uint32_t)(ccap - 1); s.n_samples = n_samples; s.fixed = fixed;
    }

    // launch(): the entry's kernel on the tables of this attempt; resize(): cap and ccap from the bounds, after an overflow
    template <class Launch, class Resize>
    int run(Launch&& launch, Resize&& resize) {
        for (;;) {
            ++attempts;
            // (with cells, path ids below 2^31: the two ids above are the fixed rows' in the cell keys)
            if (!cells && cap > (1ull << 32)) {
                set_error("%s: a table of %llu slots exceeds 32-bit path ids", pol.who, (unsigned long long)cap);
                return BLU_ERR_ALLOC;
            }
            if (cells && (cap > (1ull << 31) || ccap > (1ull << 32))) {
                set_error("%s: tables of %llu / %llu slots exceed 32-bit ids", pol.who, (unsigned long long)cap, (unsigned long long)ccap);
                return BLU_ERR_ALLOC;
            }
            HIP_CHECK(pol, mem.alloc(&keys, cap * 8, "path table"));
            if (cells) {
                HIP_CHECK(pol, mem.alloc(&ckeys, ccap * 8, "cell table"));
                HIP_CHECK(pol, mem.alloc(&cval, ccap * 8, "cell table"));
            } else {
                HIP_CHECK(pol, mem.alloc(&direct, cap * 8, "path table"));
            }
            HIP_CHECK(pol, hipMemsetAsync(keys, 0xFF, cap * 8, nullptr));
            if (cells) {
                HIP_CHECK(pol, hipMemsetAsync(ckeys, 0xFF, ccap * 8, nullptr));
                HIP_CHECK(pol, hipMemsetAsync(cval, 0, ccap * 8, nullptr));
                HIP_CHECK(pol, hipMemsetAsync(fixed, 0, fixed_bytes(), nullptr));
            } else {
                HIP_CHECK(pol, hipMemsetAsync(direct, 0, cap * 8, nullptr));
            }
            HIP_CHECK(pol, hipMemsetAsync(d_ctl, 0, sizeof ctl, nullptr));
            launch();
            HIP_CHECK(pol, hipGetLastError());
            HIP_CHECK(pol, hipMemcpy(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost));
            if (const int rc = flag_error(pol.who, ctl, n_samples, nnz); rc != BLU_OK) return rc;
            if (!(ctl[2] & FLAG_OVERFLOW)) return BLU_OK;
            if (max_probe != REPORT_PROBE_FIRST) {   // (cannot happen at load <= 1/2)
                set_error(cells ? "%s: table overflow" : "%s: path table overflow", pol.who);
                return BLU_ERR_HIP;
            }
            // an estimate was short: every table again from zero, sized from the bounds, where a probe always ends
            mem.free(keys); mem.free(direct); mem.free(ckeys); mem.free(cval);
            keys = direct = ckeys = cval = nullptr;
            if (const int rc = resize(); rc != BLU_OK) return rc;
            max_probe = (uint32_t)std::min<uint64_t>(std::max(cap, ccap), 0xFFFFFFFFull);
        }
    }

    // P of report_bound, through ctl[0]: what the report and the sample table size their retry from
    int path_bound(const ReportInput& in, unsigned long long* bound) {
        HIP_CHECK(pol, hipMemsetAsync(d_ctl, 0, 8, nullptr));
        hipLaunchKernelGGL(report_bound, bound_grid(in.n_queries), dim3(RB), 0, 0, in.recs, in.n_queries, d_ctl);
        HIP_CHECK(pol, hipGetLastError());
        HIP_CHECK(pol, hipMemcpy(bound, d_ctl, 8, hipMemcpyDeviceToHost));
        return BLU_OK;
    }

    // the device work ends here: its time by the events
    int stop(double* ms) {
        float f = 0;
        HIP_CHECK(pol, hipEventRecord(ev1, nullptr));
        HIP_CHECK(pol, hipEventSynchronize(ev1));
        HIP_CHECK(pol, hipEventElapsedTime(&f, ev0, ev1));
        *ms = f;
        return BLU_OK;
    }
};

dim3 walk_grid(uint64_t nq) { return dim3((unsigned)((nq + RB * RQ - 1) / (RB * RQ))); }   // report_paths, sample_cells

// A table's occupied slots, compacted on the device: at[i] = the index of slot i among them (report_flags and a scan;
// at[cap] = their number = n), then launch(grid, block) starts the kernel that writes rows[at[i]] for every such slot.
template <class Row>
struct Compacted {
    uint32_t* at = nullptr;
    Row* rows = nullptr;
    uint64_t n = 0;
};

template <class Row, class Launch>
int compact_table(TableRun& T, const unsigned long long* keys, uint64_t cap, const char* ids, const char* what, Compacted<Row>* c,
                  Launch&& launch) {
    void* d_tmp = nullptr;
    HIP_CHECK(T.pol, T.mem.alloc(&c->at, (cap + 1) * 4, ids));
    hipLaunchKernelGGL(report_flags, dim3((unsigned)((cap + 1 + 255) / 256)), dim3(256), 0, 0, keys, cap, c->at);
    HIP_CHECK(T.pol, hipGetLastError());
    HIP_CHECK(T.pol, T.mem.alloc(&d_tmp, scan_tmp_bytes_u32(cap + 1), "scan scratch"));   // (while the flags are written)
    HIP_CHECK(T.pol, exclusive_scan_u32(c->at, c->at, cap + 1, d_tmp));
    uint32_t n32 = 0;
    HIP_CHECK(T.pol, hipMemcpy(&n32, c->at + cap, 4, hipMemcpyDeviceToHost));
    c->n = n32;
    HIP_CHECK(T.pol, T.mem.alloc(&c->rows, c->n * sizeof(Row), what));
    launch(dim3((unsigned)((cap + 255) / 256)), dim3(256));
    HIP_CHECK(T.pol, hipGetLastError());
    return BLU_OK;
}

// paths[] (parents named by index, in any order) -> o[], parents first (depth order, input order inside a depth) and
// renamed to their place in o; at[i]: the place of path i
void parents_first(const std::vector<blu_report_path>& paths, std::vector<uint32_t>& at, blu_report_path* o) {
    const uint64_t n_paths = paths.size();
    const uint32_t NONE = REPORT_NONE;
    std::vector<uint8_t> depth(n_paths, 0xFF);
    std::vector<uint32_t> stack;
    for (uint64_t i = 0; i < n_paths; ++i) {
        uint32_t x = (uint32_t)i;
        while (depth[x] == 0xFF && paths[x].parent != NONE && depth[paths[x].parent] == 0xFF) { stack.push_back(x); x = paths[x].parent; }
        if (depth[x] == 0xFF) depth[x] = paths[x].parent == NONE ? 0 : (uint8_t)(depth[paths[x].parent] + 1);
        while (!stack.empty()) { const uint32_t y = stack.back(); stack.pop_back(); depth[y] = (uint8_t)(depth[paths[y].parent] + 1); }
    }
    std::vector<uint64_t> first(BLU_MAX_DEPTH + 1, 0);
    for (uint64_t i = 0; i < n_paths; ++i) ++first[depth[i] + 1];
    for (uint32_t k = 0; k < BLU_MAX_DEPTH; ++k) first[k + 1] += first[k];
    at.resize(n_paths);
    for (uint64_t i = 0; i < n_paths; ++i) at[i] = (uint32_t)first[depth[i]]++;
    for (uint64_t i = 0; i < n_paths; ++i) {
        blu_report_path p = paths[i];
        p.parent = p.parent == NONE ? NONE : at[p.parent];
        o[at[i]] = p;
    }
}

// The tables of a per-sample run -> blu_sample_table: the occupied slots compacted on the device, then ordered on the host.
// Shared by sample_table_device and sample_table_counts_device.
int sample_table_finish(TableRun& T, blu_sample_table* out) {
    HipPolicy& pol = T.pol;
    const uint32_t n_samples = T.n_samples;
    Compacted<blu_report_path> P;
    Compacted<blu_sample_cell> C;
    if (const int rc = compact_table(T, T.keys, T.cap, "path ids", "paths", &P, [&](dim3 g, dim3 b) {
            hipLaunchKernelGGL(report_compact, g, b, 0, 0, T.keys, (const unsigned long long*)nullptr, P.at, T.cap, P.rows);
        }); rc != BLU_OK) return rc;
    if (const int rc = compact_table(T, T.ckeys, T.ccap, "cell ids", "cells", &C, [&](dim3 g, dim3 b) {
            hipLaunchKernelGGL(sample_cells_compact, g, b, 0, 0, T.ckeys, T.cval, C.at, P.at, T.ccap, C.rows);
        }); rc != BLU_OK) return rc;
    if (const int rc = T.stop(&out->t_device_ms); rc != BLU_OK) return rc;
    const uint64_t n_paths = P.n, n_cells = C.n;
    std::vector<blu_report_path> paths(n_paths);
    std::vector<blu_sample_cell> cells(n_cells);
    std::vector<uint64_t> fixed(2 * (uint64_t)n_samples);
    HIP_CHECK(pol, DeviceArena::download(paths.data(), P.rows, n_paths));
    HIP_CHECK(pol, DeviceArena::download(cells.data(), C.rows, n_cells));
    HIP_CHECK(pol, DeviceArena::download(fixed.data(), T.fixed, fixed.size()));
    // parents first as in the report; a path's clade = the sum of its cells, direct = clade - the children's clades;
    // the cells ordered by path (a counting sort), then by sample inside a path
    const uint32_t NONE = REPORT_NONE;
    blu_report_path* o = (blu_report_path*)malloc(std::max<uint64_t>(n_paths, 1) * sizeof(blu_report_path));
    blu_sample_cell* c = (blu_sample_cell*)malloc(std::max<uint64_t>(n_cells, 1) * sizeof(blu_sample_cell));
    uint64_t* un = (uint64_t*)malloc(std::max<uint64_t>(fixed.size(), 1) * 8);
    if (!o || !c || !un) { free(o); free(c); free(un); set_error("sample table: out of memory"); return BLU_ERR_ALLOC; }
    std::vector<uint32_t> at;
    parents_first(paths, at, o);
    std::vector<uint64_t> first(n_paths + 1, 0);
    for (const blu_sample_cell& x : cells) { o[at[x.path]].clade += x.clade; ++first[at[x.path] + 1]; }
    for (uint64_t i = 0; i < n_paths; ++i) first[i + 1] += first[i];
    for (const blu_sample_cell& x : cells) { blu_sample_cell y = x; y.path = at[x.path]; c[first[y.path]++] = y; }
    for (uint64_t i = 0, lo = 0; i < n_paths; lo = first[i++])
        if (first[i] - lo > 1) std::sort(c + lo, c + first[i], [](const blu_sample_cell& a, const blu_sample_cell& b) { return a.sample < b.sample; });
    for (uint64_t i = 0; i < n_paths; ++i) o[i].direct = o[i].clade;
    for (uint64_t i = n_paths; i-- > 0;)
        if (o[i].parent != NONE) o[o[i].parent].direct -= o[i].clade;
    std::copy(fixed.begin(), fixed.end(), un);
    out->paths = o;
    out->n_paths = n_paths;
    out->cells = c;
    out->n_cells = n_cells;
    out->n_samples = n_samples;
    out->unclassified = un;
    out->unplaced = un + n_samples;
    out->table_slots = T.ccap;
    out->attempts = T.attempts;
    return BLU_OK;
}

}  // namespace

int report_device(const blu_taxonomy* tax, const ReportInput& in, blu_report* out) {
    const uint64_t nq = in.n_queries;
    TableRun T("report", false);
    if (const int rc = T.begin(); rc != BLU_OK) return rc;
    ReportDev d = report_dev(tax, in, T.d_ctl);
    T.cap = table_slots(path_guess(tax, nq));
    if (const int rc = T.run(
            [&] { T.point(d); if (nq) hipLaunchKernelGGL(report_paths, walk_grid(nq), dim3(RB), 0, 0, d); },
            [&] {
                unsigned long long bound = 0;
                const int rc = T.path_bound(in, &bound);
                T.cap = table_slots(bound);
                return rc;
            }); rc != BLU_OK) return rc;
    HipPolicy& pol = T.pol;
    Compacted<blu_report_path> P;
    if (const int rc = compact_table(T, T.keys, T.cap, "path ids", "paths", &P, [&](dim3 g, dim3 b) {
            hipLaunchKernelGGL(report_compact, g, b, 0, 0, T.keys, T.direct, P.at, T.cap, P.rows);
        }); rc != BLU_OK) return rc;
    if (const int rc = T.stop(&out->t_device_ms); rc != BLU_OK) return rc;
    const uint64_t n_paths = P.n;
    std::vector<blu_report_path> paths(n_paths);
    HIP_CHECK(pol, DeviceArena::download(paths.data(), P.rows, n_paths));
    // parents first (depth order, slot order inside a depth), then clade = direct + the children's clades
    const uint32_t NONE = REPORT_NONE;
    blu_report_path* o = n_paths ? (blu_report_path*)malloc(n_paths * sizeof(blu_report_path)) : nullptr;
    if (n_paths && !o) { set_error("report: out of memory"); return BLU_ERR_ALLOC; }
    std::vector<uint32_t> at;
    parents_first(paths, at, o);
    for (uint64_t i = 0; i < n_paths; ++i) o[i].clade = o[i].direct;
    for (uint64_t i = n_paths; i-- > 0;)
        if (o[i].parent != NONE) o[o[i].parent].clade += o[i].clade;
    out->paths = o;
    out->n_paths = n_paths;
    out->unclassified = T.ctl[0];
    out->unplaced = T.ctl[1];
    uint64_t classified = 0;
    for (uint64_t i = 0; i < n_paths; ++i) if (o[i].parent == NONE) classified += o[i].clade;
    out->total = T.ctl[0] + T.ctl[1] + classified;
    out->table_slots = T.cap;
    out->attempts = T.attempts;
    return BLU_OK;
}

int sample_table_device(const blu_taxonomy* tax, const ReportInput& in, const uint32_t* sample_of, uint32_t n_samples,
                        blu_sample_table* out) {
    const uint64_t nq = in.n_queries;
    TableRun T("sample table", true, n_samples);
    if (const int rc = T.begin(); rc != BLU_OK) return rc;
    SampleDev d{};
    d.r = report_dev(tax, in, T.d_ctl);
    d.sample_of = sample_of;
    // paths as the report sizes them; cells: the paths plus one per query (a sample's queries mostly share their upper
    // levels), at most one per level of every query
    const uint64_t guess = path_guess(tax, nq);
    T.cap = table_slots(guess);
    T.ccap = table_slots(std::min<uint64_t>(nq * std::max<uint32_t>(tax->max_depth, 1), guess + nq));
    if (const int rc = T.run(
            [&] { T.point(d); if (nq) hipLaunchKernelGGL(sample_cells, walk_grid(nq), dim3(RB), 0, 0, d); },
            [&] {   // both tables from the bound on the paths: a query reaches no more cells than paths
                unsigned long long bound = 0;
                const int rc = T.path_bound(in, &bound);
                T.cap = T.ccap = table_slots(bound);
                return rc;
            }); rc != BLU_OK) return rc;
    return sample_table_finish(T, out);
}

int sample_table_counts_device(const blu_taxonomy* tax, const ReportInput& in, const CountRows& rows, uint32_t n_samples,
                               blu_sample_table* out) {
    const uint64_t nq = in.n_queries;
    TableRun T("count table", true, n_samples, rows.nnz);
    if (const int rc = T.begin(); rc != BLU_OK) return rc;
    HipPolicy& pol = T.pol;
    CountDev d{};
    d.s.r = report_dev(tax, in, T.d_ctl);
    d.rows = rows;
    // the bounds first: P on the paths, and on the cells the sum of levels x non-zeros (one pass over the records and row_ptr)
    unsigned long long bound[2] = {0, 0};
    HIP_CHECK(pol, hipMemsetAsync(T.d_ctl, 0, sizeof T.ctl, nullptr));
    if (nq) hipLaunchKernelGGL(count_bound, bound_grid(nq), dim3(RB), 0, 0, in.recs, rows, nq, T.d_ctl);
    HIP_CHECK(pol, hipGetLastError());
    HIP_CHECK(pol, hipMemcpy(bound, T.d_ctl, sizeof bound, hipMemcpyDeviceToHost));
    // paths as the report sizes them; cells: no more than the bound, and no more than every path in every sample
    const uint64_t guess = path_guess(tax, nq);
    T.cap = table_slots(guess);
    T.ccap = table_slots(std::min<uint64_t>(bound[1], guess * std::max<uint32_t>(n_samples, 1)));
    if (const int rc = T.run(
            [&] { T.point(d.s); if (nq) hipLaunchKernelGGL(count_cells, dim3((unsigned)((nq + COUNT_Q_BLOCK - 1) / COUNT_Q_BLOCK)), dim3(RB), 0, 0, d); },
            [&] { T.cap = table_slots(bound[0]); T.ccap = table_slots(bound[1]); return BLU_OK; }); rc != BLU_OK) return rc;
    return sample_table_finish(T, out);
}

}  // namespace blu

using namespace blu;

namespace {

// What the three entries begin with: the argument checks (`needed`: the entry's own array, which may be null only when there
// are no queries), *out cleared, the column the engine rows come from and its stride, the device and, for device pointers,
// the records' alignment and the stream.  fn names the entry in the messages.  *in: the device-pointer view of the call
// (no weights); host pointers go through stage_records.
int entry_begin(const char* fn, const blu_taxonomy* tax, const blu_hits* hits, const blu_result* results, const void* needed,
                void* stream, void* out, size_t out_bytes, ReportInput* in) {
    if (!tax || !hits || !out || (hits->n_queries && (!results || !needed))) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    memset(out, 0, out_bytes);
    if (tax->device < 0) { set_error("host-only taxonomy handle: %s needs a HIP device (no CPU fallback)", fn); return BLU_ERR_NO_DEVICE; }
    const uint32_t* src = hits->packed ? hits->packed : hits->packed64 ? hits->packed64 : hits->tax_row;
    const uint32_t stride = hits->packed ? 4u : hits->packed64 ? 6u : 1u;
    if (hits->n_queries && !src) { set_error("%s: no tax_row column", fn); return BLU_ERR_INVALID_ARG; }
    if (hipSetDevice(tax->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", tax->device); return BLU_ERR_NO_DEVICE; }
    if (hits->on_device) {
        if (((uintptr_t)results & 15u) != 0) { set_error("%s: device records must be 16-byte aligned", fn); return BLU_ERR_INVALID_ARG; }
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) { set_error("%s: stream synchronise failed", fn); return BLU_ERR_HIP; }
    }
    *in = ReportInput{results, hits->n_queries, src, hits->n_hits, stride, false, nullptr};
    return BLU_OK;
}

// Host pointers: the records go up, and each record's engine row, gathered here (4 bytes a query instead of the whole
// column).  *in: the host view on entry, the staged one (rows by query) on return.
int stage_records(HipPolicy& pol, DeviceArena& mem, ReportInput* in) {
    const uint64_t nq = in->n_queries;
    std::vector<uint32_t> rows(nq, BLU_UNMATCHED_TAXID);
    for (uint64_t q = 0; q < nq; ++q)
        if (in->recs[q].status < 2 && in->recs[q].ref_row < in->n_rows) rows[q] = in->row_src[(uint64_t)in->recs[q].ref_row * in->row_stride];
    blu_result* d_recs = nullptr;
    uint32_t* d_rows = nullptr;
    HIP_CHECK(pol, mem.upload(&d_recs, in->recs, nq, "records"));
    HIP_CHECK(pol, mem.upload(&d_rows, rows.data(), nq, "rows"));
    *in = ReportInput{d_recs, nq, d_rows, nq, 1u, true, nullptr};
    return BLU_OK;
}

}  // namespace

extern "C" {

int blu_consensus_report(const blu_taxonomy* tax, const blu_hits* hits, const blu_result* results, const uint32_t* weights,
                         void* stream, blu_report* out) {
    ReportInput in{};
    if (const int rc = entry_begin("blu_consensus_report", tax, hits, results, results, stream, out, sizeof *out, &in); rc != BLU_OK) return rc;
    HipPolicy pol{"blu_consensus_report", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    try {
        in.weight = weights;
        if (!hits->on_device) {   // the weights go up beside the records
            uint32_t* d_w = nullptr;
            if (const int rc = stage_records(pol, mem, &in); rc != BLU_OK) return rc;
            if (weights) HIP_CHECK(pol, mem.upload(&d_w, weights, in.n_queries, "weights"));
            in.weight = d_w;
        }
        return report_device(tax, in, out);
    } catch (const std::bad_alloc&) { set_error("out of memory"); return BLU_ERR_ALLOC; }
}

int blu_consensus_sample_table(const blu_taxonomy* tax, const blu_hits* hits, const blu_result* results, const uint32_t* weights,
                               const uint32_t* sample_of, uint32_t n_samples, void* stream, blu_sample_table* out) {
    ReportInput in{};
    if (const int rc = entry_begin("blu_consensus_sample_table", tax, hits, results, sample_of, stream, out, sizeof *out, &in); rc != BLU_OK) return rc;
    HipPolicy pol{"blu_consensus_sample_table", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    try {
        in.weight = weights;
        if (!hits->on_device) {   // the sample ids and the weights go up beside the records
            uint32_t *d_s = nullptr, *d_w = nullptr;
            if (const int rc = stage_records(pol, mem, &in); rc != BLU_OK) return rc;
            HIP_CHECK(pol, mem.upload(&d_s, sample_of, in.n_queries, "sample ids"));
            if (weights) HIP_CHECK(pol, mem.upload(&d_w, weights, in.n_queries, "weights"));
            in.weight = d_w;
            sample_of = d_s;
        }
        return sample_table_device(tax, in, sample_of, n_samples, out);
    } catch (const std::bad_alloc&) { set_error("out of memory"); return BLU_ERR_ALLOC; }
}

int blu_consensus_sample_table_counts(const blu_taxonomy* tax, const blu_hits* hits, const blu_result* results, const blu_count_rows* rows,
                                      uint32_t n_samples, void* stream, blu_sample_table* out) {
    if (!rows) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    ReportInput in{};
    if (const int rc = entry_begin("blu_consensus_sample_table_counts", tax, hits, results, rows->row_ptr, stream, out, sizeof *out, &in); rc != BLU_OK) return rc;
    HipPolicy pol{"blu_consensus_sample_table_counts", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    const uint64_t nq = in.n_queries;
    uint64_t nnz = 0;   // the last offset: what the two arrays hold, and what no row may pass
    if (nq && hits->on_device) HIP_CHECK(pol, hipMemcpy(&nnz, rows->row_ptr + nq, 8, hipMemcpyDeviceToHost));
    else if (nq) nnz = rows->row_ptr[nq];
    if (nnz && (!rows->sample || !rows->count)) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    try {
        CountRows cr{rows->row_ptr, rows->sample, rows->count, nnz};
        if (!hits->on_device) {   // the three arrays of the rows go up beside the records
            uint64_t* d_ptr = nullptr;
            uint32_t *d_s = nullptr, *d_c = nullptr;
            if (const int rc = stage_records(pol, mem, &in); rc != BLU_OK) return rc;
            HIP_CHECK(pol, mem.upload(&d_ptr, rows->row_ptr, nq ? nq + 1 : 0, "row offsets"));
            HIP_CHECK(pol, mem.upload(&d_s, rows->sample, nnz, "sample ids"));
            HIP_CHECK(pol, mem.upload(&d_c, rows->count, nnz, "counts"));
            cr = CountRows{d_ptr, d_s, d_c, nnz};
        }
        return sample_table_counts_device(tax, in, cr, n_samples, out);
    } catch (const std::bad_alloc&) { set_error("out of memory"); return BLU_ERR_ALLOC; }
}

void blu_sample_table_free(blu_sample_table* table) {
    if (!table) return;
    free(table->paths);
    free(table->cells);
    free(table->unclassified);   // (unplaced points into the same block)
    table->paths = nullptr;
    table->cells = nullptr;
    table->unclassified = table->unplaced = nullptr;
    table->n_paths = table->n_cells = 0;
}

void blu_report_free(blu_report* report) {
    if (!report) return;
    free(report->paths);
    report->paths = nullptr;
    report->n_paths = 0;
}

}  // extern "C"
