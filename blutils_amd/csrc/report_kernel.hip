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
constexpr uint32_t FLAG_OVERFLOW = 1u, FLAG_BAD_RECORD = 2u;
constexpr uint32_t FLAG_BAD_NODE = 16u;              // (4 and 8 are the sample table's)
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
    unsigned long long* ctl;      // [CTL_WORDS] {unclassified, unplaced, flags, bad query, .., .., the query of a bad node}
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

// the occupied slots in slot order, parents renamed to their index in that order
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
    p.direct = direct[i];
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
constexpr uint32_t FLAG_BAD_SAMPLE = 4u;

struct SampleDev {
    ReportDev r;                    // the report's walk and path table (r.direct is not used); r.ctl[4]: a bad sample's query
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

__global__ __launch_bounds__(RB) void sample_cells(SampleDev d) {
    __shared__ unsigned long long s_key[CELL_LDS_SLOTS];
    __shared__ unsigned long long s_cnt[CELL_LDS_SLOTS];
    for (uint32_t i = threadIdx.x; i < CELL_LDS_SLOTS; i += RB) { s_key[i] = REPORT_EMPTY; s_cnt[i] = 0; }
    __syncthreads();
    uint32_t flags = 0;
    // block-local table first, global memory when it is crowded (w > 0: a zero weight leaves no cell behind)
    auto add = [&](uint32_t path, uint32_t s, unsigned long long w) { flags |= block_cell_add(s_key, s_cnt, d, path, s, w); };
    const uint64_t base = (uint64_t)blockIdx.x * (RB * RQ) + threadIdx.x;
    for (uint32_t k = 0; k < RQ; ++k) {
        const uint64_t q = base + (uint64_t)k * RB;
        if (q >= d.r.n_queries) break;
        const uint4* rp = reinterpret_cast<const uint4*>(d.r.recs + q);
        const uint4 a = rp[0], b = rp[1];
        const uint32_t s = d.sample_of[q];
        if (s >= d.n_samples) { flags |= FLAG_BAD_SAMPLE; d.r.ctl[4] = q; continue; }
        const uint32_t status = a.x & 0xFFu;
        const uint32_t ref_row = a.w;
        const unsigned long long mask = (unsigned long long)b.x | ((unsigned long long)b.y << 32);
        const unsigned long long w = d.r.weight ? (unsigned long long)d.r.weight[q] : 1ull;
        if (status >= 2) { if (w) add(CELL_UNCLASSIFIED, s, w); continue; }   // taxon: null
        const uint64_t idx = d.r.by_query ? q : (uint64_t)ref_row;
        uint32_t row = REPORT_NONE;
        if (idx < d.r.n_rows) row = d.r.row_src[idx * d.r.row_stride];
        const uint32_t pos = row & ((1u << BLU_ROW_BITS) - 1u);
        if (row == BLU_UNMATCHED_TAXID || pos >= d.r.n_tax) { flags |= FLAG_BAD_RECORD; d.r.ctl[3] = q; continue; }
        const uint32_t* lin = d.r.lin + (uint64_t)pos * d.r.stride;
        const uint32_t len = min(lin[0] & 0xFFu, d.r.max_depth);
        const unsigned long long m = len >= 64 ? mask : mask & ((1ull << len) - 1ull);
        if (m == 0) { if (w) add(CELL_UNPLACED, s, w); continue; }           // taxonomy: ""
        uint32_t path = REPORT_NONE;
        for (uint32_t j = 0; j < len; ++j) {
            if (!((m >> j) & 1ull)) continue;
            const uint32_t node = lin[d.r.node_base + j];
            if (reserved_first(path, node)) { flags |= FLAG_BAD_NODE; d.r.ctl[CTL_BAD_NODE] = q; break; }
            path = intern(d.r, path, node);
            if (path == REPORT_NONE) { flags |= FLAG_OVERFLOW; break; }
            if (w) add(path, s, w);
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < CELL_LDS_SLOTS; i += RB)
        if (s_key[i] != REPORT_EMPTY && s_cnt[i]) flags |= cell_flush(d, s_key[i], s_cnt[i]);
    if (flags) atomicOr(reinterpret_cast<unsigned int*>(d.r.ctl + 2), flags);
}

// the occupied path slots in slot order, parents renamed to their index in that order (report_compact without counts)
__global__ void sample_paths_compact(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ at, uint64_t cap,
                                     blu_report_path* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cap) return;
    const unsigned long long k = keys[i];
    if (k == REPORT_EMPTY) return;
    const uint32_t parent = (uint32_t)(k >> 32);
    blu_report_path p;
    p.node = (uint32_t)k;
    p.parent = parent == REPORT_NONE ? REPORT_NONE : at[parent];
    p.direct = 0;
    p.clade = 0;
    out[at[i]] = p;
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
constexpr uint32_t FLAG_BAD_ROW = 8u;

struct CountDev {
    SampleDev s;                  // s.sample_of and s.r.weight are not read; s.r.ctl[5]: the query of a bad row
    CountRows rows;
};

__global__ __launch_bounds__(RB) void count_cells(CountDev d) {
    __shared__ unsigned long long s_key[CELL_LDS_SLOTS];
    __shared__ unsigned long long s_cnt[CELL_LDS_SLOTS];
    for (uint32_t i = threadIdx.x; i < CELL_LDS_SLOTS; i += RB) { s_key[i] = REPORT_EMPTY; s_cnt[i] = 0; }
    __syncthreads();
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
        const uint4* rp = reinterpret_cast<const uint4*>(r.recs + q);
        const uint4 a = rp[0], b = rp[1];
        const uint32_t status = a.x & 0xFFu;
        const uint32_t ref_row = a.w;
        const unsigned long long mask = (unsigned long long)b.x | ((unsigned long long)b.y << 32);
        uint32_t mine = CELL_UNCLASSIFIED;      // lane k: the id of the query's k-th path
        uint32_t n_levels = 1;
        if (status < 2) {
            const uint64_t idx = r.by_query ? q : (uint64_t)ref_row;
            uint32_t row = REPORT_NONE;
            if (idx < r.n_rows) row = r.row_src[idx * r.row_stride];
            const uint32_t pos = row & ((1u << BLU_ROW_BITS) - 1u);
            if (row == BLU_UNMATCHED_TAXID || pos >= r.n_tax) { flags |= FLAG_BAD_RECORD; if (lane == 0) r.ctl[3] = q; continue; }
            const uint32_t* lin = r.lin + (uint64_t)pos * r.stride;
            const uint32_t len = min(lin[0] & 0xFFu, r.max_depth);
            const unsigned long long m = len >= 64 ? mask : mask & ((1ull << len) - 1ull);
            mine = CELL_UNPLACED;
            if (m != 0) {
                const uint32_t node = lane < len ? lin[r.node_base + lane] : 0u;   // lane j: the node of level j
                uint32_t path = REPORT_NONE;
                bool bad_node = false;
                n_levels = 0;
                for (unsigned long long t = m; t; t &= t - 1ull, ++n_levels) {
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
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < CELL_LDS_SLOTS; i += RB)
        if (s_key[i] != REPORT_EMPTY && s_cnt[i]) flags |= cell_flush(d.s, s_key[i], s_cnt[i]);
    if (flags) atomicOr(reinterpret_cast<unsigned int*>(r.ctl + 2), flags);
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

uint64_t next_pow2(uint64_t x) { uint64_t c = 1; while (c < x) c <<= 1; return c; }

// paths[] (parents named by index, in any order) -> at[i], the position of path i when parents come first: depth order,
// input order inside a depth
void parents_first(const std::vector<blu_report_path>& paths, std::vector<uint32_t>& at) {
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
}

// What a count pass leaves on the device: both tables of its last attempt, the per-sample counters, the events around the
// device work (ev0 recorded; ev1 is recorded here, after the compaction).
struct SampleTables {
    unsigned long long *keys = nullptr, *ckeys = nullptr, *cval = nullptr, *fixed = nullptr;
    uint64_t cap = 0, ccap = 0;
    uint32_t attempts = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    ~SampleTables() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); }
};

// The tables -> blu_sample_table: the occupied slots compacted on the device, then ordered on the host.  Shared by
// sample_table_device and sample_table_counts_device.
int sample_table_finish(HipPolicy& pol, DeviceArena& mem, const SampleTables& t, uint32_t n_samples, blu_sample_table* out) {
    unsigned long long *const d_keys = t.keys, *const d_ckeys = t.ckeys, *const d_cval = t.cval, *const d_fixed = t.fixed;
    const uint64_t cap = t.cap, ccap = t.ccap;
    uint32_t *d_at = nullptr, *d_cat = nullptr;
    void* d_tmp = nullptr;
    blu_report_path* d_paths = nullptr;
    blu_sample_cell* d_cells = nullptr;
    uint64_t n_paths = 0, n_cells = 0;
    std::vector<blu_report_path> paths;
    std::vector<blu_sample_cell> cells;
    std::vector<uint64_t> fixed(2 * (uint64_t)n_samples);
    {
        HIP_CHECK(pol, mem.alloc(&d_at, (cap + 1) * 4, "path ids"));
        HIP_CHECK(pol, mem.alloc(&d_cat, (ccap + 1) * 4, "cell ids"));
        HIP_CHECK(pol, mem.alloc(&d_tmp, scan_tmp_bytes_u32(std::max(cap, ccap) + 1), "scan scratch"));
        hipLaunchKernelGGL(report_flags, dim3((unsigned)((cap + 1 + 255) / 256)), dim3(256), 0, 0, d_keys, cap, d_at);
        HIP_CHECK(pol, hipGetLastError());
        HIP_CHECK(pol, exclusive_scan_u32(d_at, d_at, cap + 1, d_tmp));
        hipLaunchKernelGGL(report_flags, dim3((unsigned)((ccap + 1 + 255) / 256)), dim3(256), 0, 0, d_ckeys, ccap, d_cat);
        HIP_CHECK(pol, hipGetLastError());
        HIP_CHECK(pol, exclusive_scan_u32(d_cat, d_cat, ccap + 1, d_tmp));
        uint32_t n32[2] = {0, 0};
        HIP_CHECK(pol, hipMemcpy(&n32[0], d_at + cap, 4, hipMemcpyDeviceToHost));
        HIP_CHECK(pol, hipMemcpy(&n32[1], d_cat + ccap, 4, hipMemcpyDeviceToHost));
        n_paths = n32[0];
        n_cells = n32[1];
        HIP_CHECK(pol, mem.alloc(&d_paths, n_paths * sizeof(blu_report_path), "paths"));
        HIP_CHECK(pol, mem.alloc(&d_cells, n_cells * sizeof(blu_sample_cell), "cells"));
        hipLaunchKernelGGL(sample_paths_compact, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, 0, d_keys, d_at, cap, d_paths);
        HIP_CHECK(pol, hipGetLastError());
        hipLaunchKernelGGL(sample_cells_compact, dim3((unsigned)((ccap + 255) / 256)), dim3(256), 0, 0, d_ckeys, d_cval, d_cat, d_at, ccap, d_cells);
        HIP_CHECK(pol, hipGetLastError());
        HIP_CHECK(pol, hipEventRecord(t.ev1, nullptr));
        paths.resize(n_paths);
        cells.resize(n_cells);
        if (n_paths) HIP_CHECK(pol, hipMemcpy(paths.data(), d_paths, n_paths * sizeof(blu_report_path), hipMemcpyDeviceToHost));
        if (n_cells) HIP_CHECK(pol, hipMemcpy(cells.data(), d_cells, n_cells * sizeof(blu_sample_cell), hipMemcpyDeviceToHost));
        if (n_samples) HIP_CHECK(pol, hipMemcpy(fixed.data(), d_fixed, fixed.size() * 8, hipMemcpyDeviceToHost));
        float ms = 0;
        HIP_CHECK(pol, hipEventSynchronize(t.ev1));   // (no path, cell or sample came back: no copy has waited for the device yet)
        HIP_CHECK(pol, hipEventElapsedTime(&ms, t.ev0, t.ev1));
        out->t_device_ms = ms;
    }
    {
        // parents first as in the report; a path's clade = the sum of its cells, direct = clade - the children's clades;
        // the cells ordered by path (a counting sort), then by sample inside a path
        const uint32_t NONE = REPORT_NONE;
        std::vector<uint32_t> at;
        parents_first(paths, at);
        blu_report_path* o = (blu_report_path*)malloc(std::max<uint64_t>(n_paths, 1) * sizeof(blu_report_path));
        blu_sample_cell* c = (blu_sample_cell*)malloc(std::max<uint64_t>(n_cells, 1) * sizeof(blu_sample_cell));
        uint64_t* un = (uint64_t*)malloc(std::max<uint64_t>(fixed.size(), 1) * 8);
        if (!o || !c || !un) { free(o); free(c); free(un); set_error("sample table: out of memory"); return BLU_ERR_ALLOC; }
        for (uint64_t i = 0; i < n_paths; ++i) {
            blu_report_path p = paths[i];
            p.parent = p.parent == NONE ? NONE : at[p.parent];
            o[at[i]] = p;
        }
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
        out->table_slots = ccap;
        out->attempts = t.attempts;
    }
    return BLU_OK;
}

}  // namespace

int report_device(const blu_taxonomy* tax, const ReportInput& in, blu_report* out) {
    const uint64_t nq = in.n_queries;
    unsigned long long *d_keys = nullptr, *d_direct = nullptr, *d_ctl = nullptr;
    uint32_t* d_at = nullptr;
    void* d_tmp = nullptr;
    blu_report_path* d_paths = nullptr;
    unsigned long long ctl[CTL_WORDS] = {};
    uint64_t cap = 0, n_paths = 0;
    uint32_t attempts = 0;
    std::vector<blu_report_path> paths;
    HipPolicy pol{"report", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    struct Events { hipEvent_t ev0 = nullptr, ev1 = nullptr; ~Events() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); } } ev;
    hipEvent_t &ev0 = ev.ev0, &ev1 = ev.ev1;
    HIP_CHECK(pol, hipEventCreate(&ev0));
    HIP_CHECK(pol, hipEventCreate(&ev1));
    HIP_CHECK(pol, mem.alloc(&d_ctl, sizeof ctl, "counters"));
    {
        const uint64_t guess = std::min<uint64_t>(nq * std::max<uint32_t>(tax->max_depth, 1), 2 * tax->n_tax + 4096);
        cap = std::max<uint64_t>(next_pow2(2 * guess), 1024);
        uint32_t max_probe = REPORT_PROBE_FIRST;
        ReportDev d{};
        d.lin = tax->d_lin; d.n_tax = tax->n_tax; d.stride = tax->dev_stride; d.node_base = tax->node_base;
        d.max_depth = tax->max_depth;
        d.recs = in.recs; d.n_queries = nq; d.row_src = in.row_src; d.n_rows = in.n_rows; d.row_stride = in.row_stride;
        d.by_query = in.by_query ? 1u : 0u; d.weight = in.weight; d.ctl = d_ctl;
        HIP_CHECK(pol, hipEventRecord(ev0, nullptr));
        for (;;) {
            ++attempts;
            if (cap > (1ull << 32)) { set_error("report: a table of %llu slots exceeds 32-bit path ids", (unsigned long long)cap); return BLU_ERR_ALLOC; }
            HIP_CHECK(pol, mem.alloc(&d_keys, cap * 8, "path table"));
            HIP_CHECK(pol, mem.alloc(&d_direct, cap * 8, "path table"));
            HIP_CHECK(pol, hipMemsetAsync(d_keys, 0xFF, cap * 8, nullptr));
            HIP_CHECK(pol, hipMemsetAsync(d_direct, 0, cap * 8, nullptr));
            HIP_CHECK(pol, hipMemsetAsync(d_ctl, 0, sizeof ctl, nullptr));
            d.keys = d_keys; d.direct = d_direct; d.cap_mask = (uint32_t)(cap - 1); d.max_probe = max_probe;
            if (nq) hipLaunchKernelGGL(report_paths, dim3((unsigned)((nq + RB * RQ - 1) / (RB * RQ))), dim3(RB), 0, 0, d);
            HIP_CHECK(pol, hipGetLastError());
            HIP_CHECK(pol, hipMemcpy(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost));
            if (ctl[2] & FLAG_BAD_RECORD) {
                set_error("report: record %llu has a taxon (status 0 / 1) but its reference row names no taxonomy row",
                          (unsigned long long)ctl[3]);
                return BLU_ERR_INVALID_ARG;
            }
            if (ctl[2] & FLAG_BAD_NODE) {
                set_error("report: record %llu has a path that begins with node id 0xFFFFFFFF, which no path may begin with",
                          (unsigned long long)ctl[CTL_BAD_NODE]);
                return BLU_ERR_INVALID_ARG;
            }
            if (!(ctl[2] & FLAG_OVERFLOW)) break;
            if (max_probe != REPORT_PROBE_FIRST) { set_error("report: path table overflow"); return BLU_ERR_HIP; }   // (cannot happen at load <= 1/2)
            // the estimate was short: again from zero, sized from the bound
            mem.free(d_keys); mem.free(d_direct); d_keys = d_direct = nullptr;
            HIP_CHECK(pol, hipMemsetAsync(d_ctl, 0, 8, nullptr));
            hipLaunchKernelGGL(report_bound, dim3((unsigned)std::min<uint64_t>((nq + RB - 1) / RB, 4096)), dim3(RB), 0, 0, in.recs, nq, d_ctl);
            HIP_CHECK(pol, hipGetLastError());
            unsigned long long bound = 0;
            HIP_CHECK(pol, hipMemcpy(&bound, d_ctl, 8, hipMemcpyDeviceToHost));
            cap = std::max<uint64_t>(next_pow2(2 * bound), 1024);
            max_probe = (uint32_t)std::min<uint64_t>(cap, 0xFFFFFFFFull);
        }
        HIP_CHECK(pol, mem.alloc(&d_at, (cap + 1) * 4, "path ids"));
        hipLaunchKernelGGL(report_flags, dim3((unsigned)((cap + 1 + 255) / 256)), dim3(256), 0, 0, d_keys, cap, d_at);
        HIP_CHECK(pol, hipGetLastError());
        HIP_CHECK(pol, mem.alloc(&d_tmp, scan_tmp_bytes_u32(cap + 1), "scan scratch"));
        HIP_CHECK(pol, exclusive_scan_u32(d_at, d_at, cap + 1, d_tmp));
        uint32_t np32 = 0;
        HIP_CHECK(pol, hipMemcpy(&np32, d_at + cap, 4, hipMemcpyDeviceToHost));
        n_paths = np32;
        HIP_CHECK(pol, mem.alloc(&d_paths, n_paths * sizeof(blu_report_path), "paths"));
        hipLaunchKernelGGL(report_compact, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, 0, d_keys, d_direct, d_at, cap, d_paths);
        HIP_CHECK(pol, hipGetLastError());
        HIP_CHECK(pol, hipEventRecord(ev1, nullptr));
        paths.resize(n_paths);
        if (n_paths) HIP_CHECK(pol, hipMemcpy(paths.data(), d_paths, n_paths * sizeof(blu_report_path), hipMemcpyDeviceToHost));
        float ms = 0;
        HIP_CHECK(pol, hipEventSynchronize(ev1));   // (no path came back: no copy has waited for the device yet)
        HIP_CHECK(pol, hipEventElapsedTime(&ms, ev0, ev1));
        out->t_device_ms = ms;
    }
    {
        // parents first (depth order, slot order inside a depth), then clade = direct + the children's clades
        const uint32_t NONE = REPORT_NONE;
        std::vector<uint32_t> at;
        parents_first(paths, at);
        blu_report_path* o = n_paths ? (blu_report_path*)malloc(n_paths * sizeof(blu_report_path)) : nullptr;
        if (n_paths && !o) { set_error("report: out of memory"); return BLU_ERR_ALLOC; }
        for (uint64_t i = 0; i < n_paths; ++i) {
            blu_report_path p = paths[i];
            p.parent = p.parent == NONE ? NONE : at[p.parent];
            p.clade = p.direct;
            o[at[i]] = p;
        }
        for (uint64_t i = n_paths; i-- > 0;)
            if (o[i].parent != NONE) o[o[i].parent].clade += o[i].clade;
        out->paths = o;
        out->n_paths = n_paths;
        out->unclassified = ctl[0];
        out->unplaced = ctl[1];
        uint64_t classified = 0;
        for (uint64_t i = 0; i < n_paths; ++i) if (o[i].parent == NONE) classified += o[i].clade;
        out->total = ctl[0] + ctl[1] + classified;
        out->table_slots = cap;
        out->attempts = attempts;
    }
    return BLU_OK;
}

int sample_table_device(const blu_taxonomy* tax, const ReportInput& in, const uint32_t* sample_of, uint32_t n_samples,
                        blu_sample_table* out) {
    const uint64_t nq = in.n_queries;
    unsigned long long *d_keys = nullptr, *d_ckeys = nullptr, *d_cval = nullptr, *d_ctl = nullptr, *d_fixed = nullptr;
    unsigned long long ctl[CTL_WORDS] = {};
    uint64_t cap = 0, ccap = 0;
    const uint64_t fixed_bytes = 2 * (uint64_t)n_samples * 8;
    HipPolicy pol{"sample table", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    SampleTables T;
    uint32_t& attempts = T.attempts;
    HIP_CHECK(pol, hipEventCreate(&T.ev0));
    HIP_CHECK(pol, hipEventCreate(&T.ev1));
    HIP_CHECK(pol, mem.alloc(&d_ctl, sizeof ctl, "counters"));
    HIP_CHECK(pol, mem.alloc(&d_fixed, fixed_bytes, "per-sample counters"));
    {
        // paths as the report sizes them; cells: the paths plus one per query (a sample's queries mostly share their upper
        // levels), at most one per level of every query
        const uint64_t depth = std::max<uint32_t>(tax->max_depth, 1);
        const uint64_t guess = std::min<uint64_t>(nq * depth, 2 * tax->n_tax + 4096);
        const uint64_t cguess = std::min<uint64_t>(nq * depth, guess + nq);
        cap = std::max<uint64_t>(next_pow2(2 * guess), 1024);
        ccap = std::max<uint64_t>(next_pow2(2 * cguess), 1024);
        uint32_t max_probe = REPORT_PROBE_FIRST;
        SampleDev d{};
        d.r.lin = tax->d_lin; d.r.n_tax = tax->n_tax; d.r.stride = tax->dev_stride; d.r.node_base = tax->node_base;
        d.r.max_depth = tax->max_depth;
        d.r.recs = in.recs; d.r.n_queries = nq; d.r.row_src = in.row_src; d.r.n_rows = in.n_rows; d.r.row_stride = in.row_stride;
        d.r.by_query = in.by_query ? 1u : 0u; d.r.weight = in.weight; d.r.ctl = d_ctl;
        d.sample_of = sample_of; d.n_samples = n_samples; d.fixed = d_fixed;
        HIP_CHECK(pol, hipEventRecord(T.ev0, nullptr));
        for (;;) {
            ++attempts;
            // (path ids below 2^31: the two ids above are the fixed rows' in the cell keys)
            if (cap > (1ull << 31) || ccap > (1ull << 32)) {
                set_error("sample table: tables of %llu / %llu slots exceed 32-bit ids", (unsigned long long)cap, (unsigned long long)ccap);
                return BLU_ERR_ALLOC;
            }
            HIP_CHECK(pol, mem.alloc(&d_keys, cap * 8, "path table"));
            HIP_CHECK(pol, mem.alloc(&d_ckeys, ccap * 8, "cell table"));
            HIP_CHECK(pol, mem.alloc(&d_cval, ccap * 8, "cell table"));
            HIP_CHECK(pol, hipMemsetAsync(d_keys, 0xFF, cap * 8, nullptr));
            HIP_CHECK(pol, hipMemsetAsync(d_ckeys, 0xFF, ccap * 8, nullptr));
            HIP_CHECK(pol, hipMemsetAsync(d_cval, 0, ccap * 8, nullptr));
            HIP_CHECK(pol, hipMemsetAsync(d_ctl, 0, sizeof ctl, nullptr));
            HIP_CHECK(pol, hipMemsetAsync(d_fixed, 0, fixed_bytes, nullptr));
            d.r.keys = d_keys; d.r.cap_mask = (uint32_t)(cap - 1); d.r.max_probe = max_probe;
            d.cell_keys = d_ckeys; d.cell_val = d_cval; d.cell_mask = (uint32_t)(ccap - 1);
            if (nq) hipLaunchKernelGGL(sample_cells, dim3((unsigned)((nq + RB * RQ - 1) / (RB * RQ))), dim3(RB), 0, 0, d);
            HIP_CHECK(pol, hipGetLastError());
            HIP_CHECK(pol, hipMemcpy(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost));
            if (ctl[2] & FLAG_BAD_SAMPLE) {
                set_error("sample table: query %llu has a sample id that is not below n_samples = %u", (unsigned long long)ctl[4], n_samples);
                return BLU_ERR_INVALID_ARG;
            }
            if (ctl[2] & FLAG_BAD_RECORD) {
                set_error("sample table: record %llu has a taxon (status 0 / 1) but its reference row names no taxonomy row",
                          (unsigned long long)ctl[3]);
                return BLU_ERR_INVALID_ARG;
            }
            if (ctl[2] & FLAG_BAD_NODE) {
                set_error("sample table: record %llu has a path that begins with node id 0xFFFFFFFF, which no path may begin with",
                          (unsigned long long)ctl[CTL_BAD_NODE]);
                return BLU_ERR_INVALID_ARG;
            }
            if (!(ctl[2] & FLAG_OVERFLOW)) break;
            if (max_probe != REPORT_PROBE_FIRST) { set_error("sample table: table overflow"); return BLU_ERR_HIP; }   // (cannot happen at load <= 1/2)
            // the estimate was short: both tables again from zero, sized from the bound on paths and on cells
            mem.free(d_keys); mem.free(d_ckeys); mem.free(d_cval); d_keys = d_ckeys = d_cval = nullptr;
            HIP_CHECK(pol, hipMemsetAsync(d_ctl, 0, 8, nullptr));
            hipLaunchKernelGGL(report_bound, dim3((unsigned)std::min<uint64_t>((nq + RB - 1) / RB, 4096)), dim3(RB), 0, 0, in.recs, nq, d_ctl);
            HIP_CHECK(pol, hipGetLastError());
            unsigned long long bound = 0;
            HIP_CHECK(pol, hipMemcpy(&bound, d_ctl, 8, hipMemcpyDeviceToHost));
            cap = ccap = std::max<uint64_t>(next_pow2(2 * bound), 1024);
            max_probe = (uint32_t)std::min<uint64_t>(cap, 0xFFFFFFFFull);
        }
    }
    T.keys = d_keys; T.ckeys = d_ckeys; T.cval = d_cval; T.fixed = d_fixed; T.cap = cap; T.ccap = ccap;
    return sample_table_finish(pol, mem, T, n_samples, out);
}

int sample_table_counts_device(const blu_taxonomy* tax, const ReportInput& in, const CountRows& rows, uint32_t n_samples,
                               blu_sample_table* out) {
    const uint64_t nq = in.n_queries;
    unsigned long long *d_keys = nullptr, *d_ckeys = nullptr, *d_cval = nullptr, *d_ctl = nullptr, *d_fixed = nullptr;
    unsigned long long ctl[CTL_WORDS] = {};
    const uint64_t fixed_bytes = 2 * (uint64_t)n_samples * 8;
    HipPolicy pol{"count table", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    SampleTables T;
    HIP_CHECK(pol, hipEventCreate(&T.ev0));
    HIP_CHECK(pol, hipEventCreate(&T.ev1));
    HIP_CHECK(pol, mem.alloc(&d_ctl, sizeof ctl, "counters"));
    HIP_CHECK(pol, mem.alloc(&d_fixed, fixed_bytes, "per-sample counters"));
    CountDev d{};
    d.s.r.lin = tax->d_lin; d.s.r.n_tax = tax->n_tax; d.s.r.stride = tax->dev_stride; d.s.r.node_base = tax->node_base;
    d.s.r.max_depth = tax->max_depth;
    d.s.r.recs = in.recs; d.s.r.n_queries = nq; d.s.r.row_src = in.row_src; d.s.r.n_rows = in.n_rows; d.s.r.row_stride = in.row_stride;
    d.s.r.by_query = in.by_query ? 1u : 0u; d.s.r.ctl = d_ctl;
    d.s.n_samples = n_samples; d.s.fixed = d_fixed;
    d.rows = rows;
    HIP_CHECK(pol, hipEventRecord(T.ev0, nullptr));
    // the bounds first: P on the paths, and on the cells the sum of levels x non-zeros (one pass over the records and row_ptr)
    unsigned long long bound[2] = {0, 0};
    HIP_CHECK(pol, hipMemsetAsync(d_ctl, 0, sizeof ctl, nullptr));
    if (nq) hipLaunchKernelGGL(count_bound, dim3((unsigned)std::min<uint64_t>((nq + RB - 1) / RB, 4096)), dim3(RB), 0, 0, in.recs, rows, nq, d_ctl);
    HIP_CHECK(pol, hipGetLastError());
    HIP_CHECK(pol, hipMemcpy(bound, d_ctl, sizeof bound, hipMemcpyDeviceToHost));
    // paths as the report sizes them; cells: no more than the bound, and no more than every path in every sample
    const uint64_t guess = std::min<uint64_t>(nq * std::max<uint32_t>(tax->max_depth, 1), 2 * tax->n_tax + 4096);
    uint64_t cap = std::max<uint64_t>(next_pow2(2 * guess), 1024);
    uint64_t ccap = std::max<uint64_t>(next_pow2(2 * std::min<uint64_t>(bound[1], guess * std::max<uint32_t>(n_samples, 1))), 1024);
    uint32_t max_probe = REPORT_PROBE_FIRST;
    for (;;) {
        ++T.attempts;
        // (path ids below 2^31: the two ids above are the fixed rows' in the cell keys)
        if (cap > (1ull << 31) || ccap > (1ull << 32)) {
            set_error("count table: tables of %llu / %llu slots exceed 32-bit ids", (unsigned long long)cap, (unsigned long long)ccap);
            return BLU_ERR_ALLOC;
        }
        HIP_CHECK(pol, mem.alloc(&d_keys, cap * 8, "path table"));
        HIP_CHECK(pol, mem.alloc(&d_ckeys, ccap * 8, "cell table"));
        HIP_CHECK(pol, mem.alloc(&d_cval, ccap * 8, "cell table"));
        HIP_CHECK(pol, hipMemsetAsync(d_keys, 0xFF, cap * 8, nullptr));
        HIP_CHECK(pol, hipMemsetAsync(d_ckeys, 0xFF, ccap * 8, nullptr));
        HIP_CHECK(pol, hipMemsetAsync(d_cval, 0, ccap * 8, nullptr));
        HIP_CHECK(pol, hipMemsetAsync(d_ctl, 0, sizeof ctl, nullptr));
        HIP_CHECK(pol, hipMemsetAsync(d_fixed, 0, fixed_bytes, nullptr));
        d.s.r.keys = d_keys; d.s.r.cap_mask = (uint32_t)(cap - 1); d.s.r.max_probe = max_probe;
        d.s.cell_keys = d_ckeys; d.s.cell_val = d_cval; d.s.cell_mask = (uint32_t)(ccap - 1);
        if (nq) hipLaunchKernelGGL(count_cells, dim3((unsigned)((nq + COUNT_Q_BLOCK - 1) / COUNT_Q_BLOCK)), dim3(RB), 0, 0, d);
        HIP_CHECK(pol, hipGetLastError());
        HIP_CHECK(pol, hipMemcpy(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost));
        if (ctl[2] & FLAG_BAD_ROW) {
            set_error("count table: query %llu has a row_ptr that decreases or ends past the %llu non-zeros", (unsigned long long)ctl[5],
                      (unsigned long long)rows.nnz);
            return BLU_ERR_INVALID_ARG;
        }
        if (ctl[2] & FLAG_BAD_SAMPLE) {
            set_error("count table: query %llu has a sample id that is not below n_samples = %u", (unsigned long long)ctl[4], n_samples);
            return BLU_ERR_INVALID_ARG;
        }
        if (ctl[2] & FLAG_BAD_RECORD) {
            set_error("count table: record %llu has a taxon (status 0 / 1) but its reference row names no taxonomy row",
                      (unsigned long long)ctl[3]);
            return BLU_ERR_INVALID_ARG;
        }
        if (ctl[2] & FLAG_BAD_NODE) {
            set_error("count table: record %llu has a path that begins with node id 0xFFFFFFFF, which no path may begin with",
                      (unsigned long long)ctl[CTL_BAD_NODE]);
            return BLU_ERR_INVALID_ARG;
        }
        if (!(ctl[2] & FLAG_OVERFLOW)) break;
        if (max_probe != REPORT_PROBE_FIRST) { set_error("count table: table overflow"); return BLU_ERR_HIP; }   // (cannot happen at load <= 1/2)
        // an estimate was short: both tables again from zero, at twice their bounds, where a probe always ends
        mem.free(d_keys); mem.free(d_ckeys); mem.free(d_cval); d_keys = d_ckeys = d_cval = nullptr;
        cap = std::max<uint64_t>(next_pow2(2 * bound[0]), 1024);
        ccap = std::max<uint64_t>(next_pow2(2 * bound[1]), 1024);
        max_probe = (uint32_t)std::min<uint64_t>(std::max(cap, ccap), 0xFFFFFFFFull);
    }
    T.keys = d_keys; T.ckeys = d_ckeys; T.cval = d_cval; T.fixed = d_fixed; T.cap = cap; T.ccap = ccap;
    return sample_table_finish(pol, mem, T, n_samples, out);
}

}  // namespace blu

using namespace blu;

extern "C" {

int blu_consensus_report(const blu_taxonomy* tax, const blu_hits* hits, const blu_result* results, const uint32_t* weights,
                         void* stream, blu_report* out) {
    if (!tax || !hits || !out || (hits->n_queries && !results)) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    memset(out, 0, sizeof *out);
    if (tax->device < 0) { set_error("host-only taxonomy handle: blu_consensus_report needs a HIP device (no CPU fallback)"); return BLU_ERR_NO_DEVICE; }
    const uint32_t* src = hits->packed ? hits->packed : hits->packed64 ? hits->packed64 : hits->tax_row;
    const uint32_t stride = hits->packed ? 4u : hits->packed64 ? 6u : 1u;
    const uint64_t nq = hits->n_queries, nh = hits->n_hits;
    if (nq && !src) { set_error("blu_consensus_report: no tax_row column"); return BLU_ERR_INVALID_ARG; }
    if (hipSetDevice(tax->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", tax->device); return BLU_ERR_NO_DEVICE; }
    ReportInput in{results, nq, src, nh, stride, false, weights};
    if (hits->on_device) {
        if (((uintptr_t)results & 15u) != 0) { set_error("blu_consensus_report: device records must be 16-byte aligned"); return BLU_ERR_INVALID_ARG; }
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) { set_error("blu_consensus_report: stream synchronise failed"); return BLU_ERR_HIP; }
        try { return report_device(tax, in, out); }
        catch (const std::bad_alloc&) { set_error("out of memory"); return BLU_ERR_ALLOC; }
    }
    // host pointers: the records, each record's engine row (gathered here: 4 bytes a query instead of the whole column)
    // and the weights go up
    HipPolicy pol{"blu_consensus_report", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    blu_result* d_recs = nullptr;
    uint32_t *d_rows = nullptr, *d_w = nullptr;
    try {
        std::vector<uint32_t> rows(nq, BLU_UNMATCHED_TAXID);
        for (uint64_t q = 0; q < nq; ++q)
            if (results[q].status < 2 && results[q].ref_row < nh) rows[q] = src[(uint64_t)results[q].ref_row * stride];
        HIP_CHECK(pol, mem.alloc(&d_recs, nq * sizeof(blu_result), "records"));
        HIP_CHECK(pol, mem.alloc(&d_rows, nq * 4, "rows"));
        if (weights) HIP_CHECK(pol, mem.alloc(&d_w, nq * 4, "weights"));
        if (nq) {
            HIP_CHECK(pol, hipMemcpy(d_recs, results, nq * sizeof(blu_result), hipMemcpyHostToDevice));
            HIP_CHECK(pol, hipMemcpy(d_rows, rows.data(), nq * 4, hipMemcpyHostToDevice));
            if (weights) HIP_CHECK(pol, hipMemcpy(d_w, weights, nq * 4, hipMemcpyHostToDevice));
        }
        ReportInput hin{d_recs, nq, d_rows, nq, 1u, true, d_w};
        return report_device(tax, hin, out);
    } catch (const std::bad_alloc&) { set_error("out of memory"); return BLU_ERR_ALLOC; }
}

int blu_consensus_sample_table(const blu_taxonomy* tax, const blu_hits* hits, const blu_result* results, const uint32_t* weights,
                               const uint32_t* sample_of, uint32_t n_samples, void* stream, blu_sample_table* out) {
    if (!tax || !hits || !out || (hits->n_queries && (!results || !sample_of))) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    memset(out, 0, sizeof *out);
    if (tax->device < 0) { set_error("host-only taxonomy handle: blu_consensus_sample_table needs a HIP device (no CPU fallback)"); return BLU_ERR_NO_DEVICE; }
    const uint32_t* src = hits->packed ? hits->packed : hits->packed64 ? hits->packed64 : hits->tax_row;
    const uint32_t stride = hits->packed ? 4u : hits->packed64 ? 6u : 1u;
    const uint64_t nq = hits->n_queries, nh = hits->n_hits;
    if (nq && !src) { set_error("blu_consensus_sample_table: no tax_row column"); return BLU_ERR_INVALID_ARG; }
    if (hipSetDevice(tax->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", tax->device); return BLU_ERR_NO_DEVICE; }
    ReportInput in{results, nq, src, nh, stride, false, weights};
    if (hits->on_device) {
        if (((uintptr_t)results & 15u) != 0) { set_error("blu_consensus_sample_table: device records must be 16-byte aligned"); return BLU_ERR_INVALID_ARG; }
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) { set_error("blu_consensus_sample_table: stream synchronise failed"); return BLU_ERR_HIP; }
        try { return sample_table_device(tax, in, sample_of, n_samples, out); }
        catch (const std::bad_alloc&) { set_error("out of memory"); return BLU_ERR_ALLOC; }
    }
    // host pointers: the records, each record's engine row, the weights and the sample ids go up
    HipPolicy pol{"blu_consensus_sample_table", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    blu_result* d_recs = nullptr;
    uint32_t *d_rows = nullptr, *d_w = nullptr, *d_s = nullptr;
    try {
        std::vector<uint32_t> rows(nq, BLU_UNMATCHED_TAXID);
        for (uint64_t q = 0; q < nq; ++q)
            if (results[q].status < 2 && results[q].ref_row < nh) rows[q] = src[(uint64_t)results[q].ref_row * stride];
        HIP_CHECK(pol, mem.alloc(&d_recs, nq * sizeof(blu_result), "records"));
        HIP_CHECK(pol, mem.alloc(&d_rows, nq * 4, "rows"));
        HIP_CHECK(pol, mem.alloc(&d_s, nq * 4, "sample ids"));
        if (weights) HIP_CHECK(pol, mem.alloc(&d_w, nq * 4, "weights"));
        if (nq) {
            HIP_CHECK(pol, hipMemcpy(d_recs, results, nq * sizeof(blu_result), hipMemcpyHostToDevice));
            HIP_CHECK(pol, hipMemcpy(d_rows, rows.data(), nq * 4, hipMemcpyHostToDevice));
            HIP_CHECK(pol, hipMemcpy(d_s, sample_of, nq * 4, hipMemcpyHostToDevice));
            if (weights) HIP_CHECK(pol, hipMemcpy(d_w, weights, nq * 4, hipMemcpyHostToDevice));
        }
        ReportInput hin{d_recs, nq, d_rows, nq, 1u, true, d_w};
        return sample_table_device(tax, hin, d_s, n_samples, out);
    } catch (const std::bad_alloc&) { set_error("out of memory"); return BLU_ERR_ALLOC; }
}

int blu_consensus_sample_table_counts(const blu_taxonomy* tax, const blu_hits* hits, const blu_result* results, const blu_count_rows* rows,
                                      uint32_t n_samples, void* stream, blu_sample_table* out) {
    if (!tax || !hits || !out || !rows || (hits->n_queries && (!results || !rows->row_ptr))) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    memset(out, 0, sizeof *out);
    if (tax->device < 0) { set_error("host-only taxonomy handle: blu_consensus_sample_table_counts needs a HIP device (no CPU fallback)"); return BLU_ERR_NO_DEVICE; }
    const uint32_t* src = hits->packed ? hits->packed : hits->packed64 ? hits->packed64 : hits->tax_row;
    const uint32_t stride = hits->packed ? 4u : hits->packed64 ? 6u : 1u;
    const uint64_t nq = hits->n_queries, nh = hits->n_hits;
    if (nq && !src) { set_error("blu_consensus_sample_table_counts: no tax_row column"); return BLU_ERR_INVALID_ARG; }
    if (hipSetDevice(tax->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", tax->device); return BLU_ERR_NO_DEVICE; }
    HipPolicy pol{"blu_consensus_sample_table_counts", BLU_ERR_ALLOC};
    uint64_t nnz = 0;   // the last offset: what the two arrays hold, and what no row may pass
    if (hits->on_device) {
        if (((uintptr_t)results & 15u) != 0) { set_error("blu_consensus_sample_table_counts: device records must be 16-byte aligned"); return BLU_ERR_INVALID_ARG; }
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) { set_error("blu_consensus_sample_table_counts: stream synchronise failed"); return BLU_ERR_HIP; }
        if (nq) HIP_CHECK(pol, hipMemcpy(&nnz, rows->row_ptr + nq, 8, hipMemcpyDeviceToHost));
        if (nnz && (!rows->sample || !rows->count)) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
        ReportInput in{results, nq, src, nh, stride, false, nullptr};
        try { return sample_table_counts_device(tax, in, CountRows{rows->row_ptr, rows->sample, rows->count, nnz}, n_samples, out); }
        catch (const std::bad_alloc&) { set_error("out of memory"); return BLU_ERR_ALLOC; }
    }
    // host pointers: the records, each record's engine row and the three arrays of the rows go up
    if (nq) nnz = rows->row_ptr[nq];
    if (nnz && (!rows->sample || !rows->count)) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    DeviceArena mem(pol);
    blu_result* d_recs = nullptr;
    uint32_t *d_rows = nullptr, *d_s = nullptr, *d_c = nullptr;
    uint64_t* d_ptr = nullptr;
    try {
        std::vector<uint32_t> erows(nq, BLU_UNMATCHED_TAXID);
        for (uint64_t q = 0; q < nq; ++q)
            if (results[q].status < 2 && results[q].ref_row < nh) erows[q] = src[(uint64_t)results[q].ref_row * stride];
        HIP_CHECK(pol, mem.upload(&d_recs, results, nq, "records"));
        HIP_CHECK(pol, mem.upload(&d_rows, erows.data(), nq, "rows"));
        HIP_CHECK(pol, mem.upload(&d_ptr, rows->row_ptr, nq ? nq + 1 : 0, "row offsets"));
        HIP_CHECK(pol, mem.upload(&d_s, rows->sample, nnz, "sample ids"));
        HIP_CHECK(pol, mem.upload(&d_c, rows->count, nnz, "counts"));
        ReportInput hin{d_recs, nq, d_rows, nq, 1u, true, nullptr};
        return sample_table_counts_device(tax, hin, CountRows{d_ptr, d_s, d_c, nnz}, n_samples, out);
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
