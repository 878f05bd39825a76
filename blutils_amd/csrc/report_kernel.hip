// Taxon abundance report (include/blu_consensus.h: blu_consensus_report): the per-query records of the engine ->
// the distinct taxonomy paths with their direct counts, on the device.
//
// A query's path is exactly what the renderer writes as `taxonomy` (pipeline.cpp, Renderer::lineage): the levels j of
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
    unsigned long long* ctl;      // {unclassified, unplaced, flags, bad query}
};

__device__ __forceinline__ uint32_t mix_key(unsigned long long k) {   // murmur3 fmix64
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (uint32_t)k;
}

// slot of (parent, node), inserted if new; REPORT_NONE when max_probe slots were all taken by other keys
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
            path = intern(d, path, lin[d.node_base + j]);
            if (path == REPORT_NONE) { ok = false; break; }
        }
        if (!ok) { flags |= FLAG_OVERFLOW; continue; }
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

uint64_t next_pow2(uint64_t x) { uint64_t c = 1; while (c < x) c <<= 1; return c; }

}  // namespace

int report_device(const blu_taxonomy* tax, const ReportInput& in, blu_report* out) {
    const uint64_t nq = in.n_queries;
    unsigned long long *d_keys = nullptr, *d_direct = nullptr, *d_ctl = nullptr;
    uint32_t* d_at = nullptr;
    void* d_tmp = nullptr;
    blu_report_path* d_paths = nullptr;
    unsigned long long ctl[4] = {0, 0, 0, 0};
    uint64_t cap = 0, n_paths = 0;
    uint32_t attempts = 0;
    std::vector<blu_report_path> paths;
    HipPolicy pol{"report", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    struct Events { hipEvent_t ev0 = nullptr, ev1 = nullptr; ~Events() { if (ev0) (void)hipEventDestroy(ev0); if (ev1) (void)hipEventDestroy(ev1); } } ev;
    hipEvent_t &ev0 = ev.ev0, &ev1 = ev.ev1;
    HIP_CHECK(pol, hipEventCreate(&ev0));
    HIP_CHECK(pol, hipEventCreate(&ev1));
    HIP_CHECK(pol, mem.alloc(&d_ctl, 4 * 8, "counters"));
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
            HIP_CHECK(pol, hipMemsetAsync(d_ctl, 0, 4 * 8, nullptr));
            d.keys = d_keys; d.direct = d_direct; d.cap_mask = (uint32_t)(cap - 1); d.max_probe = max_probe;
            if (nq) hipLaunchKernelGGL(report_paths, dim3((unsigned)((nq + RB * RQ - 1) / (RB * RQ))), dim3(RB), 0, 0, d);
            HIP_CHECK(pol, hipGetLastError());
            HIP_CHECK(pol, hipMemcpy(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost));
            if (ctl[2] & FLAG_BAD_RECORD) {
                set_error("report: record %llu has a taxon (status 0 / 1) but its reference row names no taxonomy row",
                          (unsigned long long)ctl[3]);
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
        HIP_CHECK(pol, hipEventElapsedTime(&ms, ev0, ev1));
        out->t_device_ms = ms;
    }
    {
        // parents first (depth order, slot order inside a depth), then clade = direct + the children's clades
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
        std::vector<uint32_t> at(n_paths);
        for (uint64_t i = 0; i < n_paths; ++i) at[i] = (uint32_t)first[depth[i]]++;
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

void blu_report_free(blu_report* report) {
    if (!report) return;
    free(report->paths);
    report->paths = nullptr;
    report->n_paths = 0;
}

}  // extern "C"
