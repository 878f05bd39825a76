// Per-query assignment support (include/blu_consensus.h: blu_consensus_support): how many of a query's hits
// back the taxon its record names.  A second pass over what a run leaves on the device: the bit-score column, one engine
// row id per hit, the 32-byte records and the taxonomy's sorted-lineage tables.
//
// The assigned clade of a record is the set of taxonomy rows that share the first L + 1 nodes of the reference row's
// lineage, L = the highest bit of level_mask.  The rows sit in lexicographic lineage order and lcp8[i] is the number of
// leading levels sorted rows i and i + 1 share, so the clade is ONE range [lo, hi] of sorted positions: the maximal run
// around pos(R) with lcp8 >= L + 1 on both sides.  The range is found once per query; every hit is then tested with one
// compare on the low BLU_ROW_BITS bits of its row id — no lineage is read per hit.
//
// One wave per query.  The range search probes 64 entries of lcp8 at once either side of the reference row (the common
// case — a species or genus of a few rows — ends there); a longer run skips whole 16-entry blocks through the `rmq` sparse
// table, every level probed by a lane of its own, the largest power of two that still holds taken each time, and ends with
// one more 64-entry probe.  The segment is read 64 hits at a time, however long it is; each lane keeps its running maximum
// and resets its top-group counters when that rises, six integer sums and the maximum are reduced across the wave, and lane
// 0 stores the 40-byte record.  No atomics, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "hit_pass.h"

namespace blu {
namespace {

constexpr uint32_t SB = 256;                         // threads per block: four waves, four queries
constexpr uint32_t POS_MASK = (1u << BLU_ROW_BITS) - 1u;

struct SupportDev {
    const uint8_t* lcp8;          // TaxDev::lcp8
    const uint8_t* rmq;           // TaxDev::rmq
    uint32_t rmq_nb;
    uint32_t n_tax;
    const blu_result* recs;
    uint64_t n_queries;
    const unsigned long long* seg_off;
    const int32_t* bitscore;
    const uint32_t* row_src;      // engine row id of hit i: row_src[i * row_stride]
    uint32_t row_stride;
    uint64_t n_hits;
    blu_support* out;
    unsigned long long* ctl;      // {bad record seen, its query index}
};

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// hi: the last sorted position of the run of rows that share `need` levels with row `pos` (wave-uniform arguments and result)
__device__ __forceinline__ uint32_t clade_end(const SupportDev& d, uint32_t pos, uint32_t need, uint32_t lane) {
    const uint32_t last = d.n_tax - 1u;              // lcp8 has `last` entries; what follows is 0xFF padding
    uint32_t cur = pos;                              // lcp8[pos .. cur) hold
    for (;;) {
        const uint32_t i = cur + lane;
        const bool fail = i >= last || d.lcp8[i] < need;
        const unsigned long long f = __ballot(fail);
        if (f) return min(cur + (uint32_t)__ffsll((long long)f) - 1u, last);
        cur = (cur + 64u) & ~15u;                    // (a block boundary at or below: a few entries are looked at twice)
        uint32_t b = cur >> 4;
        for (;;) {                                   // whole blocks that hold, the largest power of two first
            const uint32_t w = lane < 32u ? 1u << lane : 0u;
            const bool ok = w && w <= d.rmq_nb && b <= d.rmq_nb - w && d.rmq[(uint64_t)lane * d.rmq_nb + b] >= need;
            const unsigned long long m = __ballot(ok);
            if (!m) break;
            b += 1u << (63 - __clzll((long long)m));
        }
        cur = b << 4;
        if (cur >= last) return last;
    }
}

// lo: the first sorted position of that run
__device__ __forceinline__ uint32_t clade_begin(const SupportDev& d, uint32_t pos, uint32_t need, uint32_t lane) {
    uint32_t cur = pos;                              // lcp8[cur .. pos) hold
    for (;;) {
        const bool fail = lane >= cur || d.lcp8[cur - 1u - lane] < need;
        const unsigned long long f = __ballot(fail);
        if (f) return cur - ((uint32_t)__ffsll((long long)f) - 1u);
        cur = (cur - 64u + 15u) & ~15u;              // (a block boundary at or above)
        uint32_t b = cur >> 4;                       // blocks [.., b) lie to the left
        for (;;) {
            const uint32_t w = lane < 32u ? 1u << lane : 0u;
            const bool ok = w && w <= b && d.rmq[(uint64_t)lane * d.rmq_nb + (b - w)] >= need;
            const unsigned long long m = __ballot(ok);
            if (!m) break;
            b -= 1u << (63 - __clzll((long long)m));
        }
        cur = b << 4;
        if (cur == 0) return 0;
    }
}

__global__ __launch_bounds__(SB) void support_counts(SupportDev d) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t q = (uint64_t)blockIdx.x * (SB / 64) + (threadIdx.x >> 6);
    if (q >= d.n_queries) return;                    // (wave-uniform)
    uint64_t s0, s1;
    segment_of(d.seg_off, q, d.n_hits, &s0, &s1);
    const uint4* rp = reinterpret_cast<const uint4*>(d.recs + q);
    const uint4 ra = rp[0];
    const uint2 rb = *reinterpret_cast<const uint2*>(rp + 1);
    const uint32_t status = ra.x & 0xFFu;
    const uint32_t ref_row = ra.w;
    const unsigned long long mask = (unsigned long long)rb.x | ((unsigned long long)rb.y << 32);

    // the clade: sorted positions [lo, hi]; lo > hi = none
    uint32_t lo = 1, hi = 0;
    if (status < 2u) {
        uint32_t row = BLU_UNMATCHED_TAXID;
        if ((uint64_t)ref_row < d.n_hits) row = d.row_src[(uint64_t)ref_row * d.row_stride];
        const uint32_t pos = row & POS_MASK, len = row >> BLU_ROW_BITS;
        if (row == BLU_UNMATCHED_TAXID || pos >= d.n_tax) {
            if (lane == 0) { d.ctl[0] = 1ull; d.ctl[1] = q; }
        } else if (mask == 0) {                      // taxonomy "": the empty prefix, every matched hit
            lo = 0; hi = d.n_tax - 1u;
        } else {
            const uint32_t need = 64u - (uint32_t)__clzll((long long)mask);   // L + 1
            if (need <= len) {
                hi = clade_end(d, pos, need, lane);
                lo = clade_begin(d, pos, need, lane);
            }
        }
    }

    int32_t top = INT32_MIN;
    uint32_t n_top = 0, n_top_sup = 0, n_matched = 0, n_sup = 0;
    long long bits = 0, sup_bits = 0;
    for (uint64_t i = s0 + lane; i < s1; i += 64) {
        const int32_t bs = d.bitscore[i];
        const uint32_t row = d.row_src[i * d.row_stride];
        const uint32_t pos = row & POS_MASK;
        // matched: a row of the taxonomy whose lineage parsed (a bad lineage has length 0 in its row id)
        const bool matched = row != BLU_UNMATCHED_TAXID && pos < d.n_tax && (row >> BLU_ROW_BITS) != 0u;
        const bool sup = matched && pos >= lo && pos <= hi;
        if (bs > top || i == s0 + lane) { top = bs; n_top = 0; n_top_sup = 0; }
        if (bs == top) { n_top += 1u; n_top_sup += sup ? 1u : 0u; }
        n_matched += matched ? 1u : 0u;
        n_sup += sup ? 1u : 0u;
        bits += (long long)bs;
        sup_bits += sup ? (long long)bs : 0ll;
    }
    const bool any = s0 + lane < s1;
    const int32_t wtop = wave_max32(any ? top : INT32_MIN);
    const bool in_top = any && top == wtop;
    const unsigned long long tops = wave_sum64(in_top ? ((unsigned long long)n_top << 32) | n_top_sup : 0ull);
    const unsigned long long sums = wave_sum64(((unsigned long long)n_matched << 32) | n_sup);   // (each half < 2^32: n_hits is)
    const unsigned long long wbits = wave_sum64((unsigned long long)bits);
    const unsigned long long wsup = wave_sum64((unsigned long long)sup_bits);
    if (lane == 0) {
        blu_support o;
        o.n_hits = (uint32_t)(s1 - s0);
        o.n_matched = (uint32_t)(sums >> 32);
        o.n_top = (uint32_t)(tops >> 32);
        o.n_top_support = (uint32_t)tops;
        o.n_support = (uint32_t)sums;
        o.top_score = s1 > s0 ? wtop : 0;
        o.bits = (long long)wbits;
        o.support_bits = (long long)wsup;
        d.out[q] = o;
    }
}

}  // namespace

int support_device(const blu_taxonomy* tax, const SupportInput& in, blu_support* d_out) {
    HipPolicy pol{"support", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    if (in.n_queries == 0) return BLU_OK;
    unsigned long long* d_ctl = nullptr;
    unsigned long long ctl[2] = {0, 0};
    HIP_CHECK(pol, mem.alloc(&d_ctl, sizeof ctl, "flags"));
    HIP_CHECK(pol, hipMemsetAsync(d_ctl, 0, sizeof ctl, nullptr));
    SupportDev d{};
    d.lcp8 = tax->d_lcp8; d.rmq = tax->d_rmq; d.rmq_nb = tax->rmq_nb; d.n_tax = (uint32_t)tax->n_tax;
    d.recs = in.recs; d.n_queries = in.n_queries; d.seg_off = (const unsigned long long*)in.seg_off; d.bitscore = in.bitscore;
    d.row_src = in.row_src; d.row_stride = in.row_stride; d.n_hits = in.n_hits; d.out = d_out; d.ctl = d_ctl;
    const uint64_t blocks = (in.n_queries + SB / 64 - 1) / (SB / 64);
    if (blocks > 0x7FFFFFFFull) { set_error("support: too many queries for one launch"); return BLU_ERR_INVALID_ARG; }
    hipLaunchKernelGGL(support_counts, dim3((unsigned)blocks), dim3(SB), 0, 0, d);
    HIP_CHECK(pol, hipGetLastError());
    HIP_CHECK(pol, hipMemcpy(ctl, d_ctl, sizeof ctl, hipMemcpyDeviceToHost));   // (waits for the kernel: `out` is complete)
    if (ctl[0]) {
        set_error("support: record %llu has a taxon (status 0 / 1) but its reference row names no taxonomy row", ctl[1]);
        return BLU_ERR_INVALID_ARG;
    }
    return BLU_OK;
}

}  // namespace blu

using namespace blu;

extern "C" {

int blu_consensus_support(const blu_taxonomy* tax, const blu_hits* hits, const blu_result* results, void* stream, blu_support* out) {
    if (!tax || !hits || (hits->n_queries && (!results || !out))) { set_error("null argument"); return BLU_ERR_INVALID_ARG; }
    if (tax->device < 0) { set_error("host-only taxonomy handle: blu_consensus_support needs a HIP device (no CPU fallback)"); return BLU_ERR_NO_DEVICE; }
    const uint32_t* src = hits->packed ? hits->packed : hits->packed64 ? hits->packed64 : hits->tax_row;
    const uint32_t stride = hits->packed ? 4u : hits->packed64 ? 6u : 1u;
    const uint64_t nq = hits->n_queries, nh = hits->n_hits;
    if (nq == 0) return BLU_OK;
    if (nh >= 0xFFFFFFFFull) { set_error("n_hits must be < 2^32 - 1 per call"); return BLU_ERR_INVALID_ARG; }
    if (!hits->seg_off || (nh && (!src || !hits->bitscore))) { set_error("blu_consensus_support: seg_off, bitscore and the row ids are needed"); return BLU_ERR_INVALID_ARG; }
    if (hipSetDevice(tax->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", tax->device); return BLU_ERR_NO_DEVICE; }
    if (hits->on_device) {
        if (((uintptr_t)results & 15u) != 0 || ((uintptr_t)out & 7u) != 0) { set_error("blu_consensus_support: device records must be 16-byte aligned, `out` 8-byte aligned"); return BLU_ERR_INVALID_ARG; }
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) { set_error("blu_consensus_support: stream synchronise failed"); return BLU_ERR_HIP; }
        SupportInput in{results, nq, hits->seg_off, hits->bitscore, src, stride, nh};
        try { return support_device(tax, in, out); }
        catch (const std::bad_alloc&) { set_error("out of memory"); return BLU_ERR_ALLOC; }
    }
    // host pointers: the bit-scores, one row id per hit (word 0 of a packed record, gathered here), the offsets and the
    // records go up; the counts come back
    HipPolicy pol{"blu_consensus_support", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    blu_result* d_recs = nullptr;
    uint32_t* d_rows = nullptr;
    int32_t* d_bs = nullptr;
    uint64_t* d_seg = nullptr;
    blu_support* d_out = nullptr;
    try {
        std::vector<uint32_t> gathered;
        if (stride != 1u) {
            gathered.resize(nh);
            for (uint64_t i = 0; i < nh; ++i) gathered[i] = src[i * stride];
            src = gathered.data();
        }
        HIP_CHECK(pol, mem.upload(&d_recs, results, nq, "records"));
        HIP_CHECK(pol, mem.upload(&d_seg, hits->seg_off, nq + 1, "offsets"));
        HIP_CHECK(pol, mem.upload(&d_bs, hits->bitscore, nh, "bit-scores"));
        HIP_CHECK(pol, mem.upload(&d_rows, src, nh, "rows"));
        HIP_CHECK(pol, mem.alloc(&d_out, nq * sizeof(blu_support), "counts"));
        SupportInput in{d_recs, nq, d_seg, d_bs, d_rows, 1u, nh};
        const int rc = support_device(tax, in, d_out);
        if (rc != BLU_OK) return rc;
        HIP_CHECK(pol, mem.download(out, d_out, nq));
        return BLU_OK;
    } catch (const std::bad_alloc&) { set_error("out of memory"); return BLU_ERR_ALLOC; }
}

}  // extern "C"
