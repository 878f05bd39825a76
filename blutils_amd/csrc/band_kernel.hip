// Bit-score band (include/blu_consensus.h: blu_hits_score_band): the rows of a query whose truncated bit-score
// lies inside a band under the query's top score t are given the score t, so that everything downstream — which finds the top
// group by comparing the bit-score column with its maximum — counts them as tied.  One pass over the bit-score column, between
// the parser and the engine.
//
// A wave takes BAND_QPW consecutive queries, one after the other.  A segment of up to 64 rows is one load per lane, a wave
// maximum, the integer test and one store.  A longer segment is swept twice, 64 rows at a time, however long it is: each lane
// keeps a running maximum, the maximum is reduced once, and the second sweep re-reads the rows (from L2 for any realistic
// segment), tests and stores.  In place only the lanes whose value changes store; out of place every row of a segment is
// written.  The test is 64-bit integer arithmetic throughout: t - D and b * 100000 do not fit 32 bits.
//
// Counts: a ballot / popcount per sweep, summed in a register over the wave's queries; lane 0 of each wave then adds them to the
// spread counters of hit_pass.h.  No LDS, no scratch, no second kernel.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "hit_pass.h"

namespace blu {
namespace {

constexpr uint32_t BAND_BLOCK = 256;                 // threads per block: four waves
constexpr uint32_t BAND_QPW = BLU_BAND_QUERIES_PER_WAVE;
constexpr uint32_t CNT_RAISED = 0, CNT_WIDENED = 1, CNT_WORDS = 2 * HIT_SPREAD;   // spread counters: raised rows, widened queries
constexpr long long MILLI_ONE = 100000ll;            // 100 % in milli-percent

struct BandDev {
    const int32_t* in;                 // (no __restrict__: in == out is the in-place call)
    int32_t* out;
    const unsigned long long* seg_off;
    uint64_t n_hits, n_queries;
    uint32_t mask;                     // BLU_BAND_* bits
    long long keep_milli;              // 100000 - top_percent_milli
    long long top_bits;
    unsigned long long* counts;        // [CNT_WORDS]
};

// b < t lies in the band under t: every criterion of the mask holds (an empty mask: none does)
__device__ __forceinline__ bool in_band(const BandDev& d, int32_t b, int32_t t) {
    if (b >= t || !d.mask) return false;
    bool ok = true;
    if (d.mask & BLU_BAND_TOP_BITS) ok = ok && (long long)b >= (long long)t - d.top_bits;
    if (d.mask & BLU_BAND_TOP_PERCENT) ok = ok && (long long)b * MILLI_ONE >= (long long)t * d.keep_milli;
    return ok;
}

__global__ __launch_bounds__(BAND_BLOCK) void score_band_kernel(BandDev d) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * BAND_BLOCK + threadIdx.x) >> 6;
    const bool in_place = d.in == d.out;
    unsigned long long n_raised = 0, n_widened = 0;  // (wave-uniform)
    for (uint32_t k = 0; k < BAND_QPW; ++k) {
        const uint64_t q = wave * BAND_QPW + k;
        if (q >= d.n_queries) break;                 // (wave-uniform)
        uint64_t s0, s1;
        segment_of(d.seg_off, q, d.n_hits, &s0, &s1);
        if (s0 == s1) continue;
        unsigned long long raised = 0;
        if (s1 - s0 <= 64u) {
            const uint64_t i = s0 + lane;
            const bool has = i < s1;
            const int32_t b = has ? d.in[i] : INT32_MIN;
            const int32_t t = wave_max32(b);
            const bool up = has && in_band(d, b, t);
            if (up || (has && !in_place)) d.out[i] = up ? t : b;
            raised = (unsigned long long)__popcll(__ballot(up));
        } else {
            int32_t mx = INT32_MIN;
            for (uint64_t i = s0 + lane; i < s1; i += 64) mx = max(mx, d.in[i]);
            const int32_t t = wave_max32(mx);
            for (uint64_t i0 = s0; i0 < s1; i0 += 64) {   // (wave-uniform trip count: every lane takes part in the ballot)
                const uint64_t i = i0 + lane;
                const bool has = i < s1;
                const int32_t b = has ? d.in[i] : INT32_MIN;
                const bool up = has && in_band(d, b, t);
                if (up || (has && !in_place)) d.out[i] = up ? t : b;
                raised += (unsigned long long)__popcll(__ballot(up));
            }
        }
        n_raised += raised;
        n_widened += raised ? 1ull : 0ull;
    }
    if (lane == 0) { spread_add(d.counts, CNT_RAISED, n_raised); spread_add(d.counts, CNT_WIDENED, n_widened); }
}

}  // namespace

int check_score_band(const blu_score_band* band) {
    if (!band) return BLU_OK;
    if (band->mask & ~(BLU_BAND_TOP_PERCENT | BLU_BAND_TOP_BITS)) { set_error("score band: unknown bits in the mask"); return BLU_ERR_INVALID_ARG; }
    if (band->top_percent_milli > 100000u) {
        set_error("score band: top_percent_milli must be at most 100000 (100 %%)");
        return BLU_ERR_INVALID_ARG;
    }
    if (band->top_bits >= (1ull << 32)) { set_error("score band: top_bits must be below 2^32"); return BLU_ERR_INVALID_ARG; }
    return BLU_OK;
}

int score_band_device(const int32_t* d_in, const uint64_t* d_seg_off, uint64_t n_hits, uint64_t n_queries, const blu_score_band& band,
                      hipStream_t stream, int32_t* d_out, uint64_t* n_raised, uint64_t* n_widened) {
    HipPolicy pol{"score band", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    *n_raised = *n_widened = 0;
    if (n_queries == 0 || n_hits == 0) return BLU_OK;
    const uint64_t waves = (n_queries + BAND_QPW - 1) / BAND_QPW;
    const uint64_t blocks = (waves + BAND_BLOCK / 64 - 1) / (BAND_BLOCK / 64);
    if (blocks > 0x7FFFFFFFull) { set_error("score band: too many queries for one launch"); return BLU_ERR_INVALID_ARG; }
    unsigned long long* d_counts = nullptr;
    unsigned long long counts[CNT_WORDS];
    HIP_CHECK(pol, mem.alloc(&d_counts, sizeof counts, "counts"));
    HIP_CHECK(pol, hipMemsetAsync(d_counts, 0, sizeof counts, stream));
    BandDev d{};
    d.in = d_in; d.out = d_out; d.seg_off = (const unsigned long long*)d_seg_off; d.n_hits = n_hits; d.n_queries = n_queries;
    d.mask = band.mask;
    d.keep_milli = MILLI_ONE - (long long)band.top_percent_milli;
    d.top_bits = (long long)band.top_bits;
    d.counts = d_counts;
    hipLaunchKernelGGL(score_band_kernel, dim3((unsigned)blocks), dim3(BAND_BLOCK), 0, stream, d);
    HIP_CHECK(pol, hipGetLastError());
    HIP_CHECK(pol, hipMemcpyAsync(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost, stream));
    HIP_CHECK(pol, hipStreamSynchronize(stream));    // (`out` and the counts are complete)
    *n_raised = spread_sum(counts, CNT_RAISED); *n_widened = spread_sum(counts, CNT_WIDENED);
    return BLU_OK;
}

}  // namespace blu

using namespace blu;

extern "C" {

int blu_hits_score_band(int device, const int32_t* bitscore, const uint64_t* seg_off, uint64_t n_hits, uint64_t n_queries,
                        int on_device, const blu_score_band* band, void* stream, int32_t* out, blu_score_band_stats* stats) {
    if (stats) *stats = blu_score_band_stats{n_hits, 0, n_queries, 0};
    int rc = check_score_band(band);
    if (rc != BLU_OK) return rc;
    if ((n_hits && (!bitscore || !out)) || (n_queries && !seg_off)) return refuse_null_array("blu_hits_score_band");
    const bool active = band && band->mask != 0;
    if (!active && !on_device) {                     // no band: the column as it is (no device needed)
        if (out != bitscore && n_hits) memmove(out, bitscore, n_hits * 4);
        return BLU_OK;
    }
    if (n_hits == 0) return BLU_OK;
    if ((rc = use_device("blu_hits_score_band", device)) != BLU_OK) return rc;
    HipPolicy pol{"blu_hits_score_band", BLU_ERR_ALLOC};
    uint64_t n_raised = 0, n_widened = 0;
    if (on_device) {
        HIP_CHECK(pol, hipStreamSynchronize((hipStream_t)stream));
        if (!active) {
            if (out != bitscore) HIP_CHECK(pol, hipMemcpy(out, bitscore, n_hits * 4, hipMemcpyDeviceToDevice));
            return BLU_OK;
        }
        if (n_queries == 0) {                        // (no segment names a row: nothing is raised)
            if (out != bitscore) HIP_CHECK(pol, hipMemcpy(out, bitscore, n_hits * 4, hipMemcpyDeviceToDevice));
            return BLU_OK;
        }
        rc = score_band_device(bitscore, seg_off, n_hits, n_queries, *band, (hipStream_t)stream, out, &n_raised, &n_widened);
    } else {
        // host pointers: the column and the offsets go up, the same kernel runs in place, the column comes back
        if (n_queries == 0) { if (out != bitscore) memmove(out, bitscore, n_hits * 4); return BLU_OK; }
        DeviceArena mem(pol);
        int32_t* d_bs = nullptr;
        uint64_t* d_seg = nullptr;
        HIP_CHECK(pol, mem.upload(&d_bs, bitscore, n_hits, "bit-scores"));
        HIP_CHECK(pol, mem.upload(&d_seg, seg_off, n_queries + 1, "offsets"));
        rc = score_band_device(d_bs, d_seg, n_hits, n_queries, *band, nullptr, d_bs, &n_raised, &n_widened);
        if (rc == BLU_OK) HIP_CHECK(pol, mem.download(out, d_bs, n_hits));
    }
    if (rc != BLU_OK) return rc;
    if (stats) { stats->n_raised = n_raised; stats->n_widened = n_widened; }
    return BLU_OK;
}

}  // extern "C"
