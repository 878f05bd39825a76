// What the per-query passes between the parser and the engine share: the hit filter's counters (ingest_gpu.hip), the best hit per
// subject (subject_kernel.hip), the bit-score band (band_kernel.hip), the minimum cover (cover_kernel.hip) and the support counts
// (support_kernel.hip).  Device inlines and host one-liners here; the kernels and the host code of hit_pass.hip are compiled once.
#ifndef BLU_HIT_PASS_H
#define BLU_HIT_PASS_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>

#include "blu_internal.h"
#include "ingest_prims.h"

namespace blu {

__device__ __forceinline__ int32_t wave_max32(int32_t v) {
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// the clamped segment of query q: offsets that run past the columns read and write nothing outside them, a decreasing pair is empty
__device__ __forceinline__ void segment_of(const unsigned long long* __restrict__ seg_off, uint64_t q, uint64_t n_hits, uint64_t* s0, uint64_t* s1) {
    uint64_t a = seg_off[q], b = seg_off[q + 1];
    if (b > n_hits) b = n_hits;
    if (a > b) a = b;
    *s0 = a; *s1 = b;
}

// ---- spread counters: count k of a pass is HIT_SPREAD 64-bit words, counts[k * HIT_SPREAD ..], of which a block
// adds to the one it picks by its number, so that no word takes every block's atomic; the host sums the words.
constexpr uint32_t HIT_SPREAD = 64;

// one lane (lane 0 of a wave, thread 0 of a block) adds what its wave or block summed.  A zero adds nothing: the counts that are
// zero together (no long row without a long query, no widened query without a raised row) need no test of their own.
__device__ __forceinline__ void spread_add(unsigned long long* counts, uint32_t k, unsigned long long v) {
    if (v) atomicAdd(&counts[k * HIT_SPREAD + blockIdx.x % HIT_SPREAD], v);
}
// every active lane calls it: the first lane with `pred` adds how many have it
__device__ __forceinline__ void spread_add_ballot(unsigned long long* counts, uint32_t k, bool pred) {
    const unsigned long long m = __ballot(pred);
    if (pred && (m & ((1ull << (threadIdx.x & 63u)) - 1ull)) == 0) atomicAdd(&counts[k * HIT_SPREAD + blockIdx.x % HIT_SPREAD], (unsigned long long)__popcll(m));
}
inline uint64_t spread_sum(const unsigned long long* counts, uint32_t k) {
    uint64_t s = 0;
    for (uint32_t w = 0; w < HIT_SPREAD; ++w) s += counts[k * HIT_SPREAD + w];
    return s;
}

// ---- the long queries of a pass, in query order.  d_flag[n_queries + 1]: 1 for a long query, else 0, written by the pass's short
// kernel up to n_queries (the pad word is zeroed here); n_long: their number, from the pass's counters.  *d_list_q[n_long] are the
// queries; with d_row_start[n_queries] (else null) *d_list_start[n_long + 1] gets d_row_start of each, the last entry left to the
// caller.  d_tmp: scan_tmp_bytes_u32(n_queries + 1) bytes.  The lists live in `mem`; everything runs on the null stream.
int long_query_list(HipPolicy& pol, DeviceArena& mem, uint32_t* d_flag, uint64_t n_queries, uint64_t n_long, const uint32_t* d_row_start,
                    void* d_tmp, uint32_t** d_list_q, uint32_t** d_list_start);

// ---- stable compaction of columns, one after another through ONE spare buffer: the keep words, their exclusive
// scan, the row counts before and after, and the spare of n_out elements the next column is gathered into.
struct Compaction {
    const uint32_t* keep;
    const uint32_t* pos;
    uint32_t n, n_out;
    void* spare;

    // the spare becomes the column and the column's old buffer the next spare: 8-byte columns first, so that every spare is
    // large enough.  Each column is an allocation of its own
    template <class... T>
    hipError_t rotate(T*&... col) { hipError_t e = hipSuccess; ((e = e == hipSuccess ? rotate_one(col) : e), ...); return e; }
    // the kept rows go back to the front of the column's own buffer
    template <class... T>
    hipError_t copy_back(T*... col) { hipError_t e = hipSuccess; ((e = e == hipSuccess ? copy_back_one(col) : e), ...); return e; }

  private:
    template <class T>
    hipError_t gather(const T* col) {
        static_assert(sizeof(T) == 4 || sizeof(T) == 8, "4- and 8-byte columns");
        if constexpr (sizeof(T) == 8) return compact_column_u64((const unsigned long long*)col, keep, pos, n, n_out, (unsigned long long*)spare);
        else return compact_column_u32((const uint32_t*)col, keep, pos, n, n_out, (uint32_t*)spare);
    }
    template <class T>
    hipError_t rotate_one(T*& col) { const hipError_t e = gather(col); void* old = col; col = (T*)spare; spare = old; return e; }
    template <class T>
    hipError_t copy_back_one(T* col) {
        const hipError_t e = gather(col);
        return e != hipSuccess ? e : hipMemcpyAsync(col, spare, (size_t)n_out * sizeof(T), hipMemcpyDeviceToDevice, nullptr);
    }
};

// ---- an entry point's refusals: the message names the entry point, the code is BLU_ERR_INVALID_ARG
int refuse_null_array(const char* who);
// device columns that are not 16-byte aligned (the compaction reads them 16 bytes at a time)
int check_aligned16(const char* who, const HitColumns& c);

// ---- the host-pointer route of a pass that compacts the table: the five columns, the offsets and the row map (may be null:
// none) go up, `pass` runs on the device copies (d_map null without a map), and *n_out rows and the offsets come back when
// rows were dropped -- otherwise the host arrays are what they were.
using StagedPass = std::function<int(HitColumns& c, const uint32_t* d_map, uint64_t* n_out)>;
int with_staged_columns(HipPolicy& pol, const HitColumns& host, uint64_t n_hits, uint64_t n_queries, const uint32_t* row_map, uint64_t n_map,
                        uint64_t* n_out, const StagedPass& pass);

}  // namespace blu
#endif
