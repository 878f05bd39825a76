// Pairwise sample distances (include/blu_consensus.h: blu_sample_distances): for every pair of samples the
// integers Bray-Curtis and Jaccard are ratios of — the sum of the smaller count and the number of shared features — from a
// feature x sample matrix in CSR over the features.
//
// 1. Transpose by sample.  One wave per feature writes, for each of its non-zeros, the sample id as a sort key and counts the
//    sample (integer atomic adds on vector memory); the tree's scan turns the counts into col_ptr; the tree's stable radix sort
//    orders the non-zeros by sample, and as it is stable the features ascend within a sample; a gather writes the feature and
//    the count of every sorted non-zero.  A pre-pass finds, once, where each chunk of BLU_DISTANCE_CHUNK features begins in
//    every sample's list (binary search): chunk_ptr[s][c].  The pair kernel then reads two words per (sample, chunk) instead
//    of running fourteen dependent loads per search.
// 2. Pairs, output-stationary.  Block (x, a) owns sample a and the partners b >= a in [64 x, 64 x + 64): a pair is computed once,
//    by the block of its smaller sample, and stored on both sides of the diagonal.  It walks the features in
//    chunks: a's non-zeros of the chunk are scattered into a dense LDS array of 8192 u64 (64 KB of the CU's 160 KB: two blocks
//    a CU), every wave takes its 8 partners side by side, its lanes stride over each b's non-zeros of the chunk, each reads
//    the LDS word of its feature, takes the minimum and keeps a 64-bit sum and a count; then a's entries are cleared again
//    (a few hundred stores instead of 8192).  A wave keeps the accumulators of its 8 partners in registers across the
//    chunks, reduces them across its lanes at the end and lane 0 stores the pair.  No atomics here; integer sums only, so
//    the result does not depend on which lane, wave or block met a non-zero.
// 3. total and richness: one wave per sample over its list.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csr_check.h"
#include "ingest_prims.h"

namespace blu {
namespace {

constexpr uint32_t CHUNK = BLU_DISTANCE_CHUNK;
constexpr uint32_t PB = 512;                              // threads of a pair block: eight waves
constexpr uint32_t WAVES = PB / 64;
constexpr uint32_t KP = BLU_DISTANCE_PARTNERS / WAVES;    // partners of one wave
static_assert(KP * WAVES == BLU_DISTANCE_PARTNERS, "partners divide among the waves");

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wave per feature: the sort key (sample) and value (position) of each of its non-zeros, the feature of the position,
// and the sample's count
__global__ __launch_bounds__(256) void distance_expand(const unsigned long long* row_ptr, const uint32_t* sample, uint32_t n_features,
                                                       uint32_t n_samples, uint32_t nnz, uint32_t* keys, uint32_t* vals,
                                                       uint32_t* feat_of, uint32_t* hist) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t f = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (f >= n_features) return;
    const unsigned long long e0 = row_ptr[f], e1 = min(row_ptr[f + 1], (unsigned long long)nnz);   // (checked on the host; clamped all the same)
    for (unsigned long long e = e0 + lane; e < e1; e += 64) {
        const uint32_t s = min(sample[e], n_samples - 1u);
        keys[e] = s;
        vals[e] = (uint32_t)e;
        feat_of[e] = (uint32_t)f;
        atomicAdd(&hist[s], 1u);
    }
}

__global__ __launch_bounds__(256) void distance_gather(const uint32_t* vals, const uint32_t* feat_of, const unsigned long long* count,
                                                       uint32_t nnz, uint32_t* feat, unsigned long long* cnt) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k >= nnz) return;
    const uint32_t e = min(vals[k], nnz - 1u);
    feat[k] = feat_of[e];
    cnt[k] = count[e];
}

// chunk_ptr[s * (n_chunks + 1) + c] = the first position of sample s's list whose feature is >= c * CHUNK
__global__ __launch_bounds__(256) void distance_chunk_ptr(const uint32_t* col_ptr, const uint32_t* feat, uint32_t n_samples,
                                                          uint32_t n_chunks, uint32_t* chunk_ptr) {
    const uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (uint64_t)n_samples * (n_chunks + 1u)) return;
    const uint32_t s = (uint32_t)(t / (n_chunks + 1u)), c = (uint32_t)(t % (n_chunks + 1u));
    const uint64_t bound = (uint64_t)c * CHUNK;
    uint32_t lo = col_ptr[s], hi = col_ptr[s + 1];
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if ((uint64_t)feat[mid] < bound) lo = mid + 1u; else hi = mid;
    }
    chunk_ptr[t] = lo;
}

__global__ __launch_bounds__(256) void distance_totals(const uint32_t* col_ptr, const unsigned long long* cnt, uint32_t n_samples,
                                                       unsigned long long* total, uint32_t* richness) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (s >= n_samples) return;                          // (wave-uniform)
    const uint32_t k0 = col_ptr[s], k1 = col_ptr[s + 1];
    unsigned long long sum = 0;
    for (uint32_t k = k0 + lane; k < k1; k += 64) sum += cnt[k];
    sum = wave_sum64(sum);
    if (lane == 0) { total[s] = sum; richness[s] = k1 - k0; }
}

struct PairDev {
    const uint32_t* chunk_ptr;     // [n_samples][n_chunks + 1]
    const uint32_t* feat;          // [nnz] by sample, ascending within one
    const unsigned long long* cnt; // [nnz]
    uint32_t n_samples;
    uint32_t n_chunks;
    unsigned long long* min_sum;   // [n_samples][n_samples]
    uint32_t* shared;
};

__global__ __launch_bounds__(PB) void distance_pairs(PairDev d) {
    __shared__ unsigned long long dense[CHUNK];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t a = blockIdx.y;
    const uint32_t b0 = blockIdx.x * BLU_DISTANCE_PARTNERS;
    const uint32_t stride = d.n_chunks + 1u;
    if (b0 + BLU_DISTANCE_PARTNERS <= a) return;         // (block-uniform) every partner is below `a`: block (., b) writes those pairs
    for (uint32_t i = threadIdx.x; i < CHUNK; i += PB) dense[i] = 0ull;
    unsigned long long sum[KP];
    uint32_t both[KP];
#pragma unroll
    for (uint32_t k = 0; k < KP; ++k) { sum[k] = 0ull; both[k] = 0u; }
    const uint32_t* pa = d.chunk_ptr + (uint64_t)a * stride;
    __syncthreads();
    for (uint32_t c = 0; c < d.n_chunks; ++c) {
        const uint32_t base = c * CHUNK;
        const uint32_t a0 = pa[c], a1 = pa[c + 1];
        if (a0 == a1) continue;                          // (block-uniform: nothing of `a` here, every minimum is 0)
        for (uint32_t j = a0 + threadIdx.x; j < a1; j += PB) {
            const uint32_t i = d.feat[j] - base;
            if (i < CHUNK) dense[i] = d.cnt[j];
        }
        __syncthreads();
        // the wave's partners side by side: one step takes the next 64 non-zeros of each of them, so their loads are in flight
        // together (a partner at a time, the few steps of a chunk are a chain of load latencies).  A lane past its partner's
        // end reads position 0 — there is one: `a` has non-zeros here — and adds nothing
        uint32_t j[KP], j1[KP];
#pragma unroll
        for (uint32_t k = 0; k < KP; ++k) {
            const uint32_t b = b0 + wave + k * WAVES;
            const bool mine = b >= a && b < d.n_samples; // (wave-uniform)
            const uint32_t* pb = d.chunk_ptr + (uint64_t)(mine ? b : a) * stride;
            j[k] = pb[c] + lane;
            j1[k] = mine ? pb[c + 1] : 0u;
        }
        for (;;) {
            bool more = false;
#pragma unroll
            for (uint32_t k = 0; k < KP; ++k) more |= j[k] < j1[k];
            if (!more) break;
#pragma unroll
            for (uint32_t k = 0; k < KP; ++k) {
                const bool on = j[k] < j1[k];
                const uint32_t jj = on ? j[k] : 0u;
                const uint32_t i = d.feat[jj] - base;
                const unsigned long long y = d.cnt[jj];
                const unsigned long long x = on && i < CHUNK ? dense[i] : 0ull;
                sum[k] += x < y ? x : y;
                both[k] += x != 0ull ? 1u : 0u;          // (y > 0: the list holds non-zeros only)
                j[k] = on ? j[k] + 64u : j[k];           // (no wrap: the host keeps nnz below 2^32 - 1024)
            }
        }
        __syncthreads();
        for (uint32_t j = a0 + threadIdx.x; j < a1; j += PB) {
            const uint32_t i = d.feat[j] - base;
            if (i < CHUNK) dense[i] = 0ull;
        }
        __syncthreads();
    }
#pragma unroll
    for (uint32_t k = 0; k < KP; ++k) {
        const uint32_t b = b0 + wave + k * WAVES;
        if (b < a || b >= d.n_samples) continue;
        const unsigned long long s = wave_sum64(sum[k]);
        const unsigned long long n = wave_sum64((unsigned long long)both[k]);
        if (lane == 0) {
            d.min_sum[(uint64_t)a * d.n_samples + b] = s;
            d.shared[(uint64_t)a * d.n_samples + b] = (uint32_t)n;
            d.min_sum[(uint64_t)b * d.n_samples + a] = s;      // the mirror: min and `both` are symmetric
            d.shared[(uint64_t)b * d.n_samples + a] = (uint32_t)n;
        }
    }
}

// the desc's refusals; *nnz_out = row_ptr[n_features]
int check_desc(const blu_distance_desc& d, uint64_t* nnz_out) {
    if (d.struct_size != sizeof(blu_distance_desc)) {
        set_error("blu_sample_distances: struct_size %llu is not one this library knows (%llu)", (unsigned long long)d.struct_size,
                  (unsigned long long)sizeof(blu_distance_desc));
        return BLU_ERR_INVALID_ARG;
    }
    std::vector<uint64_t> total;
    return check_csr("blu_sample_distances", d.n_features, d.n_samples, d.row_ptr, d.sample, d.count, nnz_out, total);
}

template <class T>
bool host_array(T** out, size_t n) {
    *out = (T*)calloc(n ? n : 1, sizeof(T));
    return *out != nullptr;
}

int distances_device(const blu_distance_desc& d, uint64_t nnz64, blu_sample_distance* out) {
    HipPolicy pol{"blu_sample_distances", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    const uint32_t S = d.n_samples, F = (uint32_t)d.n_features, nnz = (uint32_t)nnz64;
    const uint32_t n_chunks = (uint32_t)(((uint64_t)F + CHUNK - 1) / CHUNK);
    const uint64_t pairs = (uint64_t)S * S;
    HIP_CHECK(pol, hipStreamSynchronize((hipStream_t)d.stream));
    unsigned long long *d_row = nullptr, *d_count = nullptr, *d_cnt = nullptr, *d_total = nullptr, *d_min = nullptr;
    uint32_t *d_sample = nullptr, *d_keys = nullptr, *d_vals = nullptr, *d_keys_alt = nullptr, *d_vals_alt = nullptr, *d_feat_of = nullptr;
    uint32_t *d_hist = nullptr, *d_col = nullptr, *d_feat = nullptr, *d_chunk = nullptr, *d_rich = nullptr, *d_shared = nullptr, *d_table = nullptr;
    void *d_scan = nullptr, *d_sort = nullptr;
    HIP_CHECK(pol, mem.upload(&d_row, d.row_ptr, (size_t)F + 1, "row_ptr"));
    HIP_CHECK(pol, mem.upload(&d_sample, d.sample, nnz, "samples"));
    HIP_CHECK(pol, mem.upload(&d_count, d.count, nnz, "counts"));
    HIP_CHECK(pol, mem.alloc(&d_keys, (size_t)nnz * 4, "sort keys"));
    HIP_CHECK(pol, mem.alloc(&d_vals, (size_t)nnz * 4, "sort values"));
    HIP_CHECK(pol, mem.alloc(&d_keys_alt, (size_t)nnz * 4, "sort keys"));
    HIP_CHECK(pol, mem.alloc(&d_vals_alt, (size_t)nnz * 4, "sort values"));
    HIP_CHECK(pol, mem.alloc(&d_feat_of, (size_t)nnz * 4, "features"));
    HIP_CHECK(pol, mem.alloc(&d_hist, ((size_t)S + 1) * 4, "sample counts"));
    HIP_CHECK(pol, mem.alloc(&d_col, ((size_t)S + 1) * 4, "col_ptr"));
    HIP_CHECK(pol, mem.alloc(&d_scan, scan_tmp_bytes_u32((size_t)S + 1), "scan scratch"));
    HIP_CHECK(pol, mem.alloc(&d_table, radix_table_words(nnz) * 4, "digit table"));
    HIP_CHECK(pol, mem.alloc(&d_sort, radix_scan_tmp_bytes(nnz), "scan scratch"));
    HIP_CHECK(pol, mem.alloc(&d_feat, (size_t)nnz * 4, "features by sample"));
    HIP_CHECK(pol, mem.alloc(&d_cnt, (size_t)nnz * 8, "counts by sample"));
    HIP_CHECK(pol, mem.alloc(&d_chunk, (size_t)S * (n_chunks + 1) * 4, "chunk bounds"));
    HIP_CHECK(pol, mem.alloc(&d_total, (size_t)S * 8, "totals"));
    HIP_CHECK(pol, mem.alloc(&d_rich, (size_t)S * 4, "richness"));
    HIP_CHECK(pol, mem.alloc(&d_min, pairs * 8, "min_sum"));
    HIP_CHECK(pol, mem.alloc(&d_shared, pairs * 4, "shared"));

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    struct Events { hipEvent_t &a, &b; ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } events{ev0, ev1};
    HIP_CHECK(pol, hipEventCreate(&ev0));
    HIP_CHECK(pol, hipEventCreate(&ev1));
    HIP_CHECK(pol, hipEventRecord(ev0, nullptr));
    HIP_CHECK(pol, hipMemsetAsync(d_hist, 0, ((size_t)S + 1) * 4, nullptr));
    if (nnz) {
        hipLaunchKernelGGL(distance_expand, dim3(grid(F, 4)), dim3(256), 0, 0, d_row, d_sample, F, S, nnz, d_keys, d_vals, d_feat_of, d_hist);
        HIP_CHECK(pol, hipGetLastError());
    }
    HIP_CHECK(pol, exclusive_scan_u32(d_hist, d_col, (size_t)S + 1, d_scan));
    if (nnz) {
        int bits = 1;
        while ((1u << bits) < S) ++bits;
        uint32_t *k = d_keys, *ka = d_keys_alt, *v = d_vals, *va = d_vals_alt;
        HIP_CHECK(pol, radix_sort_pairs(&k, &ka, &v, &va, nnz, bits, d_table, d_sort));
        hipLaunchKernelGGL(distance_gather, dim3(grid(nnz)), dim3(256), 0, 0, v, d_feat_of, d_count, nnz, d_feat, d_cnt);
        HIP_CHECK(pol, hipGetLastError());
    }
    hipLaunchKernelGGL(distance_chunk_ptr, dim3(grid((uint64_t)S * (n_chunks + 1))), dim3(256), 0, 0, d_col, d_feat, S, n_chunks, d_chunk);
    HIP_CHECK(pol, hipGetLastError());
    hipLaunchKernelGGL(distance_totals, dim3(grid(S, 4)), dim3(256), 0, 0, d_col, d_cnt, S, d_total, d_rich);
    HIP_CHECK(pol, hipGetLastError());
    PairDev p{d_chunk, d_feat, d_cnt, S, n_chunks, d_min, d_shared};
    hipLaunchKernelGGL(distance_pairs, dim3((S + BLU_DISTANCE_PARTNERS - 1) / BLU_DISTANCE_PARTNERS, S), dim3(PB), 0, 0, p);
    HIP_CHECK(pol, hipGetLastError());
    HIP_CHECK(pol, hipEventRecord(ev1, nullptr));
    HIP_CHECK(pol, hipEventSynchronize(ev1));
    float ms = 0.f;
    HIP_CHECK(pol, hipEventElapsedTime(&ms, ev0, ev1));

    if (!host_array(&out->total, S) || !host_array(&out->richness, S) || !host_array(&out->min_sum, pairs) || !host_array(&out->shared, pairs)) {
        set_error("blu_sample_distances: out of memory");
        return BLU_ERR_ALLOC;
    }
    HIP_CHECK(pol, mem.download(out->total, d_total, S));
    HIP_CHECK(pol, mem.download(out->richness, d_rich, S));
    HIP_CHECK(pol, mem.download(out->min_sum, d_min, pairs));
    HIP_CHECK(pol, mem.download(out->shared, d_shared, pairs));
    out->n_samples = S;
    out->t_device_ms = (double)ms;
    return BLU_OK;
}

}  // namespace
}  // namespace blu

using namespace blu;

extern "C" {

void blu_sample_distance_free(blu_sample_distance* out) {
    if (!out) return;
    free(out->total); free(out->richness); free(out->min_sum); free(out->shared);
    memset(out, 0, sizeof *out);
}

int blu_sample_distances(const blu_distance_desc* desc, blu_sample_distance* out) {
    if (!desc || !out) { set_error("blu_sample_distances: null argument"); return BLU_ERR_INVALID_ARG; }
    memset(out, 0, sizeof *out);
    uint64_t nnz = 0;
    try {
        if (const int rc = check_desc(*desc, &nnz)) return rc;
        if (const int rc = use_device("blu_sample_distances", desc->device)) return rc;
        const int rc = distances_device(*desc, nnz, out);
        if (rc != BLU_OK) blu_sample_distance_free(out);
        return rc;
    } catch (const std::bad_alloc&) {
        blu_sample_distance_free(out);
        set_error("blu_sample_distances: out of memory");
        return BLU_ERR_ALLOC;
    }
}

}  // extern "C"
