// Rarefaction (include/blu_consensus.h: blu_sample_rarefy): every sample of a feature x sample CSR subsampled
// to `depth` reads without replacement.  Read i of sample a has the key mix64(i + stream[a]); the `depth` smallest keys of a
// sample are its kept reads.  The work is per read, not per non-zero, and a read exists only as its ordinal: nothing per read
// is ever stored.
//
// 1. Transpose by sample, as distance_kernel.hip does: one wave per feature writes the sample of each non-zero as a sort key and
//    its position in the input as the value, and counts the sample; the tree's scan gives col_ptr, its stable radix sort orders
//    the positions by sample (features ascend within one); a gather lines the counts up and a u64 exclusive scan over all of
//    them gives start[k]: the first ordinal of non-zero k is start[k] - start[col_ptr[a]].
// 2. Threshold by radix select, 8 bits a pass, 8 passes from the top digit.  The reads of the kept samples are cut into tiles
//    of TILE ordinals, one 256-thread block each (the host's prefix of tiles per sample is the grid: a non-zero of 2^31 reads is
//    32768 blocks, not one wave).  A lane hashes its ordinals; one whose key has the prefix chosen so far adds to an LDS
//    histogram of the next digit; the block adds its non-empty bins to hist[a][bin].  One wave per sample then finds the bin
//    that holds the rank, appends it to the prefix, takes the bins below it off the rank and clears the histogram.  After the
//    last pass the prefix is the depth-th smallest key T_a.  Keys of one sample are distinct (mix64 is a bijection), so
//    exactly `depth` ordinals have key <= T_a.
// 3. Count per non-zero, over the same tiles.  The block writes the kept ordinals of its tile as a bit map in LDS (a wave's
//    ballot is one 64-bit word) and scans the words' popcounts, so the kept reads below any ordinal of the tile are two LDS
//    reads; it finds the non-zeros it overlaps by two binary searches in start[], once per tile, and its threads stride over
//    them: kept[position in the input] gets the count by a plain store when the non-zero lies inside the tile, by a 64-bit
//    atomic add when it spans tiles.
// Integers only.  The histogram sums and the counts are sums of integers: no stored value depends on the launch geometry or on
// the order of the atomics.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csr_check.h"
#include "ingest_prims.h"
#include "wave_scan.h"

namespace blu {
namespace {

constexpr uint32_t TILE = BLU_RAREFY_TILE;       // ordinals of one block
constexpr uint32_t TB = 256;                     // threads of a tile's block
constexpr uint32_t STEPS = TILE / TB;            // ordinals of one thread
constexpr uint32_t WORDS = TILE / 64;            // 64-bit words of a tile's bit map
constexpr uint32_t DIGIT = 8, BINS = 1u << DIGIT, PASSES = 64 / DIGIT;
static_assert(WORDS == 4 * TB, "the popcount scan takes four words a thread");
static_assert(BINS == 4 * 64, "the pick takes four bins a lane");

__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// one wave per feature: the sort key (sample) and value (position) of each of its non-zeros, and the sample's count
__global__ __launch_bounds__(256) void rarefy_expand(const unsigned long long* row_ptr, const uint32_t* sample, uint32_t n_features,
                                                     uint32_t n_samples, uint32_t nnz, uint32_t* keys, uint32_t* vals, uint32_t* hist) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t f = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (f >= n_features) return;
    const unsigned long long e0 = row_ptr[f], e1 = min(row_ptr[f + 1], (unsigned long long)nnz);   // (checked on the host; clamped all the same)
    for (unsigned long long e = e0 + lane; e < e1; e += 64) {
        const uint32_t s = min(sample[e], n_samples - 1u);
        keys[e] = s;
        vals[e] = (uint32_t)e;
        atomicAdd(&hist[s], 1u);
    }
}

// cnt[k] = the count of the k-th non-zero by sample; cnt[nnz] = 0, so that the scan's last element is the grand total
__global__ __launch_bounds__(256) void rarefy_gather(const uint32_t* vals, const unsigned long long* count, uint32_t nnz, unsigned long long* cnt) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k > nnz) return;
    cnt[k] = k < nnz ? count[min(vals[k], nnz - 1u)] : 0ull;
}

struct TileDev {
    const uint32_t* tile_ptr;            // [n_samples + 1] the first tile of each sample (a dropped sample has none)
    const unsigned long long* stream;    // [n_samples]
    const unsigned long long* total;     // [n_samples] N_a
    uint32_t n_samples;
};

// the sample of tile t and the tile's ordinals [o0, o1).  Block-uniform
__device__ __forceinline__ uint32_t tile_of(const TileDev& d, uint32_t t, unsigned long long* o0, unsigned long long* o1) {
    uint32_t lo = 0, hi = d.n_samples;   // the last a with tile_ptr[a] <= t: there is one, as tile_ptr[0] = 0 and t < tile_ptr[n_samples]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (d.tile_ptr[mid] <= t) lo = mid; else hi = mid;
    }
    const unsigned long long n = d.total[lo];
    *o0 = min((unsigned long long)(t - d.tile_ptr[lo]) * TILE, n);
    *o1 = min(*o0 + TILE, n);
    return lo;
}

// pass p: among the ordinals whose key starts with prefix[a] (8 p bits), the histogram of the next digit
__global__ __launch_bounds__(TB) void rarefy_histogram(TileDev d, const unsigned long long* prefix, uint32_t pass, uint32_t* hist) {
    __shared__ uint32_t bins[BINS];
    unsigned long long o0, o1;
    const uint32_t a = tile_of(d, blockIdx.x, &o0, &o1);
    bins[threadIdx.x] = 0u;              // (TB == BINS)
    __syncthreads();
    const unsigned long long st = d.stream[a], want = prefix[a];
    const uint32_t above = 64u - DIGIT * pass;       // bits below the prefix; 64 in pass 0, where every key takes part
    const uint32_t shift = above - DIGIT;
    for (unsigned long long o = o0 + threadIdx.x; o < o1; o += TB) {
        const unsigned long long key = mix64(o + st);
        if (pass == 0u || (key >> above) == want) atomicAdd(&bins[(uint32_t)(key >> shift) & (BINS - 1u)], 1u);
    }
    __syncthreads();
    const uint32_t n = bins[threadIdx.x];
    if (n) atomicAdd(&hist[(uint64_t)a * BINS + threadIdx.x], n);
}
static_assert(TB == BINS, "a thread per bin");

// one wave per sample: the bin that holds the rank joins the prefix, the bins below it leave the rank, the histogram is cleared.
// rank is 1-based and at most the sum of the bins (the host keeps depth <= N_a); a histogram that does not reach it picks the
// last bin, and the host's column sums then tell
__global__ __launch_bounds__(256) void rarefy_pick(const uint32_t* tile_ptr, uint32_t n_samples, uint32_t* hist, unsigned long long* prefix,
                                                   unsigned long long* rank) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t a = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (a >= n_samples) return;                              // (wave-uniform)
    if (tile_ptr[a] == tile_ptr[a + 1]) return;              // (wave-uniform) a dropped sample
    uint32_t* h = hist + (uint64_t)a * BINS + 4u * lane;
    const uint32_t b0 = h[0], b1 = h[1], b2 = h[2], b3 = h[3];
    h[0] = 0u; h[1] = 0u; h[2] = 0u; h[3] = 0u;
    const unsigned long long r = rank[a];
    const unsigned long long mine = (unsigned long long)b0 + b1 + b2 + b3;
    // inclusive sums of the lanes' totals in 64 bits: 2^32 - 1 reads may all fall into one pass's histogram
    unsigned long long incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long up = __shfl_up(incl, o, 64);
        if ((int)lane >= o) incl += up;
    }
    const unsigned long long before = incl - mine;
    const bool holds = before < r && r <= incl;              // at most one lane
    const unsigned long long vote = __ballot(holds);
    const uint32_t owner = vote ? (uint32_t)__ffsll((long long)vote) - 1u : 63u;
    if (lane == owner) {
        unsigned long long below = before;
        uint32_t digit = 4u * lane + 3u;
        if (r <= below + b0) digit = 4u * lane;
        else if (r <= (below += b0) + b1) digit = 4u * lane + 1u;
        else if (r <= (below += b1) + b2) digit = 4u * lane + 2u;
        else below += b2;
        prefix[a] = (prefix[a] << DIGIT) | digit;
        rank[a] = r > below ? r - below : 1ull;
    }
}

struct CountDev {
    const uint32_t* col_ptr;             // [n_samples + 1]
    const unsigned long long* start;     // [nnz + 1] exclusive sums of the counts by sample
    const uint32_t* pos;                 // [nnz] position in the input of the k-th non-zero by sample
    const unsigned long long* threshold; // [n_samples] T_a
    uint32_t nnz;
    unsigned long long* kept;            // [nnz] by input position; zero on entry
};

__global__ __launch_bounds__(TB) void rarefy_count(TileDev d, CountDev c) {
    __shared__ unsigned long long bits[WORDS];
    __shared__ uint32_t below[WORDS];    // kept ordinals of the tile in the words before this one
    __shared__ uint32_t wave_sums[TB / 64];
    __shared__ uint32_t range[2];
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long o0, o1;
    const uint32_t a = tile_of(d, blockIdx.x, &o0, &o1);
    const uint32_t k0 = c.col_ptr[a], k1 = min(c.col_ptr[a + 1], c.nnz);
    if (k0 >= k1 || o0 >= o1) return;    // (block-uniform; a sample with tiles has reads, hence non-zeros)
    const unsigned long long base = c.start[k0];
    if (threadIdx.x < 2u) {
        // the last non-zero that starts at or before o0 (thread 0), before o1 (thread 1): start[k0] - base = 0 <= o0 < o1
        const unsigned long long bound = threadIdx.x == 0u ? o0 : o1 - 1ull;
        uint32_t lo = k0, hi = k1;
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (c.start[mid] - base <= bound) lo = mid; else hi = mid;
        }
        range[threadIdx.x] = lo;
    }
    const unsigned long long st = d.stream[a], T = c.threshold[a];
#pragma unroll 4
    for (uint32_t j = 0; j < STEPS; ++j) {
        const unsigned long long o = o0 + (unsigned long long)j * TB + threadIdx.x;
        const unsigned long long word = __ballot(o < o1 && mix64(o + st) <= T);
        if (lane == 0u) bits[(j * TB + threadIdx.x) >> 6] = word;
    }
    __syncthreads();
    {
        const uint32_t w = 4u * threadIdx.x;
        const uint32_t p0 = (uint32_t)__popcll(bits[w]), p1 = (uint32_t)__popcll(bits[w + 1]), p2 = (uint32_t)__popcll(bits[w + 2]),
                       p3 = (uint32_t)__popcll(bits[w + 3]);
        const uint32_t e = block_excl_scan<TB>(p0 + p1 + p2 + p3, wave_sums);
        below[w] = e; below[w + 1] = e + p0; below[w + 2] = e + p0 + p1; below[w + 3] = e + p0 + p1 + p2;
    }
    __syncthreads();
    // kept ordinals of the tile below its local ordinal i (0 .. TILE)
    const auto kept_below = [&](uint32_t i) -> uint32_t {
        if (i >= TILE) return below[WORDS - 1] + (uint32_t)__popcll(bits[WORDS - 1]);
        return below[i >> 6] + (uint32_t)__popcll(bits[i >> 6] & ((1ull << (i & 63u)) - 1ull));
    };
    const uint32_t first = range[0], last = range[1];
    for (uint32_t k = first + threadIdx.x; k <= last && k < k1; k += TB) {   // (no wrap: the host keeps nnz below 2^32 - 1024)
        const unsigned long long s0 = c.start[k] - base, s1 = c.start[k + 1] - base;
        const unsigned long long lo = max(s0, o0), hi = min(s1, o1);
        if (lo >= hi) continue;
        const uint32_t n = kept_below((uint32_t)(hi - o0)) - kept_below((uint32_t)(lo - o0));
        if (!n) continue;
        unsigned long long* out = c.kept + min(c.pos[k], c.nnz - 1u);
        if (s0 >= o0 && s1 <= o1) *out = n;                  // the whole non-zero is this tile's
        else atomicAdd(out, (unsigned long long)n);
    }
}

int refuse(const char* fmt, unsigned long long a = 0, unsigned long long b = 0) {
    set_error(fmt, a, b);
    return BLU_ERR_INVALID_ARG;
}

// the desc's refusals; total[a] = N_a, tile_ptr[n_samples + 1] = the tiles of the samples that reach the depth
int check_desc(const blu_rarefy_desc& d, uint64_t* nnz_out, std::vector<uint64_t>& total, std::vector<uint32_t>& tile_ptr) {
    if (d.struct_size != sizeof(blu_rarefy_desc))
        return refuse("blu_sample_rarefy: struct_size %llu is not one this library knows (%llu)", d.struct_size, sizeof(blu_rarefy_desc));
    if (d.depth == 0) return refuse("blu_sample_rarefy: depth is 0: a sample is rarefied to one read or more");
    if (const int rc = check_csr("blu_sample_rarefy", d.n_features, d.n_samples, d.row_ptr, d.sample, d.count, nnz_out, total)) return rc;
    if (!d.sample_stream) return refuse("blu_sample_rarefy: sample_stream is NULL");
    {
        std::vector<std::pair<uint64_t, uint32_t>> by_stream(d.n_samples);
        for (uint32_t a = 0; a < d.n_samples; ++a) by_stream[a] = {d.sample_stream[a], a};
        std::sort(by_stream.begin(), by_stream.end());
        for (uint32_t i = 1; i < d.n_samples; ++i)
            if (by_stream[i].first == by_stream[i - 1].first)
                return refuse("blu_sample_rarefy: samples %llu and %llu have the same stream: two samples of one name?", by_stream[i - 1].second,
                              by_stream[i].second);
    }
    uint64_t reads = 0;
    tile_ptr.assign((size_t)d.n_samples + 1, 0);
    for (uint32_t a = 0; a < d.n_samples; ++a) {
        if (total[a] >> 32) return refuse("blu_sample_rarefy: sample %llu has %llu reads: 2^32 or more", a, total[a]);
        const bool kept = total[a] >= d.depth;
        if (kept) reads += total[a];
        // (within 32 bits: below 2^32 reads a sample are at most 2^16 tiles, of at most 4096 samples)
        tile_ptr[a + 1] = tile_ptr[a] + (kept ? (uint32_t)((total[a] + TILE - 1) / TILE) : 0u);
    }
    if (reads > BLU_RAREFY_MAX_READS)
        return refuse("blu_sample_rarefy: the samples that reach the depth hold %llu reads: more than %llu", reads, BLU_RAREFY_MAX_READS);
    return BLU_OK;
}

// kept[nnz] by input position
int rarefy_device(const blu_rarefy_desc& d, uint64_t nnz64, const std::vector<uint64_t>& total, const std::vector<uint32_t>& tile_ptr,
                  std::vector<unsigned long long>& kept, double* t_device_ms) {
    HipPolicy pol{"blu_sample_rarefy", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    const uint32_t S = d.n_samples, F = (uint32_t)d.n_features, nnz = (uint32_t)nnz64, n_tiles = tile_ptr[S];
    HIP_CHECK(pol, hipStreamSynchronize((hipStream_t)d.stream));
    std::vector<unsigned long long> depth(S, d.depth);
    unsigned long long *d_row = nullptr, *d_count = nullptr, *d_start = nullptr, *d_stream = nullptr, *d_total = nullptr, *d_prefix = nullptr,
                       *d_rank = nullptr, *d_kept = nullptr;
    uint32_t *d_sample = nullptr, *d_keys = nullptr, *d_vals = nullptr, *d_keys_alt = nullptr, *d_vals_alt = nullptr, *d_cols = nullptr,
             *d_col = nullptr, *d_table = nullptr, *d_tile = nullptr, *d_hist = nullptr;
    void *d_scan = nullptr, *d_sort = nullptr, *d_scan64 = nullptr;
    HIP_CHECK(pol, mem.upload(&d_row, d.row_ptr, (size_t)F + 1, "row_ptr"));
    HIP_CHECK(pol, mem.upload(&d_sample, d.sample, nnz, "samples"));
    HIP_CHECK(pol, mem.upload(&d_count, d.count, nnz, "counts"));
    HIP_CHECK(pol, mem.upload(&d_stream, d.sample_stream, S, "streams"));
    HIP_CHECK(pol, mem.upload(&d_total, total.data(), S, "totals"));
    HIP_CHECK(pol, mem.upload(&d_tile, tile_ptr.data(), (size_t)S + 1, "tiles"));
    HIP_CHECK(pol, mem.upload(&d_rank, depth.data(), S, "ranks"));
    HIP_CHECK(pol, mem.alloc(&d_keys, (size_t)nnz * 4, "sort keys"));
    HIP_CHECK(pol, mem.alloc(&d_vals, (size_t)nnz * 4, "sort values"));
    HIP_CHECK(pol, mem.alloc(&d_keys_alt, (size_t)nnz * 4, "sort keys"));
    HIP_CHECK(pol, mem.alloc(&d_vals_alt, (size_t)nnz * 4, "sort values"));
    HIP_CHECK(pol, mem.alloc(&d_cols, ((size_t)S + 1) * 4, "sample counts"));
    HIP_CHECK(pol, mem.alloc(&d_col, ((size_t)S + 1) * 4, "col_ptr"));
    HIP_CHECK(pol, mem.alloc(&d_scan, scan_tmp_bytes_u32((size_t)S + 1), "scan scratch"));
    HIP_CHECK(pol, mem.alloc(&d_table, radix_table_words(nnz) * 4, "digit table"));
    HIP_CHECK(pol, mem.alloc(&d_sort, radix_scan_tmp_bytes(nnz), "scan scratch"));
    HIP_CHECK(pol, mem.alloc(&d_start, ((size_t)nnz + 1) * 8, "starts"));
    HIP_CHECK(pol, mem.alloc(&d_scan64, scan_tmp_bytes_u64((size_t)nnz + 1), "scan scratch"));
    HIP_CHECK(pol, mem.alloc(&d_prefix, (size_t)S * 8, "prefixes"));
    HIP_CHECK(pol, mem.alloc(&d_hist, (size_t)S * BINS * 4, "histograms"));
    HIP_CHECK(pol, mem.alloc(&d_kept, (size_t)nnz * 8, "kept counts"));

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    struct Events { hipEvent_t &a, &b; ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } events{ev0, ev1};
    HIP_CHECK(pol, hipEventCreate(&ev0));
    HIP_CHECK(pol, hipEventCreate(&ev1));
    HIP_CHECK(pol, hipEventRecord(ev0, nullptr));
    HIP_CHECK(pol, hipMemsetAsync(d_cols, 0, ((size_t)S + 1) * 4, nullptr));
    HIP_CHECK(pol, hipMemsetAsync(d_prefix, 0, (size_t)S * 8, nullptr));
    HIP_CHECK(pol, hipMemsetAsync(d_hist, 0, (size_t)S * BINS * 4, nullptr));
    HIP_CHECK(pol, hipMemsetAsync(d_kept, 0, (size_t)nnz * 8, nullptr));
    hipLaunchKernelGGL(rarefy_expand, dim3(grid(F, 4)), dim3(256), 0, 0, d_row, d_sample, F, S, nnz, d_keys, d_vals, d_cols);
    HIP_CHECK(pol, hipGetLastError());
    HIP_CHECK(pol, exclusive_scan_u32(d_cols, d_col, (size_t)S + 1, d_scan));
    int bits = 1;
    while ((1u << bits) < S) ++bits;
    uint32_t *k = d_keys, *ka = d_keys_alt, *v = d_vals, *va = d_vals_alt;
    HIP_CHECK(pol, radix_sort_pairs(&k, &ka, &v, &va, nnz, bits, d_table, d_sort));
    hipLaunchKernelGGL(rarefy_gather, dim3(grid((uint64_t)nnz + 1)), dim3(256), 0, 0, v, d_count, nnz, d_start);
    HIP_CHECK(pol, hipGetLastError());
    HIP_CHECK(pol, exclusive_scan_u64(d_start, d_start, (size_t)nnz + 1, d_scan64));
    const TileDev tiles{d_tile, d_stream, d_total, S};
    for (uint32_t pass = 0; pass < PASSES; ++pass) {
        hipLaunchKernelGGL(rarefy_histogram, dim3(n_tiles), dim3(TB), 0, 0, tiles, d_prefix, pass, d_hist);
        HIP_CHECK(pol, hipGetLastError());
        hipLaunchKernelGGL(rarefy_pick, dim3(grid(S, 4)), dim3(256), 0, 0, d_tile, S, d_hist, d_prefix, d_rank);
        HIP_CHECK(pol, hipGetLastError());
    }
    const CountDev c{d_col, d_start, v, d_prefix, nnz, d_kept};
    hipLaunchKernelGGL(rarefy_count, dim3(n_tiles), dim3(TB), 0, 0, tiles, c);
    HIP_CHECK(pol, hipGetLastError());
    HIP_CHECK(pol, hipEventRecord(ev1, nullptr));
    HIP_CHECK(pol, hipEventSynchronize(ev1));
    float ms = 0.f;
    HIP_CHECK(pol, hipEventElapsedTime(&ms, ev0, ev1));
    kept.resize(nnz);
    HIP_CHECK(pol, mem.download(kept.data(), d_kept, nnz));
    *t_device_ms = (double)ms;
    return BLU_OK;
}

template <class T>
bool host_array(T** out, size_t n) {
    *out = (T*)calloc(n ? n : 1, sizeof(T));
    return *out != nullptr;
}

// the output CSR from the kept counts, and the check that every kept column sums to the depth
int assemble(const blu_rarefy_desc& d, const std::vector<uint64_t>& total, const std::vector<unsigned long long>& kept, blu_rarefied* out) {
    const uint32_t S = d.n_samples;
    const uint64_t F = d.n_features;
    std::vector<uint32_t> new_id(S, UINT32_MAX);
    uint32_t K = 0;
    for (uint32_t a = 0; a < S; ++a) if (total[a] >= d.depth) new_id[a] = K++;
    std::vector<uint64_t> sum(K, 0);
    uint64_t n_out = 0;
    for (uint64_t e = 0; e < kept.size(); ++e) {
        const uint32_t a = new_id[d.sample[e]];
        if (a == UINT32_MAX) continue;
        if (kept[e] > d.count[e]) {
            set_error("blu_sample_rarefy: internal error: sample %llu keeps more reads of a feature than it has", (unsigned long long)d.sample[e]);
            return BLU_ERR_INTERNAL;
        }
        sum[a] += kept[e];
        n_out += kept[e] != 0;
    }
    if (!host_array(&out->kept_sample, K) || !host_array(&out->row_ptr, F + 1) || !host_array(&out->sample, n_out) || !host_array(&out->count, n_out)) {
        set_error("blu_sample_rarefy: out of memory");
        return BLU_ERR_ALLOC;
    }
    for (uint32_t a = 0; a < S; ++a) {
        if (new_id[a] == UINT32_MAX) continue;
        out->kept_sample[new_id[a]] = a;
        if (sum[new_id[a]] != d.depth) {
            set_error("blu_sample_rarefy: internal error: sample %llu keeps %llu reads, not the depth %llu", (unsigned long long)a,
                      (unsigned long long)sum[new_id[a]], (unsigned long long)d.depth);
            return BLU_ERR_INTERNAL;
        }
    }
    uint64_t at = 0;
    for (uint64_t f = 0; f < F; ++f) {
        for (uint64_t e = d.row_ptr[f]; e < d.row_ptr[f + 1]; ++e) {
            const uint32_t a = new_id[d.sample[e]];
            if (a == UINT32_MAX || !kept[e]) continue;
            out->sample[at] = a;
            out->count[at] = kept[e];
            ++at;
        }
        out->row_ptr[f + 1] = at;
    }
    out->n_features = F;
    out->n_kept = K;
    return BLU_OK;
}

}  // namespace
}  // namespace blu

using namespace blu;

extern "C" {

uint64_t blu_rarefy_stream(uint64_t seed, const char* name, uint64_t len) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint64_t i = 0; name && i < len; ++i) h = (h ^ (unsigned char)name[i]) * 0x100000001b3ull;
    return mix64(mix64(seed) ^ h);
}

void blu_rarefied_free(blu_rarefied* out) {
    if (!out) return;
    free(out->kept_sample); free(out->row_ptr); free(out->sample); free(out->count);
    memset(out, 0, sizeof *out);
}

int blu_sample_rarefy(const blu_rarefy_desc* desc, blu_rarefied* out) {
    if (!desc || !out) { set_error("blu_sample_rarefy: null argument"); return BLU_ERR_INVALID_ARG; }
    memset(out, 0, sizeof *out);
    uint64_t nnz = 0;
    try {
        std::vector<uint64_t> total;
        std::vector<uint32_t> tile_ptr;
        std::vector<unsigned long long> kept;
        if (const int rc = check_desc(*desc, &nnz, total, tile_ptr)) return rc;
        int rc = BLU_OK;
        if (tile_ptr[desc->n_samples]) {
            if ((rc = use_device("blu_sample_rarefy", desc->device)) != BLU_OK) return rc;
            rc = rarefy_device(*desc, nnz, total, tile_ptr, kept, &out->t_device_ms);
        } else kept.assign(nnz, 0);                          // no sample reaches the depth: nothing to select, no device asked for
        if (rc == BLU_OK) rc = assemble(*desc, total, kept, out);
        if (rc != BLU_OK) blu_rarefied_free(out);
        return rc;
    } catch (const std::bad_alloc&) {
        blu_rarefied_free(out);
        set_error("blu_sample_rarefy: out of memory");
        return BLU_ERR_ALLOC;
    }
}

}  // extern "C"
