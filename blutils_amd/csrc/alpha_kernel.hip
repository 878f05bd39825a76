// Alpha diversity and rarefaction curves (include/blu_consensus.h: blu_sample_alpha): for every sample and every
// depth D_j of an ascending ladder the six integers that observed features, Chao1, Simpson, Shannon and Good's coverage are
// ratios of, over exactly the counts blu_sample_rarefy keeps at D_j (rarefy_kernel.hip: read i of sample a has the key
// mix64(i + stream[a]), the D smallest keys stay).  The kept sets of one sample are nested along the ladder, so a read is hashed
// once per pass for all depths, not once per depth.
//
// 1. Transpose by sample and start[], as rarefy_kernel.hip step 1 (the three small kernels are restated here, as that file
//    restated distance_kernel.hip's).
// 2. Multi-rank radix select, 8 bits a pass, 8 passes from the top digit, over tiles of BLU_RAREFY_TILE ordinals.  Slot j of
//    sample a has a prefix and a rank; the prefixes do not decrease in j, so the slots with one prefix are neighbours: a group,
//    named by its first slot.  A lane hashes its ordinal once, finds the one group whose prefix the key starts with by a search
//    among the sample's <= 32 prefixes in LDS, and adds to that group's 256-bin LDS histogram: one LDS atomic a read, as in
//    rarefy_kernel.hip.  The block adds its non-empty bins to hist[a][group][bin].  One wave per (sample, slot) then reads its
//    group's histogram, appends the bin that holds its rank to its prefix (written to the other of two prefix buffers: its
//    neighbours still compare the old ones) and takes the bins below off its rank.  The host clears the histograms between
//    passes, after every slot has picked.  After the last pass prefix[a][j] is T_a(D_j), the D_j-th smallest key.
// 3. Entry levels and counts, one hash a read, over tiles of BLU_ALPHA_TILE ordinals: e(o) = the first slot whose threshold
//    the key does not pass, by a search among the thresholds in LDS; one bit map per level from ballots (32 maps of 8192 bits:
//    32 KB), the words' popcounts scanned per level; then for every (non-zero the tile overlaps, level) the reads that enter
//    there, to level[k][j] (k: the non-zero's place in the by-sample order) by a plain store when the non-zero lies inside the
//    tile, by a 32-bit atomic add when it spans tiles.
// 4. alpha_stats: a block per sample, its waves stride over the sample's non-zeros 64 at a time; a lane prefixes the level
//    counts of its non-zero into x'(j) slot by slot, the wave sums the six terms by butterfly, and lane j keeps the sums of
//    slot j in registers.  The waves' sums meet in LDS and are stored with plain stores.
// The level buffer is nnz x C words, C the slots walked at a time: the whole ladder while nnz x K stays within LEVEL_WORDS,
// else steps 3 and 4 run once per chunk of C slots (level 0 of a later chunk takes every read that entered before it).
// Raw mode (no ladder) runs steps 1 and 4 with x' = x.
// Integers only.  Every stored value is a sum of integers: none depends on the launch geometry or on the order of the atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "csr_check.h"
#include "ingest_prims.h"

namespace blu {
namespace {

constexpr uint32_t SEL_TILE = BLU_RAREFY_TILE;   // ordinals of one block of the select
constexpr uint32_t TILE = BLU_ALPHA_TILE;        // ordinals of one block of the level pass
constexpr uint32_t TB = 256;                     // threads of a tile's block
constexpr uint32_t STEPS = TILE / TB;            // ordinals of one thread
constexpr uint32_t WORDS = TILE / 64;            // 64-bit words of one level's bit map
constexpr uint32_t SLOTS = BLU_ALPHA_MAX_DEPTHS;
constexpr uint32_t DIGIT = 8, BINS = 1u << DIGIT, PASSES = 64 / DIGIT;
constexpr uint32_t SCAN_LANES = TB / SLOTS;      // threads that scan one level's words
constexpr uint32_t SCAN_WORDS = WORDS / SCAN_LANES;
constexpr uint32_t STATS_TB = 512, STATS_WAVES = STATS_TB / 64;
constexpr uint64_t LEVEL_WORDS = 1ull << 28;     // the level buffer's bound: 1 GiB
static_assert(TB == BINS, "a thread per bin");
static_assert(BINS == 4 * 64, "the pick takes four bins a lane");
static_assert(SLOTS <= 64, "a lane per slot in alpha_stats");
static_assert(SCAN_LANES == 8 && SCAN_WORDS * SCAN_LANES == WORDS, "eight neighbouring lanes scan a level");
static_assert(SLOTS * WORDS * 8 == 32768, "32 bit maps are 32 KB");

__host__ __device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// log2 x with 24 fractional bits, by squaring (include/blu_consensus.h); x >= 1
__host__ __device__ __forceinline__ unsigned long long log2_fixed(unsigned long long x) {
#ifdef __HIP_DEVICE_COMPILE__
    const uint32_t e = 63u - (uint32_t)__clzll((long long)x);
#else
    const uint32_t e = 63u - (uint32_t)__builtin_clzll(x);
#endif
    unsigned long long m = x << (63u - e), frac = 0;
    for (uint32_t i = 1; i <= 24u; ++i) {
#ifdef __HIP_DEVICE_COMPILE__
        const unsigned long long hi = __umul64hi(m, m), lo = m * m;
#else
        const unsigned __int128 p = (unsigned __int128)m * m;
        const unsigned long long hi = (unsigned long long)(p >> 64), lo = (unsigned long long)p;
#endif
        if (hi >> 63) { m = hi; frac |= 1ull << (24u - i); }
        else m = (hi << 1) | (lo >> 63);
    }
    return ((unsigned long long)e << 24) | frac;
}

// one wave per feature: the sort key (sample) and value (position) of each of its non-zeros, and the sample's count
__global__ __launch_bounds__(256) void alpha_expand(const unsigned long long* row_ptr, const uint32_t* sample, uint32_t n_features,
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
__global__ __launch_bounds__(256) void alpha_gather(const uint32_t* vals, const unsigned long long* count, uint32_t nnz, unsigned long long* cnt) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (k > nnz) return;
    cnt[k] = k < nnz ? count[min(vals[k], nnz - 1u)] : 0ull;
}

struct TileDev {
    const uint32_t* tile_ptr;            // [n_samples + 1] the first tile of each sample (a sample that reaches no depth has none)
    const unsigned long long* stream;    // [n_samples]
    const unsigned long long* total;     // [n_samples] N_a
    const uint32_t* live;                // [n_samples] the slots the sample reaches: a prefix of the ladder
    uint32_t n_samples;
    uint32_t n_slots;                    // K: the row length of the per-slot arrays
};

// the sample of tile t and the tile's ordinals [o0, o1), tiles of `tile` ordinals.  Block-uniform
__device__ __forceinline__ uint32_t tile_of(const TileDev& d, uint32_t t, uint32_t tile, unsigned long long* o0, unsigned long long* o1) {
    uint32_t lo = 0, hi = d.n_samples;   // the last a with tile_ptr[a] <= t: there is one, as tile_ptr[0] = 0 and t < tile_ptr[n_samples]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (d.tile_ptr[mid] <= t) lo = mid; else hi = mid;
    }
    const unsigned long long n = d.total[lo];
    *o0 = min((unsigned long long)(t - d.tile_ptr[lo]) * tile, n);
    *o1 = min(*o0 + tile, n);
    return lo;
}

// the first i in [0, n) with v <= sorted[i], or n
__device__ __forceinline__ uint32_t first_not_below(const unsigned long long* sorted, uint32_t n, unsigned long long v) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2u;
        if (sorted[mid] < v) lo = mid + 1u; else hi = mid;
    }
    return lo;
}

// pass p: per group of slots with one prefix (8 p bits), the histogram of the next digit among the ordinals whose key starts with it
__global__ __launch_bounds__(TB) void alpha_histogram(TileDev d, const unsigned long long* prefix, uint32_t pass, uint32_t* hist) {
    __shared__ uint32_t bins[SLOTS * BINS];
    __shared__ unsigned long long pfx[SLOTS];
    unsigned long long o0, o1;
    const uint32_t a = tile_of(d, blockIdx.x, SEL_TILE, &o0, &o1);
    const uint32_t n = min(min(d.live[a], d.n_slots), SLOTS);
    if (n == 0u) return;                 // (block-uniform; a sample with tiles reaches a depth)
    for (uint32_t i = 0; i < n; ++i) bins[i * BINS + threadIdx.x] = 0u;
    if (threadIdx.x < n) pfx[threadIdx.x] = prefix[(uint64_t)a * d.n_slots + threadIdx.x];
    __syncthreads();
    const unsigned long long st = d.stream[a];
    const uint32_t above = 64u - DIGIT * pass;       // bits below the prefix; 64 in pass 0, where every prefix is empty
    const uint32_t shift = above - DIGIT;
    for (unsigned long long o = o0 + threadIdx.x; o < o1; o += TB) {
        const unsigned long long key = mix64(o + st);
        const unsigned long long head = pass == 0u ? 0ull : key >> above;
        const uint32_t g = first_not_below(pfx, n, head);            // the first slot of the group, if there is one
        if (g < n && pfx[g] == head) atomicAdd(&bins[g * BINS + ((uint32_t)(key >> shift) & (BINS - 1u))], 1u);
    }
    __syncthreads();
    for (uint32_t g = 0; g < n; ++g) {
        if (g && pfx[g] == pfx[g - 1u]) continue;                    // (block-uniform) not the first of its group
        const uint32_t c = bins[g * BINS + threadIdx.x];
        if (c) atomicAdd(&hist[((uint64_t)a * d.n_slots + g) * BINS + threadIdx.x], c);
    }
}

// one wave per (sample, slot): the bin of its group's histogram that holds the rank joins the prefix (in `next`), the bins below
// it leave the rank.  rank is 1-based and at most the sum of the bins (the host keeps D_j <= N_a); a histogram that does not
// reach it picks the last bin, and the host's check of n then tells
__global__ __launch_bounds__(256) void alpha_pick(TileDev d, const uint32_t* hist, const unsigned long long* prefix, unsigned long long* next,
                                                  unsigned long long* rank) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t w = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t a = (uint32_t)(w / d.n_slots), j = (uint32_t)(w % d.n_slots);
    if (a >= d.n_samples) return;                            // (wave-uniform)
    if (j >= min(d.live[a], SLOTS)) return;                  // (wave-uniform) a depth the sample does not reach
    const unsigned long long* row = prefix + (uint64_t)a * d.n_slots;
    const unsigned long long mine_prefix = row[j];
    uint32_t g = j;
    while (g && row[g - 1u] == mine_prefix) --g;             // the first slot of the group
    const uint32_t* h = hist + ((uint64_t)a * d.n_slots + g) * BINS + 4u * lane;
    const uint32_t b0 = h[0], b1 = h[1], b2 = h[2], b3 = h[3];
    const unsigned long long r = rank[(uint64_t)a * d.n_slots + j];
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
        next[(uint64_t)a * d.n_slots + j] = (mine_prefix << DIGIT) | digit;
        rank[(uint64_t)a * d.n_slots + j] = r > below ? r - below : 1ull;
    }
}

struct LevelDev {
    const uint32_t* col_ptr;             // [n_samples + 1]
    const unsigned long long* start;     // [nnz + 1] exclusive sums of the counts by sample
    const unsigned long long* threshold; // [n_samples][n_slots] T_a(D_j)
    uint32_t nnz;
    uint32_t c0, width;                  // the slots [c0, c0 + width) of the ladder are walked
    uint32_t* level;                     // [nnz][width] by the by-sample order; zero on entry
};

__global__ __launch_bounds__(TB) void alpha_count(TileDev d, LevelDev c) {
    __shared__ unsigned long long bits[SLOTS * WORDS];
    __shared__ uint32_t below[SLOTS * WORDS];   // reads of the tile that enter at this level in the words before this one
    __shared__ unsigned long long thr[SLOTS];
    __shared__ uint32_t range[2];
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long o0, o1;
    const uint32_t a = tile_of(d, blockIdx.x, TILE, &o0, &o1);
    const uint32_t reach = min(min(d.live[a], d.n_slots), c.c0 + min(c.width, SLOTS));
    if (reach <= c.c0) return;           // (block-uniform) the sample reaches no slot of this chunk
    const uint32_t n = reach - c.c0;     // 1 .. SLOTS
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
    if (threadIdx.x < n) thr[threadIdx.x] = c.threshold[(uint64_t)a * d.n_slots + c.c0 + threadIdx.x];
    __syncthreads();
    const unsigned long long st = d.stream[a];
    for (uint32_t s = 0; s < STEPS; ++s) {
        const unsigned long long o = o0 + (unsigned long long)s * TB + threadIdx.x;
        const uint32_t e = o < o1 ? first_not_below(thr, n, mix64(o + st)) : n;      // n: the read enters nowhere in this chunk
        const uint32_t w = (s * TB + threadIdx.x) >> 6;
        for (uint32_t i = 0; i < n; ++i) {
            const unsigned long long word = __ballot(e == i);
            if (lane == 0u) bits[i * WORDS + w] = word;
        }
    }
    __syncthreads();
    {
        // eight neighbouring lanes scan the words of one level: SCAN_WORDS each, then the eight sums by shuffles
        const uint32_t i = threadIdx.x / SCAN_LANES, part = threadIdx.x % SCAN_LANES, w0 = i * WORDS + part * SCAN_WORDS;
        uint32_t sum = 0;
        if (i < n) for (uint32_t w = 0; w < SCAN_WORDS; ++w) sum += (uint32_t)__popcll(bits[w0 + w]);
        uint32_t incl = sum;
        for (uint32_t o = 1; o < SCAN_LANES; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o, SCAN_LANES);
            if (part >= o) incl += up;
        }
        if (i < n) {
            uint32_t run = incl - sum;
            for (uint32_t w = 0; w < SCAN_WORDS; ++w) { below[w0 + w] = run; run += (uint32_t)__popcll(bits[w0 + w]); }
        }
    }
    __syncthreads();
    // reads of the tile that enter at level i below its local ordinal p (0 .. TILE)
    const auto entered_below = [&](uint32_t i, uint32_t p) -> uint32_t {
        const uint32_t w = i * WORDS + min(p >> 6, WORDS - 1u);
        if (p >= TILE) return below[w] + (uint32_t)__popcll(bits[w]);
        return below[w] + (uint32_t)__popcll(bits[w] & ((1ull << (p & 63u)) - 1ull));
    };
    const uint32_t first = range[0], last = min(range[1], k1 - 1u);
    const uint64_t items = (uint64_t)(last - first + 1u) * n;         // (first <= last: both searches start at k0, and o0 <= o1 - 1)
    for (uint64_t it = threadIdx.x; it < items; it += TB) {
        const uint32_t k = first + (uint32_t)(it / n), i = (uint32_t)(it % n);
        const unsigned long long s0 = c.start[k] - base, s1 = c.start[k + 1] - base;
        const unsigned long long lo = max(s0, o0), hi = min(s1, o1);
        if (lo >= hi) continue;
        const uint32_t got = entered_below(i, (uint32_t)(hi - o0)) - entered_below(i, (uint32_t)(lo - o0));
        if (!got) continue;
        uint32_t* out = c.level + (uint64_t)k * c.width + i;          // (k < nnz, i < width)
        if (s0 >= o0 && s1 <= o1) *out = got;                        // the whole non-zero is this tile's
        else atomicAdd(out, got);
    }
}

struct StatsDev {
    const uint32_t* col_ptr;             // [n_samples + 1]
    const unsigned long long* start;     // [nnz + 1]
    const uint32_t* level;               // [nnz][width]; NULL in raw mode
    const uint32_t* live;                // [n_samples]; not read in raw mode
    uint32_t nnz, n_samples, n_slots;
    uint32_t c0, width;
    unsigned long long *n, *sum_sq, *sum_xlog;   // [n_samples][n_slots]
    uint32_t *observed, *singletons, *doubletons;
};

template <class T>
__device__ __forceinline__ T wave_sum(T v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a block per sample; lane j of every wave keeps the sums of slot c0 + j
__global__ __launch_bounds__(STATS_TB) void alpha_stats(StatsDev s) {
    __shared__ unsigned long long sh_n[STATS_WAVES][64], sh_sq[STATS_WAVES][64], sh_xl[STATS_WAVES][64];
    __shared__ uint32_t sh_obs[STATS_WAVES][64], sh_f1[STATS_WAVES][64], sh_f2[STATS_WAVES][64];
    const uint32_t a = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (a >= s.n_samples) return;
    const bool raw = s.level == nullptr;
    uint32_t n = 1u;
    if (!raw) {
        const uint32_t reach = min(min(s.live[a], s.n_slots), s.c0 + min(s.width, SLOTS));
        if (reach <= s.c0) return;       // (block-uniform)
        n = reach - s.c0;
    }
    const uint32_t k0 = s.col_ptr[a], k1 = min(s.col_ptr[a + 1], s.nnz);
    unsigned long long acc_n = 0, acc_sq = 0, acc_xl = 0;
    uint32_t acc_obs = 0, acc_f1 = 0, acc_f2 = 0;
    for (uint64_t kb = (uint64_t)k0 + wave * 64u; kb < k1; kb += STATS_TB) {   // (wave-uniform)
        const uint64_t k = kb + lane;
        const bool valid = k < k1;
        unsigned long long x = raw && valid ? s.start[k + 1] - s.start[k] : 0ull;
        for (uint32_t j = 0; j < n; ++j) {
            if (!raw && valid) x += s.level[k * s.width + j];
            const unsigned long long t_n = wave_sum(x), t_sq = wave_sum(x * x), t_xl = wave_sum(x > 1ull ? x * log2_fixed(x) : 0ull);
            const uint32_t t_obs = wave_sum<uint32_t>(x > 0ull), t_f1 = wave_sum<uint32_t>(x == 1ull), t_f2 = wave_sum<uint32_t>(x == 2ull);
            if (lane == j) { acc_n += t_n; acc_sq += t_sq; acc_xl += t_xl; acc_obs += t_obs; acc_f1 += t_f1; acc_f2 += t_f2; }
        }
    }
    sh_n[wave][lane] = acc_n; sh_sq[wave][lane] = acc_sq; sh_xl[wave][lane] = acc_xl;
    sh_obs[wave][lane] = acc_obs; sh_f1[wave][lane] = acc_f1; sh_f2[wave][lane] = acc_f2;
    __syncthreads();
    if (wave == 0u && lane < n) {
        for (uint32_t w = 1; w < STATS_WAVES; ++w) {
            acc_n += sh_n[w][lane]; acc_sq += sh_sq[w][lane]; acc_xl += sh_xl[w][lane];
            acc_obs += sh_obs[w][lane]; acc_f1 += sh_f1[w][lane]; acc_f2 += sh_f2[w][lane];
        }
        const uint64_t at = (uint64_t)a * s.n_slots + min(s.c0 + lane, s.n_slots - 1u);
        s.n[at] = acc_n; s.sum_sq[at] = acc_sq; s.sum_xlog[at] = acc_xl;
        s.observed[at] = acc_obs; s.singletons[at] = acc_f1; s.doubletons[at] = acc_f2;
    }
}

int refuse(const char* fmt, unsigned long long a = 0, unsigned long long b = 0) {
    set_error(fmt, a, b);
    return BLU_ERR_INVALID_ARG;
}

struct Plan {
    uint64_t nnz = 0;
    std::vector<uint64_t> total;         // [S] N_a
    std::vector<uint32_t> live;          // [S] the slots the sample reaches (raw: 1)
    std::vector<uint32_t> sel_tile_ptr;  // [S + 1] tiles of SEL_TILE ordinals of the samples that reach depths[0]
    std::vector<uint32_t> tile_ptr;      // [S + 1] the same in tiles of TILE ordinals
};

// the desc's refusals, then the plan
int check_desc(const blu_alpha_desc& d, Plan& p) {
    if (d.struct_size != sizeof(blu_alpha_desc))
        return refuse("blu_sample_alpha: struct_size %llu is not one this library knows (%llu)", d.struct_size, sizeof(blu_alpha_desc));
    if (const int rc = check_csr("blu_sample_alpha", d.n_features, d.n_samples, d.row_ptr, d.sample, d.count, &p.nnz, p.total)) return rc;
    const uint32_t K = d.n_depths, S = d.n_samples;
    if (K > BLU_ALPHA_MAX_DEPTHS) return refuse("blu_sample_alpha: %llu depths: more than %llu", K, BLU_ALPHA_MAX_DEPTHS);
    if (K && !d.depths) return refuse("blu_sample_alpha: depths is NULL");
    for (uint32_t j = 0; j < K; ++j) {
        if (d.depths[j] == 0) return refuse("blu_sample_alpha: depth %llu of the ladder is 0: a sample is rarefied to one read or more", j);
        if (j && d.depths[j] <= d.depths[j - 1])
            return refuse("blu_sample_alpha: the depths do not strictly ascend at position %llu (%llu)", j, d.depths[j]);
    }
    if (K) {
        if (!d.sample_stream) return refuse("blu_sample_alpha: sample_stream is NULL");
        std::vector<std::pair<uint64_t, uint32_t>> by_stream(S);
        for (uint32_t a = 0; a < S; ++a) by_stream[a] = {d.sample_stream[a], a};
        std::sort(by_stream.begin(), by_stream.end());
        for (uint32_t i = 1; i < S; ++i)
            if (by_stream[i].first == by_stream[i - 1].first)
                return refuse("blu_sample_alpha: samples %llu and %llu have the same stream: two samples of one name?", by_stream[i - 1].second,
                              by_stream[i].second);
    }
    uint64_t reads = 0;
    p.live.assign(S, 0);
    p.sel_tile_ptr.assign((size_t)S + 1, 0);
    p.tile_ptr.assign((size_t)S + 1, 0);
    for (uint32_t a = 0; a < S; ++a) {
        const uint64_t n = p.total[a];
        if (n >> 32) return refuse("blu_sample_alpha: sample %llu has %llu reads: 2^32 or more", a, n);
        if (K) p.live[a] = (uint32_t)(std::upper_bound(d.depths, d.depths + K, n) - d.depths);
        else p.live[a] = 1;
        const bool tiled = K && p.live[a];
        if (tiled) reads += n;
        // (within 32 bits: below 2^32 reads a sample are at most 2^19 tiles, of at most 4096 samples)
        p.sel_tile_ptr[a + 1] = p.sel_tile_ptr[a] + (tiled ? (uint32_t)((n + SEL_TILE - 1) / SEL_TILE) : 0u);
        p.tile_ptr[a + 1] = p.tile_ptr[a] + (tiled ? (uint32_t)((n + TILE - 1) / TILE) : 0u);
    }
    if (reads > BLU_RAREFY_MAX_READS)
        return refuse("blu_sample_alpha: the samples that reach the first depth hold %llu reads: more than %llu", reads, BLU_RAREFY_MAX_READS);
    return BLU_OK;
}

template <class T>
bool host_array(T** out, size_t n) {
    *out = (T*)calloc(n ? n : 1, sizeof(T));
    return *out != nullptr;
}

// the six arrays of `out` from the device
int alpha_device(const blu_alpha_desc& d, const Plan& p, blu_alpha* out) {
    HipPolicy pol{"blu_sample_alpha", BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    const uint32_t S = d.n_samples, F = (uint32_t)d.n_features, nnz = (uint32_t)p.nnz, K = d.n_depths, NS = out->n_slots;
    const size_t cells = (size_t)S * NS;
    const uint32_t width = K ? (uint32_t)std::min<uint64_t>(K, std::max<uint64_t>(LEVEL_WORDS / std::max<uint64_t>(nnz, 1), 1)) : 0u;
    HIP_CHECK(pol, hipStreamSynchronize((hipStream_t)d.stream));
    unsigned long long *d_row = nullptr, *d_count = nullptr, *d_start = nullptr, *d_stream = nullptr, *d_total = nullptr, *d_prefix = nullptr,
                       *d_next = nullptr, *d_rank = nullptr, *d_n = nullptr, *d_sq = nullptr, *d_xl = nullptr;
    uint32_t *d_sample = nullptr, *d_keys = nullptr, *d_vals = nullptr, *d_keys_alt = nullptr, *d_vals_alt = nullptr, *d_cols = nullptr,
             *d_col = nullptr, *d_table = nullptr, *d_sel_tile = nullptr, *d_tile = nullptr, *d_live = nullptr, *d_hist = nullptr,
             *d_level = nullptr, *d_obs = nullptr, *d_f1 = nullptr, *d_f2 = nullptr;
    void *d_scan = nullptr, *d_sort = nullptr, *d_scan64 = nullptr;
    HIP_CHECK(pol, mem.upload(&d_row, d.row_ptr, (size_t)F + 1, "row_ptr"));
    HIP_CHECK(pol, mem.upload(&d_sample, d.sample, nnz, "samples"));
    HIP_CHECK(pol, mem.upload(&d_count, d.count, nnz, "counts"));
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
    HIP_CHECK(pol, mem.alloc(&d_n, cells * 8, "n"));
    HIP_CHECK(pol, mem.alloc(&d_sq, cells * 8, "sum_sq"));
    HIP_CHECK(pol, mem.alloc(&d_xl, cells * 8, "sum_xlog"));
    HIP_CHECK(pol, mem.alloc(&d_obs, cells * 4, "observed"));
    HIP_CHECK(pol, mem.alloc(&d_f1, cells * 4, "singletons"));
    HIP_CHECK(pol, mem.alloc(&d_f2, cells * 4, "doubletons"));
    if (K) {
        std::vector<unsigned long long> rank(cells, 1);
        for (uint32_t a = 0; a < S; ++a) for (uint32_t j = 0; j < p.live[a]; ++j) rank[(size_t)a * K + j] = d.depths[j];
        HIP_CHECK(pol, mem.upload(&d_stream, d.sample_stream, S, "streams"));
        HIP_CHECK(pol, mem.upload(&d_total, p.total.data(), S, "totals"));
        HIP_CHECK(pol, mem.upload(&d_sel_tile, p.sel_tile_ptr.data(), (size_t)S + 1, "select tiles"));
        HIP_CHECK(pol, mem.upload(&d_tile, p.tile_ptr.data(), (size_t)S + 1, "tiles"));
        HIP_CHECK(pol, mem.upload(&d_live, p.live.data(), S, "live slots"));
        HIP_CHECK(pol, mem.upload(&d_rank, rank.data(), cells, "ranks"));
        HIP_CHECK(pol, mem.alloc(&d_prefix, cells * 8, "prefixes"));
        HIP_CHECK(pol, mem.alloc(&d_next, cells * 8, "prefixes"));
        HIP_CHECK(pol, mem.alloc(&d_hist, cells * BINS * 4, "histograms"));
        HIP_CHECK(pol, mem.alloc(&d_level, (size_t)nnz * width * 4, "level counts"));
    }

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    struct Events { hipEvent_t &a, &b; ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } events{ev0, ev1};
    HIP_CHECK(pol, hipEventCreate(&ev0));
    HIP_CHECK(pol, hipEventCreate(&ev1));
    HIP_CHECK(pol, hipEventRecord(ev0, nullptr));
    HIP_CHECK(pol, hipMemsetAsync(d_cols, 0, ((size_t)S + 1) * 4, nullptr));
    HIP_CHECK(pol, hipMemsetAsync(d_n, 0, cells * 8, nullptr));
    HIP_CHECK(pol, hipMemsetAsync(d_sq, 0, cells * 8, nullptr));
    HIP_CHECK(pol, hipMemsetAsync(d_xl, 0, cells * 8, nullptr));
    HIP_CHECK(pol, hipMemsetAsync(d_obs, 0, cells * 4, nullptr));
    HIP_CHECK(pol, hipMemsetAsync(d_f1, 0, cells * 4, nullptr));
    HIP_CHECK(pol, hipMemsetAsync(d_f2, 0, cells * 4, nullptr));
    hipLaunchKernelGGL(alpha_expand, dim3(grid(F, 4)), dim3(256), 0, 0, d_row, d_sample, F, S, nnz, d_keys, d_vals, d_cols);
    HIP_CHECK(pol, hipGetLastError());
    HIP_CHECK(pol, exclusive_scan_u32(d_cols, d_col, (size_t)S + 1, d_scan));
    int bits = 1;
    while ((1u << bits) < S) ++bits;
    uint32_t *k = d_keys, *ka = d_keys_alt, *v = d_vals, *va = d_vals_alt;
    HIP_CHECK(pol, radix_sort_pairs(&k, &ka, &v, &va, nnz, bits, d_table, d_sort));
    hipLaunchKernelGGL(alpha_gather, dim3(grid((uint64_t)nnz + 1)), dim3(256), 0, 0, v, d_count, nnz, d_start);
    HIP_CHECK(pol, hipGetLastError());
    HIP_CHECK(pol, exclusive_scan_u64(d_start, d_start, (size_t)nnz + 1, d_scan64));
    StatsDev st{d_col, d_start, nullptr, d_live, nnz, S, NS, 0u, 1u, d_n, d_sq, d_xl, d_obs, d_f1, d_f2};
    if (K) {
        const TileDev sel{d_sel_tile, d_stream, d_total, d_live, S, K}, tiles{d_tile, d_stream, d_total, d_live, S, K};
        HIP_CHECK(pol, hipMemsetAsync(d_prefix, 0, cells * 8, nullptr));
        for (uint32_t pass = 0; pass < PASSES; ++pass) {
            HIP_CHECK(pol, hipMemsetAsync(d_hist, 0, cells * BINS * 4, nullptr));
            hipLaunchKernelGGL(alpha_histogram, dim3(p.sel_tile_ptr[S]), dim3(TB), 0, 0, sel, d_prefix, pass, d_hist);
            HIP_CHECK(pol, hipGetLastError());
            hipLaunchKernelGGL(alpha_pick, dim3(grid(cells, 4)), dim3(256), 0, 0, sel, d_hist, d_prefix, d_next, d_rank);
            HIP_CHECK(pol, hipGetLastError());
            std::swap(d_prefix, d_next);
        }
        for (uint32_t c0 = 0; c0 < K; c0 += width) {
            HIP_CHECK(pol, hipMemsetAsync(d_level, 0, (size_t)nnz * width * 4, nullptr));
            const LevelDev lv{d_col, d_start, d_prefix, nnz, c0, width, d_level};
            hipLaunchKernelGGL(alpha_count, dim3(p.tile_ptr[S]), dim3(TB), 0, 0, tiles, lv);
            HIP_CHECK(pol, hipGetLastError());
            st.level = d_level; st.c0 = c0; st.width = width;
            hipLaunchKernelGGL(alpha_stats, dim3(S), dim3(STATS_TB), 0, 0, st);
            HIP_CHECK(pol, hipGetLastError());
        }
    } else {
        hipLaunchKernelGGL(alpha_stats, dim3(S), dim3(STATS_TB), 0, 0, st);
        HIP_CHECK(pol, hipGetLastError());
    }
    HIP_CHECK(pol, hipEventRecord(ev1, nullptr));
    HIP_CHECK(pol, hipEventSynchronize(ev1));
    float ms = 0.f;
    HIP_CHECK(pol, hipEventElapsedTime(&ms, ev0, ev1));
    HIP_CHECK(pol, mem.download(out->n, d_n, cells));
    HIP_CHECK(pol, mem.download(out->sum_sq, d_sq, cells));
    HIP_CHECK(pol, mem.download(out->sum_xlog, d_xl, cells));
    HIP_CHECK(pol, mem.download(out->observed, d_obs, cells));
    HIP_CHECK(pol, mem.download(out->singletons, d_f1, cells));
    HIP_CHECK(pol, mem.download(out->doubletons, d_f2, cells));
    out->t_device_ms = (double)ms;
    return BLU_OK;
}

// every present slot holds exactly its depth (raw: the sample's reads); an absent one holds nothing
int self_check(const blu_alpha_desc& d, const Plan& p, const blu_alpha& out) {
    for (uint32_t a = 0; a < d.n_samples; ++a) {
        for (uint32_t j = 0; j < out.n_slots; ++j) {
            const size_t at = (size_t)a * out.n_slots + j;
            const uint64_t want = !out.present[at] ? 0 : d.n_depths ? d.depths[j] : p.total[a];
            if (out.n[at] != want) {
                set_error("blu_sample_alpha: internal error: sample %llu holds %llu reads at the depth %llu", (unsigned long long)a,
                          (unsigned long long)out.n[at], (unsigned long long)want);
                return BLU_ERR_INTERNAL;
            }
        }
    }
    return BLU_OK;
}

}  // namespace
}  // namespace blu

using namespace blu;

extern "C" {

uint64_t blu_alpha_log2(uint64_t x) { return x ? log2_fixed(x) : 0; }

void blu_alpha_free(blu_alpha* out) {
    if (!out) return;
    free(out->present); free(out->n); free(out->observed); free(out->singletons); free(out->doubletons); free(out->sum_sq); free(out->sum_xlog);
    memset(out, 0, sizeof *out);
}

int blu_sample_alpha(const blu_alpha_desc* desc, blu_alpha* out) {
    if (!desc || !out) { set_error("blu_sample_alpha: null argument"); return BLU_ERR_INVALID_ARG; }
    memset(out, 0, sizeof *out);
    try {
        Plan p;
        if (const int rc = check_desc(*desc, p)) return rc;
        const uint32_t S = desc->n_samples, K = desc->n_depths;
        out->n_samples = S;
        out->n_slots = K ? K : 1u;
        const size_t cells = (size_t)S * out->n_slots;
        if (!host_array(&out->present, cells) || !host_array(&out->n, cells) || !host_array(&out->observed, cells) ||
            !host_array(&out->singletons, cells) || !host_array(&out->doubletons, cells) || !host_array(&out->sum_sq, cells) ||
            !host_array(&out->sum_xlog, cells)) {
            blu_alpha_free(out);
            set_error("blu_sample_alpha: out of memory");
            return BLU_ERR_ALLOC;
        }
        for (uint32_t a = 0; a < S; ++a) for (uint32_t j = 0; j < p.live[a]; ++j) out->present[(size_t)a * out->n_slots + j] = 1;
        int rc = BLU_OK;
        // raw mode without a non-zero, a ladder that no sample reaches: every integer is 0, nothing to count, no device asked for
        if (K ? p.tile_ptr[S] != 0 : p.nnz != 0) {
            if ((rc = use_device("blu_sample_alpha", desc->device)) == BLU_OK) rc = alpha_device(*desc, p, out);
        }
        if (rc == BLU_OK) rc = self_check(*desc, p, *out);
        if (rc != BLU_OK) blu_alpha_free(out);
        return rc;
    } catch (const std::bad_alloc&) {
        blu_alpha_free(out);
        set_error("blu_sample_alpha: out of memory");
        return BLU_ERR_ALLOC;
    }
}

}  // extern "C"
