// The device primitives the library's GPU programs share (ingest_prims.h): device-wide exclusive prefix sums, the stable radix
// sort of (key, value) pairs, the line index of a device text and the stable compaction of one column.  Every kernel is written
// here, no device library is called; the host wrappers launch on the null stream.  At the end, the primitives on their own for
// the tests (include/blu_consensus.h: blu_dev_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "blu_consensus.h"
#include "ingest_prims.h"
#include "wave_scan.h"

namespace blu {
namespace {

// ---- device-wide exclusive prefix sum (u32 / u64), three launches: sums of 4096-element blocks, a one-block scan of those sums,
// the blocks again with their offsets.  The arrays scanned here are bookkeeping (newline counts per 4 KiB tile, string lengths,
// top-row counts: 2 M elements at most per 100 M rows), so reading them twice costs microseconds; written here rather than
// taken from a library so that the ingest's device code is the kernels in this file plus two radix sorts.
constexpr int SCAN_THREADS = 1024, SCAN_ITEMS = 4, SCAN_BLOCK = SCAN_THREADS * SCAN_ITEMS;

template <class T>
__device__ __forceinline__ T wave_incl_scan_t(T v) {
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) { const T u = __shfl_up(v, d); if (lane >= d) v += u; }
    return v;
}
// exclusive prefix of v over the 1024 threads of the block, and the block's total; `wave_tot` = LDS, 16 entries
template <class T>
__device__ __forceinline__ T block_excl_scan_t(T v, T* wave_tot, T* total) {
    const T incl = wave_incl_scan_t(v);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) wave_tot[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < SCAN_THREADS / 64; ++w) { const T x = wave_tot[w]; all += x; if (w < wave) before += x; }
    __syncthreads();
    *total = all;
    return before + incl - v;
}
template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void scan_block_sums(const T* __restrict__ in, size_t n, T* __restrict__ block_sum) {
    __shared__ T wave_tot[SCAN_THREADS / 64];
    const size_t base = ((size_t)blockIdx.x * SCAN_THREADS + threadIdx.x) * SCAN_ITEMS;
    T v = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) if (base + k < n) v += in[base + k];
    T total;
    (void)block_excl_scan_t(v, wave_tot, &total);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}
template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void scan_block_offsets(const T* __restrict__ block_sum, size_t n_blocks, T* __restrict__ block_off) {
    __shared__ T wave_tot[SCAN_THREADS / 64];
    T carry = 0;
    for (size_t b0 = 0; b0 < n_blocks; b0 += SCAN_THREADS) {        // (one block: the sums of 4096-element blocks are few)
        const size_t b = b0 + threadIdx.x;
        const T v = b < n_blocks ? block_sum[b] : (T)0;
        T total;
        const T ex = block_excl_scan_t(v, wave_tot, &total);
        if (b < n_blocks) block_off[b] = carry + ex;
        carry += total;
    }
}
template <class T>
__global__ __launch_bounds__(SCAN_THREADS) void scan_apply(const T* __restrict__ in, size_t n, const T* __restrict__ block_off, T* __restrict__ out) {
    __shared__ T wave_tot[SCAN_THREADS / 64];
    const size_t base = ((size_t)blockIdx.x * SCAN_THREADS + threadIdx.x) * SCAN_ITEMS;
    T x[SCAN_ITEMS], v = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) { x[k] = base + k < n ? in[base + k] : (T)0; v += x[k]; }
    T total;
    T run = block_off[blockIdx.x] + block_excl_scan_t(v, wave_tot, &total);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) { if (base + k < n) out[base + k] = run; run += x[k]; }
}
template <class T> size_t scan_tmp_bytes(size_t n) { return 2 * ((n + SCAN_BLOCK - 1) / SCAN_BLOCK) * sizeof(T) + 16; }
// out[i] = in[0] + ... + in[i - 1] for i < n, modulo 2^(8 sizeof(T)); in == out is allowed: scan_block_sums only reads, and
// scan_apply reads each element into a register of the thread that writes it back (tests/test_gpu_prims.py checks both
// ways).  tmp: scan_tmp_bytes<T>(n) bytes of device memory
template <class T>
hipError_t exclusive_scan_dev(const T* in, T* out, size_t n, void* tmp) {
    if (n == 0) return hipSuccess;
    const size_t n_blocks = (n + SCAN_BLOCK - 1) / SCAN_BLOCK;
    T* const block_sum = (T*)tmp;
    T* const block_off = block_sum + n_blocks;
    hipLaunchKernelGGL((scan_block_sums<T>), dim3((unsigned)n_blocks), dim3(SCAN_THREADS), 0, 0, in, n, block_sum);
    hipLaunchKernelGGL((scan_block_offsets<T>), dim3(1), dim3(SCAN_THREADS), 0, 0, (const T*)block_sum, n_blocks, block_off);
    hipLaunchKernelGGL((scan_apply<T>), dim3((unsigned)n_blocks), dim3(SCAN_THREADS), 0, 0, in, n, (const T*)block_off, out);
    return hipGetLastError();
}

// ---- stable radix sort of (key, value) pairs of 32-bit words, least significant digit first, 8 bits per pass: regroups the rows
// of a file whose queries are not contiguous (key = query id, value = row: file order inside a query survives because every
// pass is stable).  Per pass: a 256-bin histogram per 4096-element block, one prefix sum over the (digit, block) table, and a
// scatter in which an element's place = the table's entry for (its digit, its block) + the elements of that digit before it
// in the block — counted per round of 1024 by wave (ballot match masks: the rank inside the wave) and across waves in LDS.
constexpr int RS_THREADS = 1024, RS_ITEMS = 4, RS_BLOCK = RS_THREADS * RS_ITEMS;

__global__ __launch_bounds__(RS_THREADS) void radix_hist(const uint32_t* __restrict__ keys, uint32_t n, uint32_t shift, uint32_t n_blocks,
                                                         uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    if (threadIdx.x < 256) h[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = (size_t)blockIdx.x * RS_BLOCK;
#pragma unroll
    for (int r = 0; r < RS_ITEMS; ++r) {
        const size_t i = base + (size_t)r * RS_THREADS + threadIdx.x;
        if (i < n) atomicAdd(&h[(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 256) hist[(size_t)threadIdx.x * n_blocks + blockIdx.x] = h[threadIdx.x];   // digit-major: the prefix sum runs over digits, then blocks
}

__global__ __launch_bounds__(RS_THREADS) void radix_scatter(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in, uint32_t n,
                                                            uint32_t shift, uint32_t n_blocks, const uint32_t* __restrict__ offs,
                                                            uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out) {
    __shared__ uint32_t next[256];                           // where the block's next element of each digit goes
    __shared__ uint32_t wcount[RS_THREADS / 64][256];        // this round: elements per (wave, digit), then their first place
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    if (tid < 256) next[tid] = offs[(size_t)tid * n_blocks + blockIdx.x];
    const size_t base = (size_t)blockIdx.x * RS_BLOCK;
    for (int r = 0; r < RS_ITEMS; ++r) {
        for (uint32_t k = tid; k < (RS_THREADS / 64) * 256; k += RS_THREADS) (&wcount[0][0])[k] = 0;
        __syncthreads();
        const size_t i = base + (size_t)r * RS_THREADS + tid;
        const bool valid = i < n;
        const uint32_t key = valid ? keys_in[i] : 0u, d = (key >> shift) & 255u;
        unsigned long long same = __ballot(valid);           // lanes of this wave with a valid element of the same digit
#pragma unroll
        for (int b = 0; b < 8; ++b) { const unsigned long long bb = __ballot((d >> b) & 1u); same &= ((d >> b) & 1u) ? bb : ~bb; }
        const uint32_t rank_in_wave = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && rank_in_wave == 0) wcount[wave][d] = (uint32_t)__popcll(same);
        __syncthreads();
        if (tid < 256) {                                      // digit `tid`: the waves' first places, in wave order
            uint32_t run = next[tid];
#pragma unroll
            for (uint32_t w = 0; w < RS_THREADS / 64; ++w) { const uint32_t c = wcount[w][tid]; wcount[w][tid] = run; run += c; }
            next[tid] = run;
        }
        __syncthreads();
        if (valid) { const uint32_t at = wcount[wave][d] + rank_in_wave; keys_out[at] = key; vals_out[at] = vals_in[i]; }
        __syncthreads();
    }
}

// sorts n pairs by the low 8 * ceil(bits / 8) bits of the key (callers pass keys < 2^bits, so: by the key); the sorted arrays are
// (*keys, *vals) on return (the two buffers of each swap roles per pass).  table: 2 x 256 x ceil(n / 4096) words of device memory; scan_tmp: scan_tmp_bytes<uint32_t>(256 x ceil(n / 4096))
static hipError_t radix_sort_pairs_dev(uint32_t** keys, uint32_t** keys_alt, uint32_t** vals, uint32_t** vals_alt, uint32_t n, int bits,
                                       uint32_t* table, void* scan_tmp) {
    if (n == 0) return hipSuccess;
    const uint32_t n_blocks = (uint32_t)(((size_t)n + RS_BLOCK - 1) / RS_BLOCK);
    const size_t cells = (size_t)256 * n_blocks;
    uint32_t* const hist = table;
    uint32_t* const offs = table + cells;
    for (int shift = 0; shift < bits; shift += 8) {
        hipLaunchKernelGGL(radix_hist, dim3(n_blocks), dim3(RS_THREADS), 0, 0, (const uint32_t*)*keys, n, (uint32_t)shift, n_blocks, hist);
        const hipError_t e = exclusive_scan_dev<uint32_t>(hist, offs, cells, scan_tmp);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(radix_scatter, dim3(n_blocks), dim3(RS_THREADS), 0, 0, (const uint32_t*)*keys, (const uint32_t*)*vals, n, (uint32_t)shift, n_blocks,
                           (const uint32_t*)offs, *keys_alt, *vals_alt);
        std::swap(*keys, *keys_alt);
        std::swap(*vals, *vals_alt);
    }
    return hipGetLastError();
}

// ---- 1. line index ---------------------------------------------------------------------------------------
constexpr int TILE_THREADS = 256;
constexpr uint64_t TILE_BYTES = TILE_THREADS * 16;

__device__ __forceinline__ uint32_t nl_mask16(const uint4 v, uint64_t base, uint64_t size) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xFF;
        if (c == '\n' && base + k < size) m |= 1u << k;
    }
    return m;
}

__global__ __launch_bounds__(TILE_THREADS) void count_newlines(const uint4* __restrict__ text, uint64_t size, uint32_t* __restrict__ tile_count) {
    const uint64_t base = ((uint64_t)blockIdx.x * TILE_THREADS + threadIdx.x) * 16;
    uint32_t c = 0;
    if (base < size) c = __popc(nl_mask16(text[base / 16], base, size));
    __shared__ uint32_t wave_sums[TILE_THREADS / 64];
    const uint32_t total = block_sum<TILE_THREADS>(c, wave_sums);
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(TILE_THREADS) void write_line_starts(const uint4* __restrict__ text, uint64_t size, const uint32_t* __restrict__ tile_base,
                                                                  uint64_t* __restrict__ line_start) {
    const uint64_t base = ((uint64_t)blockIdx.x * TILE_THREADS + threadIdx.x) * 16;
    uint32_t m = 0;
    if (base < size) m = nl_mask16(text[base / 16], base, size);
    __shared__ uint32_t wave_sums[TILE_THREADS / 64];
    const uint32_t before = block_excl_scan<TILE_THREADS>((uint32_t)__popc(m), wave_sums);
    uint64_t k = (uint64_t)tile_base[blockIdx.x] + before;
    while (m) {
        const int b = __ffs(m) - 1;
        m &= m - 1;
        line_start[++k] = base + b + 1;     // line k+1 starts after newline k
    }
}
// ---- stable compaction of one column (the keep words of the hit filter: 1 = kept)
enum : uint32_t { KEEP_YES = 1 };
// One column of the parsed rows: element i goes to out[pos[i]] when keep[i] is set, pos = the exclusive prefix sum of the keep
// words — so file order survives and nothing is placed by an atomic.  A thread takes 16 bytes of the column (two 8-byte or
// four 4-byte elements) and their keep words in one load each; the kept elements of neighbouring lanes land next to each
// other.  n_out = the kept count: no store goes beyond it whatever the keep words hold.
constexpr int COMPACT_THREADS = 256;
template <class T>
__global__ __launch_bounds__(COMPACT_THREADS) void compact_column(const T* __restrict__ in, const uint32_t* __restrict__ keep,
                                                                  const uint32_t* __restrict__ pos, uint32_t n, uint32_t n_out, T* __restrict__ out) {
    constexpr uint32_t V = 16 / sizeof(T);
    struct alignas(16) Elems { T v[V]; };
    struct alignas(4 * V) Keeps { uint32_t k[V]; };
    const uint64_t base = ((uint64_t)blockIdx.x * COMPACT_THREADS + threadIdx.x) * V;
    if (base >= n) return;
    uint32_t at = pos[base];
    if (base + V <= n) {
        const Elems x = *reinterpret_cast<const Elems*>(in + base);
        const Keeps k = *reinterpret_cast<const Keeps*>(keep + base);
#pragma unroll
        for (uint32_t j = 0; j < V; ++j) if (k.k[j] == KEEP_YES && at < n_out) out[at++] = x.v[j];
    } else {
        for (uint64_t j = base; j < n; ++j) if (keep[j] == KEEP_YES && at < n_out) out[at++] = in[j];
    }
}
}  // namespace

// ---- the host wrappers (ingest_prims.h)
uint64_t line_tiles(uint64_t size) { return (size + TILE_BYTES - 1) / TILE_BYTES; }
hipError_t line_count(const unsigned char* d_text, uint64_t size, uint32_t* d_tile, uint32_t* d_base, void* d_tmp, uint32_t* n_newlines) {
    const uint64_t n_tiles = line_tiles(size);
    if (n_tiles) hipLaunchKernelGGL(count_newlines, dim3((unsigned)n_tiles), dim3(TILE_THREADS), 0, 0, (const uint4*)d_text, size, d_tile);
    hipError_t e = hipMemset(d_tile + n_tiles, 0, 4);
    if (e == hipSuccess) e = exclusive_scan_dev<uint32_t>(d_tile, d_base, (size_t)n_tiles + 1, d_tmp);   // (also reports the launch above)
    if (e == hipSuccess) e = hipMemcpy(n_newlines, d_base + n_tiles, 4, hipMemcpyDeviceToHost);
    return e;
}
hipError_t line_write(const unsigned char* d_text, uint64_t size, const uint32_t* d_base, uint64_t* d_line, uint64_t n_lines, bool open_tail) {
    const uint64_t n_tiles = line_tiles(size);
    hipError_t e = hipMemset(d_line, 0, 8);
    if (e != hipSuccess) return e;
    if (n_tiles) hipLaunchKernelGGL(write_line_starts, dim3((unsigned)n_tiles), dim3(TILE_THREADS), 0, 0, (const uint4*)d_text, size, d_base, d_line);
    e = hipGetLastError();
    if (e != hipSuccess || !open_tail) return e;
    const uint64_t end = size + 1;
    return hipMemcpy(d_line + n_lines, &end, 8, hipMemcpyHostToDevice);
}
size_t scan_tmp_bytes_u32(size_t n) { return scan_tmp_bytes<uint32_t>(n); }
size_t scan_tmp_bytes_u64(size_t n) { return scan_tmp_bytes<unsigned long long>(n); }
hipError_t exclusive_scan_u32(const uint32_t* in, uint32_t* out, size_t n, void* tmp) { return exclusive_scan_dev<uint32_t>(in, out, n, tmp); }
hipError_t exclusive_scan_u64(const unsigned long long* in, unsigned long long* out, size_t n, void* tmp) {
    return exclusive_scan_dev<unsigned long long>(in, out, n, tmp);
}
hipError_t compact_column_u32(const uint32_t* in, const uint32_t* keep, const uint32_t* pos, uint32_t n, uint32_t n_out, uint32_t* out) {
    if (n) hipLaunchKernelGGL((compact_column<uint32_t>), grid(n, COMPACT_THREADS * 4), dim3(COMPACT_THREADS), 0, 0, in, keep, pos, n, n_out, out);
    return hipGetLastError();
}
hipError_t compact_column_u64(const unsigned long long* in, const uint32_t* keep, const uint32_t* pos, uint32_t n, uint32_t n_out,
                              unsigned long long* out) {
    if (n) hipLaunchKernelGGL((compact_column<unsigned long long>), grid(n, COMPACT_THREADS * 2), dim3(COMPACT_THREADS), 0, 0, in, keep, pos, n, n_out, out);
    return hipGetLastError();
}
size_t radix_table_words(uint32_t n) { return (size_t)2 * 256 * (((size_t)n + RS_BLOCK - 1) / RS_BLOCK); }
size_t radix_scan_tmp_bytes(uint32_t n) { return scan_tmp_bytes<uint32_t>((size_t)256 * (((size_t)n + RS_BLOCK - 1) / RS_BLOCK)); }
hipError_t radix_sort_pairs(uint32_t** keys, uint32_t** keys_alt, uint32_t** vals, uint32_t** vals_alt, uint32_t n, int bits,
                            uint32_t* table, void* scan_tmp) {
    return radix_sort_pairs_dev(keys, keys_alt, vals, vals_alt, n, bits, table, scan_tmp);
}
void load_dev_prims() {
    hipFuncAttributes attr;
    (void)hipFuncGetAttributes(&attr, (const void*)count_newlines);
}

}  // namespace blu

// ---- (introspection) the primitives above on their own (include/blu_consensus.h: blu_dev_*), for the tests: each call
// synchronises the device on entry and on return and allocates its own scratch.  The product paths call blu:: directly.
using namespace blu;

namespace {

int dev_enter(int device, const char* who) {
    if (const int rc = use_device(who, device)) return rc;
    const hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) { set_error("%s: hipDeviceSynchronize failed: %s", who, hipGetErrorString(e)); return BLU_ERR_HIP; }
    return BLU_OK;
}

}  // namespace

extern "C" {

int blu_dev_exclusive_scan(int device, const void* in, void* out, uint64_t n, int elem_bytes) {
    static const char WHO[] = "blu_dev_exclusive_scan";
    if ((elem_bytes != 4 && elem_bytes != 8) || (n && (!in || !out))) { set_error("%s: invalid argument", WHO); return BLU_ERR_INVALID_ARG; }
    if (const int rc = dev_enter(device, WHO)) return rc;
    HipPolicy pol{WHO, BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    void* tmp = nullptr;
    HIP_CHECK(pol, mem.alloc(&tmp, elem_bytes == 4 ? scan_tmp_bytes_u32(n) : scan_tmp_bytes_u64(n), "scan scratch"));
    if (elem_bytes == 4) HIP_CHECK(pol, exclusive_scan_u32((const uint32_t*)in, (uint32_t*)out, n, tmp));
    else HIP_CHECK(pol, exclusive_scan_u64((const unsigned long long*)in, (unsigned long long*)out, n, tmp));
    HIP_CHECK(pol, hipDeviceSynchronize());
    return BLU_OK;
}

int blu_dev_radix_sort_pairs(int device, uint32_t* keys, uint32_t* vals, uint32_t n, int bits) {
    static const char WHO[] = "blu_dev_radix_sort_pairs";
    if (bits < 0 || bits > 32 || (n && (!keys || !vals))) { set_error("%s: invalid argument", WHO); return BLU_ERR_INVALID_ARG; }
    if (const int rc = dev_enter(device, WHO)) return rc;
    if (n == 0) return BLU_OK;
    HipPolicy pol{WHO, BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    uint32_t *keys_alt = nullptr, *vals_alt = nullptr, *table = nullptr;
    void* tmp = nullptr;
    HIP_CHECK(pol, mem.alloc(&keys_alt, (size_t)n * 4, "alternate keys"));
    HIP_CHECK(pol, mem.alloc(&vals_alt, (size_t)n * 4, "alternate values"));
    HIP_CHECK(pol, mem.alloc(&table, radix_table_words(n) * 4, "digit table"));
    HIP_CHECK(pol, mem.alloc(&tmp, radix_scan_tmp_bytes(n), "scan scratch"));
    uint32_t *k = keys, *ka = keys_alt, *v = vals, *va = vals_alt;
    HIP_CHECK(pol, radix_sort_pairs(&k, &ka, &v, &va, n, bits, table, tmp));
    if (k != keys) {   // an odd number of passes: the result is in the scratch pair
        HIP_CHECK(pol, hipMemcpy(keys, k, (size_t)n * 4, hipMemcpyDeviceToDevice));
        HIP_CHECK(pol, hipMemcpy(vals, v, (size_t)n * 4, hipMemcpyDeviceToDevice));
    }
    HIP_CHECK(pol, hipDeviceSynchronize());
    return BLU_OK;
}

int blu_dev_line_index(int device, const unsigned char* text, uint64_t size, uint64_t* line, uint64_t cap, uint64_t* n_newlines) {
    static const char WHO[] = "blu_dev_line_index";
    if (!n_newlines || (size && !text) || ((uintptr_t)text & 15u) || (cap && !line)) { set_error("%s: invalid argument", WHO); return BLU_ERR_INVALID_ARG; }
    *n_newlines = 0;
    if (const int rc = dev_enter(device, WHO)) return rc;
    const uint64_t n_tiles = line_tiles(size);
    HipPolicy pol{WHO, BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    uint32_t *d_tile = nullptr, *d_tile_base = nullptr, n32 = 0;
    void* tmp = nullptr;
    HIP_CHECK(pol, mem.alloc(&d_tile, (n_tiles + 1) * 4, "line index"));
    HIP_CHECK(pol, mem.alloc(&d_tile_base, (n_tiles + 1) * 4, "line index"));
    HIP_CHECK(pol, mem.alloc(&tmp, scan_tmp_bytes_u32(n_tiles + 1), "scan scratch"));
    HIP_CHECK(pol, line_count(text, size, d_tile, d_tile_base, tmp, &n32));
    // the total in 64 bits on the host: the device scan of the tile counts is u32 and wraps
    std::vector<uint32_t> tiles(n_tiles);
    if (n_tiles) HIP_CHECK(pol, hipMemcpy(tiles.data(), d_tile, n_tiles * 4, hipMemcpyDeviceToHost));
    uint64_t total = 0;
    for (uint32_t t : tiles) total += t;
    *n_newlines = total;
    if (total > 0xFFFFFFFFull || total + 1 > cap) {
        set_error("%s: %llu newlines need %llu line entries (cap %llu, at most 2^32 newlines)", WHO, (unsigned long long)total,
                  (unsigned long long)(total + 1), (unsigned long long)cap);
        return BLU_ERR_INVALID_ARG;
    }
    HIP_CHECK(pol, line_write(text, size, d_tile_base, line, total + 1, false));
    HIP_CHECK(pol, hipDeviceSynchronize());
    return BLU_OK;
}

}  // extern "C"
