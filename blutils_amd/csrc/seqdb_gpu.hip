// `blu build-db kraken2` and the sequence half of `blu build-db qiime2` on the GPU: the `blastdbcmd -entry all` listing with
// sequences -> library.fna + prelim_map.txt (kraken2) or the qiime2 .fna (reference: core/src/use_cases/
// build_kraken_db_from_ncbi_files/generate_fasta_file.rs:45-109, generate_taxonomies_file.rs:15-36,
// build_qiime_db_from_blutils_db/mod.rs:90-150; DESIGN.md "Sequence export" lists every rule with its rs: line and test).
//
// The listing is streamed: a reader thread fills pinned chunks with read() (cut at the last newline, the rest carried into the
// next chunk; a chunk without a newline grows until the line fits), the calling thread runs each chunk through the device,
// and a writer thread write()s the finished bytes, so reading chunk k+1, device work on chunk k and writing chunk k-1
// overlap.  Pinned input and output staging are double-buffered; device memory is bounded by the largest chunk.
//
// Per chunk (null stream of the call's device):
//   bytes     one thread per 16 bytes: two-space separators (the greedy left-to-right split of str::split("  "): a space
//             starts a separator when an even number of spaces precede it in its run and the next byte is a space), counted
//             per 4 KiB tile, scanned and written as a sorted position list; the first byte that breaks UTF-8 (a local
//             test: every lead byte owns its continuation bytes, every continuation byte has an owner within 3 bytes)
//   lines     the ingest's newline count + scan + line starts, then one thread per line: its separators by binary search in
//             the position list, the trimmed pieces, the kraken2 taxid as usize, the output lengths; u64 exclusive scans
//   write     the .fna: one thread per 16 output bytes (one 16-byte store each), its line found by binary search over the
//             output offsets, every byte's source in closed form (kraken2 body byte k: row q = k / 81, column m = k % 81;
//             m == 80 is an inserted newline, otherwise it is sequence byte 80 q + m); prelim_map.txt: one thread per line
// No thread walks a sequence: its end is the next separator from the position list and its bytes are copied, upper-cased
// and wrapped by the output threads.  No device library is called; byte work bound by memory, no MFMA.
//
// `build-db sintax` / `build-db dada2` (blu_seqdb_export_labelled; neither is in the reference, DESIGN.md "Labelled FASTA
// export") run the same three threads, byte scan, separator list and line index.  The labels of the taxonomy rows, their
// (offset, length) and the taxid table (taxid_probe.h: the ingest's) go up once per call; per chunk
//   label lines   one thread per line: the pieces and the taxid as for kraken2, the probe, the row's label, the record's length
//                 (0 for a line that is skipped) and the skip word that counts it
//   ascii         one thread per 16 listing bytes: a byte >= 0x80 inside a sequence piece is the line's error, whether or
//                 not the line is written (the refusals do not depend on the taxonomies file)
//   write         one thread per 16 output bytes as above; a header byte is a constant, a listing byte or a label-blob byte
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <poll.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "blu_consensus.h"
#include "blu_internal.h"
#include "blu_pipeline.h"
#include "ingest_prims.h"
#include "seqdb_labels.h"
#include "taxid_probe.h"
#include "text_dev.h"

namespace blu {
namespace {

constexpr int TPB = 256;
constexpr uint64_t TILE = TPB * 16;               // bytes per block of the byte kernels (= the ingest's line tiles)
constexpr uint32_t NONE32 = 0xFFFFFFFFu;
constexpr uint64_t PAD = 64;                      // zero bytes after a chunk on the device

// error words: (line << 3) | code, atomicMin: the first bad line wins
enum : uint64_t { E_PIECES = 1, E_NONASCII = 2, E_TAXID = 3 };

__device__ __forceinline__ uint32_t byte_at(const uint4& v, int k) {
    const uint32_t x = (k & 8) ? ((k & 4) ? v.w : v.z) : ((k & 4) ? v.y : v.x);
    return (x >> (8 * (k & 3))) & 0xFFu;
}

// spaces immediately before position p (the run may start in an earlier thread's bytes: only runs of spaces are walked)
__device__ __forceinline__ uint32_t spaces_before(const unsigned char* __restrict__ text, uint64_t p) {
    uint32_t r = 0;
    while (p > 0 && text[p - 1] == ' ') { --p; ++r; }
    return r;
}

// separator starts among the thread's 16 bytes [base, base + 16) ∩ [0, size), as a bit mask
__device__ __forceinline__ uint32_t sep_mask(const unsigned char* __restrict__ text, uint64_t size, uint64_t base, const uint4& v) {
    if (base >= size) return 0;
    uint32_t run = (byte_at(v, 0) == ' ') ? spaces_before(text, base) : 0;
    const uint32_t next16 = text[base + 16];                    // padded past the end
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t c = byte_at(v, k);
        const uint32_t nx = k < 15 ? byte_at(v, k + 1) : next16;
        const bool in = base + k + 1 < size;                    // the pair lies inside the chunk
        m |= (c == ' ' && nx == ' ' && in && (run & 1) == 0) ? (1u << k) : 0u;
        run = c == ' ' ? run + 1 : 0;
    }
    return m;
}

__device__ __forceinline__ bool is_cont(uint32_t c) { return (c & 0xC0u) == 0x80u; }
__device__ __forceinline__ uint32_t lead_need(uint32_t c) {
    return (c >= 0xC2 && c <= 0xDF) ? 1 : (c >= 0xE0 && c <= 0xEF) ? 2 : (c >= 0xF0 && c <= 0xF4) ? 3 : 0;
}
// str::from_utf8 decided byte by byte: p is bad if it is a lead byte whose continuation bytes are missing or out of range
// (overlong forms, surrogates, > U+10FFFF), a byte that is never valid, or a continuation byte no lead byte owns
__device__ __forceinline__ bool utf8_bad_at(const unsigned char* __restrict__ text, uint64_t p, uint32_t c) {
    if (c < 0x80) return false;
    if (is_cont(c)) {
        for (uint32_t d = 1; d <= 3; ++d) {
            if (p < d) return true;
            const uint32_t q = text[p - d];
            if (is_cont(q)) continue;
            return lead_need(q) < d;
        }
        return true;
    }
    const uint32_t need = lead_need(c);
    if (need == 0) return true;
    const uint32_t lo = c == 0xE0 ? 0xA0 : c == 0xF0 ? 0x90 : 0x80;
    const uint32_t hi = c == 0xED ? 0x9F : c == 0xF4 ? 0x8F : 0xBF;
    const uint32_t b1 = text[p + 1];                            // padded: a zero past the end is not a continuation
    if (b1 < lo || b1 > hi) return true;
    for (uint32_t d = 2; d <= need; ++d)
        if (!is_cont(text[p + d])) return true;
    return false;
}

template <class T>
__device__ __forceinline__ T block_excl_scan(T v, T* total) {
    __shared__ T part[TPB / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    T x = v;
    for (int d = 1; d < 64; d <<= 1) { const T y = __shfl_up(x, d); if (lane >= d) x += y; }
    if (lane == 63) part[w] = x;
    __syncthreads();
    T before = 0, all = 0;
    for (int k = 0; k < TPB / 64; ++k) { before += k < w ? part[k] : 0; all += part[k]; }
    __syncthreads();
    *total = all;
    return before + x - v;
}

// pass 1 over the bytes: separators per tile, and the first byte that is not UTF-8 (atomicMin)
__global__ __launch_bounds__(TPB) void seqdb_scan_bytes(const unsigned char* __restrict__ text, uint64_t size,
                                                        uint32_t* __restrict__ tile_sep, unsigned long long* __restrict__ first_bad) {
    const uint64_t base = ((uint64_t)blockIdx.x * TPB + threadIdx.x) * 16;
    const uint4 v = base < size ? *reinterpret_cast<const uint4*>(text + base) : make_uint4(0, 0, 0, 0);
    const uint32_t m = sep_mask(text, size, base, v);
    if (base < size && ((v.x | v.y | v.z | v.w) & 0x80808080u)) {
        for (int k = 0; k < 16; ++k) {
            if (base + k >= size) break;
            if (utf8_bad_at(text, base + k, byte_at(v, k))) { atomicMin(first_bad, (unsigned long long)(base + k)); break; }
        }
    }
    uint32_t total;
    (void)block_excl_scan<uint32_t>((uint32_t)__popc(m), &total);
    if (threadIdx.x == 0) tile_sep[blockIdx.x] = total;
}

// pass 2: the separator positions, in order (tile_base: exclusive scan of the tile counts)
__global__ __launch_bounds__(TPB) void seqdb_sep_write(const unsigned char* __restrict__ text, uint64_t size,
                                                       const uint32_t* __restrict__ tile_base, uint64_t* __restrict__ sep) {
    const uint64_t base = ((uint64_t)blockIdx.x * TPB + threadIdx.x) * 16;
    const uint4 v = base < size ? *reinterpret_cast<const uint4*>(text + base) : make_uint4(0, 0, 0, 0);
    uint32_t m = sep_mask(text, size, base, v);
    uint32_t total;
    uint32_t at = tile_base[blockIdx.x] + block_excl_scan<uint32_t>((uint32_t)__popc(m), &total);
    while (m) {
        const int k = __ffs(m) - 1;
        sep[at++] = base + k;
        m &= m - 1;
    }
}

__device__ __forceinline__ uint64_t lower_bound(const uint64_t* __restrict__ a, uint64_t n, uint64_t x) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}
// last index i in [lo, hi] with a[i] <= x (a[lo] <= x holds)
template <class T>
__device__ __forceinline__ uint64_t last_le(const T* __restrict__ a, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) { const uint64_t mid = (lo + hi + 1) >> 1; if (a[mid] <= x) lo = mid; else hi = mid - 1; }
    return lo;
}

// usize::from_str (core::num, from_str_radix): one optional leading '+', then decimal digits only, no overflow
__device__ __forceinline__ bool parse_usize(const unsigned char* __restrict__ text, uint64_t a, uint64_t b, unsigned long long* out) {
    if (a < b && text[a] == '+') ++a;
    if (a >= b) return false;
    unsigned long long v = 0;
    for (; a < b; ++a) {                                         // stops at the 21st digit at the latest (overflow)
        const uint32_t d = (uint32_t)text[a] - '0';
        if (d > 9 || v > (~0ull - d) / 10) return false;
        v = v * 10 + d;
    }
    *out = v;
    return true;
}

struct LineOut {
    uint64_t* acc_a; uint32_t* acc_n;       // trimmed pieces: accession, taxid, oid (qiime2), sequence
    uint64_t* tax_a; uint32_t* tax_n;
    uint64_t* oid_a; uint32_t* oid_n;
    uint64_t* seq_a; uint64_t* seq_n;
    unsigned long long* num;                // kraken2: the taxid as usize
    unsigned long long* fna_len;            // [n + 1] (the last is 0: the scan's total)
    unsigned long long* map_len;            // [n + 1] kraken2
    unsigned long long* err;                // (line << 3) | code
    uint32_t* stop_line;                    // first line holding the first non-UTF-8 byte
    unsigned long long* max_line;
};

// one thread per line: pieces, taxid, output lengths
__global__ __launch_bounds__(TPB) void seqdb_lines(const unsigned char* __restrict__ text, const uint64_t* __restrict__ line, uint32_t n,
                                                   const uint64_t* __restrict__ sep, uint64_t n_sep, int qiime,
                                                   const unsigned long long* __restrict__ first_bad, LineOut o) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    unsigned long long len = 0;
    if (i < n) {
        const uint64_t ls = line[i], le = line[i + 1] - 1;      // [ls, le): the line without its newline
        len = le - ls;
        const unsigned long long fb = *first_bad;
        if (fb >= ls && fb < le) atomicMin(o.stop_line, i);
        const uint32_t K = qiime ? 3 : 2;                        // separators before the sequence piece
        const uint64_t j = lower_bound(sep, n_sep, ls);
        unsigned long long fna = 0, map = 0;
        if (j + K - 1 >= n_sep || sep[j + K - 1] >= le) {
            atomicMin(o.err, ((unsigned long long)i << 3) | E_PIECES);   // rs:71-75 expect(er_msg) panics
        } else {
            uint64_t a0 = ls, b0 = sep[j];
            uint64_t a1 = sep[j] + 2, b1 = sep[j + 1];
            uint64_t a2 = a1, b2 = a1;
            if (qiime) { a2 = sep[j + 1] + 2; b2 = sep[j + 2]; }
            uint64_t as = sep[j + K - 1] + 2;
            uint64_t bs = (j + K < n_sep && sep[j + K] < le) ? sep[j + K] : le;   // a further separator ends the sequence
            trim(text, a0, b0); trim(text, a1, b1); trim(text, a2, b2); trim(text, as, bs);
            o.acc_a[i] = a0; o.acc_n[i] = (uint32_t)(b0 - a0);
            o.tax_a[i] = a1; o.tax_n[i] = (uint32_t)(b1 - a1);
            o.oid_a[i] = a2; o.oid_n[i] = (uint32_t)(b2 - a2);
            const uint64_t L = bs - as;
            o.seq_a[i] = as; o.seq_n[i] = L;
            if (qiime) {
                fna = 1 + (b1 - a1) + 1 + (b2 - a2) + 1 + (b0 - a0) + 1 + L + 1;            // mod.rs:137-139
            } else {
                unsigned long long v = 0;
                if (!parse_usize(text, a1, b1, &v)) atomicMin(o.err, ((unsigned long long)i << 3) | E_TAXID);   // rs:98 unwrap
                o.num[i] = v;
                fna = 14 + (b1 - a1) + 1 + (b0 - a0) + 1 + L + (L ? (L - 1) / 80 : 0) + 1;  // rs:78-90
                const uint32_t d = n_digits(v);
                map = 19 + d + 1 + (b0 - a0) + 1 + d + 1;                                   // generate_taxonomies_file.rs:30
            }
        }
        o.fna_len[i] = fna;
        if (!qiime) o.map_len[i] = map;
    }
    for (int d = 32; d > 0; d >>= 1) len = max(len, (unsigned long long)__shfl_down(len, d));
    if ((threadIdx.x & 63) == 0 && len) atomicMax(o.max_line, len);
}

struct LineIn {
    const unsigned long long* off;          // [n + 1] exclusive scan of the lengths
    const uint64_t* acc_a; const uint32_t* acc_n;
    const uint64_t* tax_a; const uint32_t* tax_n;
    const uint64_t* oid_a; const uint32_t* oid_n;
    const uint64_t* seq_a; const uint64_t* seq_n;
};

// ">kraken:taxid|" as two little-endian words
constexpr unsigned long long KR0 = 0x3a6e656b61726b3eull;   // ">kraken:"
constexpr unsigned long long KR1 = 0x00007c6469786174ull;   // "taxid|"

// one thread per 16 output bytes of the .fna; each writes one aligned 16-byte word (the buffer is padded to whole tiles)
__global__ __launch_bounds__(TPB) void seqdb_write_fna(const unsigned char* __restrict__ text, uint32_t n, LineIn L, int qiime,
                                                       unsigned long long* __restrict__ err, unsigned char* __restrict__ out) {
    __shared__ uint64_t range[2];
    const unsigned long long total = L.off[n];
    const uint64_t ob = (uint64_t)blockIdx.x * TILE;
    if (threadIdx.x < 2) {
        const uint64_t x = threadIdx.x == 0 ? ob : min(ob + TILE, (uint64_t)total) - 1;
        range[threadIdx.x] = last_le(L.off, 0, n - 1, x);
    }
    __syncthreads();
    const uint64_t o0 = ob + (uint64_t)threadIdx.x * 16;
    if (o0 >= total) { *reinterpret_cast<uint4*>(out + o0) = make_uint4(0, 0, 0, 0); return; }
    uint64_t i = last_le(L.off, range[0], range[1], o0);
    uint64_t start = L.off[i], next = L.off[i + 1];
    uint64_t acc_a = L.acc_a[i], tax_a = L.tax_a[i], oid_a = L.oid_a[i], seq_a = L.seq_a[i];
    uint32_t acc_n = L.acc_n[i], tax_n = L.tax_n[i], oid_n = L.oid_n[i];
    uint64_t seq_n = L.seq_n[i];
    bool nonascii = false;
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint64_t o = o0 + k;
        uint32_t c = 0;
        if (o < total) {
            if (o >= next) {                                     // the next record (lengths are > 0 below the total)
                if (qiime == 0 && nonascii) atomicMin(err, ((unsigned long long)i << 3) | E_NONASCII);
                nonascii = false;
                do { ++i; start = next; next = L.off[i + 1]; } while (o >= next);
                acc_a = L.acc_a[i]; tax_a = L.tax_a[i]; oid_a = L.oid_a[i]; seq_a = L.seq_a[i];
                acc_n = L.acc_n[i]; tax_n = L.tax_n[i]; oid_n = L.oid_n[i]; seq_n = L.seq_n[i];
            }
            uint64_t r = o - start;
            if (qiime) {                                         // >TAXID-OID-ACC\nSEQ\n
                if (r == 0) c = '>';
                else if ((r -= 1) < tax_n) c = text[tax_a + r];
                else if ((r -= tax_n) == 0) c = '-';
                else if ((r -= 1) < oid_n) c = text[oid_a + r];
                else if ((r -= oid_n) == 0) c = '-';
                else if ((r -= 1) < acc_n) c = text[acc_a + r];
                else if ((r -= acc_n) == 0) c = '\n';
                else if ((r -= 1) < seq_n) c = text[seq_a + r];
                else c = '\n';
            } else {                                             // >kraken:taxid|TAXID|ACC\nSEQ in 80-column lines\n
                const uint64_t body = seq_n + (seq_n ? (seq_n - 1) / 80 : 0);
                if (r < 14) c = (uint32_t)(((r < 8 ? KR0 : KR1) >> (8 * (r & 7))) & 0xFF);
                else if ((r -= 14) < tax_n) c = text[tax_a + r];
                else if ((r -= tax_n) == 0) c = '|';
                else if ((r -= 1) < acc_n) c = text[acc_a + r];
                else if ((r -= acc_n) == 0) c = '\n';
                else if ((r -= 1) < body) {
                    const uint64_t q = r / 81, m = r - q * 81;
                    if (m == 80) c = '\n';
                    else {
                        c = text[seq_a + q * 80 + m];
                        nonascii = nonascii || c >= 0x80;
                        c = (c >= 'a' && c <= 'z') ? c - 32 : c;   // str::to_uppercase on ASCII
                    }
                } else c = '\n';
            }
        }
        w[k >> 2] |= c << (8 * (k & 3));
    }
    if (qiime == 0 && nonascii) atomicMin(err, ((unsigned long long)i << 3) | E_NONASCII);
    *reinterpret_cast<uint4*>(out + o0) = make_uint4(w[0], w[1], w[2], w[3]);
}

// kraken2 prelim_map.txt: one thread per line, `TAXID\tkraken:taxid|N|ACC\tN\n`
__global__ __launch_bounds__(TPB) void seqdb_write_map(const unsigned char* __restrict__ text, uint32_t n, const unsigned long long* __restrict__ off,
                                                       const unsigned long long* __restrict__ len, const uint64_t* __restrict__ acc_a,
                                                       const uint32_t* __restrict__ acc_n, const unsigned long long* __restrict__ num,
                                                       unsigned char* __restrict__ out) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    if (i >= n || len[i] == 0) return;
    unsigned char* o = out + off[i];
    const char* head = "TAXID\tkraken:taxid|";
    for (int k = 0; k < 19; ++k) *o++ = (unsigned char)head[k];
    const unsigned long long v = num[i];
    const uint32_t d = n_digits(v);
    put_digits(o, v, d); o += d;
    *o++ = '|';
    const uint64_t a = acc_a[i];
    for (uint32_t k = 0; k < acc_n[i]; ++k) *o++ = text[a + k];
    *o++ = '\t';
    put_digits(o, v, d); o += d;
    *o = '\n';
}

// ---- the labelled formats ----------------------------------------------------------------------------------------------
// the labels of the taxonomy rows as the kernels see them: row r's label is blob[off[r], off[r] + len[r]), len 0 = none
struct DevLabels {
    const unsigned char* blob;
    const unsigned long long* off;
    const uint32_t* len;
    DevTaxidMap map;
    int sintax;
};

constexpr unsigned long long SKIP_UNKNOWN = 1ull, SKIP_UNLABELLED = 1ull << 32;   // the two counts share one scanned word

// one thread per line: pieces and taxid as seqdb_lines (kraken2), then the join.  What LineOut's fields hold here: tax_a /
// tax_n the label's offset in the blob and its length, map_len the skip word; oid_* and num are not used
__global__ __launch_bounds__(TPB) void seqdb_label_lines(const unsigned char* __restrict__ text, const uint64_t* __restrict__ line, uint32_t n,
                                                         const uint64_t* __restrict__ sep, uint64_t n_sep,
                                                         const unsigned long long* __restrict__ first_bad, DevLabels lab, LineOut o) {
    const uint32_t i = blockIdx.x * TPB + threadIdx.x;
    unsigned long long len = 0;
    if (i < n) {
        const uint64_t ls = line[i], le = line[i + 1] - 1;
        len = le - ls;
        const unsigned long long fb = *first_bad;
        if (fb >= ls && fb < le) atomicMin(o.stop_line, i);
        const uint64_t j = lower_bound(sep, n_sep, ls);
        unsigned long long fna = 0, skip = 0;
        uint64_t seq_a = 0, seq_n = 0;
        if (j + 1 >= n_sep || sep[j + 1] >= le) {
            atomicMin(o.err, ((unsigned long long)i << 3) | E_PIECES);
        } else {
            uint64_t a0 = ls, b0 = sep[j];
            uint64_t a1 = sep[j] + 2, b1 = sep[j + 1];
            uint64_t as = sep[j + 1] + 2;
            uint64_t bs = (j + 2 < n_sep && sep[j + 2] < le) ? sep[j + 2] : le;
            trim(text, a0, b0); trim(text, a1, b1); trim(text, as, bs);
            o.acc_a[i] = a0; o.acc_n[i] = (uint32_t)(b0 - a0);
            seq_a = as; seq_n = bs - as;
            unsigned long long v = 0;
            if (!parse_usize(text, a1, b1, &v)) {
                atomicMin(o.err, ((unsigned long long)i << 3) | E_TAXID);
            } else {
                // the table's keys are i64 (a taxid of the taxonomies file above i64::MAX is stored as i64::MAX and a negative
                // one as it is): a listing taxid of 2^63 or more equals none of them by value
                const uint32_t row = v >> 63 ? BLU_UNMATCHED_TAXID : taxid_lookup(lab.map, (long long)v);
                const uint32_t ln = row == BLU_UNMATCHED_TAXID ? 0 : lab.len[row];
                if (row == BLU_UNMATCHED_TAXID) skip = SKIP_UNKNOWN;
                else if (ln == 0) skip = SKIP_UNLABELLED;
                else {
                    o.tax_a[i] = lab.off[row]; o.tax_n[i] = ln;
                    fna = lab.sintax ? 1 + (b0 - a0) + 5 + ln + 2 + seq_n + 1      // >ACC;tax=LABEL;\nSEQ\n
                                     : 1 + (unsigned long long)ln + 1 + seq_n + 1;   // >LABEL\nSEQ\n
                }
            }
        }
        o.seq_a[i] = seq_a; o.seq_n[i] = seq_n;             // (no pieces: an empty sequence, for seqdb_label_ascii)
        o.fna_len[i] = fna;
        o.map_len[i] = skip;
    }
    for (int d = 32; d > 0; d >>= 1) len = max(len, (unsigned long long)__shfl_down(len, d));
    if ((threadIdx.x & 63) == 0 && len) atomicMax(o.max_line, len);
}

// one thread per 16 listing bytes: a byte >= 0x80 that lies in its line's sequence piece.  All but a few threads leave after
// one load and one test; the others find their line once by binary search over the line starts
__global__ __launch_bounds__(TPB) void seqdb_label_ascii(const unsigned char* __restrict__ text, uint64_t size, const uint64_t* __restrict__ line,
                                                         uint32_t n, const uint64_t* __restrict__ seq_a, const uint64_t* __restrict__ seq_n,
                                                         unsigned long long* __restrict__ err) {
    const uint64_t base = ((uint64_t)blockIdx.x * TPB + threadIdx.x) * 16;
    if (base >= size || n == 0) return;
    const uint4 v = *reinterpret_cast<const uint4*>(text + base);
    if (((v.x | v.y | v.z | v.w) & 0x80808080u) == 0) return;
    uint64_t i = last_le(line, 0, n - 1, base);
    for (int k = 0; k < 16; ++k) {
        const uint64_t p = base + k;
        if (p >= size) break;
        if (byte_at(v, k) < 0x80) continue;
        while (p >= line[i + 1]) ++i;                           // (p < size <= line[n])
        if (p >= seq_a[i] && p - seq_a[i] < seq_n[i]) { atomicMin(err, ((unsigned long long)i << 3) | E_NONASCII); break; }
    }
}

constexpr unsigned long long SX_TAX = 0x0000003d7861743bull;   // ";tax=" as a little-endian word

// one thread per 16 output bytes of the labelled .fna, as seqdb_write_fna: L.tax_a / L.tax_n are the label's place in blob
__global__ __launch_bounds__(TPB) void seqdb_write_labelled(const unsigned char* __restrict__ text, const unsigned char* __restrict__ blob,
                                                            uint32_t n, LineIn L, int sintax, unsigned char* __restrict__ out) {
    __shared__ uint64_t range[2];
    const unsigned long long total = L.off[n];
    const uint64_t ob = (uint64_t)blockIdx.x * TILE;
    if (threadIdx.x < 2) {
        const uint64_t x = threadIdx.x == 0 ? ob : min(ob + TILE, (uint64_t)total) - 1;
        range[threadIdx.x] = last_le(L.off, 0, n - 1, x);
    }
    __syncthreads();
    const uint64_t o0 = ob + (uint64_t)threadIdx.x * 16;
    if (o0 >= total) { *reinterpret_cast<uint4*>(out + o0) = make_uint4(0, 0, 0, 0); return; }
    uint64_t i = last_le(L.off, range[0], range[1], o0);       // the last line that starts at or before o0: it is not empty
    uint64_t start = L.off[i], next = L.off[i + 1];
    uint64_t acc_a = L.acc_a[i], lab_a = L.tax_a[i], seq_a = L.seq_a[i];
    uint32_t acc_n = sintax ? L.acc_n[i] : 0, lab_n = L.tax_n[i];
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint64_t o = o0 + k;
        uint32_t c = 0;
        if (o < total) {
            if (o >= next) {                                     // the next record that has bytes (skipped lines have none)
                do { ++i; start = next; next = L.off[i + 1]; } while (o >= next);
                acc_a = L.acc_a[i]; lab_a = L.tax_a[i]; seq_a = L.seq_a[i];
                acc_n = sintax ? L.acc_n[i] : 0; lab_n = L.tax_n[i];
            }
            uint64_t r = o - start;
            const uint64_t last = next - start - 1;              // the record's final newline
            if (r == 0) c = '>';
            else if (r == last) c = '\n';
            else {
                r -= 1;
                bool done = false;
                if (sintax) {                                    // ACC;tax=
                    if (r < acc_n) { c = text[acc_a + r]; done = true; }
                    else if ((r -= acc_n) < 5) { c = (uint32_t)((SX_TAX >> (8 * r)) & 0xFF); done = true; }
                    else r -= 5;
                }
                if (!done) {
                    if (r < lab_n) c = blob[lab_a + r];
                    else if ((r -= lab_n) < (sintax ? 2u : 1u)) c = (sintax && r == 0) ? ';' : '\n';
                    else {
                        c = text[seq_a + (r - (sintax ? 2 : 1))];
                        c = (c >= 'a' && c <= 'z') ? c - 32 : c;
                    }
                }
            }
        }
        w[k >> 2] |= c << (8 * (k & 3));
    }
    *reinterpret_cast<uint4*>(out + o0) = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace

namespace {

// a device buffer that only grows (bytes rounded up, 1/8 slack so that chunks of similar sizes reuse it); a failed
// allocation is noted in the caller's policy
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    ~DevBuf() { if (p) (void)hipFree(p); }
    template <class T>
    hipError_t get(T** out, size_t bytes, const char* what, HipPolicy& pol) {
        if (bytes > cap) {
            if (p) (void)hipFree(p);
            p = nullptr; cap = 0;
            const size_t want = ((bytes + bytes / 8) + 4095) & ~(size_t)4095;
            if (const hipError_t e = pol.noted(hipMalloc(&p, want), want, what); e != hipSuccess) { p = nullptr; return e; }
            cap = want;
        }
        *out = (T*)p;
        return hipSuccess;
    }
};

// pinned host staging that only grows; contents are kept on growth when asked
struct Pinned {
    unsigned char* p = nullptr;
    size_t cap = 0;
    ~Pinned() { if (p) (void)hipHostFree(p); }
    bool grow(size_t bytes, size_t keep) {
        if (bytes <= cap) return true;
        unsigned char* q = nullptr;
        if (hipHostMalloc((void**)&q, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (keep) memcpy(q, p, keep);
        if (p) (void)hipHostFree(p);
        p = q; cap = bytes;
        return true;
    }
};

// a queue of slot numbers between two threads; -1 ends it
struct Chan {
    std::mutex m;
    std::condition_variable cv;
    std::deque<int> q;
    void push(int v) { { std::lock_guard<std::mutex> g(m); q.push_back(v); } cv.notify_one(); }
    int pop() {
        std::unique_lock<std::mutex> g(m);
        cv.wait(g, [&] { return !q.empty(); });
        const int v = q.front();
        q.pop_front();
        return v;
    }
};

struct InSlot { Pinned buf; size_t len = 0; };
struct OutSlot { Pinned fna, map; size_t fna_len = 0, map_len = 0; };

struct Export {
    const blu_seqdb_desc& D;
    blu_seqdb_stats& S;
    std::string input;                      // the input's name in messages
    int in_fd = -1, fna_fd = -1, map_fd = -1;
    std::string map_tmp;
    size_t chunk = 0;

    InSlot in[2];
    OutSlot out[2];
    Chan in_full, in_free, out_full, out_free;
    std::atomic<bool> stop{false};
    std::string read_err, write_err;        // set by the reader / writer thread before it ends
    double t_read = 0, t_write = 0;
    HipPolicy pol{"seqdb", BLU_ERR_ALLOC};  // (the device stage's: the calling thread's)

    // the labelled formats: the host's labels (null for kraken2 / qiime2), their device copies, the skipped lines so far
    const LabelSet* labels = nullptr;
    DevBuf d_blob, d_lab_off, d_lab_len, d_lab_tab;
    DevLabels lab{};
    uint64_t n_unknown = 0, n_unlabelled = 0;
    double t_label_upload = 0;

    // device buffers (one set: the device stage is the calling thread's, chunk after chunk)
    DevBuf d_text, d_tile, d_tbase, d_stile, d_sbase, d_scan, d_line, d_sep, d_cnt, d_acc_a, d_acc_n, d_tax_a, d_tax_n, d_oid_a,
        d_oid_n, d_seq_a, d_seq_n, d_num, d_fna_len, d_fna_off, d_map_len, d_map_off, d_fna, d_map;

    Export(const blu_seqdb_desc& d, blu_seqdb_stats& s) : D(d), S(s) {}

    // ---- reader thread: chunks cut at their last newline, the rest carried into the next chunk
    void reader() {
        std::vector<unsigned char> carry;
        bool eof = false;
        while (!eof) {
            const int s = in_free.pop();
            if (s < 0 || stop.load()) break;
            InSlot& I = in[s];
            if (!I.buf.grow(std::max(chunk, carry.size() + chunk / 2 + 1), 0)) { read_err = "pinned host allocation failed"; break; }
            if (!carry.empty()) memcpy(I.buf.p, carry.data(), carry.size());
            size_t len = carry.size(), scanned = carry.size();
            size_t cut = 0;
            bool ok = true;
            for (;;) {
                if (len == I.buf.cap) {
                    const unsigned char* nl = scanned < len ? (const unsigned char*)memrchr(I.buf.p + scanned, '\n', len - scanned) : nullptr;
                    if (nl) { cut = (size_t)(nl - I.buf.p) + 1; break; }
                    scanned = len;                                   // a line longer than the chunk: grow until it fits
                    if (!I.buf.grow(I.buf.cap * 2, len)) { read_err = "pinned host allocation failed"; ok = false; break; }
                }
                struct pollfd pf = {in_fd, POLLIN, 0};
                const int pr = poll(&pf, 1, 200);
                if (stop.load()) { ok = false; break; }
                if (pr < 0 && errno != EINTR) { read_err = std::string("poll: ") + strerror(errno); ok = false; break; }
                if (pr <= 0) continue;
                const double t0 = now_s();
                const ssize_t r = read(in_fd, I.buf.p + len, I.buf.cap - len);
                t_read += 1e3 * (now_s() - t0);
                if (r < 0) {
                    if (errno == EINTR || errno == EAGAIN) continue;
                    read_err = std::string("read: ") + strerror(errno); ok = false; break;
                }
                if (r == 0) { eof = true; cut = len; break; }
                len += (size_t)r;
            }
            if (!ok) break;
            carry.assign(I.buf.p + cut, I.buf.p + len);
            I.len = cut;
            if (cut) in_full.push(s);
            else in_free.push(s);
        }
        in_full.push(-1);
    }

    // ---- writer thread
    void writer() {
        for (;;) {
            const int s = out_full.pop();
            if (s < 0) break;
            OutSlot& O = out[s];
            const double t0 = now_s();
            const bool ok = write_all(fna_fd, O.fna.p, O.fna_len) && (map_fd < 0 || write_all(map_fd, O.map.p, O.map_len));
            t_write += 1e3 * (now_s() - t0);
            if (!ok && write_err.empty()) { write_err = strerror(errno); stop = true; }
            out_free.push(s);
        }
    }

    // ---- the labels, once per call
    int upload_labels() {
        const double t0 = now_s();
        const LabelSet& H = *labels;
        unsigned char* blob; unsigned long long* off; uint32_t* len; TaxidMap::E* tab;
        HIP_CHECK(pol, d_blob.get(&blob, H.blob.size() + PAD, "labels", pol));
        HIP_CHECK(pol, d_lab_off.get(&off, H.off.size() * 8 + PAD, "labels", pol));
        HIP_CHECK(pol, d_lab_len.get(&len, H.len.size() * 4 + PAD, "labels", pol));
        HIP_CHECK(pol, d_lab_tab.get(&tab, H.row_of.tab.size() * sizeof(TaxidMap::E), "taxid map", pol));
        if (!H.blob.empty()) HIP_CHECK(pol, hipMemcpy(blob, H.blob.data(), H.blob.size(), hipMemcpyHostToDevice));
        if (!H.off.empty()) {
            HIP_CHECK(pol, hipMemcpy(off, H.off.data(), H.off.size() * 8, hipMemcpyHostToDevice));
            HIP_CHECK(pol, hipMemcpy(len, H.len.data(), H.len.size() * 4, hipMemcpyHostToDevice));
        }
        HIP_CHECK(pol, hipMemcpy(tab, H.row_of.tab.data(), H.row_of.tab.size() * sizeof(TaxidMap::E), hipMemcpyHostToDevice));
        lab = DevLabels{blob, off, len, DevTaxidMap{tab, H.row_of.tab.size() - 1}, D.format == BLU_SEQDB_SINTAX};
        t_label_upload = 1e3 * (now_s() - t0);
        return BLU_OK;
    }

    // ---- one chunk on the device into O; *done: a stop or an error ended the listing in this chunk (set once O is filled)
    int chunk_on_device(const InSlot& I, OutSlot& O, uint64_t line_base, bool* done) {
        const int qiime = D.format == BLU_SEQDB_QIIME2;
        const bool kraken = D.format == BLU_SEQDB_KRAKEN2;
        const uint64_t size = I.len;
        S.n_chunks += 1;
        if (size >= (1ull << 32) - TILE) { set_error("seqdb: %s: a line of 4 GiB or more near line %llu is not supported", input.c_str(),
                                                     (unsigned long long)line_base + 1); return BLU_ERR_INVALID_ARG; }
        const uint64_t n_tiles = (size + TILE - 1) / TILE;
        unsigned char* text;
        HIP_CHECK(pol, d_text.get(&text, n_tiles * TILE + PAD, "chunk", pol));
        HIP_CHECK(pol, hipMemcpy(text, I.buf.p, size, hipMemcpyHostToDevice));
        HIP_CHECK(pol, hipMemset(text + size, 0, n_tiles * TILE + PAD - size));
        uint32_t *tile, *tbase, *stile, *sbase;
        unsigned long long* cnt;                         // [0] first bad byte, [1] error word, [2] max line, [3] stop line (u32)
        void* tmp;
        HIP_CHECK(pol, d_tile.get(&tile, (n_tiles + 1) * 4, "line index", pol));
        HIP_CHECK(pol, d_tbase.get(&tbase, (n_tiles + 1) * 4, "line index", pol));
        HIP_CHECK(pol, d_stile.get(&stile, (n_tiles + 1) * 4, "separators", pol));
        HIP_CHECK(pol, d_sbase.get(&sbase, (n_tiles + 1) * 4, "separators", pol));
        HIP_CHECK(pol, d_cnt.get(&cnt, 64, "counters", pol));
        HIP_CHECK(pol, hipMemset(cnt, 0xFF, 16));
        HIP_CHECK(pol, hipMemset(cnt + 2, 0, 8));
        HIP_CHECK(pol, hipMemset(cnt + 3, 0xFF, 8));
        HIP_CHECK(pol, d_scan.get(&tmp, std::max(scan_tmp_bytes_u32(n_tiles + 1), scan_tmp_bytes_u64(1)), "scan", pol));
        uint32_t n_nl = 0, n_sep32 = 0;
        HIP_CHECK(pol, line_count(text, size, tile, tbase, tmp, &n_nl));
        hipLaunchKernelGGL(seqdb_scan_bytes, dim3(grid(n_tiles, 1)), dim3(TPB), 0, 0, text, size, stile, cnt);
        HIP_CHECK(pol, hipGetLastError());
        HIP_CHECK(pol, hipMemset(stile + n_tiles, 0, 4));
        HIP_CHECK(pol, exclusive_scan_u32(stile, sbase, n_tiles + 1, tmp));
        HIP_CHECK(pol, hipMemcpy(&n_sep32, sbase + n_tiles, 4, hipMemcpyDeviceToHost));
        const bool tail = I.buf.p[size - 1] != '\n';     // only the last chunk of the listing may end without a newline
        const uint64_t n = (uint64_t)n_nl + (tail ? 1 : 0), n_sep = n_sep32;
        if (n >= NONE32 - 1) { set_error("seqdb: %s: 2^32 lines in one chunk are not supported", input.c_str()); return BLU_ERR_INVALID_ARG; }
        uint64_t *line, *sep;
        HIP_CHECK(pol, d_line.get(&line, (n + 2) * 8, "line index", pol));
        HIP_CHECK(pol, d_sep.get(&sep, (n_sep + 1) * 8, "separators", pol));
        HIP_CHECK(pol, line_write(text, size, tbase, line, n, tail));
        hipLaunchKernelGGL(seqdb_sep_write, dim3(grid(n_tiles, 1)), dim3(TPB), 0, 0, text, size, sbase, sep);
        HIP_CHECK(pol, hipGetLastError());

        LineOut lo;
        HIP_CHECK(pol, d_acc_a.get(&lo.acc_a, n * 8, "pieces", pol)); HIP_CHECK(pol, d_acc_n.get(&lo.acc_n, n * 4, "pieces", pol));
        HIP_CHECK(pol, d_tax_a.get(&lo.tax_a, n * 8, "pieces", pol)); HIP_CHECK(pol, d_tax_n.get(&lo.tax_n, n * 4, "pieces", pol));
        HIP_CHECK(pol, d_oid_a.get(&lo.oid_a, n * 8, "pieces", pol)); HIP_CHECK(pol, d_oid_n.get(&lo.oid_n, n * 4, "pieces", pol));
        HIP_CHECK(pol, d_seq_a.get(&lo.seq_a, n * 8, "pieces", pol)); HIP_CHECK(pol, d_seq_n.get(&lo.seq_n, n * 8, "pieces", pol));
        HIP_CHECK(pol, d_num.get(&lo.num, n * 8, "taxids", pol));
        unsigned long long *fna_off, *map_off;
        HIP_CHECK(pol, d_fna_len.get(&lo.fna_len, (n + 1) * 8, "lengths", pol)); HIP_CHECK(pol, d_fna_off.get(&fna_off, (n + 1) * 8, "lengths", pol));
        HIP_CHECK(pol, d_map_len.get(&lo.map_len, (n + 1) * 8, "lengths", pol)); HIP_CHECK(pol, d_map_off.get(&map_off, (n + 1) * 8, "lengths", pol));
        lo.err = cnt + 1; lo.max_line = cnt + 2; lo.stop_line = (uint32_t*)(cnt + 3);
        HIP_CHECK(pol, hipMemset(lo.fna_len + n, 0, 8));
        HIP_CHECK(pol, hipMemset(lo.map_len, 0, (n + 1) * 8));
        if (labels) {
            hipLaunchKernelGGL(seqdb_label_lines, dim3(grid(n)), dim3(TPB), 0, 0, text, line, (uint32_t)n, sep, n_sep, cnt, lab, lo);
            HIP_CHECK(pol, hipGetLastError());
            hipLaunchKernelGGL(seqdb_label_ascii, dim3(grid(n_tiles, 1)), dim3(TPB), 0, 0, text, size, line, (uint32_t)n, lo.seq_a, lo.seq_n,
                               lo.err);
        } else {
            hipLaunchKernelGGL(seqdb_lines, dim3(grid(n)), dim3(TPB), 0, 0, text, line, (uint32_t)n, sep, n_sep, qiime, cnt, lo);
        }
        HIP_CHECK(pol, hipGetLastError());
        HIP_CHECK(pol, d_scan.get(&tmp, std::max(scan_tmp_bytes_u32(n_tiles + 1), scan_tmp_bytes_u64(n + 1)), "scan", pol));
        HIP_CHECK(pol, exclusive_scan_u64(lo.fna_len, fna_off, n + 1, tmp));
        if (!qiime) HIP_CHECK(pol, exclusive_scan_u64(lo.map_len, map_off, n + 1, tmp));   // (labelled: the skip words)
        unsigned long long fna_total = 0, map_total = 0;
        HIP_CHECK(pol, hipMemcpy(&fna_total, fna_off + n, 8, hipMemcpyDeviceToHost));
        if (kraken) HIP_CHECK(pol, hipMemcpy(&map_total, map_off + n, 8, hipMemcpyDeviceToHost));
        const uint64_t fna_tiles = (fna_total + TILE - 1) / TILE;
        unsigned char *fna, *map = nullptr;
        HIP_CHECK(pol, d_fna.get(&fna, fna_tiles * TILE + PAD, "output", pol));
        if (fna_total) {                                  // (labelled: a chunk whose lines are all skipped writes nothing)
            const LineIn li{fna_off, lo.acc_a, lo.acc_n, lo.tax_a, lo.tax_n, lo.oid_a, lo.oid_n, lo.seq_a, lo.seq_n};
            if (labels)
                hipLaunchKernelGGL(seqdb_write_labelled, dim3((unsigned)fna_tiles), dim3(TPB), 0, 0, text, lab.blob, (uint32_t)n, li,
                                   lab.sintax, fna);
            else
                hipLaunchKernelGGL(seqdb_write_fna, dim3((unsigned)fna_tiles), dim3(TPB), 0, 0, text, (uint32_t)n, li, qiime, lo.err, fna);
            HIP_CHECK(pol, hipGetLastError());
        }
        if (kraken) {
            HIP_CHECK(pol, d_map.get(&map, map_total + PAD, "output", pol));
            hipLaunchKernelGGL(seqdb_write_map, dim3(grid(n)), dim3(TPB), 0, 0, text, (uint32_t)n, map_off, lo.map_len, lo.acc_a, lo.acc_n,
                               lo.num, map);
            HIP_CHECK(pol, hipGetLastError());
        }
        unsigned long long c[4];
        HIP_CHECK(pol, hipMemcpy(c, cnt, 32, hipMemcpyDeviceToHost));
        S.max_line_bytes = std::max<uint64_t>(S.max_line_bytes, c[2]);
        const uint64_t stop_line = (uint32_t)c[3], err_line = c[1] == ~0ull ? NONE32 : (c[1] >> 3);
        const uint64_t keep = std::min<uint64_t>({n, stop_line, err_line});   // records before the first stop or error
        unsigned long long keep_off[2] = {fna_total, map_total};
        uint64_t keep_in = size;
        if (keep < n) {
            HIP_CHECK(pol, hipMemcpy(&keep_off[0], fna_off + keep, 8, hipMemcpyDeviceToHost));
            if (kraken) HIP_CHECK(pol, hipMemcpy(&keep_off[1], map_off + keep, 8, hipMemcpyDeviceToHost));
            HIP_CHECK(pol, hipMemcpy(&keep_in, line + keep, 8, hipMemcpyDeviceToHost));
        }
        if (labels) {                                      // the skipped lines among those kept
            unsigned long long skipped = 0;
            HIP_CHECK(pol, hipMemcpy(&skipped, map_off + keep, 8, hipMemcpyDeviceToHost));
            n_unknown += skipped & 0xFFFFFFFFull;
            n_unlabelled += skipped >> 32;
        }
        if (!O.fna.grow(keep_off[0] + 1, 0) || !O.map.grow(keep_off[1] + 1, 0)) {
            set_error("seqdb: pinned host allocation of %llu bytes failed", keep_off[0] + keep_off[1]);
            return BLU_ERR_ALLOC;
        }
        if (keep_off[0]) HIP_CHECK(pol, hipMemcpy(O.fna.p, fna, keep_off[0], hipMemcpyDeviceToHost));
        if (keep_off[1]) HIP_CHECK(pol, hipMemcpy(O.map.p, map, keep_off[1], hipMemcpyDeviceToHost));
        O.fna_len = keep_off[0];
        O.map_len = keep_off[1];
        S.n_lines += keep;
        S.input_bytes += keep_in;
        S.fna_bytes += keep_off[0];
        S.map_bytes += keep_off[1];
        *done = keep < n;
        if (keep < n && stop_line <= err_line) {           // read_line returned Err: the loop ends quietly (rs:64)
            S.invalid_utf8_line = line_base + stop_line + 1;
        } else if (keep < n) {
            const uint32_t code = (uint32_t)(c[1] & 7);
            const char* why = code == E_PIECES ? (qiime ? "Invalid line detected on blastdbcmd response: fewer than four pieces separated by two spaces"
                                                        : "Invalid line detected on blastdbcmd response: fewer than three pieces separated by two spaces")
                            : code == E_TAXID ? "the taxid is not an unsigned integer (usize)"
                                              : "the sequence holds a byte >= 0x80 (not an IUPAC letter)";
            set_error("seqdb: %s: line %llu: %s", input.c_str(), (unsigned long long)(line_base + err_line + 1), why);
            return BLU_ERR_PARSE;
        }
        return BLU_OK;
    }

    int run() {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0) { (void)hipGetLastError(); set_error("seqdb: no HIP device"); return BLU_ERR_NO_DEVICE; }
        if (D.device < 0 || D.device >= n_dev) { set_error("seqdb: device %d does not exist (%d devices)", D.device, n_dev); return BLU_ERR_INVALID_ARG; }
        HIP_CHECK(pol, hipSetDevice(D.device));
        if (labels) { if (const int rc = upload_labels(); rc != BLU_OK) return rc; }
        chunk = D.chunk_bytes ? (size_t)D.chunk_bytes : (size_t)BLU_SEQDB_DEFAULT_CHUNK;
        chunk = std::max<size_t>(chunk, 4096);
        input = D.input_path ? D.input_path : ("fd " + std::to_string(D.input_fd));
        int own_fd = -1;
        if (D.input_fd >= 0) in_fd = D.input_fd;
        else {
            own_fd = in_fd = open(D.input_path, O_RDONLY | O_CLOEXEC);
            if (in_fd < 0) { set_error("seqdb: cannot open %s: %s", D.input_path, strerror(errno)); return BLU_ERR_IO; }
        }
        struct Closer { int* fd; ~Closer() { if (*fd >= 0) close(*fd); } } c_in{&own_fd}, c_fna{&fna_fd}, c_map{&map_fd};
        fna_fd = open(D.fna_path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
        if (fna_fd < 0) { set_error("seqdb: cannot create %s: %s", D.fna_path, strerror(errno)); return BLU_ERR_IO; }
        if (D.format == BLU_SEQDB_KRAKEN2) {             // written beside, renamed once the whole listing is through (mod.rs:43-50)
            map_tmp = std::string(D.map_path) + ".partial";
            map_fd = open(map_tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
            if (map_fd < 0) { set_error("seqdb: cannot create %s: %s", map_tmp.c_str(), strerror(errno)); return BLU_ERR_IO; }
        }
        in_free.push(0); in_free.push(1);
        out_free.push(0); out_free.push(1);
        std::thread rd([this] { reader(); });
        std::thread wr([this] { writer(); });
        int rc = BLU_OK;
        uint64_t line_base = 0;
        for (;;) {
            const int s = in_full.pop();
            if (s < 0) break;
            const int o = out_free.pop();
            const double t0 = now_s();
            bool done = false;
            const uint64_t lines_before = S.n_lines;
            rc = chunk_on_device(in[s], out[o], line_base, &done);
            S.t_gpu_ms += 1e3 * (now_s() - t0);
            line_base += S.n_lines - lines_before;
            in_free.push(s);
            // a line the export refuses (BLU_ERR_PARSE with *done set) leaves the records before it in the slot: they are
            // written like any other chunk's, so that the .fna does not depend on where the chunks were cut
            if (rc == BLU_OK || (rc == BLU_ERR_PARSE && done)) out_full.push(o);
            else out_free.push(o);
            if (rc != BLU_OK || done || stop.load()) break;
        }
        stop = true;
        in_free.push(-1);
        rd.join();
        out_full.push(-1);
        wr.join();
        S.t_read_ms = t_read;
        S.t_write_ms = t_write;
        if (rc == BLU_OK && !write_err.empty()) { set_error("seqdb: writing the output failed: %s", write_err.c_str()); rc = BLU_ERR_IO; }
        if (rc == BLU_OK && !read_err.empty()) { set_error("seqdb: reading %s failed: %s", input.c_str(), read_err.c_str()); rc = BLU_ERR_IO; }
        if (map_fd >= 0) {
            close(map_fd);
            map_fd = -1;
            if (rc == BLU_OK && rename(map_tmp.c_str(), D.map_path) != 0) {
                set_error("seqdb: cannot create %s: %s", D.map_path, strerror(errno));
                rc = BLU_ERR_IO;
            }
            if (rc != BLU_OK) unlink(map_tmp.c_str());      // the reference panics before prelim_map.txt is written
        }
        return rc;
    }
};

}  // namespace
}  // namespace blu

extern "C" int blu_seqdb_export(const blu_seqdb_desc* desc, blu_seqdb_stats* stats) {
    if (!desc || !desc->fna_path || (desc->input_fd < 0 && !desc->input_path) ||
        (desc->format != BLU_SEQDB_KRAKEN2 && desc->format != BLU_SEQDB_QIIME2) || (desc->format == BLU_SEQDB_KRAKEN2 && !desc->map_path)) {
        blu::set_error("blu_seqdb_export: null or invalid argument");
        return BLU_ERR_INVALID_ARG;
    }
    blu_seqdb_stats local;
    blu_seqdb_stats& S = stats ? *stats : local;
    memset(&S, 0, sizeof S);
    const double t0 = blu::now_s();
    blu::Export e(*desc, S);
    const int rc = e.run();
    S.t_wall_ms = 1e3 * (blu::now_s() - t0);
    return rc;
}

extern "C" int blu_seqdb_export_labelled(const blu_seqdb_label_desc* desc, blu_seqdb_label_stats* stats) {
    if (!desc || !desc->fna_path || !desc->taxonomies_file || (desc->input_fd < 0 && !desc->input_path) ||
        (desc->format != BLU_SEQDB_SINTAX && desc->format != BLU_SEQDB_DADA2)) {
        blu::set_error("blu_seqdb_export_labelled: null or invalid argument");
        return BLU_ERR_INVALID_ARG;
    }
    blu_seqdb_label_stats local;
    blu_seqdb_label_stats& T = stats ? *stats : local;
    memset(&T, 0, sizeof T);
    const double t0 = blu::now_s();
    blu::LabelSet labels;
    if (const int rc = blu::load_label_set(desc->taxonomies_file, desc->use_taxid != 0, desc->format, labels); rc != BLU_OK) return rc;
    T.n_rows = labels.taxid.size();
    T.label_bytes = labels.blob.size();
    T.t_labels_ms = 1e3 * (blu::now_s() - t0);
    blu_seqdb_desc d{};
    d.format = desc->format;
    d.input_fd = desc->input_fd;
    d.input_path = desc->input_path;
    d.fna_path = desc->fna_path;
    d.chunk_bytes = desc->chunk_bytes;
    d.device = desc->device;
    blu_seqdb_stats S;
    memset(&S, 0, sizeof S);
    blu::Export e(d, S);
    e.labels = &labels;
    const int rc = e.run();
    T.n_lines = S.n_lines; T.input_bytes = S.input_bytes; T.fna_bytes = S.fna_bytes; T.n_chunks = S.n_chunks;
    T.max_line_bytes = S.max_line_bytes; T.invalid_utf8_line = S.invalid_utf8_line;
    T.n_unknown_taxid = e.n_unknown; T.n_unlabelled = e.n_unlabelled;
    T.t_read_ms = S.t_read_ms; T.t_gpu_ms = S.t_gpu_ms; T.t_write_ms = S.t_write_ms;
    T.t_labels_ms += e.t_label_upload;
    T.t_wall_ms = 1e3 * (blu::now_s() - t0);
    return rc;
}
