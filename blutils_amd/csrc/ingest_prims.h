// Pieces of the GPU ingest (ingest_gpu.hip) that the taxonomies-database builder (taxdb_gpu.hip) reuses.  They are host
// wrappers around the ingest's own kernels, which stay compiled once, in ingest_gpu.hip.
#ifndef BLU_INGEST_PRIMS_H
#define BLU_INGEST_PRIMS_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace blu {

// ---- line index of a device text d_text[0, size), padded with >= 64 zero bytes (16-byte loads)
// tiles of the newline count
uint64_t line_tiles(uint64_t size);
// d_tile[k] = newlines in tile k (n = line_tiles(size) entries)
hipError_t line_count_tiles(const unsigned char* d_text, uint64_t size, uint32_t* d_tile);
// d_line[k + 1] = offset after newline k, from the exclusive scan of the tile counts; d_line[0] is the caller's
hipError_t line_write_starts(const unsigned char* d_text, uint64_t size, const uint32_t* d_tile_base, uint64_t* d_line);

// ---- device-wide exclusive prefix sums: out[i] = in[0] + ... + in[i - 1] (wrapping); tmp = scan_tmp_bytes_*(n) bytes.
// in == out is allowed (every element is read and written by the same thread, after the block sums are taken)
size_t scan_tmp_bytes_u32(size_t n);
size_t scan_tmp_bytes_u64(size_t n);
hipError_t exclusive_scan_u32(const uint32_t* in, uint32_t* out, size_t n, void* tmp);
hipError_t exclusive_scan_u64(const unsigned long long* in, unsigned long long* out, size_t n, void* tmp);

// ---- stable LSD radix sort of (key, value) pairs, 8 bits per pass, ceil(bits / 8) passes: the pairs end ordered by the low
// 8 * ceil(bits / 8) bits of the key (equal keys in input order), which is the whole key for the keys < 2^bits the callers
// must pass.  bits = 0: no pass.  The sorted pairs are (*keys, *vals) on return (the alternate buffers after an odd number
// of passes).  table: radix_table_words(n) words; scan_tmp: radix_scan_tmp_bytes(n) bytes
size_t radix_table_words(uint32_t n);
size_t radix_scan_tmp_bytes(uint32_t n);
hipError_t radix_sort_pairs(uint32_t** keys, uint32_t** keys_alt, uint32_t** vals, uint32_t** vals_alt, uint32_t n, int bits,
                            uint32_t* table, void* scan_tmp);

// ---- file -> HBM through pinned staging (pread, never mapped); BLU_OK, BLU_ERR_IO, or BLU_INGEST_FALLBACK (HIP staging)
int upload_file(int fd, size_t size, unsigned char* d_text, int device, std::string* err);

// ---- device -> pageable host memory by a pool of host threads
struct D2HPiece { char* dst; const char* src; size_t bytes; };
void d2h_add(std::vector<D2HPiece>& v, void* dst, const void* src, size_t bytes, size_t piece = 8u << 20);
hipError_t d2h_parallel(const std::vector<D2HPiece>& pieces, int device, unsigned max_threads = 16);

}  // namespace blu
#endif
