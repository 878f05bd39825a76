// The kernels and host code the per-query passes share (hit_pass.h, blu_internal.h): the list of a pass's long queries, the
// compaction of the five columns by a pass's keep words, the staging of host columns, and the refusals of their entry points.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "hit_pass.h"
#include "ingest.h"

namespace blu {
namespace {

constexpr uint32_t MARKER_BLOCK = 256;

// list_q[j] = the j-th long query and, with row_start, list_start[j] = its start among the long rows
__global__ void long_list_kernel(const uint32_t* __restrict__ long_flag, const uint32_t* __restrict__ flag_pos,
                                 const uint32_t* __restrict__ row_start, uint64_t n_queries, uint32_t n_long,
                                 uint32_t* __restrict__ list_q, uint32_t* __restrict__ list_start) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_queries || !long_flag[q]) return;
    const uint32_t j = flag_pos[q];
    if (j >= n_long) return;
    list_q[j] = (uint32_t)q;
    if (row_start) list_start[j] = row_start[q];
}

// seg_off[q] -> the kept rows before it: scan[min(seg_off[q], n_hits)], the total as the last entry
__global__ void kept_offsets_kernel(unsigned long long* __restrict__ seg_off, uint64_t n_queries, const uint32_t* __restrict__ scan,
                                    uint64_t n_hits) {
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q > n_queries) return;
    const unsigned long long o = seg_off[q];
    seg_off[q] = scan[q == n_queries || o > n_hits ? n_hits : o];
}

__global__ __launch_bounds__(MARKER_BLOCK) void count_marker_kernel(const uint32_t* __restrict__ tax, uint64_t n, uint32_t marker,
                                                                     unsigned long long* __restrict__ count) {
    const uint64_t i = (uint64_t)blockIdx.x * MARKER_BLOCK + threadIdx.x;
    spread_add_ballot(count, 0, i < n && tax[i] == marker);
}

}  // namespace

int long_query_list(HipPolicy& pol, DeviceArena& mem, uint32_t* d_flag, uint64_t n_queries, uint64_t n_long, const uint32_t* d_row_start,
                    void* d_tmp, uint32_t** d_list_q, uint32_t** d_list_start) {
    uint32_t *d_fpos = nullptr, *d_starts = nullptr;
    HIP_CHECK(pol, mem.alloc(&d_fpos, (n_queries + 1) * 4, "long positions"));
    HIP_CHECK(pol, mem.alloc(d_list_q, n_long * 4, "long queries"));
    if (d_row_start) { HIP_CHECK(pol, mem.alloc(&d_starts, (n_long + 1) * 4, "long starts")); *d_list_start = d_starts; }
    HIP_CHECK(pol, hipMemsetAsync(d_flag + n_queries, 0, 4, nullptr));
    HIP_CHECK(pol, exclusive_scan_u32(d_flag, d_fpos, n_queries + 1, d_tmp));
    hipLaunchKernelGGL(long_list_kernel, grid(n_queries), dim3(256), 0, nullptr, (const uint32_t*)d_flag, (const uint32_t*)d_fpos, d_row_start,
                       n_queries, (uint32_t)n_long, *d_list_q, d_starts);
    HIP_CHECK(pol, hipGetLastError());
    return BLU_OK;
}

HitColumns columns_of(DeviceHits& dev) { return HitColumns{&dev.bitscore, &dev.align_len, &dev.tax_desc_row, &dev.acc_rank, &dev.pident, dev.seg_off}; }

int check_hit_counts(const char* what, uint64_t n_hits, uint64_t n_queries) {
    if (n_hits >= (1ull << 32)) { set_error("%s: n_hits must be below 2^32", what); return BLU_ERR_INVALID_ARG; }
    if (n_queries >= (1ull << 32)) { set_error("%s: n_queries must be below 2^32", what); return BLU_ERR_INVALID_ARG; }
    return BLU_OK;
}

int use_device(const char* who, int device) {
    if (hipSetDevice(device) == hipSuccess) return BLU_OK;
    (void)hipGetLastError();
    set_error("%s: hipSetDevice(%d) failed", who, device);
    return BLU_ERR_NO_DEVICE;
}

int refuse_null_array(const char* who) { set_error("%s: null array with a non-zero count", who); return BLU_ERR_INVALID_ARG; }

int check_aligned16(const char* who, const HitColumns& c) {
    if ((((uintptr_t)*c.bitscore | (uintptr_t)*c.align_len | (uintptr_t)*c.tax_desc_row | (uintptr_t)*c.acc_rank | (uintptr_t)*c.pident) & 15u) == 0) return BLU_OK;
    set_error("%s: device columns must be 16-byte aligned", who);
    return BLU_ERR_INVALID_ARG;
}

int compact_kept_device(const char* who, HitColumns& c, uint64_t n_hits, uint64_t n_queries, const uint32_t* d_keep, bool all_kept, bool rotate,
                        uint32_t unmatched_marker, uint64_t* n_hits_out, uint64_t* n_unmatched, std::vector<void*>* retired) {
    HipPolicy pol{who, BLU_ERR_ALLOC};
    DeviceArena mem(pol);
    *n_hits_out = n_hits;
    uint32_t* d_pos = nullptr;
    unsigned long long* d_cnt = nullptr;
    HIP_CHECK(pol, mem.alloc(&d_cnt, HIT_SPREAD * 8, "unmatched count"));
    auto count_unmatched = [&](uint64_t n) -> int {
        if (!n_unmatched) return BLU_OK;
        unsigned long long cnt[HIT_SPREAD];
        HIP_CHECK(pol, hipMemsetAsync(d_cnt, 0, sizeof cnt, nullptr));
        if (n) hipLaunchKernelGGL(count_marker_kernel, grid(n, MARKER_BLOCK), dim3(MARKER_BLOCK), 0, nullptr, (const uint32_t*)*c.tax_desc_row, n, unmatched_marker, d_cnt);
        HIP_CHECK(pol, hipGetLastError());
        HIP_CHECK(pol, hipMemcpy(cnt, d_cnt, sizeof cnt, hipMemcpyDeviceToHost));
        *n_unmatched = spread_sum(cnt, 0);
        return BLU_OK;
    };
    if (n_hits == 0 || all_kept) return count_unmatched(n_hits);   // every row kept: the columns are not touched
    void* d_tmp = nullptr;
    HIP_CHECK(pol, mem.alloc(&d_pos, (n_hits + 1) * 4, "keep positions"));
    HIP_CHECK(pol, mem.alloc(&d_tmp, scan_tmp_bytes_u32(n_hits + 1), "scan work"));
    HIP_CHECK(pol, exclusive_scan_u32(d_keep, d_pos, n_hits + 1, d_tmp));
    uint32_t n_out = 0;
    HIP_CHECK(pol, hipMemcpy(&n_out, d_pos + n_hits, 4, hipMemcpyDeviceToHost));
    mem.free(d_tmp);
    Compaction cp{d_keep, d_pos, (uint32_t)n_hits, n_out, nullptr};
    HIP_CHECK(pol, mem.alloc(&cp.spare, std::max<size_t>((size_t)n_out, 1) * 8, "compaction spare"));
    if (rotate) mem.release(cp.spare);               // (from here the spare is one of the caller's buffers or goes to `retired`)
    const hipError_t e = rotate ? cp.rotate(*c.pident, *c.bitscore, *c.align_len, *c.tax_desc_row, *c.acc_rank)
                                : cp.copy_back(*c.pident, *c.bitscore, *c.align_len, *c.tax_desc_row, *c.acc_rank);
    if (rotate) { if (retired) retired->push_back(cp.spare); else (void)hipFree(cp.spare); }
    HIP_CHECK(pol, e);
    hipLaunchKernelGGL(kept_offsets_kernel, grid(n_queries + 1), dim3(256), 0, nullptr, c.seg_off, n_queries, (const uint32_t*)d_pos, n_hits);
    HIP_CHECK(pol, hipGetLastError());
    *n_hits_out = n_out;
    if (const int rc = count_unmatched(n_out)) return rc;
    HIP_CHECK(pol, hipStreamSynchronize(nullptr));
    return BLU_OK;
}

int with_staged_columns(HipPolicy& pol, const HitColumns& host, uint64_t n_hits, uint64_t n_queries, const uint32_t* row_map, uint64_t n_map,
                        uint64_t* n_out, const StagedPass& pass) {
    DeviceArena mem(pol);
    int32_t *d_bs = nullptr, *d_aln = nullptr;
    uint32_t *d_tax = nullptr, *d_acc = nullptr, *d_map = nullptr;
    double* d_pid = nullptr;
    unsigned long long* d_seg = nullptr;
    const uint64_t n_off = n_queries ? n_queries + 1 : 0;
    HIP_CHECK(pol, mem.upload(&d_bs, *host.bitscore, n_hits, "bit-scores"));
    HIP_CHECK(pol, mem.upload(&d_aln, *host.align_len, n_hits, "alignment lengths"));
    HIP_CHECK(pol, mem.upload(&d_tax, *host.tax_desc_row, n_hits, "taxonomy rows"));
    HIP_CHECK(pol, mem.upload(&d_acc, *host.acc_rank, n_hits, "accession ranks"));
    HIP_CHECK(pol, mem.upload(&d_pid, *host.pident, n_hits, "identities"));
    HIP_CHECK(pol, mem.upload(&d_seg, host.seg_off, n_off, "offsets"));
    if (row_map) HIP_CHECK(pol, mem.upload(&d_map, row_map, n_map, "row map"));
    HitColumns c{&d_bs, &d_aln, &d_tax, &d_acc, &d_pid, d_seg};
    *n_out = n_hits;
    if (const int rc = pass(c, d_map, n_out)) return rc;
    if (*n_out >= n_hits) return BLU_OK;
    HIP_CHECK(pol, mem.download(*host.bitscore, d_bs, *n_out));
    HIP_CHECK(pol, mem.download(*host.align_len, d_aln, *n_out));
    HIP_CHECK(pol, mem.download(*host.tax_desc_row, d_tax, *n_out));
    HIP_CHECK(pol, mem.download(*host.acc_rank, d_acc, *n_out));
    HIP_CHECK(pol, mem.download(*host.pident, d_pid, *n_out));
    HIP_CHECK(pol, mem.download(host.seg_off, d_seg, n_off));
    return BLU_OK;
}

}  // namespace blu
