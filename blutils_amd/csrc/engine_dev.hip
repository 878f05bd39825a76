// The engine on the columns the GPU ingest left on the device (ingest.h: device_run_consensus): taxonomy rows -> engine row ids,
// the packed side records or the columns, one blu_consensus_run with device pointers, and the top-score rows of the rendered
// queries compacted for the writer.  DeviceHits, the owner of those columns, is freed here too.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "blu_consensus.h"
#include "ingest.h"
#include "ingest_prims.h"

namespace blu {

namespace {
constexpr uint32_t ROW_NO_TAXID = BLU_UNMATCHED_TAXID;
__device__ __forceinline__ uint32_t engine_row_of(uint32_t r, const uint32_t* __restrict__ fwd, uint64_t n_tax) {
    return (r == ROW_NO_TAXID || r >= n_tax) ? ROW_NO_TAXID : fwd[r];
}
// k = round(p * 1000) is used only if fl(k / 1000.0) == p bit for bit for every row (the 20 B/hit layout is lossless then)
__device__ __forceinline__ bool milli_of(double p, uint32_t* k_out) {
    bool ok = p >= 0.0 && p < 4.0e6;
    uint32_t k = 0;
    if (ok) {
        k = (uint32_t)(p * 1000.0 + 0.5);
        const double back = (double)k / 1000.0;
        ok = __double_as_longlong(back) == __double_as_longlong(p);
    }
    *k_out = k;
    return ok;
}
// 16-byte side records of the packed layout (include/blu_consensus.h: blu_hits.packed) straight from the ingest's columns
// (what blu_hits_pack builds from engine row ids, pack_kernel.hip, here straight from the taxonomy rows of the join: word 1 =
// milli-percent perc_identity | shape hint of the row << 17)
__global__ void pack_side_records(const uint32_t* __restrict__ desc_row, const double* __restrict__ pid, const int32_t* __restrict__ aln,
                                  const uint32_t* __restrict__ acc, uint64_t n, const uint32_t* __restrict__ fwd, uint64_t n_tax,
                                  const uint16_t* __restrict__ hint_of_pos, uint4* __restrict__ rec, uint32_t* __restrict__ inexact) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k;
    if (!milli_of(pid[i], &k) || k >= BLU_PACKED_PIDENT_LIMIT) *inexact = 1u;
    const uint32_t row = engine_row_of(desc_row[i], fwd, n_tax);
    const uint32_t pos = row & ((1u << BLU_ROW_BITS) - 1u);
    const uint32_t hint = (row != ROW_NO_TAXID && pos < n_tax) ? (uint32_t)hint_of_pos[pos] : 0u;
    rec[i] = make_uint4(row, (k & BLU_KTHR_NEVER) | (hint << BLU_KTHR_BITS), (uint32_t)aln[i], acc[i]);
}
__global__ void to_engine_rows(const uint32_t* __restrict__ desc_row, uint64_t n, const uint32_t* __restrict__ fwd, uint64_t n_tax,
                               uint32_t* __restrict__ rows) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) rows[i] = engine_row_of(desc_row[i], fwd, n_tax);
}
__global__ void to_milli(const double* __restrict__ pid, uint64_t n, uint32_t* __restrict__ milli, uint32_t* __restrict__ inexact) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t k;
    if (!milli_of(pid[i], &k)) *inexact = 1u;
    milli[i] = k;
}

// Top-score rows of the rendered queries (status 0 / 1), one wave per TOP_QPW consecutive queries: the lanes sweep a
// segment 64 rows at a time.  Pass 1 counts (out_rows == nullptr), pass 2 writes the rows at the scanned offsets.
constexpr uint32_t TOP_QPW = 8;
__global__ __launch_bounds__(256) void top_rows_kernel(const blu_result* __restrict__ recs, const unsigned long long* __restrict__ seg_off,
                                                       const int32_t* __restrict__ bitscore, uint64_t n_queries,
                                                       unsigned long long* __restrict__ count, const unsigned long long* __restrict__ off,
                                                       const uint32_t* __restrict__ desc_row, const uint32_t* __restrict__ acc,
                                                       const int32_t* __restrict__ aln, const double* __restrict__ pid,
                                                       TopRow* __restrict__ out_rows, int32_t* __restrict__ out_score) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    for (uint32_t k = 0; k < TOP_QPW; ++k) {
        const uint64_t q = wave * TOP_QPW + k;
        if (q >= n_queries) return;
        const blu_result r = recs[q];
        unsigned long long n_top = 0;
        if (r.status < 2 && r.ref_row != 0xFFFFFFFFu) {
            const int32_t top = bitscore[r.ref_row];
            const unsigned long long b = seg_off[q], e = seg_off[q + 1];
            const unsigned long long base = out_rows ? off[q] : 0;
            for (unsigned long long i0 = b; i0 < e; i0 += 64) {
                const unsigned long long i = i0 + lane;
                const bool hit = i < e && bitscore[i] == top;
                const unsigned long long m = __ballot(hit);
                if (out_rows && hit) {
                    const unsigned long long at = base + n_top + __popcll(m & ((1ull << lane) - 1));
                    TopRow t;
                    t.row = (uint32_t)i; t.desc_row = desc_row[i]; t.acc_rank = acc[i]; t.align_len = aln[i]; t.pident = pid[i];
                    out_rows[at] = t;
                }
                n_top += __popcll(m);
            }
            if (out_score && lane == 0) out_score[q] = top;
        } else if (out_score && lane == 0) out_score[q] = 0;
        if (!out_rows && lane == 0) count[q] = n_top;
    }
}
}  // namespace

DeviceHits::~DeviceHits() {
    if (device < 0) return;
    (void)hipSetDevice(device);
    for (void* p : {(void*)bitscore, (void*)align_len, (void*)tax_desc_row, (void*)acc_rank, (void*)pident, seg_block})
        if (p) (void)hipFree(p);
    for (void* p : trash) (void)hipFree(p);
}

int device_run_consensus(const blu_taxonomy* tax, DeviceHits& dev, const uint32_t* fwd, uint64_t n_tax, int strategy, blu_result* out,
                         TopTable* top, DeviceRecords* kept) {
    uint32_t *d_fwd = nullptr, *d_milli = nullptr, *d_rows = nullptr, *d_flag = nullptr;
    uint4* d_rec = nullptr;
    blu_result* d_out = nullptr;
    unsigned long long* d_cnt = nullptr;   // [2 (Q + 1)]: counts, then their exclusive scan
    void* d_tmp = nullptr;
    TopRow* d_top = nullptr;
    int32_t* d_score = nullptr;
    uint32_t inexact = 0;
    const uint64_t n = dev.n_hits, nq = dev.n_queries;
    if (hipSetDevice(dev.device) != hipSuccess) { set_error("hipSetDevice(%d) failed", dev.device); return BLU_ERR_NO_DEVICE; }
    HipPolicy pol{"GPU ingest", BLU_ERR_HIP};
    DeviceArena mem(pol);
    // the work buffers are freed with the columns (DeviceHits::trash), whichever way this is left: ten hipFree calls were
    // 10-15 ms of this function
    struct ToTrash { DeviceArena& mem; DeviceHits& dev; ~ToTrash() { mem.hand_over(dev.trash); } } to_trash{mem, dev};
    HIP_CHECK(pol, mem.alloc(&d_fwd, n_tax * 4, "row map"));
    HIP_CHECK(pol, hipMemcpy(d_fwd, fwd, n_tax * 4, hipMemcpyHostToDevice));
    HIP_CHECK(pol, mem.alloc(&d_flag, 4, "flag"));
    HIP_CHECK(pol, hipMemset(d_flag, 0, 4));
    HIP_CHECK(pol, mem.alloc(&d_out, nq * sizeof(blu_result), "records"));
    {
        blu_hits h{};
        h.bitscore = dev.bitscore;
        h.seg_off = (const uint64_t*)dev.seg_off;
        // packed layout: a top row's four values in one memory line (if the records do not fit, or a perc_identity is not
        // exactly k/1000, the columns go in)
        bool packed = n && mem.alloc(&d_rec, n * 16, "packed records") == hipSuccess;
        if (!packed) (void)hipGetLastError();
        if (packed) {
            hipLaunchKernelGGL(pack_side_records, grid(n), dim3(256), 0, 0, dev.tax_desc_row, dev.pident, dev.align_len, dev.acc_rank, n,
                               d_fwd, n_tax, tax->d_hint_of_pos, d_rec, d_flag);
            HIP_CHECK(pol, hipMemcpy(&inexact, d_flag, 4, hipMemcpyDeviceToHost));
            if (inexact) { mem.free(d_rec); d_rec = nullptr; packed = false; }
        }
        if (packed) h.packed = (const uint32_t*)d_rec;
        else {
            HIP_CHECK(pol, mem.alloc(&d_rows, n * 4, "engine rows"));
            if (n) hipLaunchKernelGGL(to_engine_rows, grid(n), dim3(256), 0, 0, dev.tax_desc_row, n, d_fwd, n_tax, d_rows);
            h.tax_row = d_rows; h.align_len = dev.align_len; h.acc_rank = dev.acc_rank;
            if (!inexact && n) {   // the records did not fit: milli-percent column
                HIP_CHECK(pol, mem.alloc(&d_milli, n * 4, "milli-percent column"));
                hipLaunchKernelGGL(to_milli, grid(n), dim3(256), 0, 0, dev.pident, n, d_milli, d_flag);
                HIP_CHECK(pol, hipMemcpy(&inexact, d_flag, 4, hipMemcpyDeviceToHost));
            }
            if (inexact || !n) h.pident = dev.pident; else h.pident_milli = d_milli;
        }
        h.n_hits = n; h.n_queries = nq; h.on_device = 1;
        blu_run_params rp{strategy, 0, nullptr};
        const int rc = blu_consensus_run(tax, &h, &rp, d_out);
        if (rc != BLU_OK) return rc;
        if (kept) { kept->recs = d_out; kept->rows = packed ? (const uint32_t*)d_rec : d_rows; kept->row_stride = packed ? 4u : 1u; }
    }
    HIP_CHECK(pol, hipStreamSynchronize(nullptr));
    {
        std::vector<D2HPiece> pieces;
        d2h_add(pieces, out, d_out, nq * sizeof(blu_result));
        HIP_CHECK(pol, d2h_parallel(pieces, dev.device));
    }
    if (top) {
        const uint64_t waves = (nq + TOP_QPW - 1) / TOP_QPW;
        const dim3 g((unsigned)((waves * 64 + 255) / 256));
        HIP_CHECK(pol, mem.alloc(&d_cnt, (nq + 1) * 8 * 2, "top-row counts"));
        HIP_CHECK(pol, hipMemset(d_cnt, 0, (nq + 1) * 8 * 2));
        HIP_CHECK(pol, mem.alloc(&d_score, nq * 4, "top scores"));
        if (nq) hipLaunchKernelGGL(top_rows_kernel, g, dim3(256), 0, 0, d_out, dev.seg_off, dev.bitscore, nq, d_cnt, nullptr, nullptr, nullptr,
                                   nullptr, nullptr, nullptr, nullptr);
        HIP_CHECK(pol, mem.alloc(&d_tmp, scan_tmp_bytes_u64((size_t)nq + 1), "scan scratch"));
        HIP_CHECK(pol, exclusive_scan_u64(d_cnt, d_cnt + nq + 1, (size_t)nq + 1, d_tmp));
        top->off.resize(nq + 1);
        HIP_CHECK(pol, hipMemcpy(top->off.data(), d_cnt + nq + 1, (nq + 1) * 8, hipMemcpyDeviceToHost));
        const uint64_t n_top = top->off[nq];
        HIP_CHECK(pol, mem.alloc(&d_top, n_top * sizeof(TopRow), "top rows"));
        if (nq) hipLaunchKernelGGL(top_rows_kernel, g, dim3(256), 0, 0, d_out, dev.seg_off, dev.bitscore, nq, nullptr, d_cnt + nq + 1,
                                   dev.tax_desc_row, dev.acc_rank, dev.align_len, dev.pident, d_top, d_score);
        top->rows.resize(n_top);
        top->score.resize(nq);
        HIP_CHECK(pol, hipStreamSynchronize(nullptr));
        std::vector<D2HPiece> pieces;
        d2h_add(pieces, top->rows.data(), d_top, n_top * sizeof(TopRow));
        d2h_add(pieces, top->score.data(), d_score, nq * 4);
        HIP_CHECK(pol, d2h_parallel(pieces, dev.device));
    }
    return BLU_OK;
}
void load_engine_dev() {
    hipFuncAttributes attr;
    (void)hipFuncGetAttributes(&attr, (const void*)top_rows_kernel);
}

}  // namespace blu
