// Measurement aid (not product code; the library has no CPU path for this pass): the pair integers of
// blu_sample_distances on one host thread, for scripts/distance_bench.py to time beside the device.
//   distance_host_merge  the same order of work as the device kernel: the CSR transposed by sample, then for every pair
//                        a <= b a merge of the two sorted feature lists
//   distance_host_rows   by feature: every pair of a row's non-zeros adds into the S x S matrices (the order of work a
//                        sparse table allows: F (dS)^2 instead of F dS S)
#include <cstdint>
#include <vector>

extern "C" {

void distance_host_merge(uint64_t n_features, uint32_t n_samples, const uint64_t* row_ptr, const uint32_t* sample, const uint64_t* count,
                         uint64_t* min_sum, uint32_t* shared) {
    const uint32_t S = n_samples;
    const uint64_t nnz = row_ptr[n_features];
    std::vector<uint64_t> col(S + 1, 0), at(S), cnt(nnz);
    std::vector<uint32_t> feat(nnz);
    for (uint64_t e = 0; e < nnz; ++e) ++col[sample[e] + 1];
    for (uint32_t s = 0; s < S; ++s) col[s + 1] += col[s];
    for (uint32_t s = 0; s < S; ++s) at[s] = col[s];
    for (uint64_t f = 0; f < n_features; ++f)
        for (uint64_t e = row_ptr[f]; e < row_ptr[f + 1]; ++e) { const uint64_t k = at[sample[e]]++; feat[k] = (uint32_t)f; cnt[k] = count[e]; }
    for (uint32_t a = 0; a < S; ++a) {
        for (uint32_t b = a; b < S; ++b) {
            uint64_t i = col[a], j = col[b], m = 0;
            const uint64_t ie = col[a + 1], je = col[b + 1];
            uint32_t n = 0;
            while (i < ie && j < je) {
                const uint32_t fa = feat[i], fb = feat[j];
                if (fa == fb) { m += cnt[i] < cnt[j] ? cnt[i] : cnt[j]; ++n; ++i; ++j; }
                else if (fa < fb) ++i;
                else ++j;
            }
            min_sum[(uint64_t)a * S + b] = min_sum[(uint64_t)b * S + a] = m;
            shared[(uint64_t)a * S + b] = shared[(uint64_t)b * S + a] = n;
        }
    }
}

void distance_host_rows(uint64_t n_features, uint32_t n_samples, const uint64_t* row_ptr, const uint32_t* sample, const uint64_t* count,
                        uint64_t* min_sum, uint32_t* shared) {
    const uint64_t S = n_samples;
    for (uint64_t k = 0; k < S * S; ++k) { min_sum[k] = 0; shared[k] = 0; }
    for (uint64_t f = 0; f < n_features; ++f) {
        const uint64_t e0 = row_ptr[f], e1 = row_ptr[f + 1];
        for (uint64_t i = e0; i < e1; ++i) {
            const uint64_t x = count[i];
            uint64_t* mrow = min_sum + sample[i] * S;
            uint32_t* srow = shared + sample[i] * S;
            for (uint64_t j = e0; j < e1; ++j) { mrow[sample[j]] += x < count[j] ? x : count[j]; ++srow[sample[j]]; }
        }
    }
}

}  // extern "C"
