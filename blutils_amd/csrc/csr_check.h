// What the library refuses about a feature x sample CSR given in host arrays (include/blu_consensus.h: blu_distance_desc and
// blu_rarefy_desc carry the same one), decided on the host before any device is asked for.  Host code only.
#ifndef BLU_CSR_CHECK_H
#define BLU_CSR_CHECK_H

#include <cstdint>
#include <vector>

#include "blu_internal.h"

namespace blu {

// BLU_OK, or BLU_ERR_INVALID_ARG with a message that starts with `who`; total[s] = the sum of sample s's counts (each below 2^63)
inline int check_csr(const char* who, uint64_t n_features, uint32_t n_samples, const uint64_t* row_ptr, const uint32_t* sample,
                     const uint64_t* count, uint64_t* nnz_out, std::vector<uint64_t>& total) {
    using ull = unsigned long long;
    const auto refuse = [&](const char* fmt, ull a, ull b = 0) { set_error(fmt, who, a, b); return (int)BLU_ERR_INVALID_ARG; };
    if (n_samples == 0 || n_samples > BLU_DISTANCE_MAX_SAMPLES) return refuse("%s: n_samples %llu is outside 1 .. %llu", n_samples, BLU_DISTANCE_MAX_SAMPLES);
    if (n_features >= (1ull << 31)) return refuse("%s: n_features %llu is 2^31 or more", n_features);
    if (!row_ptr) { set_error("%s: row_ptr is NULL", who); return BLU_ERR_INVALID_ARG; }
    if (row_ptr[0] != 0) return refuse("%s: feature 0: row_ptr[0] is %llu, not 0", row_ptr[0]);
    for (uint64_t f = 0; f < n_features; ++f)
        if (row_ptr[f + 1] < row_ptr[f]) return refuse("%s: feature %llu: row_ptr decreases", f);
    const uint64_t nnz = row_ptr[n_features];
    if (nnz > 0xFFFFFC00ull) return refuse("%s: %llu non-zeros: more than 2^32 - 1024", nnz);   // (a position + a block's stride fits 32 bits)
    if (nnz && (!sample || !count)) { set_error("%s: sample or count is NULL", who); return BLU_ERR_INVALID_ARG; }
    total.assign(n_samples, 0);
    for (uint64_t f = 0; f < n_features; ++f) {
        for (uint64_t e = row_ptr[f]; e < row_ptr[f + 1]; ++e) {
            const uint32_t s = sample[e];
            if (s >= n_samples) return refuse("%s: feature %llu: sample id %llu is not below n_samples", f, s);
            if (e > row_ptr[f] && s <= sample[e - 1])
                return refuse("%s: feature %llu: sample %llu does not ascend (unsorted or repeated)", f, s);
            if (count[e] == 0) return refuse("%s: feature %llu: a zero count (sample %llu)", f, s);
            if (count[e] >> 63 || (total[s] += count[e]) >> 63)
                return refuse("%s: sample %llu: its counts add up to 2^63 or more (at feature %llu)", s, f);
        }
    }
    *nnz_out = nnz;
    return BLU_OK;
}

}  // namespace blu
#endif
