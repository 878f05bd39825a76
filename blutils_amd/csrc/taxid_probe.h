// The device side of TaxidMap (ingest.h): the table as the kernels see it and the probe, shared by the GPU ingest
// (ingest_gpu.hip) and the labelled sequence export (seqdb_gpu.hip).  The names stay in an unnamed namespace, as they were
// when the ingest alone had them: each translation unit has its own copy and the ingest's kernels keep their symbols.
#ifndef BLU_TAXID_PROBE_H
#define BLU_TAXID_PROBE_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "blu_consensus.h"
#include "ingest.h"

namespace blu {
namespace {

struct DevTaxidMap { const TaxidMap::E* tab; uint64_t mask; };

// the row of taxid k, or BLU_UNMATCHED_TAXID (TaxidMap::find_or on the device: the same hash, linear probing; the table
// is at most half full, so an unused entry ends every chain)
__device__ __forceinline__ uint32_t taxid_lookup(const DevTaxidMap& t, long long k) {
    unsigned long long x = (unsigned long long)k * 0x9E3779B97F4A7C15ull;
    x ^= x >> 32;
    uint64_t i = x & t.mask;
    for (;;) {
        const TaxidMap::E e = t.tab[i];
        if (!e.used) return BLU_UNMATCHED_TAXID;
        if (e.key == k) return e.val;
        i = (i + 1) & t.mask;
    }
}

}  // namespace
}  // namespace blu
#endif
