// One entry of the `taxonomies` array of a *.blutils.json as the device renderers write it (serde_json::to_string_pretty of
// TaxonomyMapUnit at depth 2): the pieces, serde's string escapes and the byte writers.  Shared by `build-db blu`
// (taxdb_gpu.hip) and `build-db lineages` (lineage_db_gpu.hip), so that both write the same bytes per entry.
#ifndef BLU_TAXMAP_ENTRY_DEV_H
#define BLU_TAXMAP_ENTRY_DEV_H

#include <hip/hip_runtime.h>

#include <cstdint>

#include "text_dev.h"

namespace blu {

// every entry starts with ",\n" and the host drops the first two bytes of the array
#define H0 ",\n    {\n      \"taxid\": "
#define H1 ",\n      \"rank\": \""
#define H2 "\",\n      \"numericLineage\": \""
#define H3 "\",\n      \"textLineage\": \""
#define H4 "\",\n      \"accessions\": [\n"
#define A0 "        {\n          \"accession\": \""
#define A1 "\",\n          \"oid\": \""
#define A2 "\"\n        }"
#define A_NEXT ",\n"
#define A_LAST "\n      ]\n    }"
constexpr uint32_t cl(const char* s) { return *s ? 1 + cl(s + 1) : 0; }

// bytes of a string once serde_json has escaped it
__device__ __forceinline__ uint32_t esc_bytes(uint32_t c) {
    if (c == '"' || c == '\\' || c == '\b' || c == '\f' || c == '\n' || c == '\r' || c == '\t') return 2;
    return c < 0x20 ? 6 : 1;
}
__device__ __forceinline__ uint32_t esc_len(const unsigned char* __restrict__ text, uint64_t a, uint64_t b) {
    uint32_t n = 0;
    for_bytes(text, a, b, [&](uint32_t c, uint64_t) { n += esc_bytes(c); return true; });
    return n;
}

__device__ __forceinline__ unsigned char* put(unsigned char* o, const char* s) { while (*s) *o++ = (unsigned char)*s++; return o; }
__device__ __forceinline__ unsigned char* put_bytes(unsigned char* o, const unsigned char* s, unsigned long long n) {
    for (unsigned long long k = 0; k < n; ++k) o[k] = s[k];
    return o + n;
}
__device__ __forceinline__ unsigned char* put_escaped(unsigned char* o, const unsigned char* text, uint64_t a, uint32_t n) {
    const char* hex = "0123456789abcdef";
    for_bytes(text, a, a + n, [&](uint32_t c, uint64_t) {
        switch (c) {
            case '"': *o++ = '\\'; *o++ = '"'; break;
            case '\\': *o++ = '\\'; *o++ = '\\'; break;
            case '\b': *o++ = '\\'; *o++ = 'b'; break;
            case '\f': *o++ = '\\'; *o++ = 'f'; break;
            case '\n': *o++ = '\\'; *o++ = 'n'; break;
            case '\r': *o++ = '\\'; *o++ = 'r'; break;
            case '\t': *o++ = '\\'; *o++ = 't'; break;
            default:
                if (c < 0x20) { o = put(o, "\\u00"); *o++ = (unsigned char)hex[c >> 4]; *o++ = (unsigned char)hex[c & 15]; }
                else *o++ = (unsigned char)c;
        }
        return true;
    });
    return o;
}

}  // namespace blu
#endif
