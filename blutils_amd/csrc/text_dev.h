// Device text helpers shared by the taxonomies-database builder (taxdb_gpu.hip) and the sequence export (seqdb_gpu.hip).
// The text they read is padded past its end (>= 16 bytes) so that aligned 16-byte loads never leave the allocation.
#ifndef BLU_TEXT_DEV_H
#define BLU_TEXT_DEV_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace blu {

__device__ __forceinline__ bool is_ws(uint32_t c) { return c == ' ' || (c >= 9 && c <= 13); }   // str::trim, ASCII range

// visit bytes of text[a, b) through aligned 16-byte loads (the text is padded past its end); f returns false to stop
template <class F>
__device__ __forceinline__ void for_bytes(const unsigned char* __restrict__ text, uint64_t a, uint64_t b, F&& f) {
    for (uint64_t w = a & ~15ull; w < b; w += 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(text + w);
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint64_t p = w + k;
            if (p < a || p >= b) continue;
            const uint32_t x = (k & 8) ? ((k & 4) ? v.w : v.z) : ((k & 4) ? v.y : v.x);   // (no array: stays in registers unrolled or not)
            if (!f((x >> (8 * (k & 3))) & 0xFFu, p)) return;
        }
    }
}

// str::from_utf8 on a line (Rust rejects overlong forms, surrogates and code points above U+10FFFF, as this does)
__device__ __forceinline__ bool utf8_valid(const unsigned char* __restrict__ text, uint64_t a, uint64_t b) {
    uint32_t need = 0, lo = 0x80, hi = 0xBF;
    bool ok = true;
    for_bytes(text, a, b, [&](uint32_t c, uint64_t) {
        if (need == 0) {
            if (c < 0x80) return true;
            if (c >= 0xC2 && c <= 0xDF) { need = 1; lo = 0x80; hi = 0xBF; }
            else if (c == 0xE0) { need = 2; lo = 0xA0; hi = 0xBF; }
            else if ((c >= 0xE1 && c <= 0xEC) || c == 0xEE || c == 0xEF) { need = 2; lo = 0x80; hi = 0xBF; }
            else if (c == 0xED) { need = 2; lo = 0x80; hi = 0x9F; }
            else if (c == 0xF0) { need = 3; lo = 0x90; hi = 0xBF; }
            else if (c >= 0xF1 && c <= 0xF3) { need = 3; lo = 0x80; hi = 0xBF; }
            else if (c == 0xF4) { need = 3; lo = 0x80; hi = 0x8F; }
            else { ok = false; return false; }
            return true;
        }
        if (c < lo || c > hi) { ok = false; return false; }
        lo = 0x80; hi = 0xBF; --need;
        return true;
    });
    return ok && need == 0;
}

// decimal digits of v, and v written as d digits at out[0, d)
__device__ __forceinline__ uint32_t n_digits(unsigned long long v) { uint32_t d = 1; while (v >= 10) { v /= 10; ++d; } return d; }
__device__ __forceinline__ void put_digits(unsigned char* out, unsigned long long v, uint32_t d) {
    for (uint32_t k = d; k > 0; --k) { out[k - 1] = (unsigned char)('0' + v % 10); v /= 10; }
}

__device__ __forceinline__ void trim(const unsigned char* __restrict__ text, uint64_t& a, uint64_t& b) {
    while (a < b && is_ws(text[a])) ++a;
    while (b > a && is_ws(text[b - 1])) --b;
}

}  // namespace blu
#endif
