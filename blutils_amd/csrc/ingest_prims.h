// Host side shared by the library's GPU programs: the GPU ingest (ingest_gpu.hip), the engine on its columns, the taxon
// report (report_kernel.hip), `build-db blu` (taxdb_gpu.hip) and the kraken2 / qiime2 export (seqdb_gpu.hip).
//   - the error path of a HIP call (HipPolicy, hip_fail, HIP_CHECK) and the owner of one call's device memory (DeviceArena)
//   - the device primitives (line index, prefix sums, radix sort, column compaction): host wrappers around kernels that are
//     compiled once, in dev_prims.hip; the upload and the parallel download of dev_io.cpp; a whole text file with its line
//     index (load_text), for the two `build-db` builders that read theirs at once
//   - host one-liners: a monotonic clock, launch grids, write_all, JSON string escapes
#ifndef BLU_INGEST_PRIMS_H
#define BLU_INGEST_PRIMS_H

#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <string_view>
#include <thread>
#include <vector>

#include "blu_internal.h"

namespace blu {

// ---- the error path.  Each entry point passes its policy in: a failed HIP call that ran out of device memory returns
// oom_rc, any other failure BLU_ERR_HIP.  The message is "<who>: <call> failed: <HIP's text>"; an allocation names its
// bytes and label instead of the call.  why set: running out of memory is a fall-back, not an error (the GPU ingest hands
// the file to the CPU parser): the reason goes to *why and no message is set.
struct HipPolicy {
    const char* who;
    int oom_rc;
    std::string* why = nullptr;
    size_t alloc_bytes = 0;            // the allocation that failed last (DeviceArena::alloc, DevBuf), for the message
    const char* alloc_what = nullptr;
    // an allocation's status, noted on the way back to its caller
    hipError_t noted(hipError_t e, size_t bytes, const char* what) { alloc_bytes = bytes; alloc_what = e == hipSuccess ? nullptr : what; return e; }
};

// sets the message, clears HIP's last error, returns the policy's code
inline int hip_fail(HipPolicy& pol, hipError_t e, const char* call) {
    (void)hipGetLastError();
    const bool oom = e == hipErrorOutOfMemory;
    if (oom && pol.why) *pol.why = "not enough free device memory";
    else if (pol.alloc_what)
        set_error("%s: device allocation of %zu bytes (%s) failed: %s", pol.who, pol.alloc_bytes, pol.alloc_what, hipGetErrorString(e));
    else set_error("%s: %s failed: %s", pol.who, call, hipGetErrorString(e));
    pol.alloc_what = nullptr;
    return oom ? pol.oom_rc : BLU_ERR_HIP;
}

#define HIP_CHECK(pol, x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return ::blu::hip_fail((pol), e_, #x); } while (0)

// The device allocations of one call: whatever is still recorded is freed when the arena goes, whichever way the call is
// left.  alloc() returns HIP's status and leaves the verdict to the caller (HIP_CHECK, or a fall-back of its own).
struct DeviceArena {
    HipPolicy& pol;
    std::vector<void*> ptrs;
    // keep: free() leaves the buffer to the end of the call (on some boxes an allocation that follows a hipFree of GBs takes
    // 0.1 - 0.4 s per GB: 0.3 s of a 0.7 s ingest); the GPU ingest sets it when the device has room for it
    bool keep = false;

    explicit DeviceArena(HipPolicy& p) : pol(p) {}
    DeviceArena(const DeviceArena&) = delete;
    DeviceArena& operator=(const DeviceArena&) = delete;
    ~DeviceArena() { free_all(); }

    template <class T>
    hipError_t alloc(T** out, size_t bytes, const char* what) {
        void* p = nullptr;
        const hipError_t e = pol.noted(hipMalloc(&p, std::max<size_t>(bytes, 16)), bytes, what);
        if (e == hipSuccess) { ptrs.push_back(p); *out = (T*)p; }
        return e;
    }
    // a device copy of host[0, n): allocated whatever n is, filled when there is something to fill it with
    template <class T>
    hipError_t upload(T** out, const void* host, size_t n, const char* what) {
        const hipError_t e = alloc(out, n * sizeof(T), what);
        return e == hipSuccess && n ? hipMemcpy(*out, host, n * sizeof(T), hipMemcpyHostToDevice) : e;
    }
    // n elements back to the host (the buffer may be any device memory)
    template <class T>
    static hipError_t download(void* host, const T* dev, size_t n) {
        return n ? hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
    }
    void free(void* p) {
        if (keep) return;
        auto it = std::find(ptrs.begin(), ptrs.end(), p);
        if (it == ptrs.end()) return;
        (void)hipFree(p);
        ptrs.erase(it);
    }
    void release(void* p) {   // ownership moves elsewhere
        auto it = std::find(ptrs.begin(), ptrs.end(), p);
        if (it != ptrs.end()) ptrs.erase(it);
    }
    // every recorded buffer goes to `to` (DeviceHits::trash: freed with the device columns, off the caller's path)
    void hand_over(std::vector<void*>& to) { to.insert(to.end(), ptrs.begin(), ptrs.end()); ptrs.clear(); }
    void free_all() { for (void* p : ptrs) (void)hipFree(p); ptrs.clear(); }
};

// ---- line index of a device text d_text[0, size), padded with >= 64 zero bytes (16-byte loads): line k is
// [line[k], line[k + 1] - 1).  Two steps, so that the caller sizes line[] (and applies its own limit) in between.
// tiles of the newline count
uint64_t line_tiles(uint64_t size);
// 1. the newlines: tile counts, the pad entry, their exclusive scan into d_base, the total to the host (u32: it wraps at
//    2^32).  d_tile, d_base: line_tiles(size) + 1 words; d_tmp: scan_tmp_bytes_u32(line_tiles(size) + 1) bytes
hipError_t line_count(const unsigned char* d_text, uint64_t size, uint32_t* d_tile, uint32_t* d_base, void* d_tmp, uint32_t* n_newlines);
// 2. line[0] = 0, line[k + 1] = offset after newline k; open_tail (the last line has no newline): line[n_lines] = size + 1
hipError_t line_write(const unsigned char* d_text, uint64_t size, const uint32_t* d_base, uint64_t* d_line, uint64_t n_lines, bool open_tail);

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

// ---- stable compaction of one column: in[i] goes to out[pos[i]] where keep[i] == 1, pos = the exclusive scan of the keep words
// (the hit filter's kernel); no store lands at or beyond n_out.  in, keep and pos are read 16 bytes at a time:
// 16-byte aligned.  Launched on the null stream; returns the launch's status
hipError_t compact_column_u32(const uint32_t* in, const uint32_t* keep, const uint32_t* pos, uint32_t n, uint32_t n_out, uint32_t* out);
hipError_t compact_column_u64(const unsigned long long* in, const uint32_t* keep, const uint32_t* pos, uint32_t n, uint32_t n_out,
                              unsigned long long* out);

// makes the runtime load the code object of dev_prims.hip now (warm_up_device), not at the first use of one of the above
// (hidden: the library exports what it exported before the primitives had a file of their own)
__attribute__((visibility("hidden"))) void load_dev_prims();

// ---- file -> HBM through pinned staging (pread, never mapped); BLU_OK, BLU_ERR_IO, or BLU_INGEST_FALLBACK (HIP staging)
int upload_file(int fd, size_t size, unsigned char* d_text, int device, std::string* err);
// file -> padded device text in the arena: (size rounded up to 16) + 64 bytes, the 64 after `size` zeroed, the file
// uploaded; *open_tail: its last byte is not a newline.  A file that cannot be read is BLU_ERR_IO ("<who>: reading <name>
// failed"); a staging path that fails is a fall-back under a policy with `why`, else BLU_ERR_HIP.  `allocated` runs once
// the padded buffer is there (a trace lap)
int upload_text(int fd, size_t size, int device, const char* name, DeviceArena& mem, unsigned char** d_text, bool* open_tail,
                const std::function<void()>& allocated = nullptr);

// ---- a whole text file in HBM with its line index (the `build-db` builders): line k is [line[k], line[k + 1] - 1).  Errors
// name the path; at most 2^31 - 17 lines
struct DeviceText {
    std::string path;
    size_t size = 0;
    unsigned char* d = nullptr;
    uint64_t* line = nullptr;
    uint32_t n_lines = 0;
};
inline int load_text(const char* path, int device, DeviceArena& mem, DeviceText& t) {
    HipPolicy& pol = mem.pol;
    t.path = path;
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) { set_error("build-db: cannot open %s: %s", path, strerror(errno)); return BLU_ERR_IO; }
    struct FdCloser { int fd; ~FdCloser() { close(fd); } } closer{fd};
    struct stat sb;
    if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) { set_error("build-db: %s is not a regular file", path); return BLU_ERR_IO; }
    t.size = (size_t)sb.st_size;
    if (t.size >= (1ull << 40)) { set_error("build-db: %s is too large (%zu bytes)", path, t.size); return BLU_ERR_INVALID_ARG; }
    bool open_tail = false;
    if (const int rc = upload_text(fd, t.size, device, path, mem, &t.d, &open_tail); rc != BLU_OK) return rc;
    const uint64_t n_tiles = line_tiles(t.size);
    uint32_t *tile = nullptr, *base = nullptr, n_nl = 0;
    void* tmp = nullptr;
    HIP_CHECK(pol, mem.alloc(&tile, (n_tiles + 1) * 4, "line index"));
    HIP_CHECK(pol, mem.alloc(&base, (n_tiles + 1) * 4, "line index"));
    HIP_CHECK(pol, mem.alloc(&tmp, scan_tmp_bytes_u32(n_tiles + 1), "line index"));
    HIP_CHECK(pol, line_count(t.d, t.size, tile, base, tmp, &n_nl));
    const uint64_t n = (uint64_t)n_nl + (open_tail ? 1 : 0);
    if (n >= 0x7FFFFFF0ull) { set_error("build-db: %s has 2^31 lines or more", path); return BLU_ERR_INVALID_ARG; }
    t.n_lines = (uint32_t)n;
    HIP_CHECK(pol, mem.alloc(&t.line, (n + 2) * 8, "line index"));
    HIP_CHECK(pol, line_write(t.d, t.size, base, t.line, n, open_tail));
    return BLU_OK;
}

// ---- device -> pageable host memory by a pool of host threads
struct D2HPiece { char* dst; const char* src; size_t bytes; };
void d2h_add(std::vector<D2HPiece>& v, void* dst, const void* src, size_t bytes, size_t piece = 8u << 20);
hipError_t d2h_parallel(const std::vector<D2HPiece>& pieces, int device, unsigned max_threads = 16);

// ---- host one-liners
// host threads of a parallel step: BLU_INGEST_THREADS, else the machine's; at least one, at most `cap`
inline unsigned ingest_threads(unsigned cap) {
    unsigned nt = std::thread::hardware_concurrency();
    if (const char* env = getenv("BLU_INGEST_THREADS")) nt = (unsigned)atoi(env);
    return std::max(1u, std::min(nt, cap));
}

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// blocks of `block` threads over n items (at least one)
inline unsigned grid(uint64_t n, uint64_t block = 256) { return (unsigned)std::max<uint64_t>((n + block - 1) / block, 1); }

inline bool write_all(int fd, const void* buf, size_t n) {
    const char* p = (const char*)buf;
    while (n) {
        const ssize_t w = write(fd, p, std::min<size_t>(n, 1u << 30));
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) return false;
        p += w; n -= (size_t)w;
    }
    return true;
}

// body of a JSON string (no quotes), serde_json's escapes: runs of plain bytes are appended whole
template <class O>
void json_esc(O& o, const char* p, size_t n) {
    size_t i0 = 0;
    for (size_t i = 0; i < n; ++i) {
        const unsigned char c = (unsigned char)p[i];
        if (c >= 0x20 && c != '"' && c != '\\') continue;
        o.append(p + i0, i - i0);
        i0 = i + 1;
        switch (c) {
            case '"': o += "\\\""; break; case '\\': o += "\\\\"; break; case '\n': o += "\\n"; break;
            case '\r': o += "\\r"; break; case '\t': o += "\\t"; break; case '\b': o += "\\b"; break; case '\f': o += "\\f"; break;
            default: { char b[8]; snprintf(b, sizeof b, "\\u%04x", c); o += b; }
        }
    }
    o.append(p + i0, n - i0);
}
template <class O>
void json_str(O& o, std::string_view s) {
    o.push_back('"');
    json_esc(o, s.data(), s.size());
    o.push_back('"');
}

}  // namespace blu
#endif
