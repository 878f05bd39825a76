// Host code that moves bytes between files, host memory and the device for the library's GPU programs (ingest_prims.h):
// file -> HBM through pinned staging, and device -> pageable host memory by a pool of host threads.  No kernels.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "ingest.h"
#include "ingest_prims.h"

namespace blu {

// The text goes page cache -> pinned staging -> HBM without ever being mapped into the process: three reader threads,
// each with two pinned slots, pread() a piece while the previous one is on the wire.  What the parts cost on a box
// (scripts/probe/upload_probe.hip, 6.7 GB): the copies alone 0.12 s (56 GB/s, the PCIe rate; one stream carries 50 of it),
// pread alone 30 GB/s per thread, so two or three readers keep the wire busy — and EVERY hipStreamCreate 15 ms (the first
// one of the process 40-170 ms: an HSA queue each).  Six readers with a stream and a hipHostMalloc each, as this was
// written first, spent more time setting up than copying.  Hence: one pinned block for all slots, and all copies on the
// null stream, which the kernels that follow need anyway (in order on one queue: a slot's event still says when it is free).
// Mapping the file and handing it to hipMemcpy moves the bytes as fast (the runtime pins the page-cache pages) but
// costs 0.06 s to populate and 0.07-0.10 s to unmap 6.7 GB of page table.
int upload_file(int fd, size_t size, unsigned char* d_text, int device, std::string* err) {
    unsigned nt = 3;
    if (const char* env = getenv("BLU_UPLOAD_THREADS")) nt = (unsigned)atoi(env);
    const size_t piece = 8u << 20, n_pieces = (size + piece - 1) / piece;
    nt = std::max(1u, std::min<unsigned>(std::min(nt, 16u), (unsigned)std::max<size_t>(n_pieces, 1)));
    std::atomic<size_t> next{0};
    std::atomic<int> failed{0};      // 1: the file could not be read; 2: the staging path could not be set up or used (HIP)
    std::vector<std::string> errs(nt + 1);
    auto fail = [&](unsigned t, const char* what, hipError_t e) {
        errs[t] = std::string(what) + ": " + (e == hipSuccess ? strerror(errno) : hipGetErrorString(e));
        int none = 0;
        failed.compare_exchange_strong(none, e == hipSuccess ? 1 : 2);
    };
    char* block = nullptr;
    std::vector<hipEvent_t> events((size_t)nt * 2, nullptr);
    const bool trace = getenv("BLU_INGEST_TRACE") != nullptr;
    const double t_in = now_s();
    hipError_t e0 = hipHostMalloc((void**)&block, (size_t)nt * 2 * piece, hipHostMallocDefault);
    for (size_t k = 0; k < events.size() && e0 == hipSuccess; ++k) e0 = hipEventCreateWithFlags(&events[k], hipEventDisableTiming);
    if (e0 != hipSuccess) fail(nt, "staging set-up", e0);
    const double t_setup = now_s();
    auto work = [&](unsigned t) {
        char* const slots = block + (size_t)t * 2 * piece;
        hipEvent_t* const ev = &events[(size_t)t * 2];
        bool busy[2] = {false, false};
        hipError_t e = hipSetDevice(device);
        if (e != hipSuccess) fail(t, "hipSetDevice", e);
        unsigned turn = 0;
        while (!failed.load(std::memory_order_relaxed)) {
            const size_t k = next.fetch_add(1);
            if (k >= n_pieces) break;
            const unsigned sl = turn++ & 1;
            if (busy[sl] && (e = hipEventSynchronize(ev[sl])) != hipSuccess) { fail(t, "hipEventSynchronize", e); break; }
            const size_t off = k * piece, len = std::min(piece, size - off);
            size_t got = 0;
            while (got < len) {
                const ssize_t r = pread(fd, slots + sl * piece + got, len - got, (off_t)(off + got));
                if (r < 0 && errno == EINTR) continue;
                if (r <= 0) { fail(t, "pread", hipSuccess); break; }
                got += (size_t)r;
            }
            if (got < len) break;
            if ((e = hipMemcpyAsync(d_text + off, slots + sl * piece, len, hipMemcpyHostToDevice, nullptr)) != hipSuccess) { fail(t, "hipMemcpyAsync", e); break; }
            if ((e = hipEventRecord(ev[sl], nullptr)) != hipSuccess) { fail(t, "hipEventRecord", e); break; }
            busy[sl] = true;
        }
    };
    if (!failed) {
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < nt; ++t) pool.emplace_back(work, t);
        work(0);
        for (auto& th : pool) th.join();
    }
    {   // the slots are free once everything queued has been sent (also on the way out of a failure: copies may be in flight)
        const double t_queued = now_s();
        const hipError_t e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess && !failed) fail(nt, "hipStreamSynchronize", e);
        if (trace) fprintf(stderr, "[ingest-gpu]   upload: pinned block + events %.3f s, pieces read and queued %.3f s, last ones on the wire %.3f s\n",
                           t_setup - t_in, t_queued - t_setup, now_s() - t_queued);
    }
    for (hipEvent_t ev : events) if (ev) (void)hipEventDestroy(ev);
    if (block) (void)hipHostFree(block);
    if (failed) {
        for (auto& m : errs) if (!m.empty()) { *err = m; break; }
        (void)hipGetLastError();
        return failed == 1 ? BLU_ERR_IO : BLU_INGEST_FALLBACK;   // (no pinned memory to be had, say: the CPU parser takes the file)
    }
    return BLU_OK;
}

int upload_text(int fd, size_t size, int device, const char* name, DeviceArena& mem, unsigned char** d_text, bool* open_tail,
                const std::function<void()>& allocated) {
    HipPolicy& pol = mem.pol;
    HIP_CHECK(pol, mem.alloc(d_text, ((size + 15) & ~(size_t)15) + 64, name));
    HIP_CHECK(pol, hipMemset(*d_text + size, 0, 64));
    if (allocated) allocated();
    *open_tail = false;
    if (size == 0) return BLU_OK;
    std::string io;
    const int rc = upload_file(fd, size, *d_text, device, &io);
    if (rc == BLU_INGEST_FALLBACK && pol.why) { *pol.why = "the pinned staging path failed (" + io + ")"; return rc; }
    if (rc != BLU_OK) { set_error("%s: reading %s failed: %s", pol.who, name, io.c_str()); return rc == BLU_ERR_IO ? BLU_ERR_IO : BLU_ERR_HIP; }
    char last = 0;
    if (pread(fd, &last, 1, (off_t)(size - 1)) != 1) { set_error("%s: reading %s failed", pol.who, name); return BLU_ERR_IO; }
    *open_tail = last != '\n';
    return BLU_OK;
}

// Device -> pageable host memory in 8 MiB pieces by a pool of host threads: the first touch of the fresh destination pages
// (and the runtime's pinning of them) costs more than the transfer, and it parallelises.
void d2h_add(std::vector<D2HPiece>& v, void* dst, const void* src, size_t bytes, size_t piece) {
    for (size_t o = 0; o < bytes; o += piece) v.push_back({(char*)dst + o, (const char*)src + o, std::min(piece, bytes - o)});
}
hipError_t d2h_parallel(const std::vector<D2HPiece>& pieces, int device, unsigned max_threads) {
    if (pieces.empty()) return hipSuccess;
    const unsigned nt = ingest_threads(std::min<unsigned>(max_threads, (unsigned)pieces.size()));
    std::vector<hipError_t> errs(nt, hipSuccess);
    std::atomic<size_t> next{0};
    auto work = [&](unsigned t) {
        (void)hipSetDevice(device);
        for (size_t k = next.fetch_add(1); k < pieces.size() && errs[t] == hipSuccess; k = next.fetch_add(1))
            errs[t] = hipMemcpy(pieces[k].dst, pieces[k].src, pieces[k].bytes, hipMemcpyDeviceToHost);
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < nt; ++t) pool.emplace_back(work, t);
    work(0);
    for (auto& th : pool) th.join();
    for (hipError_t e : errs) if (e != hipSuccess) return e;
    return hipSuccess;
}
}  // namespace blu
