// Host check of the stream kernel's task queue arithmetic (blu_internal.h: task_deal / task_of_claim), built with the address
// and undefined-behaviour sanitizers and run as a program of its own by tests/test_task_claim_host.py.
//
// For every table size and grid below, every block's queue is walked in claim order (n = 0, 1, ..) and checked three ways:
//   * the ranges [q0, q0 + nq) of all blocks partition [0, n_queries) exactly;
//   * every tail piece is a multiple of 8 queries and at least 16, except the very last one of the table;
//   * entry for entry they are what the strided loop dealt before there was a queue (wave w: tasks w, w + n_waves, .. below
//     the whole rounds, then its piece of the tail) — that arithmetic is kept here as the reference.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "blu_internal.h"

namespace {

struct Range { uint32_t q0, nq; };

// The strided deal: the tasks of wave `wave`, in the order it ran them.  Its whole-round tasks were 64 queries long
// unconditionally; when the 64-query tasks fill the rounds exactly and the table's last task is a partial one, the lanes past
// the table's end ran on whatever followed the offsets.  That one task is the only place where the queue differs from the
// strided deal: the reference is cut at n_q there, every cut is counted, and check() requires that a table has exactly one
// when n_tasks64 % n_waves == 0 && n_q % 64 != 0 and none otherwise.
unsigned long long g_cuts = 0;
template <class F>
uint32_t strided_tasks(uint32_t n_q32, uint32_t n_waves, uint32_t wave, F&& each) {   // each(k, range) per task; returns their number
    const uint32_t WAVE = 64;
    uint32_t t_full, tail_q0, tail_nq;
    {
        const uint32_t n_tasks64 = n_q32 / WAVE + ((n_q32 % WAVE) != 0u ? 1u : 0u);
        t_full = n_tasks64 / n_waves * n_waves;
        const uint32_t q_full = t_full == n_tasks64 ? n_q32 : t_full * WAVE;
        uint32_t tail_q = (((n_q32 - q_full) + n_waves - 1u) / n_waves + 7u) / 8u * 8u;
        tail_q = tail_q < 16u ? 16u : (tail_q > WAVE ? WAVE : tail_q);
        const uint64_t p0 = (uint64_t)q_full + (uint64_t)wave * tail_q;
        tail_q0 = p0 < n_q32 ? (uint32_t)p0 : n_q32;
        tail_nq = n_q32 - tail_q0 < tail_q ? n_q32 - tail_q0 : tail_q;
    }
    uint32_t k = 0;
    uint32_t task = wave;
    bool in_tail = task >= t_full, tail_done = false;
    for (; !in_tail || (tail_nq != 0u && !tail_done); tail_done = in_tail, task += n_waves, in_tail = task >= t_full) {
        const uint32_t q0 = in_tail ? tail_q0 : task * WAVE;
        uint32_t nq = in_tail ? tail_nq : WAVE;
        if (nq > n_q32 - q0) { nq = n_q32 - q0; ++g_cuts; }
        each(k++, Range{q0, nq});
    }
    return k;
}

unsigned long long g_cases = 0, g_entries = 0;

#define REQUIRE(cond, ...)                                                       \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "FAIL %s:%d %s — ", __FILE__, __LINE__, #cond); \
            std::fprintf(stderr, __VA_ARGS__);                                   \
            std::fprintf(stderr, "\n");                                          \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

void check(uint32_t n_q, uint32_t n_blocks, uint32_t W) {
    const uint32_t n_waves = n_blocks * W;
    const blu::TaskDeal d = blu::task_deal(n_q, n_blocks, W);
    REQUIRE(d.own % W == 0 && d.tail_q % 8 == 0 && d.tail_q >= 16 && d.tail_q <= 64, "n_q %u waves %u", n_q, n_waves);
    const uint32_t rounds = d.own / W;
    std::vector<uint32_t> len(n_blocks);
    const unsigned long long cuts_before = g_cuts;
    // every block's queue in claim order, entry for entry against the strided deal of its waves
    for (uint32_t b = 0; b < n_blocks; ++b) {
        uint32_t total_ref = 0, q0 = 0, nq = 0;
        for (uint32_t i = 0; i < W; ++i)                       // the k-th task of wave b W + i is entry k W + i, its piece entry own + i
            total_ref += strided_tasks(n_q, n_waves, b * W + i, [&](uint32_t k, Range r) {
                REQUIRE(k <= rounds, "n_q %u waves %u wave %u: %u tasks in %u rounds", n_q, n_waves, b * W + i, k + 1, rounds);
                const uint32_t n = k < rounds ? k * W + i : d.own + i;
                blu::task_of_claim(n, b, n_blocks, W, n_q, d, q0, nq);
                REQUIRE(r.q0 == q0 && r.nq == nq && nq != 0, "n_q %u waves %u block %u entry %u: [%u, +%u) != strided [%u, +%u)", n_q, n_waves,
                        b, n, q0, nq, r.q0, r.nq);
                REQUIRE((uint64_t)q0 + nq <= n_q, "n_q %u waves %u block %u entry %u: past the table", n_q, n_waves, b, n);
            });
        uint32_t n = 0;
        for (;; ++n) {                                         // the queue in claim order: it ends at the first empty entry
            blu::task_of_claim(n, b, n_blocks, W, n_q, d, q0, nq);
            if (nq == 0) break;
        }
        len[b] = n;
        REQUIRE(n == total_ref, "n_q %u waves %u block %u: %u entries, the strided deal has %u tasks", n_q, n_waves, b, n, total_ref);
        REQUIRE(n >= d.own && n <= d.own + W, "n_q %u waves %u block %u: queue length %u", n_q, n_waves, b, n);
        for (uint32_t m = n; m < d.own + 3 * W + 2; ++m) {      // an empty queue stays empty: every wave of the block overshoots once
            blu::task_of_claim(m, b, n_blocks, W, n_q, d, q0, nq);
            REQUIRE(nq == 0, "n_q %u waves %u block %u: entry %u after the end of the queue", n_q, n_waves, b, m);
        }
        g_entries += n;
    }
    // the partition: whole-round tasks ascend with (k, b, i), the pieces with (b, p)
    uint64_t cursor = 0;
    for (uint32_t k = 0; k < rounds; ++k)
        for (uint32_t b = 0; b < n_blocks; ++b)
            for (uint32_t i = 0; i < W; ++i) {
                uint32_t q0, nq;
                blu::task_of_claim(k * W + i, b, n_blocks, W, n_q, d, q0, nq);
                REQUIRE(q0 == cursor && (nq == 64 || (nq != 0 && cursor + nq == n_q)), "n_q %u waves %u: task (%u, %u, %u) = [%u, +%u) at cursor %llu",
                        n_q, n_waves, k, b, i, q0, nq, (unsigned long long)cursor);
                cursor += nq;
            }
    for (uint32_t b = 0; b < n_blocks; ++b)
        for (uint32_t p = 0; d.own + p < len[b]; ++p) {
            uint32_t q0, nq;
            blu::task_of_claim(d.own + p, b, n_blocks, W, n_q, d, q0, nq);
            REQUIRE(q0 == cursor && nq != 0, "n_q %u waves %u: piece (%u, %u) = [%u, +%u) at cursor %llu", n_q, n_waves, b, p, q0, nq,
                    (unsigned long long)cursor);
            cursor += nq;
            REQUIRE((nq % 8 == 0 && nq >= 16) || cursor == n_q, "n_q %u waves %u: piece (%u, %u) of %u queries is not the last", n_q, n_waves,
                    b, p, nq);
        }
    REQUIRE(cursor == n_q, "n_q %u waves %u: the queues cover %llu queries", n_q, n_waves, (unsigned long long)cursor);
    const uint32_t n_tasks64 = n_q / 64 + (n_q % 64 != 0 ? 1u : 0u);
    const bool partial_last_in_a_whole_round = n_tasks64 % n_waves == 0 && n_q % 64 != 0;
    REQUIRE(g_cuts - cuts_before == (partial_last_in_a_whole_round ? 1ull : 0ull), "n_q %u waves %u: the strided reference was cut %llu times", n_q, n_waves,
            g_cuts - cuts_before);
    ++g_cases;
}

}  // namespace

int main() {
    // {blocks, waves per block}: 12 and 16 waves (milli-percent builds with and without the ring; f64 builds without it), 11 (f64, ring)
    const uint32_t grids[7][2] = {{1, 11}, {1, 12}, {1, 16}, {131, 12}, {256, 11}, {256, 12}, {256, 16}};
    for (const auto& g : grids) {
        const uint32_t n_waves = g[0] * g[1];
        for (uint32_t n_q = 0; n_q <= 20000; ++n_q) check(n_q, g[0], g[1]);
        for (uint32_t k = 0; k <= 4; ++k)
            for (int d = -65; d <= 65; ++d) {
                const int64_t n_q = (int64_t)n_waves * 64 * k + d;
                if (n_q >= 0) check((uint32_t)n_q, g[0], g[1]);
            }
    }
    REQUIRE(g_cuts != 0, "no table with a partial last task in a whole round was walked (%llu tables)", g_cases);
    std::printf("task_claim_host ok: %llu tables, %llu queue entries, %llu cuts of the reference\n", g_cases, g_entries, g_cuts);
    return 0;
}
