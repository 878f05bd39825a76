// Internal declarations shared by the host side and the HIP kernels of
// libblu_consensus.so.  Not part of the ABI (include/blu_consensus.h is).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "blu_consensus.h"

namespace blu {

// canonical rank codes: 0..8 = LinnaeanRank enum kinds (linnaean_ranks.rs:16-29),
// >= 9 = Other(slug), interned in order of first appearance
enum RankKind : uint16_t { K_UNDEFINED = 0, K_DOMAIN, K_KINGDOM, K_PHYLUM, K_CLASS, K_ORDER, K_FAMILY, K_GENUS,
                           K_SPECIES, K_FIRST_OTHER };

struct RankInfo {
    std::string display;  // impl Display (linnaean_ranks.rs:74-89)
    std::string serde;    // serde camelCase name / raw Other string
};

// Device view of the taxonomy (passed to kernels by value).
//
// Lineage rows sit in LEXICOGRAPHIC order of their node sequences (row index = "pos"; engine row ids are
// pos | lineage length << BLU_ROW_BITS, so the streaming phase needs no taxonomy lookup).  One row:
//   word 0             len | shape << 8   (len 0 = lineage that fails parse_taxonomy)
//   bytes 4+j, 24+j    0x80 | a_j and 0x80 | b_j, j < 20: how many sorted rows to the left (a) / right (b) of this one still
//                      share its levels 0..j, saturated at 127 (levels the row does not have: 0x80).  The levels shared by a
//                      group spanning [lo, hi] around this row are the levels with a_j >= pos - lo and b_j >= hi - pos, four
//                      levels per 32-bit subtraction (bit 7 of a byte survives `byte - distance` exactly when the run is long
//                      enough); exact when both distances are <= 127 — wider groups, and agreement deeper than 20 levels, use
//                      the lcp8 / rmq tables below
//   word 11+j          node id of level j   interned (Display(rank), identifier)
// i.e. one 128-byte line for lineages of up to 20 levels (stride 32 words; deeper taxonomies get longer rows).  What the finalisation needs per LEVEL — cutoff, rank code, max-allowed-rank code — depends on the
// row's shape only: codes[shape][cstride], one word per level =
//   cutoff id (12 bits) | canonical rank code (10 bits) << 12 | max-allowed-rank code (10 bits) << 22
// (a few hundred KB, re-read by every query, so it stays in L2).  Cutoffs are stored by id into `cutvals`, the
// table of the few hundred DISTINCT f64 cutoff values of this (taxonomy, backbone) pair, held in LDS.
struct TaxDev {
    const uint32_t* lin;     // [n_tax][stride]
    const uint32_t* codes;   // [n_shapes][cstride]
    const uint32_t* kthr;    // [n_shapes][cstride] per level: smallest milli-percent identity k with fl(k / 1000) >= cutoff (17 bits,
                             // BLU_KTHR_NEVER if none below it) | (fl(that k / 1000) == cutoff) << 17: `>=` and `>` as integer compares
                             // | canonical rank code << BLU_LVL_RANK_SHIFT | (max-allowed-rank code is BLU_MAR_NEVER_EQUAL, else
                             // the rank code itself) << BLU_LVL_NEVER_SHIFT: the integer level tests and the record read nothing else
    uint32_t cstride;        // words per shape row, multiple of 16
    // lcp8[i] = number of leading levels shared by sorted rows i and i+1.  In that order the levels shared by a
    // whole group of rows = min(lcp8[lo .. hi-1]) for the group's smallest/largest pos: a range-minimum query
    // replaces the per-row level scan of find_multi_taxa_consensus.rs:137-180.
    const uint8_t* lcp8;     // [n_tax - 1], padded with 0xFF to a multiple of 16 (+16)
    const uint8_t* rmq;      // sparse table over 16-entry blocks of lcp8: level k at rmq + k * rmq_nb, entry j = min of blocks j .. j+2^k-1
    uint32_t rmq_nb;         // blocks per level
    const double* cutvals;   // [n_cutvals] distinct cutoff values (NaN included, compared by bit pattern)
    uint32_t n_cutvals;
    uint64_t n_tax;
    uint32_t stride;         // words per lineage row, multiple of 32 (128 bytes)
    uint32_t node_base;      // word of the row where the node ids start (BLU_ROW_NODE_BASE)
    uint32_t max_depth;      // longest lineage: bounds the length bits of a (possibly corrupt) row id
    uint32_t n_shapes;       // rows of codes / kthr (>= 1): bounds a (possibly corrupt) shape id
    // Shared levels of a WIDE group (more than BLU_ROW_RUN_MAX sorted rows either side of the reference row) without the
    // range-minimum tables.  A node of the taxonomy with at least BLU_WIDE_MIN rows is "wide"; every node that holds a wide
    // group is wide, and so is each of its ancestors, so the wide nodes form a small tree (15 k nodes at 2.4 M taxids).
    //   wblk[pos >> 6]    deepest wide node around each sorted position of a 64-row block: {w0 | w1 << 16, w2 | s1 << 16 | s2 << 24} —
    //                     w0 up to offset s1, w1 up to s2, w2 after (node id + 1, 0 = none); s1 == BLU_WBLK_OVERFLOW: more than two
    //                     changes inside the block, ask the range-minimum tables
    //   wchain[w][16]     end (exclusive sorted position) of the ancestor at level i of wide node w - 1, i = 0 .. its own level;
    //                     0 beyond.  Row 0 is all zeros (no wide node).
    // The group [lo, hi] shares exactly the levels i with hi < wchain[w(lo)][i]: the nodes that hold lo AND hi are wide, hold lo,
    // and are therefore that chain's prefix.  0.3 MB + 1 MB, hot in L2, instead of four lines of the 5 MB lcp8 / rmq tables.
    const uint2* wblk = nullptr;       // null: no wide tables (more than 65534 wide nodes, or a wide node deeper than 32 levels)
    const uint32_t* wchain = nullptr;  // [n_wide + 1][BLU_WCHAIN]
    const uint32_t* wchain_hi = nullptr;   // levels 16 .. 31 of the chains, when wide_levels > 16
    uint32_t wide_levels = 0;          // deepest wide node's level + 1
};
#define BLU_WIDE_MIN 128u          // rows of a node from which it is "wide" (a wide group spans at least BLU_ROW_RUN_MAX + 2 rows)
#define BLU_WCHAIN 16u             // chain entries per table row
#define BLU_WBLK_SHIFT 6u          // 64 sorted positions per wblk entry
#define BLU_WBLK_OVERFLOW 0xFFu

#define BLU_ROW_IV_LEVELS 20u    // levels whose neighbour run lengths sit in the row (words 1..10)
#define BLU_ROW_RUN_MAX 127u     // a run length byte saturates here
#define BLU_ROW_NODE_BASE 11u    // first node-id word of a row
#define BLU_KTHR_BITS 17u
#define BLU_KTHR_NEVER ((1u << BLU_KTHR_BITS) - 1u)
#define BLU_LVL_RANK_SHIFT 18u
#define BLU_LVL_NEVER_SHIFT 28u
#define BLU_HINT_BITS 15u        // shape hint of a packed side record: word 1 = pident_milli | (shape id + 1) << BLU_KTHR_BITS, 0 = none
#define BLU_PACK_CUT_BITS 12u
#define BLU_PACK_CODE_BITS 10u
#define BLU_PACK_CODE_MASK ((1u << BLU_PACK_CODE_BITS) - 1u)
#define BLU_PACK_NEVER (BLU_PACK_CODE_MASK - 1u)   // BLU_MAR_NEVER_EQUAL in 10 bits

struct HitsDev {
    const int32_t* bitscore;
    const uint32_t* tax_row;
    const double* pident;          // f64 layout, or nullptr
    const uint32_t* pident_milli;  // milli-percent layout, or nullptr
    const uint32_t* packed;        // packed layout: 4 words per hit {tax_row, pident_milli | shape hint << 17, align_len, acc_rank}, or nullptr
    const int32_t* align_len;
    const uint32_t* acc_rank;
    const uint64_t* seg_off;
    uint64_t n_hits;
    uint64_t n_queries;
    const uint32_t* packed64 = nullptr;   // 6 words per hit {tax_row, shape hint << 17, align_len, acc_rank, pident f64 lo, hi}, or nullptr
};

// How the stream kernel deals its wave tasks (consensus_kernel.hip, the head of the task loop).  Tasks are 64
// consecutive queries while there is a whole round of them (one task per wave of the grid: n_blocks x W); the queries left after
// the last whole round are cut into one piece per wave, tail_q queries each (a multiple of 8, at least 16, at most 64).  Block b
// owns the tasks b W + i + k n_waves (i < W, k < rounds) and the pieces of its W waves, and its waves CLAIM them from a queue
// of the block's own in the order n = k W + i, pieces last: the block sweeps the table in step with the others, as a strided
// loop would, but a wave that gets cheap tasks takes more of them.
struct TaskDeal {
    uint32_t own;      // entries of a block's queue that are whole-round tasks: rounds x W
    uint32_t tail_q;   // queries per tail piece
};
__host__ __device__ inline TaskDeal task_deal(uint32_t n_q, uint32_t n_blocks, uint32_t W) {
    const uint32_t n_waves = n_blocks * W;
    const uint32_t n_tasks64 = n_q / 64u + ((n_q % 64u) != 0u ? 1u : 0u);
    const uint32_t rounds = n_tasks64 / n_waves;
    const uint32_t t_full = rounds * n_waves;                            // tasks of the whole rounds
    const uint32_t q_full = t_full == n_tasks64 ? n_q : t_full * 64u;
    uint32_t tail_q = (((n_q - q_full) + n_waves - 1u) / n_waves + 7u) / 8u * 8u;   // (at most 64: the tail is less than a round)
    tail_q = tail_q < 16u ? 16u : (tail_q > 64u ? 64u : tail_q);
    return TaskDeal{rounds * W, tail_q};
}
// Entry n of block b's queue -> queries [q0, q0 + nq).  nq = 0: nothing there, and nothing at any later n either (the pieces
// ascend with n) — the claiming wave is done.  (The last whole-round task is cut at n_q: when the 64-query tasks fill the
// rounds exactly, the last of them may be a partial one.)
__host__ __device__ inline void task_of_claim(uint32_t n, uint32_t b, uint32_t n_blocks, uint32_t W, uint32_t n_q, TaskDeal d,
                                              uint32_t& q0, uint32_t& nq) {
    if (n < d.own) {
        q0 = ((n / W) * (n_blocks * W) + b * W + n % W) * 64u;
        nq = n_q - q0 < 64u ? n_q - q0 : 64u;
        return;
    }
    const uint32_t p = n - d.own;                                        // the piece wave b W + p of a strided deal would take
    const uint64_t q_full = (uint64_t)d.own * n_blocks * 64u < n_q ? (uint64_t)d.own * n_blocks * 64u : n_q;
    const uint64_t p0 = q_full + (uint64_t)(b * W + p) * d.tail_q;
    q0 = p < W && p0 < n_q ? (uint32_t)p0 : n_q;
    nq = n_q - q0 < d.tail_q ? n_q - q0 : d.tail_q;
}

// launch wrapper implemented in consensus_kernel.hip
// worklist: n_queries uint32 slots; work_count: {queue length, blocks done}, zero between runs (the worklist kernel
// leaves them so)
// kind_dev: device address of a pinned host word the run's classification goes to (may be null); known_kind: 1 / 2 = launch
// the stream kernel with / without the bit-score ring alone, anything else = classify on the device and launch both
int launch_consensus(const TaxDev& tax, const HitsDev& hits, int strategy, blu_result* out, void* stream,
                     int device, int num_cus, uint32_t* worklist, uint32_t* work_count, uint32_t* kind_dev, uint32_t known_kind);
const char* consensus_kernel_name();
void consensus_last_geometry(uint32_t* grid, uint32_t* block);

// report_kernel.hip: the taxon abundance report of one run's records (device pointers; blu_consensus_report stages host ones).
// The engine row of record q is row_src[idx * row_stride], idx = its ref_row (< n_rows), or q itself when by_query.
struct ReportInput {
    const blu_result* recs;
    uint64_t n_queries;
    const uint32_t* row_src;
    uint64_t n_rows;
    uint32_t row_stride;
    bool by_query;
    const uint32_t* weight;   // [n_queries] or null
};
int report_device(const blu_taxonomy* tax, const ReportInput& in, blu_report* out);
// the per-sample table of the same records: sample_of[n_queries] on the device
int sample_table_device(const blu_taxonomy* tax, const ReportInput& in, const uint32_t* sample_of, uint32_t n_samples,
                        blu_sample_table* out);
// the per-sample table of the same records from count rows (blu_count_rows on the device, nnz = row_ptr[n_queries] as the
// caller read it); in.weight is not read
struct CountRows {
    const uint64_t* row_ptr;
    const uint32_t* sample;
    const uint32_t* count;
    uint64_t nnz;
};
int sample_table_counts_device(const blu_taxonomy* tax, const ReportInput& in, const CountRows& rows, uint32_t n_samples,
                               blu_sample_table* out);

// support_kernel.hip: the per-query support counts of one run's records (device pointers, d_out too; blu_consensus_support
// stages host ones).  The engine row of hit i is row_src[i * row_stride].  Returns when d_out is complete.
struct SupportInput {
    const blu_result* recs;
    uint64_t n_queries;
    const uint64_t* seg_off;
    const int32_t* bitscore;
    const uint32_t* row_src;
    uint32_t row_stride;
    uint64_t n_hits;
};
int support_device(const blu_taxonomy* tax, const SupportInput& in, blu_support* d_out);

// band_kernel.hip: the bit-score band on a device column (device pointers; blu_hits_score_band stages host ones).  d_out == d_in
// is the in-place call.  Runs on `stream` and returns when d_out and the two counts are complete.  The device is the current one.
#define BLU_BAND_QUERIES_PER_WAVE 4u   // consecutive queries of one wave; four waves a block
// a band's arguments: BLU_ERR_INVALID_ARG (and the message) for unknown mask bits, top_percent_milli > 100000 or top_bits >= 2^32;
// a null band is fine.  The one set of refusals of blu_hits_score_band and of the pipeline's entry points.
int check_score_band(const blu_score_band* band);
int score_band_device(const int32_t* d_in, const uint64_t* d_seg_off, uint64_t n_hits, uint64_t n_queries, const blu_score_band& band,
                      hipStream_t stream, int32_t* d_out, uint64_t* n_raised, uint64_t* n_widened);

// hit_pass.hip: what the passes below share (hit_pass.h has the rest: device inlines, the long-query list, the staging).
// The five columns of a table and its offsets; a column is named by the address of its pointer, which a rotation replaces.
struct HitColumns { int32_t** bitscore; int32_t** align_len; uint32_t** tax_desc_row; uint32_t** acc_rank; double** pident; unsigned long long* seg_off; };
// the columns the GPU ingest left on the device (ingest.h)
struct DeviceHits;
HitColumns columns_of(DeviceHits& dev);
// BLU_ERR_INVALID_ARG ("<what>: n_hits must be below 2^32", or n_queries) for a count of 2^32 or more
int check_hit_counts(const char* what, uint64_t n_hits, uint64_t n_queries);
// hipSetDevice; BLU_ERR_NO_DEVICE and "<who>: hipSetDevice(<device>) failed" when it fails (HIP's last error is cleared)
int use_device(const char* who, int device);
// The compaction for any pass that gives verdicts in this form: d_keep[n_hits + 1] = 1 / 0 per row and a last word 0 -> the scan of
// the keep words, the five gathers, seg_off rewritten, the unmatched rows (tax_desc_row == the marker; n_unmatched may be null)
// recounted.  rotate: each column is its own hipMalloc allocation and may be replaced -- the compacted column takes the spare buffer,
// the column's old buffer becomes the next spare and the last one is pushed to *retired (null: freed); else the kept rows are copied
// back to the front of the same buffers.  all_kept (or n_hits == 0): nothing moves and d_keep is not read, only *n_unmatched is
// counted.  `who` names the pass in messages.  Null stream of the current device; returns when its outputs are complete.
int compact_kept_device(const char* who, HitColumns& c, uint64_t n_hits, uint64_t n_queries, const uint32_t* d_keep, bool all_kept, bool rotate,
                        uint32_t unmatched_marker, uint64_t* n_hits_out, uint64_t* n_unmatched, std::vector<void*>* retired);

// subject_kernel.hip: the best hit per subject on device columns (device pointers; blu_hits_subject_keep / blu_hits_subject_best stage
// host ones).  Everything runs on the null stream of the current device and the calls return when their outputs are complete.
#define BLU_SUBJECT_QUERIES_PER_WAVE 4u   // consecutive queries of one wave in the short kernel; four waves a block
// BLU_ERR_INVALID_ARG (and the message) for unknown mask bits; a null selection is fine
int check_subject_best(const blu_subject_best* sel);
// the verdicts: d_keep[n_hits] = 1 / 0
int subject_keep_device(const int32_t* d_bitscore, const uint32_t* d_acc_rank, const uint64_t* d_seg_off, uint64_t n_hits, uint64_t n_queries,
                        uint32_t* d_keep, uint64_t* n_kept, uint64_t* n_thinned);
// the verdicts and the compaction (compact_kept_device, above).  count_only: no pass, only *n_unmatched is counted
int subject_best_device(HitColumns& c, uint64_t n_hits, uint64_t n_queries, bool rotate, uint32_t unmatched_marker,
                        uint64_t* n_hits_out, uint64_t* n_unmatched, uint64_t* n_thinned, std::vector<void*>* retired, bool count_only);
// the same on the columns the GPU ingest left on the device: compacted by rotation, the retired buffer goes to its trash, n_hits
// shrinks and seg_off is rewritten in place; *unmatched: the kept rows with no taxonomy row
int subject_best_hits(DeviceHits& dev, blu_subject_best_stats* stats, uint64_t* unmatched);

// cover_kernel.hip: the minimum cover on device columns (device pointers; blu_hits_cover_keep / blu_hits_cover_apply stage host
// ones).  Everything runs on the null stream of the current device — the taxonomy's — and the calls return when
// their outputs are complete.
#define BLU_COVER_QUERIES_PER_WAVE 4u     // consecutive queries of one wave in the short kernel; four waves a block
// BLU_ERR_INVALID_ARG (and a message that says "min cover") for a value outside 50001 .. 100000
int check_min_cover(int64_t min_cover_milli);
// the verdicts: d_keep[n_hits] = 1 / 0, d_depth[n_queries] (may be null) = d*, BLU_NONE_U8 for a query left alone.  d_tax_row holds
// engine row ids, or desc rows when d_row_map[n_tax] is given
int cover_keep_device(const blu_taxonomy* tax, const int32_t* d_bitscore, const uint32_t* d_tax_row, const uint32_t* d_row_map,
                      const uint64_t* d_seg_off, uint64_t n_hits, uint64_t n_queries, uint32_t min_cover_milli, uint32_t* d_keep,
                      uint8_t* d_depth, blu_min_cover_stats* stats);
// the verdicts and the compaction
int cover_apply_device(const blu_taxonomy* tax, HitColumns& c, const uint32_t* d_row_map, uint64_t n_hits, uint64_t n_queries,
                       uint32_t min_cover_milli, bool rotate, uint32_t unmatched_marker, uint64_t* n_hits_out, uint64_t* n_unmatched,
                       blu_min_cover_stats* stats, std::vector<void*>* retired);
// the same on the columns the GPU ingest left on the device, which hold desc rows: fwd[n_tax] (host; blu_taxonomy_row_map's forward
// table) goes up once; compacted by rotation as subject_best_hits does
int cover_hits(const blu_taxonomy* tax, DeviceHits& dev, const uint32_t* fwd, uint64_t n_tax, uint32_t min_cover_milli,
               blu_min_cover_stats* stats, uint64_t* unmatched);

void set_error(const char* fmt, ...);
// LinnaeanRank::from_str (linnaean_ranks.rs:52-72): enum kind 0..8, or K_FIRST_OTHER with the slug in *other
uint16_t parse_rank(const char* name, std::string* other);

}  // namespace blu

struct blu_taxonomy {
    int device = -1;
    int num_cus = 0;
    uint64_t n_tax = 0;
    uint32_t stride = 16;
    uint32_t sc = 16;
    uint32_t max_depth = 0;
    blu_cutoff_config cfg{};
    std::vector<blu::RankInfo> ranks;        // by canonical code
    std::vector<uint32_t> h_lin;             // host copy of the lineage rows
    std::vector<double> h_cut;               // [n_shapes * sc]
    std::vector<uint32_t> h_codes;           // [n_shapes * sc]
    std::vector<uint8_t> h_isdef;            // [n_shapes * sc]
    uint32_t n_shapes = 0;
    std::unordered_map<int64_t, uint32_t> taxid_row;
    unsigned char* d_block = nullptr;   // ONE device allocation; the table pointers below are views into it (a hipFree each cost 1.5-2 ms)
    uint32_t* d_lin = nullptr;
    std::vector<uint32_t> order;             // engine row id -> desc row
    uint8_t* d_lcp8 = nullptr;
    uint8_t* d_rmq = nullptr;
    uint32_t rmq_nb = 0;
    uint2* d_wblk = nullptr;                 // wide-group tables (TaxDev::wblk, wchain, wchain_hi); null = not built
    uint32_t* d_wchain = nullptr;
    uint32_t* d_wchain_hi = nullptr;
    uint32_t wide_levels = 0;
    uint32_t n_wide = 0;
    std::vector<uint8_t> h_lcp8;             // host copies of the span tables (blu_taxonomy_shared_levels: the tests' view of them)
    std::vector<uint8_t> h_rmq;
    std::vector<uint2> h_wblk;
    std::vector<uint32_t> h_wchain, h_wchain_hi;
    std::vector<uint32_t> pos_of;            // caller's tax_row -> sorted position
    std::vector<uint16_t> hint_of_pos;       // sorted position -> shape hint of the packed layout (shape id + 1, 0 = none)
    uint16_t* d_hint_of_pos = nullptr;
    double* d_cutvals = nullptr;
    uint32_t* d_codes = nullptr;
    uint32_t* d_kthr = nullptr;
    uint32_t n_cutvals = 0;
    uint32_t dev_stride = 32;                // words per DEVICE row
    uint32_t node_base = 1;                  // see TaxDev
    uint64_t device_bytes = 0;
    // per-handle scratch of the run call (worklist of long / overflowing queries); grown on demand,
    // so one handle must not be used by two concurrent blu_consensus_run calls
    mutable uint32_t* ws_worklist = nullptr;
    mutable uint32_t* ws_count = nullptr;
    mutable uint64_t ws_capacity = 0;
    mutable uint32_t* ws_pack_flag = nullptr;        // blu_hits_pack's "a value does not fit the record" word
    // which stream kernel the handle's last table wanted (consensus_kernel.hip: blu_classify_tasks): a pinned host word the
    // device writes, its device address, and the number of run calls so far
    mutable uint32_t* ws_kind_host = nullptr;
    mutable uint32_t* ws_kind_dev = nullptr;
    mutable uint64_t ws_calls = 0;
    // the table the remembered kind and queue length belong to: the pointers of its offsets, bit-scores and side values, its query
    // and row counts (a caching allocator hands the same offsets address to the next table of the same size: all five must agree)
    mutable const void* ws_kind_key_ptr[3] = {nullptr, nullptr, nullptr};
    mutable uint64_t ws_kind_key_n[2] = {0, 0};
    // Staging buffers of the host-pointer path of blu_consensus_run (two sets: a table staged in chunks is double-buffered),
    // kept with the handle and grown on demand instead of seven hipMalloc / hipFree pairs per call; [k][slot]: slot 0 bit-scores,
    // 1 side values (records, or the perc_identity column), 2 tax rows, 3 align_length, 4 accession ranks, 5 offsets, 6 records out
    mutable void* ws_stage[2][7] = {{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}};
    mutable size_t ws_stage_bytes[2][7] = {{0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0}};
};
