// hj_host.h -- what the parts of the C ABI's host layer (hj_api*.hip) share: the context with its state grouped by
// lifetime, its device buffers and events, the call records behind the *_info entry points, and the few helpers every
// part uses. Private to csrc/: nothing in here is part of include/htm_hashjoin.h.
#pragma once

#include "../../include/htm_hashjoin.h"
#include "hj_common.h"
#include "hj_table.h"
#include "hj_pairs.h"
#include "hj_columns.h"
#include "hj_prj.h"
#include "hj_rand.h"

#include <string>

namespace hjapi {
using namespace hj;

enum Ev { EV_CLEAR0, EV_BUILD0, EV_BUILD1, EV_KW0, EV_KW1, EV_KC0, EV_KC1, EV_KO0, EV_KO1, EV_PROBE0, EV_PROBE1, EV_PRJ0, EV_PRJ_PART, EV_PRJ1, EV_PRJ_S0, EV_PRJ_S1, EV_RP0, EV_RP_PART, EV_RP_JOIN0, EV_RP1, EV_COUNT };
// every device buffer the library owns (hj_ctx::buf)
enum Buf {
    B_CTR, B_TABLE,
    B_OWNER, B_QUEUE,           // ownership build (variant 2) / deferred queue of variants 2 and 3
    B_QUEUE_COUNT,              // kOwnMaxChunks words, deferred tuples per phase-A workgroup of the window build
    B_FIT,                      // kSampleWords words (launch_sample_locality)
    B_BOUNDS,                   // variant 3: per-chunk slot ranges (wave_bounds_bytes)
    B_HTM_CONFLICTS, B_HTM_OWN_COUNTS,          // htm: conflicts listed per chunk; their counts in the window build
    B_HTM_OVF_COUNT, B_HTM_OVF_BASE, B_HTM_SCAN,
    B_HTM_OVERFLOW,             // overflow buckets (index 0 unused)
    B_CALL_WORDS,               // the counter words of the last call of every kind: one block per Call (call_words, below)
    B_R_MARKS,                  // HJ_FLAG_TRACK_R_MATCHES: one bit per R row (RMarks, hj_pairs.h)
    B_R_SWEEP,                  // ... and the sweep's block counts, their total and its scan workspace (r_sweep_count_words)
    B_GATHER2_WORK,             // hj_gather2_dev: the workspace of its variable-length columns (gather2_work_words(nRows)), grown by the call
    B_MARK_SWEEP,               // hj_mark_rows_dev: the sweep's workspace for a caller's plane (r_sweep_count_words(rows))
    B_AGG,                      // hj_prj_agg_begin: 256 bytes of words (the matches of the last hj_prj_probe_agg_dev), then the match-count
                                // plane and HJ_AGG_MAX_COLS accumulator planes of 8 bytes per R tuple, in resident order (agg_planes)
    B_GROUPS_WORK,              // hj_key_groups_dev: its workspace (key_groups_work_bytes(nRows): the table, the first-row plane, the ranks, the sweep's counts), grown by the call
    B_SORT_WORK,                // hj_sort_rows_dev: its workspace (sort_layout(nRows, key bytes).bytes: two key planes, two row planes, the histogram, the scan sums), grown by the call
    B_WINDOW_WORK,              // hj_window_rows_dev: its workspace (window_layout(nPos).bytes: the head bytes, the end plane, the chunk summaries), grown by the call
    B_FRAMES_WORK,              // hj_window_frames_dev: its workspace (frames_layout(nPos).bytes: the head bytes, the end plane, two 8-byte planes, the chunk summaries), grown by the call
    B_RANGE_WORK,               // hj_range_pairs_dev: its workspace (range_layout(rRows, sRows).bytes: the pivots, the bound planes, the chunk words, the difference plane), grown by the call
    B_TMP, B_PART_R, B_PART_S, B_WORK,          // PRJ workspace
    B_PRJ_RES,                  // resident R: its final offsets / fragment counts and the work-item list (prj_resident_carve)
    B_STAGE_R, B_STAGE_S,       // staging for hj_run
    B_SHARD0, B_SHARD1, B_SHARD2, B_SHARD3,     // work buffer of hj_ctx::shards.plan[i]
    B_COUNT
};

// One device buffer; the capacity is in bytes, always.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    template <typename T> T* as() const { return static_cast<T*>(p); }
    // at least `need` bytes. A buffer that is too small is freed and allocated anew: its content is lost, and *replaced
    // is set (left alone otherwise)
    int reserve(hj_ctx* c, size_t need, bool* replaced = nullptr);
};

// The last call of one kind, as its *_info entry point reports it (call_info, hj_api_rows.hip): what the caller asked for,
// the few words the host knows about how the call cut its input (extra), and the pair of events around the call's work.
// `called` and `timed` die separately: see hj_ctx::call. What the DEVICE counts during the call lies in the kind's block of
// buf[B_CALL_WORDS] (call_words): kCallWords 64-bit words = 128 bytes, one L2 line, so the atomics of two kinds never meet
// in one line. The words of a block, from word 0:
//   CALL_PAIRS                  the output cursor (= rows found), HJ_JOIN_LEFT's unmatched S tuples
//   CALL_GATHER                 the NULL rows, the out-of-range entries
//   CALL_GATHER2                the same two, then HJ_GATHER_MAX_COLS totals: the bytes of each column
//   CALL_VERIFY, _WHERE, _ASOF  the output cursor (= pairs kept), the pairs dropped unread
//   CALL_PAIRS_AGG              the pairs applied, the pairs skipped
//   CALL_GROUPS                 probe steps, word collisions, NULL-keyed rows, the failure word
//   CALL_WINDOW                 partitions, peer runs, skipped entries
//   CALL_FRAMES                 partitions, 0, skipped entries
//   CALL_RANGE                  pairs (64 bits, exact), S rows with a pair, S rows with a NULL or NaN bound, rows indexed
// CALL_R_ROWS, CALL_MARK_ROWS and CALL_GROUPS find their total in their sweep's workspace, CALL_PRJ_AGG its words in front of
// buf[B_AGG], CALL_SORT counts nothing on the device, CALL_RANGE_INDEX leaves its counts in the caller's dHead (extra[0]).
enum Call { CALL_PAIRS, CALL_R_ROWS, CALL_GATHER, CALL_GATHER2, CALL_VERIFY, CALL_WHERE, CALL_ASOF, CALL_MARK_ROWS, CALL_PRJ_AGG, CALL_PAIRS_AGG, CALL_GROUPS, CALL_SORT, CALL_WINDOW, CALL_RANGE_INDEX, CALL_RANGE, CALL_FRAMES, CALL_COUNT };
struct CallRecord {
    bool called = false, timed = false;
    uint64_t capacity = 0, rows = 0;            // rows: the call's S tuples (pairs), map rows (gather), plane rows (mark rows)
    uint32_t kind = 0;                          // pairs: the hj_join_kind
    uint64_t extra[4] = {0, 0, 0, 0};           // sort: passes, chunks, chunkRows, workspace bytes; window and frames: chunks, workspace bytes
    hipEvent_t ev[2] = {nullptr, nullptr};      // the first in front of the call's work, the second (call_end) behind it
};
constexpr uint32_t kCallWords = 16;
static_assert(2 + HJ_GATHER_MAX_COLS <= kCallWords, "the largest user of a block is hj_gather2_dev: two counts and a total per column");

// pinned host words the device copies into: the locality sampler's answer (sample_variant; hj_join_dev reads fit[0..1]
// after it) and, apart from it, the overflow buckets the LDS chain phase of build_htm asks for
struct Pinned { unsigned int fit[8]; unsigned int chainGroups; };
}  // namespace hjapi

struct hj_ctx {
    // ---- for the context's life (create_common .. hj_destroy); params, plan and prjMaxSlice are hj_reserve's
    int device = 0;
    int nCU = 256;                // of THIS context's device (grids are sized per context, never from process statics)
    hipStream_t stream = nullptr;
    bool ownStream = false;
    hj_params params{};
    hjapi::DevBuf buf[hjapi::B_COUNT];          // hj_destroy frees exactly these
    hj::Counters* dCtr() const { return buf[hjapi::B_CTR].as<hj::Counters>(); }   // the counters: allocated at creation, used by every call
    hj::Counters* hCtr = nullptr;               // pinned copy of the counters
    hjapi::Pinned* pin = nullptr;
    unsigned long long* hPreferred = nullptr;   // pinned: Counters::preferred of the last device-side pick (0: none yet)
    unsigned long long* dPreferred = nullptr;   // the same word as the device addresses it (the sampler stores into it)
    hj::ShardCheck sc{0, 0, 0, 0};              // hj_set_shard_check; mask 0 = off
    hj::PrjPlan plan{};
    uint64_t prjMaxSlice = 0;                   // sSize of the last PRJ / AUTO hj_reserve: the largest slice a probe takes
    std::string err;

    // ---- the operation -- a table build with its probes, or a radix join. Reset by begin_operation, which fills in the sizes.
    struct Op {
        uint64_t rSize = 0, sSize = 0;
        uint64_t tableSize = 0;                 // live table (2*rSize; htm: 4 slots per bucket) of the last build, in buf[B_TABLE]
        uint32_t hshift = 0;                    // home-slot shift of that table (hj_common.h); 0 unless it is a radix shard
        uint32_t algoUsed = 0, variantUsed = 1;
        bool built = false;
        bool probeStartsAtBuildEnd = false;     // the probe was enqueued right behind the build on the library's own stream: EV_BUILD1 is its start
        bool streamAtBuildEnd = false;          // nothing has been enqueued since EV_BUILD1 (own stream only)
        // the ring pre-pass of the build (hj_wave_seams): tuples it cut into chunks (0: it was not enqueued), and whether
        // it was gated on the variant the device picked
        uint64_t wavePreN = 0;
        bool wavePreGated = false;
        // the workgroup-window build (hj_own_info): tuples it cut into chunks (0: it was not enqueued, or hj_reserve has
        // replaced the owner table since), and whether it was gated on the variant the device picked
        uint64_t ownN = 0;
        bool ownGated = false;
        // the ring build of this table retires slot codes (kWaveCodes): 0 no, 1 by the size rule, 2 forced by HJ_FLAG_SLOT_CODES
        uint32_t codesRoad = 0;
    } op;
    // ---- the bucketised table of --algo htm (hj_htm.hip; 4 slots per bucket in buf[B_TABLE]). Reset by begin_operation.
    struct Htm {
        bool built = false;
        uint32_t buckets = 0;                   // numBuckets of the build
        bool chainsFellBack = false;            // build_htm went round a second time with the generic chain kernels (hj_result.compactFallback bit 8)
        // the LDS chain phase (hj_htm_chain_info): 0 not tried, 1 held, 2 handed over; the cause mask of a hand-over
        // (Counters::htmChainBail of the first attempt); overflow buckets of the parts
        uint32_t chainState = 0; uint64_t chainCause = 0, chainGroups = 0;
    } htm;
    // ---- R-side match marks (HJ_FLAG_TRACK_R_MATCHES): the plane describes the last build -- hj_build_dev or
    // hj_prj_build_dev -- while `built`; rows base .. base + rows - 1 are bits 0 .. rows - 1. Reset by begin_operation and
    // when hj_reserve replaces the plane (forget_marks, which also forgets call[CALL_R_ROWS]).
    struct Marks { bool built = false; uint64_t rows = 0, base = 0; } marks;
    // ---- the last radix join. Reset by begin_operation.
    struct Prj { bool ran = false, optimistic = false; } prj;       // optimistic: it enqueued the histogram-free passes
    // ---- PRJ with a resident R (hj_prj_build_dev / hj_prj_probe_dev): R's final offsets / fragment counts and the work-item
    // list live in buf[B_PRJ_RES], R's keys in buf[B_PART_R]. Reset by begin_operation and when hj_reserve replaces one of
    // its buffers.
    struct Resident {
        bool on = false;                        // R is partitioned and nothing has replaced it since
        hj::PrjPlan plan{};                     // the plan R was partitioned with (radix bits, R's layout)
        uint64_t nR = 0;
        bool rows = false;                      // R holds {key, row} elements (reserved with HJ_FLAG_KEEP_ROW_IDS)
        bool probeOpt = false;                  // the last probe since the build enqueued the histogram-free passes for its slice
    } res;
    // ---- the aggregation over the resident R (hj_prj_agg_begin .. hj_prj_agg_rows_dev): its columns, the R tuples its planes
    // in buf[B_AGG] hold, the probes since the begin. Reset by begin_operation; worth nothing without res.on.
    struct Agg { bool on = false; uint32_t nCols = 0; uint64_t nR = 0, probes = 0; hj::AggOps ops{}; } agg;
    // ---- the last call of each kind (CallRecord). begin_operation forgets the TIME of the pairs call (its facts stay) and
    // the whole R-rows call, which hj_reserve also forgets with the plane, and it ends the probes of an aggregation. Every
    // other kind -- the calls on rows, row maps and pair lists of hj_api_rows.hip -- belongs to no build and no operation and
    // is never forgotten.
    hjapi::CallRecord call[hjapi::CALL_COUNT];
    // ---- streaming Zipf generator (hj_zipf_open / hj_zipf_next_dev). Reset by zipf_release (open, close, destroy).
    struct Zipf {
        hjhost::GlibcRand* rng = nullptr;
        double* lut = nullptr; uint32_t* alphabet = nullptr; uint32_t alphabetSize = 0;   // device
        int* rawHost[2] = {nullptr, nullptr}; int* rawDev[2] = {nullptr, nullptr}; uint64_t rawCap = 0;
        hipEvent_t done[2] = {nullptr, nullptr}; int flip = 0;
    } zipf;
    // ---- shard helper: up to 4 inputs may sit between their histogram and their scatter (plan[i] works in
    // buf[B_SHARD0 + i]). Never reset: a slot is reused.
    struct ShardPlan { const uint64_t* in = nullptr; uint64_t n = 0; uint32_t nShards = 0, mode = 0; uint64_t stamp = 0; };
    struct Shards { ShardPlan plan[4]; uint64_t stamp = 0; } shards;
    // ---- timing: the events live as long as the context; begin_operation unsets all of them. h2d_us is hj_run's.
    struct Timing { hipEvent_t ev[hjapi::EV_COUNT]{}; bool set[hjapi::EV_COUNT]{}; double h2d_us = 0; } time;
};

namespace hjapi {

inline int fail(hj_ctx* c, int code, const char* what, hipError_t e = hipSuccess)
{
    if (c) c->err = e == hipSuccess ? std::string(what) : std::string(what) + ": " + hipGetErrorString(e);
    return code;
}

// "fn: what", for the checks that serve several entry points
inline int fail(hj_ctx* c, int code, const char* fn, const char* what) { return fail(c, code, (std::string(fn) + ": " + what).c_str()); }

#define HJ_HIP(c, call)                                                     \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess)                                               \
            return fail((c), e_ == hipErrorOutOfMemory ? HJ_ERR_OOM : HJ_ERR_HIP, #call, e_); \
    } while (0)

// Every entry point that may enqueue work: the stream then no longer ends at EV_BUILD1 -- noted even when the arguments
// are rejected next. (hj_probe_dev takes the value over first, see there.)
#define HJ_ENTER(c, argsOk)                                   \
    do {                                                      \
        if (c) (c)->op.streamAtBuildEnd = false;              \
        if (!(c) || !(argsOk)) return HJ_ERR_INVALID;         \
    } while (0)

// the counter block of the last call of kind `which` (allocated and zeroed at creation)
inline unsigned long long* call_words(const hj_ctx* c, Call which) { return c->buf[B_CALL_WORDS].as<unsigned long long>() + (size_t)which * kCallWords; }

// hj_key_hash*_dev, hj_key_groups_dev and their host twins: a keyMask of 0 means every bit
inline uint32_t effective_mask(uint32_t keyMask) { return keyMask ? keyMask : 0xFFFFFFFFu; }

inline bool is_pow2(uint64_t v) { return v && !(v & (v - 1)); }
inline uint32_t probe_len(const hj_params& p) { return p.probeLength ? p.probeLength : 4; }

inline int DevBuf::reserve(hj_ctx* c, size_t need, bool* replaced)
{
    if (need <= bytes) return HJ_OK;
    if (replaced) *replaced = true;
    if (p) {
        // work enqueued earlier may still use the old buffer (hipFree waits for the device anyway: written out so that
        // no caller has to think about it)
        HJ_HIP(c, hipStreamSynchronize(c->stream));
        HJ_HIP(c, hipFree(p));
        p = nullptr; bytes = 0;
    }
    HJ_HIP(c, hipMalloc(&p, need));
    bytes = need;
    return HJ_OK;
}

inline uint32_t auto_radix_bits(uint64_t nR)
{
    // >= NUM_RADIX_BITS (prj_params.h:16) and enough that an average R partition
    // fills at most half of the LDS table; two passes of <= 8 bits
    uint32_t bits = 14;
    while (bits < 16 && (nR >> bits) > 16384) ++bits;
    return bits;
}

inline int record(hj_ctx* c, Ev e)
{
    HJ_HIP(c, hipEventRecord(c->time.ev[e], c->stream));
    c->time.set[e] = true;
    return HJ_OK;
}

inline double elapsed_us(hj_ctx* c, Ev a, Ev b)
{
    if (!c->time.set[a] || !c->time.set[b]) return 0.0;
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->time.ev[a], c->time.ev[b]) != hipSuccess) return 0.0;
    return (double)ms * 1000.0;
}

// The pair of events a launcher records around its dominant kernel, marked as set where it is handed over
inline KernelEvents bracket(hj_ctx* c, Ev before)
{
    c->time.set[before] = c->time.set[before + 1] = true;
    return KernelEvents{c->time.ev[before], c->time.ev[before + 1]};
}

// behind the work of a call that has a record: its second event, and what its *_info is to report
inline int call_end(hj_ctx* c, Call which, uint64_t capacity, uint64_t rows, uint32_t kind = 0)
{
    CallRecord& r = c->call[which];
    HJ_HIP(c, hipEventRecord(r.ev[1], c->stream));
    r.called = r.timed = true;
    r.capacity = capacity; r.rows = rows; r.kind = kind;
    return HJ_OK;
}

// the marks plane describes no build any more (and the rows of the last sweep were those of that build)
inline void forget_marks(hj_ctx* c) { c->marks = {}; c->call[CALL_R_ROWS].called = false; }

// A new operation (a build or a whole radix join) starts: nothing of the last one is timed, built or resident any more,
// and the counters are zeroed on the stream. What the operation builds it flags at its end, once everything is enqueued.
inline int begin_operation(hj_ctx* c, uint64_t rSize, uint64_t sSize, uint64_t tableSize)
{
    HJ_HIP(c, hipSetDevice(c->device));
    for (bool& set : c->time.set) set = false;
    c->op = {}; c->htm = {}; c->prj = {}; c->res = {}; c->agg = {};
    forget_marks(c);
    c->call[CALL_PAIRS].timed = false;          // hj_pairs_info keeps the call's facts and reports no time
    c->call[CALL_PRJ_AGG].called = false;       // the probes of an aggregation end with it
    c->op.rSize = rSize; c->op.sSize = sSize; c->op.tableSize = tableSize;
    HJ_HIP(c, hipMemsetAsync(c->dCtr(), 0, sizeof(Counters), c->stream));
    return HJ_OK;
}

// Which LDS builds a table of tableSize slots for n elements can take: 2 (own), 3 (wave) and 4 (compact) need their
// buffers (hj_reserve) and a table of at least one window / ring.
// 4 = the compact ring build (4-byte table, hj_build_wave.hip): what "rings" means whenever it can be tried; if it meets
// something it cannot handle, the classic ring build (3) enqueued behind it, gated on the device, redoes the table.
struct BuildCaps { bool own, wave, compact; };
inline BuildCaps build_caps(const hj_ctx* c, uint64_t n, uint64_t tableSize)
{
    BuildCaps k;
    k.own = n && own_supported(tableSize) && c->buf[B_OWNER].bytes >= own_owner_bytes(tableSize) &&
            c->buf[B_QUEUE].bytes >= own_queue_bytes(n);
    k.wave = n && wave_supported(tableSize) && c->buf[B_QUEUE].bytes >= wave_queue_bytes(n, c->nCU);
    // HJ_FLAG_KEEP_ROW_IDS: the compact table drops the index words hj_probe_pairs_dev reads -- never tried, never picked
    k.compact = k.wave && wave_compact_supported(tableSize, probe_len(c->params)) && !(c->params.flags & HJ_FLAG_KEEP_ROW_IDS);
    return k;
}

// The build kernel a request for `variant` ends up with when the context cannot run it: 4 without the compact rings ->
// the classic ones, 3 without rings -> the window or global atomics, 2 without the window -> global atomics; 0 (the
// locality pre-round picks) stays 0 only while there is an LDS build to pick.
inline uint32_t settle_variant(uint32_t variant, const BuildCaps& can)
{
    if (variant == 4 && !can.compact) variant = 3;
    if (variant == 3 && !can.wave) variant = can.own ? 2 : 1;
    if (variant == 2 && !can.own) variant = 1;
    if (variant == 0 && !can.own && !can.wave) variant = 1;
    return variant;
}

// The counters as they are once the stream has drained, in c->hCtr; fold: with the shards added into the totals
// (fold_counter_shards), for the callers that read a sum
inline int read_counters(hj_ctx* c, bool fold)
{
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipMemcpyAsync(c->hCtr, c->dCtr(), sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    if (fold) fold_counter_shards(c->hCtr);
    return HJ_OK;
}

// ---- R-side match marks at a build (hj_build_dev / hj_prj_build_dev) of a context reserved with HJ_FLAG_TRACK_R_MATCHES:
// marks_begin checks that the plane takes rSize rows and zeroes it on the stream, marks_built -- once the build is
// enqueued -- says what the plane now describes. Neither does anything on a context without the flag.
inline bool tracks(const hj_ctx* c) { return (c->params.flags & HJ_FLAG_TRACK_R_MATCHES) != 0; }
inline size_t marks_bytes(uint64_t rows) { return (size_t)((rows + 31) / 32) * sizeof(uint32_t); }
inline int marks_begin(hj_ctx* c, const char* fn, uint64_t rSize)
{
    if (!tracks(c)) return HJ_OK;
    if (marks_bytes(rSize) > c->buf[B_R_MARKS].bytes || r_sweep_count_words(rSize) * sizeof(uint32_t) > c->buf[B_R_SWEEP].bytes)
        return fail(c, HJ_ERR_STATE, fn, "hj_reserve() not called for this rSize (match marks)");
    HJ_HIP(c, hipSetDevice(c->device));
    c->op.streamAtBuildEnd = false;
    HJ_HIP(c, hipMemsetAsync(c->buf[B_R_MARKS].p, 0, marks_bytes(rSize), c->stream));
    return HJ_OK;
}
inline void marks_built(hj_ctx* c, uint64_t rSize, uint64_t idxBase)
{
    if (!tracks(c)) return;
    forget_marks(c);
    c->marks.built = true; c->marks.rows = rSize; c->marks.base = idxBase;
}
// the marks a materialising probe of `kind` sets: none unless the context tracks, the plane describes the table or the
// resident R being probed, and the kind produces R rows
inline bool marks_for(const hj_ctx* c, uint32_t kind, RMarks* mk)
{
    if (!tracks(c) || !c->marks.built || kind > HJ_JOIN_LEFT) return false;
    *mk = RMarks{c->buf[B_R_MARKS].as<uint32_t>(), (uint32_t)c->marks.base, (uint32_t)c->marks.rows};
    return true;
}

// What both materialising probes check of their arguments (fn: the entry point's name, for the texts). `state`: the probe's own
// call-order error or nullptr, ranking behind a bad kind. *planeR: the kind writes R rows (SEMI and ANTI ignore dOutR)
inline int pairs_args(hj_ctx* c, const char* fn, uint32_t kind, const char* state, uint64_t sSize, uint64_t sIdxBase,
                      const uint32_t* dOutS, const uint32_t* dOutR, uint64_t capacity, bool* planeR)
{
    if (kind > HJ_JOIN_ANTI) return fail(c, HJ_ERR_INVALID, fn, "kind must be an hj_join_kind");
    *planeR = kind <= HJ_JOIN_LEFT;
    if (state) return fail(c, HJ_ERR_STATE, fn, state);
    if (capacity && (!dOutS || (*planeR && !dOutR))) return fail(c, HJ_ERR_INVALID, fn, "output pointer NULL with capacity > 0");
    if (sIdxBase > 0xFFFFFFFFull || sIdxBase + sSize > 0xFFFFFFFFull) return fail(c, HJ_ERR_INVALID, fn, "S row range exceeds 2^32 - 1");
    return HJ_OK;
}

// the planes of an aggregation over nR resident tuples, carved from buf[B_AGG]
inline size_t agg_bytes(uint64_t nR, uint32_t nCols) { return 256 + (size_t)(1 + nCols) * nR * sizeof(unsigned long long); }
inline AggPlanes agg_planes(const hj_ctx* c)
{
    unsigned long long* const base = reinterpret_cast<unsigned long long*>(c->buf[B_AGG].as<char>() + 256);
    AggPlanes pl{};
    pl.count = base;
    for (uint32_t i = 0; i < c->agg.nCols; ++i) pl.acc[i] = base + (size_t)(1 + i) * c->agg.nR;
    return pl;
}

// ---- defined in one part, used by another. hj_api_table.hip: the locality pre-round read back on the host (c->pin->fit),
// and hj_build_dev with the build kernel as an argument (0: hj_params.buildVariant decides); hj_api_tools.hip: zipf_release
int sample_variant(hj_ctx* c, const void* d, bool key32, uint64_t n, uint64_t tableSize, uint32_t hshift, const BuildCaps& can,
                   uint32_t* variant, bool htm = false);
int build_table(hj_ctx* c, const uint64_t* dR, uint64_t rSize, uint64_t idxBase, uint32_t forceVariant);
void zipf_release(hj_ctx* c);

}  // namespace hjapi
