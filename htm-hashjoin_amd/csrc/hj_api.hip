// hj_api.hip -- implementation of the C ABI in include/htm_hashjoin.h.
// Host-side glue only: argument checks, device memory, stream order, HIP-event
// timing. All arithmetic on tuples happens in hj_kernels.hip / hj_prj.hip.
// There is no CPU fallback in here: every operator needs a gfx950 device.

#include "../../include/htm_hashjoin.h"
#include "hj_device.h"
#include "hj_rand.h"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace hj;

namespace {
enum Ev { EV_CLEAR0, EV_BUILD0, EV_BUILD1, EV_KW0, EV_KW1, EV_KC0, EV_KC1, EV_KO0, EV_KO1, EV_PROBE0, EV_PROBE1, EV_PRJ0, EV_PRJ_PART, EV_PRJ1, EV_PRJ_S0, EV_PRJ_S1, EV_RP0, EV_RP_PART, EV_RP_JOIN0, EV_RP1, EV_PAIRS0, EV_PAIRS1, EV_RROWS0, EV_RROWS1, EV_COUNT };
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
    B_PAIRS_CURSOR,             // materialising probe (hj_probe_join_dev): the output cursor, then HJ_JOIN_LEFT's unmatched S tuples
    B_R_MARKS,                  // HJ_FLAG_TRACK_R_MATCHES: one bit per R row (RMarks, hj_device.h)
    B_R_SWEEP,                  // ... and the sweep's block counts, their total and its scan workspace (r_sweep_count_words)
    B_GATHER_CTR,               // hj_gather_dev: the NULL rows and the out-of-range entries of the last call (two 64-bit words)
    B_VERIFY_CTR,               // hj_pairs_verify_dev: the output cursor (= pairs kept), then the candidates dropped (two 64-bit words)
    B_MARK_SWEEP,               // hj_mark_rows_dev: the sweep's workspace for a caller's plane (r_sweep_count_words(rows))
    B_TMP, B_PART_R, B_PART_S, B_WORK,          // PRJ workspace
    B_PRJ_RES,                  // resident R: its final offsets / fragment counts and the work-item list (prj_resident_carve)
    B_STAGE_R, B_STAGE_S,       // staging for hj_run
    B_SHARD0, B_SHARD1, B_SHARD2, B_SHARD3,     // work buffer of hj_ctx::shard[i]
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
}

struct hj_ctx {
    int device = 0;
    int nCU = 256;                // of THIS context's device (grids are sized per context, never from process statics)
    hipStream_t stream = nullptr;
    bool ownStream = false;
    hj_params params{};
    DevBuf buf[B_COUNT];          // hj_destroy frees exactly these
    Counters* dCtr() const { return buf[B_CTR].as<Counters>(); }     // the counters: allocated at creation, used by every call
    // open-addressing table (buf[B_TABLE]: the slots incl. slack)
    uint64_t tableSize = 0;       // live table (2*rSize) of the last build
    uint32_t hshift = 0;             // home-slot shift of the current table (hj_device.h); 0 unless it is a radix shard
    ShardCheck sc{0, 0, 0, 0};       // hj_set_shard_check; mask 0 = off
    uint64_t rSize = 0, sSize = 0;
    bool built = false;
    bool probeStartsAtBuildEnd = false;         // the probe was enqueued right behind the build on the library's own stream: EV_BUILD1 is its start
    bool streamAtBuildEnd = false;              // nothing has been enqueued since EV_BUILD1 (own stream only)
    unsigned int* hFit = nullptr;               // pinned
    unsigned long long* hPreferred = nullptr;   // pinned: Counters::preferred of the last device-side pick (0: none yet)
    unsigned long long* dPreferred = nullptr;   // the same word as the device addresses it (the sampler stores into it)
    // bucketised table of --algo htm (hj_htm.hip): the table itself lives in buf[B_TABLE] (4 slots per bucket)
    bool htmBuilt = false;
    bool htmGenericChains = false;              // build_htm's second attempt: no routing, generic chain kernels
    bool htmChainsFellBack = false;             // ... and that it happened (hj_result.compactFallback bit 8)
    // the LDS chain phase of the last build_htm (hj_htm_chain_info): 0 not tried, 1 held, 2 handed over; the cause mask of a
    // hand-over (Counters::htmChainBail of the first attempt: the second one resets the counters); overflow buckets of the parts
    uint32_t htmChainState = 0;
    uint64_t htmChainCause = 0, htmChainGroups = 0;
    uint32_t htmBuckets = 0;                    // numBuckets of the last htm build
    uint64_t htmOverflowUsed = 0;
    // streaming Zipf generator (hj_zipf_open / hj_zipf_next_dev)
    hjhost::GlibcRand* zipfRng = nullptr;
    double* zipfLut = nullptr; uint32_t* zipfAlphabet = nullptr; uint32_t zipfAlphabetSize = 0;   // device
    int* zipfRawHost[2] = {nullptr, nullptr}; int* zipfRawDev[2] = {nullptr, nullptr}; uint64_t zipfRawCap = 0;
    hipEvent_t zipfDone[2] = {nullptr, nullptr}; int zipfFlip = 0;
    uint32_t variantUsed = 1;
    // the ring pre-pass of the last build (hj_wave_seams): tuples it cut into chunks (0: it was not enqueued), and whether
    // it was gated on the variant the device picked
    uint64_t wavePreN = 0;
    bool wavePreGated = false;
    uint64_t pairsCapacity = 0;                 // materialising probe (hj_probe_join_dev): the capacity of the last call,
    uint32_t pairsKind = HJ_JOIN_INNER;         // ... its join kind and its sSize (hj_pairs_info)
    uint64_t pairsS = 0;
    // R-side match marks (HJ_FLAG_TRACK_R_MATCHES): the plane describes the last build -- hj_build_dev or hj_prj_build_dev on
    // a context reserved with the flag -- while marksBuilt; rows base .. base + rows - 1 are bits 0 .. rows - 1
    bool marksBuilt = false;
    uint64_t marksRows = 0, marksBase = 0;
    bool rRowsCalled = false;                   // hj_r_rows_dev ran since that build; its capacity (hj_r_rows_info)
    uint64_t rRowsCapacity = 0;
    // hj_gather_dev: it belongs to no build and no operation, so its events are its own (begin_operation forgets ev[])
    bool gatherCalled = false;                  // ... ran on this context; the rows of the last call (hj_gather_info)
    uint64_t gatherRows = 0;
    hipEvent_t evGather[2] = {nullptr, nullptr};
    // hj_pairs_verify_dev and hj_mark_rows_dev: like the gather, no part of a build or an operation
    bool verifyCalled = false;                  // ... ran on this context; the capacity of the last call (hj_verify_info)
    uint64_t verifyCapacity = 0;
    hipEvent_t evVerify[2] = {nullptr, nullptr};
    bool markRowsCalled = false;                // the same for hj_mark_rows_dev: its rows and capacity (hj_mark_rows_info)
    uint64_t markRowsRows = 0, markRowsCapacity = 0;
    hipEvent_t evMarkRows[2] = {nullptr, nullptr};
    Counters* hCtr = nullptr;     // pinned copy of the counters
    // PRJ
    PrjPlan plan{};
    uint32_t forceVariant = 0;                  // hj_join_dev(AUTO) has already sampled: build with this variant
    uint32_t algoUsed = 0;
    bool prjRan = false;
    bool prjOptimistic = false;   // the last radix join enqueued the histogram-free passes
    // PRJ with a resident R (hj_prj_build_dev / hj_prj_probe_dev): R's final offsets / fragment counts and the work-item
    // list live in buf[B_PRJ_RES], R's keys in buf[B_PART_R]
    uint64_t prjMaxSlice = 0;                   // sSize of the last PRJ / AUTO hj_reserve: the largest slice a probe takes
    bool resident = false;                      // R is partitioned and nothing has replaced it since
    PrjPlan resPlan{};                          // the plan R was partitioned with (radix bits, R's layout)
    uint64_t resR = 0;
    bool resRows = false;                       // the resident R holds {key, row} elements (reserved with HJ_FLAG_KEEP_ROW_IDS)
    bool resProbed = false, resProbeOpt = false;   // a probe ran since the build; its slice enqueued the histogram-free passes
    // shard helper: up to 4 inputs may sit between their histogram and their scatter (shard[i] works in buf[B_SHARD0 + i])
    struct ShardPlan { const uint64_t* in = nullptr; uint64_t n = 0; uint32_t nShards = 0, mode = 0; uint64_t stamp = 0; };
    ShardPlan shard[4];
    uint64_t shardStamp = 0;
    // timing
    hipEvent_t ev[EV_COUNT]{};
    bool evSet[EV_COUNT]{};
    double h2d_us = 0;
    std::string err;
};

namespace {

int fail(hj_ctx* c, int code, const char* what, hipError_t e = hipSuccess)
{
    if (c) {
        char buf[512];
        if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
        else snprintf(buf, sizeof buf, "%s", what);
        c->err = buf;
    }
    return code;
}

#define HJ_HIP(c, call)                                                     \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess)                                               \
            return fail((c), e_ == hipErrorOutOfMemory ? HJ_ERR_OOM : HJ_ERR_HIP, #call, e_); \
    } while (0)

bool is_pow2(uint64_t v) { return v && !(v & (v - 1)); }

uint32_t probe_len(const hj_params& p) { return p.probeLength ? p.probeLength : 4; }

int DevBuf::reserve(hj_ctx* c, size_t need, bool* replaced)
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

uint32_t auto_radix_bits(uint64_t nR)
{
    // >= NUM_RADIX_BITS (prj_params.h:16) and enough that an average R partition
    // fills at most half of the LDS table; two passes of <= 8 bits
    uint32_t bits = 14;
    while (bits < 16 && (nR >> bits) > 16384) ++bits;
    return bits;
}

int record(hj_ctx* c, Ev e)
{
    HJ_HIP(c, hipEventRecord(c->ev[e], c->stream));
    c->evSet[e] = true;
    return HJ_OK;
}

double elapsed_us(hj_ctx* c, Ev a, Ev b)
{
    if (!c->evSet[a] || !c->evSet[b]) return 0.0;
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev[a], c->ev[b]) != hipSuccess) return 0.0;
    return (double)ms * 1000.0;
}

// The pair of events a launcher records around its dominant kernel, marked as set where it is handed over
KernelEvents bracket(hj_ctx* c, Ev before)
{
    c->evSet[before] = c->evSet[before + 1] = true;
    return KernelEvents{c->ev[before], c->ev[before + 1]};
}

// Every entry point that may enqueue work: the stream then no longer ends at EV_BUILD1 -- noted even when the arguments
// are rejected next. (hj_probe_dev takes the value over first, see there.)
#define HJ_ENTER(c, argsOk)                                   \
    do {                                                      \
        if (c) (c)->streamAtBuildEnd = false;                 \
        if (!(c) || !(argsOk)) return HJ_ERR_INVALID;         \
    } while (0)

// A new operation (a build or a whole radix join) starts: nothing of the last one is timed, built or resident any more,
// and the counters are zeroed on the stream. What the operation builds it flags at its end, once everything is enqueued.
int begin_operation(hj_ctx* c, uint64_t rSize, uint64_t sSize, uint64_t tableSize)
{
    HJ_HIP(c, hipSetDevice(c->device));
    for (bool& b : c->evSet) b = false;
    c->built = c->htmBuilt = c->prjRan = c->resident = false;
    c->marksBuilt = c->rRowsCalled = false;
    c->wavePreN = 0;
    c->rSize = rSize; c->sSize = sSize; c->tableSize = tableSize;
    HJ_HIP(c, hipMemsetAsync(c->dCtr(), 0, sizeof(Counters), c->stream));
    return HJ_OK;
}

// Which LDS builds a table of tableSize slots for n elements can take: 2 (own), 3 (wave) and 4 (compact) need their
// buffers (hj_reserve) and a table of at least one window / ring.
// 4 = the compact ring build (4-byte table, hj_build_wave.hip): what "rings" means whenever it can be tried; if it meets
// something it cannot handle, the classic ring build (3) enqueued behind it, gated on the device, redoes the table.
struct BuildCaps { bool own, wave, compact; };
BuildCaps build_caps(const hj_ctx* c, uint64_t n, uint64_t tableSize)
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
static uint32_t settle_variant(uint32_t variant, const BuildCaps& can)
{
    if (variant == 4 && !can.compact) variant = 3;
    if (variant == 3 && !can.wave) variant = can.own ? 2 : 1;
    if (variant == 2 && !can.own) variant = 1;
    if (variant == 0 && !can.own && !can.wave) variant = 1;
    return variant;
}

// One build as its launchers see it (hj_device.h): the context's table, counters and stream around the caller's input
static BuildJob build_job(hj_ctx* c, const void* R, bool key32, uint64_t n, uint32_t hshift, uint64_t tableSize, uint32_t probeLen,
                          uint64_t idxBase, ShardCheck sc)
{
    BuildJob job{};
    job.R = R; job.key32 = key32; job.n = n; job.idxBase = idxBase;
    job.table = c->buf[B_TABLE].as<uint64_t>(); job.tableSize = tableSize; job.hshift = hshift; job.probeLen = probeLen; job.sc = sc;
    job.nCU = c->nCU; job.ctr = c->dCtr(); job.s = c->stream;
    return job;
}

// The counters as they are once the stream has drained, in c->hCtr; fold: with the shards added into the totals
// (fold_counter_shards), for the callers that read a sum
static int read_counters(hj_ctx* c, bool fold)
{
    HJ_HIP(c, hipMemcpyAsync(c->hCtr, c->dCtr(), sizeof(Counters), hipMemcpyDeviceToHost, c->stream));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    if (fold) fold_counter_shards(c->hCtr);
    return HJ_OK;
}

int create_common(int device, void* stream, bool own, hj_ctx** out)
{
    if (!out) return HJ_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return HJ_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return HJ_ERR_INVALID;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return HJ_ERR_HIP;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return HJ_ERR_NO_DEVICE;  // kernels are gfx950-only
    if (hipSetDevice(device) != hipSuccess) return HJ_ERR_HIP;
    // the kernels with more than 64 KiB of dynamic LDS need the attribute on EVERY device they run on
    if (own_set_attributes() != hipSuccess || prj_set_attributes() != hipSuccess) return HJ_ERR_HIP;
    hj_ctx* c = new (std::nothrow) hj_ctx();
    if (!c) return HJ_ERR_OOM;
    c->device = device;
    c->nCU = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (own) {
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return HJ_ERR_HIP; }
        c->ownStream = true;
    } else {
        c->stream = static_cast<hipStream_t>(stream);
    }
    bool ok = c->buf[B_CTR].reserve(c, sizeof(Counters)) == HJ_OK &&
              hipHostMalloc(reinterpret_cast<void**>(&c->hCtr), sizeof(Counters)) == hipSuccess &&
              c->buf[B_QUEUE_COUNT].reserve(c, kOwnMaxChunks * sizeof(uint32_t)) == HJ_OK &&
              c->buf[B_FIT].reserve(c, kSampleWords * sizeof(unsigned int)) == HJ_OK &&
              hipHostMalloc(reinterpret_cast<void**>(&c->hFit), 8 * sizeof(unsigned int)) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void**>(&c->hPreferred), sizeof(unsigned long long), hipHostMallocMapped) == hipSuccess &&
              hipHostGetDevicePointer(reinterpret_cast<void**>(&c->dPreferred), c->hPreferred, 0) == hipSuccess &&
              c->buf[B_BOUNDS].reserve(c, wave_bounds_bytes(c->nCU)) == HJ_OK &&
              c->buf[B_PAIRS_CURSOR].reserve(c, 2 * sizeof(unsigned long long)) == HJ_OK &&
              hipMemset(c->buf[B_PAIRS_CURSOR].p, 0, 2 * sizeof(unsigned long long)) == hipSuccess &&
              c->buf[B_GATHER_CTR].reserve(c, 2 * sizeof(unsigned long long)) == HJ_OK &&
              hipEventCreate(&c->evGather[0]) == hipSuccess && hipEventCreate(&c->evGather[1]) == hipSuccess &&
              c->buf[B_VERIFY_CTR].reserve(c, 2 * sizeof(unsigned long long)) == HJ_OK &&
              hipEventCreate(&c->evVerify[0]) == hipSuccess && hipEventCreate(&c->evVerify[1]) == hipSuccess &&
              hipEventCreate(&c->evMarkRows[0]) == hipSuccess && hipEventCreate(&c->evMarkRows[1]) == hipSuccess;
    for (int i = 0; ok && i < EV_COUNT; ++i) ok = hipEventCreate(&c->ev[i]) == hipSuccess;
    if (!ok) { hj_destroy(c); return HJ_ERR_HIP; }
    hipMemset(c->dCtr(), 0, sizeof(Counters));
    memset(c->hCtr, 0, sizeof(Counters));
    *c->hPreferred = 0;
    *out = c;
    return HJ_OK;
}

}  // namespace

extern "C" {

int hj_abi_version(void) { return HJ_ABI_VERSION; }

int hj_device_count(int* count)
{
    if (!count) return HJ_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { *count = 0; return HJ_ERR_NO_DEVICE; }
    *count = n;
    return HJ_OK;
}

int hj_create(int device, hj_ctx** out) { return create_common(device, nullptr, true, out); }

int hj_create_on_stream(int device, void* hip_stream, hj_ctx** out) { return create_common(device, hip_stream, false, out); }

static void zipf_release(hj_ctx* c)
{
    delete c->zipfRng; c->zipfRng = nullptr;
    if (c->zipfLut) hipFree(c->zipfLut);
    if (c->zipfAlphabet) hipFree(c->zipfAlphabet);
    c->zipfLut = nullptr; c->zipfAlphabet = nullptr; c->zipfAlphabetSize = 0;
    for (int i = 0; i < 2; ++i) {
        if (c->zipfRawHost[i]) hipHostFree(c->zipfRawHost[i]);
        if (c->zipfRawDev[i]) hipFree(c->zipfRawDev[i]);
        if (c->zipfDone[i]) hipEventDestroy(c->zipfDone[i]);
        c->zipfRawHost[i] = nullptr; c->zipfRawDev[i] = nullptr; c->zipfDone[i] = nullptr;
    }
    c->zipfRawCap = 0;
}

void hj_destroy(hj_ctx* c)
{
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream || !c->ownStream) hipStreamSynchronize(c->stream);
    zipf_release(c);
    if (c->stream || !c->ownStream) hipStreamSynchronize(c->stream);
    for (const DevBuf& b : c->buf) if (b.p) hipFree(b.p);
    if (c->hCtr) hipHostFree(c->hCtr);
    if (c->hFit) hipHostFree(c->hFit);
    if (c->hPreferred) hipHostFree(c->hPreferred);
    for (int i = 0; i < EV_COUNT; ++i) if (c->ev[i]) hipEventDestroy(c->ev[i]);
    for (hipEvent_t e : c->evGather) if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->evVerify) if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->evMarkRows) if (e) hipEventDestroy(e);
    if (c->ownStream && c->stream) hipStreamDestroy(c->stream);
    delete c;
}

const char* hj_strerror(int status)
{
    switch (status) {
        case HJ_OK: return "ok";
        case HJ_ERR_INVALID: return "invalid argument";
        case HJ_ERR_NO_DEVICE: return "no gfx950 HIP device (this library has no CPU fallback)";
        case HJ_ERR_HIP: return "HIP runtime error";
        case HJ_ERR_OOM: return "out of device memory";
        case HJ_ERR_KEY_RANGE: return "tuple outside the DataGen layout (payload bits set or value 0)";
        case HJ_ERR_UNKNOWN_ALGO: return "unknown algo";
        case HJ_ERR_STATE: return "call order violated";
        default: return "unknown status";
    }
}

const char* hj_last_error(const hj_ctx* c) { return c ? c->err.c_str() : "null context"; }

int hj_synchronize(hj_ctx* c)
{
    HJ_ENTER(c, true);
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    return HJ_OK;
}

int hj_reserve(hj_ctx* c, const hj_params* params, uint64_t rSize, uint64_t sSize)
{
    if (!c || !params) return HJ_ERR_INVALID;
    if (params->algo > HJ_ALGO_AUTO) return fail(c, HJ_ERR_UNKNOWN_ALGO, "hj_reserve: algo");
    if (rSize == 0) return fail(c, HJ_ERR_INVALID, "hj_reserve: rSize == 0");
    // the marks are indexed by R row: only HJ_ALGO_HTM keeps the rows whatever the flags
    const bool track = (params->flags & HJ_FLAG_TRACK_R_MATCHES) != 0;
    if (track && params->algo != HJ_ALGO_HTM && !(params->flags & HJ_FLAG_KEEP_ROW_IDS))
        return fail(c, HJ_ERR_INVALID, "hj_reserve: HJ_FLAG_TRACK_R_MATCHES needs HJ_FLAG_KEEP_ROW_IDS on open addressing and PRJ / AUTO");
    HJ_HIP(c, hipSetDevice(c->device));
    c->params = *params;
    HJ_HIP(c, hipStreamSynchronize(c->stream));          // buffers may be replaced below; and a new workload starts without an expectation
    *c->hPreferred = 0;
    if (track) {
        // one bit per R row in 32-bit words (the sweep reads whole words: rounded up to 16 bytes), and the sweep's workspace
        bool replaced = false;
        int rc = c->buf[B_R_MARKS].reserve(c, (((rSize + 31) / 32 + 3) & ~3ull) * sizeof(uint32_t), &replaced);
        if (!rc) rc = c->buf[B_R_SWEEP].reserve(c, r_sweep_count_words(rSize) * sizeof(uint32_t));
        if (replaced) c->marksBuilt = c->rRowsCalled = false;       // the plane of the last build is gone
        if (rc) return rc;
    }
    if (params->algo == HJ_ALGO_PRJ || params->algo == HJ_ALGO_AUTO) {
        if (rSize >= 0xFFFFFFFFull || sSize >= 0xFFFFFFFFull)
            return fail(c, HJ_ERR_INVALID, "hj_reserve: PRJ sizes must be < 2^32 tuples per device");
        uint32_t bits = params->radixBits ? params->radixBits : auto_radix_bits(rSize);
        if (bits < 1 || bits > 16) return fail(c, HJ_ERR_INVALID, "hj_reserve: radixBits must be in [1,16]");
        if (params->prjMode > 2) return fail(c, HJ_ERR_INVALID, "hj_reserve: prjMode must be 0, 1 or 2");
        c->plan = prj_plan(rSize, sSize, bits, params->prjMode);
        const uint64_t nmax = rSize > sSize ? rSize : sSize;
        // +2 tuples: the 16-byte sweeps may touch one tuple past an odd end
        // prjRes: the resident R's offsets (hj_prj_build_dev) and the probes' work items, for slices up to sSize
        bool replaced = false;      // a resident R does not survive the replacement of any of the five
        int rc = c->buf[B_TMP].reserve(c, (nmax + 2) * sizeof(uint64_t), &replaced);
        if (!rc) rc = c->buf[B_PART_R].reserve(c, (rSize + 2) * sizeof(uint64_t), &replaced);
        if (!rc && sSize) rc = c->buf[B_PART_S].reserve(c, (sSize + 2) * sizeof(uint64_t), &replaced);
        if (!rc) rc = c->buf[B_WORK].reserve(c, c->plan.workspaceBytes, &replaced);
        if (!rc) rc = c->buf[B_PRJ_RES].reserve(c, prj_resident_bytes(bits, sSize), &replaced);
        if (replaced) c->resident = false;
        if (rc) return rc;
        c->prjMaxSlice = sSize;
        if (params->algo == HJ_ALGO_PRJ) return HJ_OK;      // AUTO also needs the open-addressing buffers below
        // ... when the table join can take this R at all (it wants a power-of-two size, as the reference does);
        // otherwise AUTO simply is the radix join, which has no such restriction
        if (!is_pow2(rSize) || rSize > (1ull << 31)) return HJ_OK;
    }
    if (params->algo == HJ_ALGO_HTM) {
        // the bucketised table (HTMHashBuild.hpp:61-72): nextpow2(rSize/3 + 1) buckets of 32 bytes = 4 slots each;
        // any rSize (the hash is (key/3) & mask, not tied to rSize being a power of two)
        if (rSize > (1ull << 31)) return fail(c, HJ_ERR_INVALID, "hj_reserve: rSize > 2^31 per device");
        const uint64_t nb = htm_num_buckets(rSize);
        int rc = c->buf[B_TABLE].reserve(c, (4 * nb + kTableSlack) * sizeof(uint64_t));
        if (rc) return rc;
        // rings (variant 3), workgroup window (2) or global atomics (1): buffers for the larger need of the first two
        size_t qb = wave_queue_bytes(rSize, c->nCU), cb = wave_conflict_bytes(rSize, c->nCU);
        if (own_supported(4 * nb)) {
            if (own_queue_bytes(rSize) > qb) qb = own_queue_bytes(rSize);
            if (own_conflict_bytes(rSize, c->nCU) > cb) cb = own_conflict_bytes(rSize, c->nCU);
            if ((rc = c->buf[B_OWNER].reserve(c, own_owner_bytes(4 * nb)))) return rc;
            if ((rc = c->buf[B_HTM_OWN_COUNTS].reserve(c, own_conflict_count_bytes(rSize, c->nCU)))) return rc;
        }
        if ((rc = c->buf[B_QUEUE].reserve(c, qb))) return rc;
        if ((rc = c->buf[B_HTM_CONFLICTS].reserve(c, cb))) return rc;
        if ((rc = c->buf[B_HTM_OVF_COUNT].reserve(c, nb * sizeof(unsigned int)))) return rc;
        if ((rc = c->buf[B_HTM_OVF_BASE].reserve(c, nb * sizeof(uint32_t)))) return rc;
        return c->buf[B_HTM_SCAN].reserve(c, scan_workspace_words(nb) * sizeof(uint32_t));
    }
    if (!is_pow2(rSize)) return fail(c, HJ_ERR_INVALID, "hj_reserve: rSize must be a power of two (DataGen.hpp:28, NoCCHashBuild.hpp:36)");
    if (rSize > (1ull << 31)) return fail(c, HJ_ERR_INVALID, "hj_reserve: rSize > 2^31 per device");
    int rc = c->buf[B_TABLE].reserve(c, (2 * rSize + kTableSlack) * sizeof(uint64_t));
    if (rc) return rc;
    if (params->buildVariant > 4) return fail(c, HJ_ERR_INVALID, "hj_reserve: buildVariant must be 0, 1, 2, 3 or 4");
    if (params->buildVariant != 1 && (own_supported(2 * rSize) || wave_supported(2 * rSize))) {
        // 1/8 headroom: a radix shard may receive slightly more than its nominal share (hj_build_keys_dev)
        size_t qb = own_queue_bytes(rSize + rSize / 8);
        if (wave_queue_bytes(rSize + rSize / 8, c->nCU) > qb) qb = wave_queue_bytes(rSize + rSize / 8, c->nCU);
        if (own_supported(2 * rSize) && (rc = c->buf[B_OWNER].reserve(c, own_owner_bytes(2 * rSize)))) return rc;
        if ((rc = c->buf[B_QUEUE].reserve(c, qb))) return rc;
    }
    return HJ_OK;
}

// Locality pre-round, host-side form (hj_join_dev with HJ_ALGO_AUTO only: the choice between table join and radix join
// changes which buffers and kernels are used at all, so it is read back; hj_build_dev decides on the device, see
// build_common). 256 sample tiles of R. Answer = the build kernel worth taking:
//   3  the wavefront-private rings (hj_build_wave.hip) if at most 1/128 of the sampled tuples would fall outside
//      their ring (tight locality: the reference's default shuffle window of 16, anything up to ~100 positions);
//   2  the workgroup window (hj_build_own.hip) if it would have to defer at most 3/4 of the tuples (variant_for_sample,
//      hj_device.h: what it defers costs about what global atomics cost for every tuple);
//   1  global atomics otherwise (no locality: hj_join_dev(AUTO) then takes the radix join instead).
static int sample_variant(hj_ctx* c, const void* d, bool key32, uint64_t n, uint64_t tableSize, uint32_t hshift,
                          const BuildCaps& can, uint32_t* variant, bool htm = false)
{
    const uint32_t nSample = 256;
    unsigned int* const fit = c->buf[B_FIT].as<unsigned int>();
    HJ_HIP(c, launch_sample_locality(d, key32, n, tableSize, hshift, nSample, fit, c->stream, htm));
    HJ_HIP(c, hipMemcpyAsync(c->hFit, fit, 8 * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    *variant = variant_for_sample(c->hFit[0], c->hFit[1], c->hFit[2], can.own, can.wave, can.compact, c->hFit[3], c->hFit[4]);
    return HJ_OK;
}

// Shared by hj_build_dev (DataGen tuples) and hj_build_keys_dev (bare keys of a radix shard).
// R-side match marks at a build (hj_build_dev / hj_prj_build_dev) of a context reserved with HJ_FLAG_TRACK_R_MATCHES:
// marks_begin checks that the plane takes rSize rows and zeroes it on the stream, marks_built -- once the build is
// enqueued -- says what the plane now describes. Neither does anything on a context without the flag.
static bool tracks(const hj_ctx* c) { return (c->params.flags & HJ_FLAG_TRACK_R_MATCHES) != 0; }
static size_t marks_bytes(uint64_t rows) { return (size_t)((rows + 31) / 32) * sizeof(uint32_t); }
static int marks_begin(hj_ctx* c, const char* fn, uint64_t rSize)
{
    if (!tracks(c)) return HJ_OK;
    if (marks_bytes(rSize) > c->buf[B_R_MARKS].bytes || r_sweep_count_words(rSize) * sizeof(uint32_t) > c->buf[B_R_SWEEP].bytes)
        return fail(c, HJ_ERR_STATE, (std::string(fn) + ": hj_reserve() not called for this rSize (match marks)").c_str());
    HJ_HIP(c, hipSetDevice(c->device));
    c->streamAtBuildEnd = false;
    HJ_HIP(c, hipMemsetAsync(c->buf[B_R_MARKS].p, 0, marks_bytes(rSize), c->stream));
    return HJ_OK;
}
static void marks_built(hj_ctx* c, uint64_t rSize, uint64_t idxBase)
{
    if (!tracks(c)) return;
    c->marksBuilt = true; c->marksRows = rSize; c->marksBase = idxBase;
    c->rRowsCalled = false;
}
// the marks a materialising probe of `kind` sets: none unless the context tracks, the plane describes the table or the
// resident R being probed, and the kind produces R rows
static bool marks_for(const hj_ctx* c, uint32_t kind, RMarks* mk)
{
    if (!tracks(c) || !c->marksBuilt || kind > HJ_JOIN_LEFT) return false;
    *mk = RMarks{c->buf[B_R_MARKS].as<uint32_t>(), (uint32_t)c->marksBase, (uint32_t)c->marksRows};
    return true;
}

static int build_common(hj_ctx* c, const void* d, bool key32, uint64_t n, uint32_t hshift,
                        uint64_t tableSize, uint64_t idxBase)
{
    int rc;
    if ((rc = begin_operation(c, n, 0, tableSize))) return rc;
    c->hshift = hshift;
    if ((rc = record(c, EV_CLEAR0))) return rc;
    const BuildCaps can = build_caps(c, n, tableSize);
    const uint32_t variant = settle_variant(c->forceVariant ? c->forceVariant : c->params.buildVariant, can);
    c->variantUsed = (variant == 4) ? 0 : variant;     // 0: decided on the device (4 may fall back to 3), reported from Counters::variant
    c->algoUsed = c->params.algo == HJ_ALGO_AUTO ? (uint32_t)HJ_ALGO_ATOMIC : c->params.algo;
    const BuildJob job = build_job(c, d, key32, n, hshift, tableSize, probe_len(c->params), idxBase, c->sc);
    const WaveBufs wave{c->buf[B_BOUNDS].p, c->buf[B_QUEUE].p};
    const OwnBufs own{c->buf[B_OWNER].p, c->buf[B_QUEUE].p, c->buf[B_QUEUE_COUNT].as<uint32_t>()};
    const unsigned long long* word = &job.ctr->variant;
    c->wavePreGated = variant == 0;
    // The classic rings (3) of a context that keeps no row ids retire planar: 4-byte keys for the probe, the index words in a
    // plane of their own that only the deferred walks read. Behind them the packed classic build stays enqueued, gated on the
    // word k_wave_fixup sets when the planar build had to give up (Counters::planarFail); not needed, its launches return at once.
    const int classicMode = (c->params.flags & HJ_FLAG_KEEP_ROW_IDS) ? kWaveClassic : kWavePlanar;
    auto classic_tail = [&](Gate gate) -> hipError_t {
        hipError_t e = launch_build_wave(job, wave, gate, kWaveTail, classicMode);
        if (e != hipSuccess || classicMode == kWaveClassic) return e;
        return launch_build_wave(job, wave, Gate{&job.ctr->packedRedo, 1}, kWaveMain | kWaveTail, kWaveClassic);
    };
    // The dominant kernel of each LDS variant is bracketed by its own pair of events (bracket(); hj_result.buildPhaseA_us).
    if (variant == 0) {
        // The locality pre-round decides ON THE DEVICE (this call stays asynchronous: no read-back). Behind it the kernels
        // of the candidate variants are enqueued, each gated on the word the pre-round writes; the ones not chosen return
        // at once (~4.5 us each). Which candidates: all of them the first time; afterwards only what the context's PREVIOUS
        // pick preferred (Counters::preferred, which the sampler also stores into pinned host memory, read here without
        // waiting) -- with the classic rings behind the compact ones. The pick is taken among the enqueued variants, and
        // every LDS build is correct on any input (what does not fit its rings / window goes through its deferred phase),
        // so a workload that changes its locality class costs one slow step, never a wrong one, and the next step follows
        // it (round-2 VERDICT, launch tail: 23 -> 9 launches in the steady state).
        const uint32_t expect = (uint32_t)*reinterpret_cast<volatile unsigned long long*>(c->hPreferred);
        const uint32_t all = 2u | (can.own ? 4u : 0u) | (can.wave ? 8u : 0u) | (can.compact ? 16u : 0u);
        uint32_t allowed = all;
        if (expect == 4 && can.compact) allowed = 16u | 8u;
        else if (expect == 3 && can.wave) allowed = 8u;
        else if (expect == 2 && can.own) allowed = 4u;
        else if (expect == 1) allowed = 2u;
        const bool enqCompact = (allowed >> 4) & 1u, enqWave = (allowed >> 3) & 1u, enqOwn = (allowed >> 2) & 1u, enqGlobal = (allowed >> 1) & 1u;
        SamplePick pick;
        pick.ctr = job.ctr; pick.hostPreferred = c->dPreferred; pick.allowedMask = allowed;
        pick.canOwn = can.own; pick.canWave = can.wave; pick.canCompact = can.compact;
        HJ_HIP(c, launch_sample_locality(d, key32, n, tableSize, hshift, 256, job.ctr->fit, c->stream, false, pick, true));
        if ((rc = record(c, EV_BUILD0))) return rc;
        // phase A of the LDS variants, each dominant kernel inside its own pair of events, then their tails. (An event
        // record costs the stream ~5 us -- step timeline at 2^22, tools/step_timeline.sh --, so nothing is recorded that
        // hj_fetch does not read.)
        if (enqWave) {
            c->wavePreN = n;
            HJ_HIP(c, launch_build_wave(job, wave, Gate{word, 3, 4}, kWavePre));
            if (enqCompact)
                HJ_HIP(c, launch_build_wave(job, wave, Gate{word, 4}, kWaveMain, kWaveCompact, bracket(c, EV_KC0)));
            HJ_HIP(c, launch_build_wave(job, wave, Gate{word, 3}, kWaveMain, classicMode, bracket(c, EV_KW0)));
        }
        if (enqOwn)
            HJ_HIP(c, launch_build_own(job, own, Gate{word, 2}, 1, bracket(c, EV_KO0)));
        if (enqWave) {
            if (enqCompact)
                HJ_HIP(c, launch_build_wave(job, wave, Gate{word, 4}, kWaveTail, kWaveCompact));
            HJ_HIP(c, classic_tail(Gate{word, 3}));
        }
        if (enqOwn)
            HJ_HIP(c, launch_build_own(job, own, Gate{word, 2}, 2));
        if (enqGlobal) {
            launch_fill_empty(job.table, tableSize + kTableSlack, Gate{word, 1}, c->stream, job.ctr, tableSize);
            launch_build_atomic_min(job, Gate{word, 1});
        }
    } else if (variant == 4) {
        // the compact rings, asked for by the caller: the classic rings stay enqueued behind them as the gated fallback
        launch_set_variant(job.ctr, 4, c->stream);
        c->wavePreN = n;
        if ((rc = record(c, EV_BUILD0))) return rc;
        HJ_HIP(c, launch_build_wave(job, wave, Gate{word, 4}, kWavePre | kWaveMain, kWaveCompact, bracket(c, EV_KC0)));
        HJ_HIP(c, launch_build_wave(job, wave, Gate{word, 3}, kWaveMain, classicMode, bracket(c, EV_KW0)));
        HJ_HIP(c, launch_build_wave(job, wave, Gate{word, 4}, kWaveTail, kWaveCompact));
        HJ_HIP(c, classic_tail(Gate{word, 3}));
    } else if (variant == 3) {
        c->wavePreN = n;
        if ((rc = record(c, EV_BUILD0))) return rc;
        HJ_HIP(c, launch_build_wave(job, wave, Gate{nullptr, 0}, kWavePre | kWaveMain, classicMode, bracket(c, EV_KW0)));
        HJ_HIP(c, classic_tail(Gate{nullptr, 0}));
    } else if (variant == 2) {
        if ((rc = record(c, EV_BUILD0))) return rc;
        HJ_HIP(c, launch_build_own(job, own, Gate{nullptr, 0}, 3, bracket(c, EV_KO0)));
    } else {
        launch_fill_empty(job.table, tableSize + kTableSlack, Gate{nullptr, 0}, c->stream);
        launch_set_full_range(tableSize, job.ctr, Gate{nullptr, 0}, c->stream);
        HJ_HIP(c, hipGetLastError());
        if ((rc = record(c, EV_BUILD0))) return rc;
        if (n) launch_build_atomic_min(job, Gate{nullptr, 0});
    }
    HJ_HIP(c, hipGetLastError());
    if ((rc = record(c, EV_BUILD1))) return rc;
    c->built = true;
    c->streamAtBuildEnd = c->ownStream; c->probeStartsAtBuildEnd = false;
    return HJ_OK;
}

// room for `need` overflow buckets behind index 0 (unused); a new area gets 1/8 + 64 buckets of headroom
static int reserve_htm_overflow(hj_ctx* c, uint64_t need)
{
    DevBuf& b = c->buf[B_HTM_OVERFLOW];
    if ((need + 1) * 4 * sizeof(uint64_t) <= b.bytes) return HJ_OK;
    return b.reserve(c, (need + need / 8 + 64 + 1) * 4 * sizeof(uint64_t));
}

// --algo htm: the bucketised table (hj_htm.hip). Not asynchronous: the number of conflicts is read back once, to size
// the overflow area (the reference, too, builds its chains in a serial phase after the parallel build, :231-279).
static int build_htm(hj_ctx* c, const uint64_t* dR, uint64_t rSize, uint64_t idxBase)
{
    const uint32_t nb = htm_num_buckets(rSize);
    const uint64_t slots = 4ull * nb;
    if ((slots + kTableSlack) * sizeof(uint64_t) > c->buf[B_TABLE].bytes || nb * sizeof(unsigned int) > c->buf[B_HTM_OVF_COUNT].bytes ||
        nb * sizeof(uint32_t) > c->buf[B_HTM_OVF_BASE].bytes || scan_workspace_words(nb) * sizeof(uint32_t) > c->buf[B_HTM_SCAN].bytes ||
        c->buf[B_QUEUE].bytes < wave_queue_bytes(rSize, c->nCU) || c->buf[B_HTM_CONFLICTS].bytes < wave_conflict_bytes(rSize, c->nCU))
        return fail(c, HJ_ERR_STATE, "hj_build_dev: hj_reserve() not called for this rSize (htm)");
    if (idxBase + rSize > 0xFFFFFFFFull) return fail(c, HJ_ERR_INVALID, "hj_build_dev: index range exceeds 2^32 - 1");
    int rc;
    if ((rc = begin_operation(c, rSize, 0, slots))) return rc;
    c->hshift = 0; c->htmBuckets = nb;
    if (!c->htmGenericChains) { c->htmChainsFellBack = false; c->htmChainState = 0; c->htmChainCause = 0; c->htmChainGroups = 0; }
    if ((rc = record(c, EV_CLEAR0))) return rc;
    const BuildJob job = build_job(c, dR, false, rSize, 0, slots, 3, idxBase, ShardCheck{0, 0, 0, 0});
    uint64_t* const htmConflicts = c->buf[B_HTM_CONFLICTS].as<uint64_t>();
    uint32_t* const ownCounts = c->buf[B_HTM_OWN_COUNTS].as<uint32_t>();
    unsigned int* const ovfCount = c->buf[B_HTM_OVF_COUNT].as<unsigned int>();
    uint32_t* const ovfBase = c->buf[B_HTM_OVF_BASE].as<uint32_t>();
    uint32_t* const scan = c->buf[B_HTM_SCAN].as<uint32_t>();
    void* const bounds = c->buf[B_BOUNDS].p;
    // locality pre-round with the bucketised table's own hash (bucket = key / 3 keeps the key order): the rings if they
    // will do, the workgroup window for looser locality (shuffle windows up to ~2000 positions), else global atomics.
    // The window also lists its conflicts: two buffers more than build_caps asks for
    BuildCaps can = build_caps(c, rSize, slots);
    can.own = can.own && c->buf[B_HTM_CONFLICTS].bytes >= own_conflict_bytes(rSize, c->nCU) &&
              c->buf[B_HTM_OWN_COUNTS].bytes >= own_conflict_count_bytes(rSize, c->nCU);
    can.compact = false;
    uint32_t variant = settle_variant(c->params.buildVariant, can);      // the compact rings: the classic ones here
    if (variant == 0 && (rc = sample_variant(c, dR, false, rSize, slots, 0, can, &variant, true))) return rc;   // answers within `can`
    c->variantUsed = variant; c->algoUsed = HJ_ALGO_HTM;
    const WaveSlices sl = variant == 2 ? own_conflict_layout(rSize, c->nCU, ownCounts) : wave_conflict_layout(rSize, c->nCU, bounds);
    // the rings: chains in LDS (hj_htm.hip) unless an earlier attempt on this relation had to give up
    const uint32_t nParts = sl.nChunks * htm_chain_parts(sl.sliceLen);
    const bool ldsChains = variant == 3 && !c->htmGenericChains && htm_chain_tries(sl.nChunks, sl.sliceLen, nb);
    if (variant == 2) {
        if ((rc = record(c, EV_BUILD0))) return rc;
        const OwnBufs own{c->buf[B_OWNER].p, c->buf[B_QUEUE].p, c->buf[B_QUEUE_COUNT].as<uint32_t>(), htmConflicts, ownCounts};
        HJ_HIP(c, launch_build_own(job, own, Gate{nullptr, 0}, 3, bracket(c, EV_KO0)));
    } else if (variant == 3) {
        c->wavePreN = rSize; c->wavePreGated = false;
        if ((rc = record(c, EV_BUILD0))) return rc;
        const WaveBufs wave{bounds, c->buf[B_QUEUE].p, htmConflicts, ldsChains};
        HJ_HIP(c, launch_build_wave(job, wave, Gate{nullptr, 0}, kWaveAll, kWaveClassic, bracket(c, EV_KW0)));
        if (ldsChains) {
            // the chain phase in LDS, first half: overflow buckets per part of a slice, scanned (one word more: the total)
            HJ_HIP(c, hipMemsetAsync(ovfBase + nParts, 0, sizeof(uint32_t), c->stream));
            HJ_HIP(c, launch_htm_chain_count(htmConflicts, sl.counts, WaveScratch(c->nCU, bounds).bounds, sl.nChunks, sl.sliceLen, nb,
                                             ovfBase, ovfCount, job.ctr, c->stream));
            HJ_HIP(c, launch_exclusive_scan_u32(ovfBase, (uint64_t)nParts + 1, scan, c->stream));
            HJ_HIP(c, hipMemcpyAsync(c->hFit, ovfBase + nParts, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        }
    } else {
        launch_fill_empty(job.table, slots + kTableSlack, Gate{nullptr, 0}, c->stream);
        launch_set_full_range(slots, job.ctr, Gate{nullptr, 0}, c->stream);
        HJ_HIP(c, hipGetLastError());
        if ((rc = record(c, EV_BUILD0))) return rc;
        HJ_HIP(c, launch_htm_build_global(dR, rSize, sl.sliceLen, sl.nChunks, job.table, slots, idxBase, htmConflicts,
                                          const_cast<uint32_t*>(sl.counts), job.ctr, c->stream));
    }
    // chains -- only if some bucket overflowed (one read-back of the conflict count): count per bucket, reserve overflow
    // buckets by one scan, fill them in index order, link
    if ((rc = read_counters(c, true))) return rc;
    const uint64_t conflicts = c->hCtr->conflicts;              // >= overflow buckets needed
    c->htmOverflowUsed = conflicts;
    if (ldsChains && c->hCtr->htmChainBail) {
        // an input the LDS chain phase cannot take (hj_htm.hip): once more, unrouted, with the generic chain kernels
        c->htmChainCause = c->hCtr->htmChainBail;               // kept here: the second attempt zeroes the counters
        c->htmGenericChains = true;
        rc = build_htm(c, dR, rSize, idxBase);
        c->htmGenericChains = false;
        c->htmChainsFellBack = true;
        c->htmChainState = 2;
        return rc;
    }
    if (ldsChains) {
        const uint64_t groups = c->hFit[0];                     // overflow buckets the parts need, exactly
        c->htmChainState = 1; c->htmChainGroups = groups;
        if (conflicts) {
            if ((rc = reserve_htm_overflow(c, groups))) return rc;
            HJ_HIP(c, launch_htm_chain_fill(htmConflicts, sl.nChunks, sl.sliceLen, nb, ovfBase, ovfCount, job.table,
                                            c->buf[B_HTM_OVERFLOW].as<uint64_t>(), job.ctr, c->stream));
        }
    } else if (conflicts) {
        HJ_HIP(c, launch_htm_count(htmConflicts, sl.counts, sl.nChunks, sl.sliceLen, nb, ovfCount, ovfBase, c->stream));
        HJ_HIP(c, launch_exclusive_scan_u32(ovfBase, nb, scan, c->stream));
        if ((rc = reserve_htm_overflow(c, conflicts))) return rc;
        HJ_HIP(c, launch_htm_chains(htmConflicts, sl.counts, sl.nChunks, sl.sliceLen, job.table, nb, ovfCount, ovfBase,
                                    c->buf[B_HTM_OVERFLOW].as<uint64_t>(), conflicts, job.ctr, c->stream));
    }
    if ((rc = record(c, EV_BUILD1))) return rc;
    c->built = true; c->htmBuilt = true;
    c->streamAtBuildEnd = c->ownStream; c->probeStartsAtBuildEnd = false;
    return HJ_OK;
}

int hj_build_dev(hj_ctx* c, const uint64_t* dR, uint64_t rSize, uint64_t idxBase)
{
    if (!c || !dR) return HJ_ERR_INVALID;
    if (c->params.algo == HJ_ALGO_PRJ) return fail(c, HJ_ERR_STATE, "hj_build_dev: context is reserved for PRJ");
    const bool htm = c->params.algo == HJ_ALGO_HTM;
    if (htm && !rSize) return HJ_ERR_INVALID;
    if (!htm) {
        if (!is_pow2(rSize) || (2 * rSize + kTableSlack) * sizeof(uint64_t) > c->buf[B_TABLE].bytes)
            return fail(c, HJ_ERR_STATE, "hj_build_dev: hj_reserve() not called for this rSize");
        // indices stay below 2^32 - 1: (index << 32 | key) of index = key = 0xFFFFFFFF would be the empty pattern
        if (idxBase + rSize > 0xFFFFFFFFull) return fail(c, HJ_ERR_INVALID, "hj_build_dev: index range exceeds 2^32 - 1");
    }
    // the marks of the build before: cleared in front of the build, outside everything it times
    int rc;
    if ((rc = marks_begin(c, "hj_build_dev", rSize))) return rc;
    rc = htm ? build_htm(c, dR, rSize, idxBase) : build_common(c, dR, false, rSize, 0, 2 * rSize, idxBase);
    if (rc == HJ_OK) marks_built(c, rSize, idxBase);
    return rc;
}

int hj_build_keys_dev(hj_ctx* c, const uint32_t* dKeys, uint64_t n, uint32_t homeShift, uint64_t tableSize)
{
    if (!c || (!dKeys && n)) return HJ_ERR_INVALID;
    if (c->params.algo == HJ_ALGO_PRJ || c->params.algo == HJ_ALGO_HTM)
        return fail(c, HJ_ERR_STATE, "hj_build_keys_dev: context is reserved for PRJ / htm");
    if (tracks(c)) return fail(c, HJ_ERR_STATE, "hj_build_keys_dev: a context reserved with HJ_FLAG_TRACK_R_MATCHES takes no bare keys");
    if (homeShift > 6) return fail(c, HJ_ERR_INVALID, "hj_build_keys_dev: homeShift must be in [0,6]");
    if (!is_pow2(tableSize) || (tableSize + kTableSlack) * sizeof(uint64_t) > c->buf[B_TABLE].bytes)
        return fail(c, HJ_ERR_STATE, "hj_build_keys_dev: hj_reserve() not called for this table size");
    if (n > 0xFFFFFFFFull) return fail(c, HJ_ERR_INVALID, "hj_build_keys_dev: index range exceeds 2^32 - 1");
    return build_common(c, dKeys, true, n, homeShift, tableSize, 0);
}

int hj_probe_dev(hj_ctx* c, const uint64_t* dS, uint64_t sSize)
{
    if (!c || (!dS && sSize)) return HJ_ERR_INVALID;
    if (!c->built) return fail(c, HJ_ERR_STATE, "hj_probe_dev: no table (call hj_build_dev first)");
    HJ_HIP(c, hipSetDevice(c->device));
    int rc;
    // the probe's start: the build's end event if this is the very next thing on the library's own stream (one event
    // record less per step), an event of its own otherwise
    c->probeStartsAtBuildEnd = c->streamAtBuildEnd;
    c->streamAtBuildEnd = false;
    if (!c->probeStartsAtBuildEnd && (rc = record(c, EV_PROBE0))) return rc;
    const uint64_t* const table = c->buf[B_TABLE].as<uint64_t>();
    if (sSize && c->htmBuilt) launch_htm_probe(dS, sSize, table, c->htmBuckets, c->buf[B_HTM_OVERFLOW].as<uint64_t>(), c->dCtr(), c->stream);
    else if (sSize) launch_probe(dS, false, sSize, table, c->tableSize, c->hshift, probe_len(c->params), c->sc, c->dCtr(), c->stream);
    if ((rc = record(c, EV_PROBE1))) return rc;
    HJ_HIP(c, hipGetLastError());
    c->sSize += sSize;
    return HJ_OK;
}

// The one host sequence of the materialising table probe; fn: the entry point's name, for the error texts
static int probe_join(hj_ctx* c, const char* fn, uint32_t kind, const uint64_t* dS, uint64_t sSize, uint64_t sIdxBase, uint32_t* dOutS,
                      uint32_t* dOutR, uint64_t capacity)
{
    if (!c || (!dS && sSize)) return HJ_ERR_INVALID;
    const std::string f(fn);
    if (kind > HJ_JOIN_ANTI) return fail(c, HJ_ERR_INVALID, (f + ": kind must be an hj_join_kind").c_str());
    const bool planeR = kind <= HJ_JOIN_LEFT;            // SEMI and ANTI write S rows only: dOutR is ignored
    // decided on the host: whether the table keeps its index words is chosen on the device (Counters::tableFormat), so
    // the call keys on what hj_reserve was promised
    if (c->params.algo == HJ_ALGO_PRJ) return fail(c, HJ_ERR_STATE, (f + ": a PRJ context keeps no row ids").c_str());
    if (!c->built) return fail(c, HJ_ERR_STATE, (f + ": no table (call hj_build_dev first)").c_str());
    if (!c->htmBuilt && !(c->params.flags & HJ_FLAG_KEEP_ROW_IDS))
        return fail(c, HJ_ERR_STATE, (f + ": open-addressing context reserved without HJ_FLAG_KEEP_ROW_IDS").c_str());
    if (capacity && (!dOutS || (planeR && !dOutR))) return fail(c, HJ_ERR_INVALID, (f + ": output pointer NULL with capacity > 0").c_str());
    if (sIdxBase > 0xFFFFFFFFull || sIdxBase + sSize > 0xFFFFFFFFull)
        return fail(c, HJ_ERR_INVALID, (f + ": S row range exceeds 2^32 - 1").c_str());
    if (!c->htmBuilt && probe_len(c->params) > pairs_max_probe_len())
        return fail(c, HJ_ERR_INVALID, (f + ": probeLength above 8").c_str());
    if (sSize == 0) return HJ_OK;
    HJ_HIP(c, hipSetDevice(c->device));
    c->streamAtBuildEnd = false;
    int rc;
    const PairsOut out{dOutS, planeR ? dOutR : nullptr, capacity, c->buf[B_PAIRS_CURSOR].as<unsigned long long>()};
    HJ_HIP(c, hipMemsetAsync(out.cursor, 0, 2 * sizeof(unsigned long long), c->stream));
    if ((rc = record(c, EV_PAIRS0))) return rc;
    const uint64_t* const table = c->buf[B_TABLE].as<uint64_t>();
    RMarks mk;
    const RMarks* const marks = marks_for(c, kind, &mk) ? &mk : nullptr;
    if (c->htmBuilt) launch_htm_probe_pairs(kind, dS, sSize, sIdxBase, table, c->htmBuckets, c->buf[B_HTM_OVERFLOW].as<uint64_t>(), out, c->nCU, c->dCtr(), c->stream, marks);
    else launch_probe_pairs(kind, dS, sSize, sIdxBase, table, c->tableSize, c->hshift, probe_len(c->params), c->sc, out, c->nCU, c->dCtr(), c->stream, marks);
    if ((rc = record(c, EV_PAIRS1))) return rc;
    HJ_HIP(c, hipGetLastError());
    c->pairsCapacity = capacity; c->pairsKind = kind; c->pairsS = sSize;
    c->sSize += sSize;
    return HJ_OK;
}

// (No R row is HJ_NO_ROW: hj_build_dev and build_htm refuse idxBase + rSize > 2^32 - 1, hj_build_keys_dev n > 2^32 - 1, so
// the largest row is 2^32 - 2 and HJ_JOIN_LEFT needs no check of its own.)
int hj_probe_join_dev(hj_ctx* c, uint32_t kind, const uint64_t* dS, uint64_t sSize, uint64_t sIdxBase, uint32_t* dOutS, uint32_t* dOutR,
                      uint64_t capacity)
{
    return probe_join(c, "hj_probe_join_dev", kind, dS, sSize, sIdxBase, dOutS, dOutR, capacity);
}

int hj_probe_pairs_dev(hj_ctx* c, const uint64_t* dS, uint64_t sSize, uint64_t sIdxBase, uint32_t* dOutS, uint32_t* dOutR,
                       uint64_t capacity)
{
    return probe_join(c, "hj_probe_pairs_dev", HJ_JOIN_INNER, dS, sSize, sIdxBase, dOutS, dOutR, capacity);
}

int hj_pairs_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    unsigned long long words[2] = {0, 0};        // the cursor = rows found; LEFT's unmatched S tuples
    HJ_HIP(c, hipMemcpy(words, c->buf[B_PAIRS_CURSOR].p, sizeof words, hipMemcpyDeviceToHost));
    const unsigned long long found = words[0];
    out[0] = found;
    out[1] = found < c->pairsCapacity ? found : c->pairsCapacity;
    out[2] = (uint64_t)(elapsed_us(c, EV_PAIRS0, EV_PAIRS1) + 0.5);
    // unmatched S tuples of the call: SEMI wrote one row per matched tuple, ANTI one per unmatched one
    out[3] = c->pairsKind == HJ_JOIN_LEFT ? words[1] : c->pairsKind == HJ_JOIN_SEMI ? c->pairsS - found
           : c->pairsKind == HJ_JOIN_ANTI ? found : 0;
    return HJ_OK;
}

// ---- R-side match marks ---------------------------------------------------
// what the three calls need: a context reserved with the flag whose plane describes its last build
static int marks_state(hj_ctx* c, const char* fn)
{
    const std::string f(fn);
    if (!tracks(c)) return fail(c, HJ_ERR_STATE, (f + ": context reserved without HJ_FLAG_TRACK_R_MATCHES").c_str());
    if (!c->marksBuilt) return fail(c, HJ_ERR_STATE, (f + ": the last build was not hj_build_dev / hj_prj_build_dev (or there was none)").c_str());
    return HJ_OK;
}

int hj_r_marks_clear(hj_ctx* c)
{
    HJ_ENTER(c, true);
    if (const int rc = marks_state(c, "hj_r_marks_clear")) return rc;
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipMemsetAsync(c->buf[B_R_MARKS].p, 0, marks_bytes(c->marksRows), c->stream));
    return HJ_OK;
}

int hj_r_rows_dev(hj_ctx* c, uint32_t which, uint32_t* dOutR, uint64_t capacity)
{
    HJ_ENTER(c, true);
    if (const int rc = marks_state(c, "hj_r_rows_dev")) return rc;
    if (which > HJ_R_MATCHED) return fail(c, HJ_ERR_INVALID, "hj_r_rows_dev: which must be HJ_R_UNMATCHED or HJ_R_MATCHED");
    if (capacity && !dOutR) return fail(c, HJ_ERR_INVALID, "hj_r_rows_dev: output pointer NULL with capacity > 0");
    HJ_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = record(c, EV_RROWS0))) return rc;
    const RMarks mk{c->buf[B_R_MARKS].as<uint32_t>(), (uint32_t)c->marksBase, (uint32_t)c->marksRows};
    HJ_HIP(c, launch_r_sweep(mk, which == HJ_R_MATCHED, dOutR, capacity, c->buf[B_R_SWEEP].as<uint32_t>(), c->stream));
    if ((rc = record(c, EV_RROWS1))) return rc;
    c->rRowsCalled = true; c->rRowsCapacity = capacity;
    return HJ_OK;
}

int hj_r_rows_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    if (const int rc = marks_state(c, "hj_r_rows_info")) return rc;
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    out[0] = out[1] = out[2] = 0;               // no hj_r_rows_dev since the build
    out[3] = c->marksRows;
    if (!c->rRowsCalled) return HJ_OK;
    uint32_t produced = 0;                      // the word behind the block counts: their total after the scan
    HJ_HIP(c, hipMemcpy(&produced, c->buf[B_R_SWEEP].as<uint32_t>() + r_sweep_blocks(c->marksRows), sizeof produced, hipMemcpyDeviceToHost));
    out[0] = produced;
    out[1] = produced < c->rRowsCapacity ? produced : c->rRowsCapacity;
    out[2] = (uint64_t)(elapsed_us(c, EV_RROWS0, EV_RROWS1) + 0.5);
    return HJ_OK;
}

// ---- gather through a row map ----------------------------------------------
static bool gather_width_ok(uint32_t w) { return w == 1 || w == 2 || w == 4 || w == 8 || w == 16; }

int hj_gather_dev(hj_ctx* c, const uint32_t* dMap, uint64_t nRows, uint32_t rowBase, uint64_t srcRows, const hj_gather_col* cols,
                  uint32_t nCols, uint32_t* dValid)
{
    HJ_ENTER(c, true);
    if (nCols > HJ_GATHER_MAX_COLS) return fail(c, HJ_ERR_INVALID, "hj_gather_dev: more than HJ_GATHER_MAX_COLS columns");
    if (nCols && !cols) return fail(c, HJ_ERR_INVALID, "hj_gather_dev: cols NULL with nCols > 0");
    if (nRows > 0xFFFFFFFFull || srcRows > 0xFFFFFFFFull) return fail(c, HJ_ERR_INVALID, "hj_gather_dev: nRows or srcRows above 2^32 - 1");
    if (nRows && !dMap) return fail(c, HJ_ERR_INVALID, "hj_gather_dev: dMap NULL with nRows > 0");
    if (nRows && !nCols && !dValid) return fail(c, HJ_ERR_INVALID, "hj_gather_dev: neither a column nor a validity plane");
    GatherCols k{};
    for (uint32_t i = 0; i < nCols; ++i) {
        const hj_gather_col& col = cols[i];
        if (!gather_width_ok(col.width)) return fail(c, HJ_ERR_INVALID, "hj_gather_dev: a width that is not 1, 2, 4, 8 or 16");
        if (col.reserved) return fail(c, HJ_ERR_INVALID, "hj_gather_dev: hj_gather_col.reserved must be 0");
        const uintptr_t low = col.width - 1;
        if (!col.dst || (reinterpret_cast<uintptr_t>(col.dst) & low))
            return fail(c, HJ_ERR_INVALID, "hj_gather_dev: a dst that is NULL or not aligned to its width");
        if (srcRows && (!col.src || (reinterpret_cast<uintptr_t>(col.src) & low)))      // srcRows 0: src is never read
            return fail(c, HJ_ERR_INVALID, "hj_gather_dev: a src that is NULL or not aligned to its width");
        k.col[i] = GatherCol{col.src, col.dst, col.width, 0, {col.fill[0], col.fill[1]}};
    }
    if (nRows == 0) return HJ_OK;
    HJ_HIP(c, hipSetDevice(c->device));
    unsigned long long* const counts = c->buf[B_GATHER_CTR].as<unsigned long long>();
    HJ_HIP(c, hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), c->stream));
    HJ_HIP(c, hipEventRecord(c->evGather[0], c->stream));
    HJ_HIP(c, launch_gather(dMap, nRows, rowBase, srcRows, k, nCols, dValid, counts, c->stream));
    HJ_HIP(c, hipEventRecord(c->evGather[1], c->stream));
    c->gatherCalled = true; c->gatherRows = nRows;
    return HJ_OK;
}

int hj_gather_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    out[0] = out[1] = out[2] = out[3] = 0;      // no hj_gather_dev yet
    if (!c->gatherCalled) return HJ_OK;
    unsigned long long words[2] = {0, 0};        // NULL rows, out-of-range entries
    HJ_HIP(c, hipMemcpy(words, c->buf[B_GATHER_CTR].p, sizeof words, hipMemcpyDeviceToHost));
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->evGather[0], c->evGather[1]) != hipSuccess) ms = 0;
    out[0] = c->gatherRows;
    out[1] = words[0];
    out[2] = (uint64_t)((double)ms * 1000.0 + 0.5);
    out[3] = words[1];
    return HJ_OK;
}

// ---- joins on real key columns: hash, verify, sweep of a caller's plane -----
// The columns of a call, checked: nCols, widths, reserved, and the pointers of the sides in use (rows > 0 on that side)
static const char* key_cols_error(const hj_key_col* cols, uint32_t nCols, bool useS, bool useR)
{
    if (nCols == 0 || nCols > HJ_KEY_MAX_COLS) return "nCols must be 1 .. HJ_KEY_MAX_COLS";
    if (!cols) return "cols NULL";
    for (uint32_t i = 0; i < nCols; ++i) {
        const hj_key_col& col = cols[i];
        if (!gather_width_ok(col.width)) return "a width that is not 1, 2, 4, 8 or 16";
        if (col.reserved) return "hj_key_col.reserved must be 0";
        const uintptr_t low = col.width - 1;
        if (useS && (!col.s || (reinterpret_cast<uintptr_t>(col.s) & low))) return "an S column that is NULL or not aligned to its width";
        if (useR && (!col.r || (reinterpret_cast<uintptr_t>(col.r) & low))) return "an R column that is NULL or not aligned to its width";
    }
    return nullptr;
}

// hj_key_hash_dev's and hj_key_hash_host's arguments -> the kernel's columns; the message of what is wrong, or nullptr
static const char* key_hash_args(const hj_key_col* cols, uint32_t nCols, uint32_t side, uint64_t nRows, const uint64_t* out, KeyCols* k)
{
    if (side > HJ_KEY_SIDE_R) return "side must be HJ_KEY_SIDE_S or HJ_KEY_SIDE_R";
    if (nRows > 0xFFFFFFFFull) return "nRows above 2^32 - 1";
    if (const char* what = key_cols_error(cols, nCols, nRows && side == HJ_KEY_SIDE_S, nRows && side == HJ_KEY_SIDE_R)) return what;
    if (nRows && !out) return "output pointer NULL with nRows > 0";
    for (uint32_t i = 0; i < nCols; ++i) { k->p[i] = side == HJ_KEY_SIDE_S ? cols[i].s : cols[i].r; k->width[i] = cols[i].width; }
    return nullptr;
}

int hj_key_hash_dev(hj_ctx* c, const hj_key_col* cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask, uint64_t* dOutTuples)
{
    HJ_ENTER(c, true);
    KeyCols k{};
    if (const char* what = key_hash_args(cols, nCols, side, nRows, dOutTuples, &k))
        return fail(c, HJ_ERR_INVALID, (std::string("hj_key_hash_dev: ") + what).c_str());
    if (nRows == 0) return HJ_OK;
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, launch_key_hash(k, nCols, nRows, keyMask ? keyMask : 0xFFFFFFFFu, dOutTuples, c->stream));
    return HJ_OK;
}

int hj_key_hash_host(const hj_key_col* cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask, uint64_t* outTuples)
{
    KeyCols k{};
    if (key_hash_args(cols, nCols, side, nRows, outTuples, &k)) return HJ_ERR_INVALID;
    key_hash_host(k, nCols, nRows, keyMask ? keyMask : 0xFFFFFFFFu, outTuples);
    return HJ_OK;
}

int hj_pairs_verify_dev(hj_ctx* c, const uint32_t* dMapS, const uint32_t* dMapR, uint64_t nPairs, uint32_t sRowBase, uint64_t sRows,
                        uint64_t rRows, const hj_key_col* cols, uint32_t nCols, uint32_t* dOutS, uint32_t* dOutR, uint64_t capacity,
                        uint32_t* dSMarks, uint32_t* dRMarks)
{
    HJ_ENTER(c, true);
    if (nPairs > 0xFFFFFFFFull || sRows > 0xFFFFFFFFull || rRows > 0xFFFFFFFFull)
        return fail(c, HJ_ERR_INVALID, "hj_pairs_verify_dev: nPairs, sRows or rRows above 2^32 - 1");
    if (const char* what = key_cols_error(cols, nCols, sRows != 0, rRows != 0))
        return fail(c, HJ_ERR_INVALID, (std::string("hj_pairs_verify_dev: ") + what).c_str());
    if (nPairs && (!dMapS || !dMapR)) return fail(c, HJ_ERR_INVALID, "hj_pairs_verify_dev: a map NULL with nPairs > 0");
    if (nPairs && capacity && (!dOutS || !dOutR)) return fail(c, HJ_ERR_INVALID, "hj_pairs_verify_dev: an output pointer NULL with capacity > 0");
    KeyColsSR k{};
    for (uint32_t i = 0; i < nCols; ++i) { k.s[i] = cols[i].s; k.r[i] = cols[i].r; k.width[i] = cols[i].width; }
    HJ_HIP(c, hipSetDevice(c->device));
    const PairsOut out{dOutS, dOutR, capacity, c->buf[B_VERIFY_CTR].as<unsigned long long>()};
    HJ_HIP(c, hipMemsetAsync(out.cursor, 0, 2 * sizeof(unsigned long long), c->stream));
    HJ_HIP(c, hipEventRecord(c->evVerify[0], c->stream));
    HJ_HIP(c, launch_pairs_verify(dMapS, dMapR, nPairs, sRowBase, (uint32_t)sRows, (uint32_t)rRows, k, nCols, out, dSMarks, dRMarks, c->stream));
    HJ_HIP(c, hipEventRecord(c->evVerify[1], c->stream));
    c->verifyCalled = true; c->verifyCapacity = capacity;
    return HJ_OK;
}

int hj_verify_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    out[0] = out[1] = out[2] = out[3] = 0;      // no hj_pairs_verify_dev yet
    if (!c->verifyCalled) return HJ_OK;
    unsigned long long words[2] = {0, 0};        // pairs kept, candidates dropped
    HJ_HIP(c, hipMemcpy(words, c->buf[B_VERIFY_CTR].p, sizeof words, hipMemcpyDeviceToHost));
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->evVerify[0], c->evVerify[1]) != hipSuccess) ms = 0;
    out[0] = words[0];
    out[1] = words[0] < c->verifyCapacity ? words[0] : c->verifyCapacity;
    out[2] = (uint64_t)((double)ms * 1000.0 + 0.5);
    out[3] = words[1];
    return HJ_OK;
}

int hj_mark_rows_dev(hj_ctx* c, const uint32_t* dMarks, uint64_t rows, uint32_t rowBase, uint32_t which, uint32_t* dOut, uint64_t capacity)
{
    HJ_ENTER(c, true);
    if (which > HJ_R_MATCHED) return fail(c, HJ_ERR_INVALID, "hj_mark_rows_dev: which must be HJ_R_UNMATCHED or HJ_R_MATCHED");
    if (rows > 0xFFFFFFFFull || (uint64_t)rowBase + rows > 0xFFFFFFFFull)
        return fail(c, HJ_ERR_INVALID, "hj_mark_rows_dev: rows or rowBase + rows above 2^32 - 1");
    if (rows && !dMarks) return fail(c, HJ_ERR_INVALID, "hj_mark_rows_dev: dMarks NULL with rows > 0");
    if (rows && capacity && !dOut) return fail(c, HJ_ERR_INVALID, "hj_mark_rows_dev: output pointer NULL with capacity > 0");
    HJ_HIP(c, hipSetDevice(c->device));
    if (const int rc = c->buf[B_MARK_SWEEP].reserve(c, r_sweep_count_words(rows) * sizeof(uint32_t))) return rc;
    HJ_HIP(c, hipEventRecord(c->evMarkRows[0], c->stream));
    // the sweep reads the plane and never writes it
    const RMarks mk{const_cast<uint32_t*>(dMarks), rowBase, (uint32_t)rows};
    HJ_HIP(c, launch_r_sweep(mk, which == HJ_R_MATCHED, dOut, capacity, c->buf[B_MARK_SWEEP].as<uint32_t>(), c->stream));
    HJ_HIP(c, hipEventRecord(c->evMarkRows[1], c->stream));
    c->markRowsCalled = true; c->markRowsRows = rows; c->markRowsCapacity = capacity;
    return HJ_OK;
}

int hj_mark_rows_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    out[0] = out[1] = out[2] = out[3] = 0;      // no hj_mark_rows_dev yet
    if (!c->markRowsCalled) return HJ_OK;
    uint32_t produced = 0;                      // the word behind the block counts: their total after the scan (no block: no row)
    if (c->markRowsRows)
        HJ_HIP(c, hipMemcpy(&produced, c->buf[B_MARK_SWEEP].as<uint32_t>() + r_sweep_blocks(c->markRowsRows), sizeof produced, hipMemcpyDeviceToHost));
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->evMarkRows[0], c->evMarkRows[1]) != hipSuccess) ms = 0;
    out[0] = produced;
    out[1] = produced < c->markRowsCapacity ? produced : c->markRowsCapacity;
    out[2] = (uint64_t)((double)ms * 1000.0 + 0.5);
    out[3] = c->markRowsRows;
    return HJ_OK;
}

int hj_probe_keys_dev(hj_ctx* c, const uint32_t* dKeys, uint64_t n)
{
    HJ_ENTER(c, dKeys || !n);
    if (!c->built || c->htmBuilt) return fail(c, HJ_ERR_STATE, "hj_probe_keys_dev: no open-addressing table (build first)");
    HJ_HIP(c, hipSetDevice(c->device));
    int rc;
    c->probeStartsAtBuildEnd = false;
    if ((rc = record(c, EV_PROBE0))) return rc;
    if (n) launch_probe(dKeys, true, n, c->buf[B_TABLE].as<uint64_t>(), c->tableSize, c->hshift, probe_len(c->params), c->sc, c->dCtr(), c->stream);
    if ((rc = record(c, EV_PROBE1))) return rc;
    HJ_HIP(c, hipGetLastError());
    c->sSize += n;
    return HJ_OK;
}

static PrjBuffers prj_buffers(const hj_ctx* c)
{
    return PrjBuffers{c->buf[B_TMP].as<uint64_t>(), c->buf[B_PART_R].as<uint64_t>(), c->buf[B_PART_S].as<uint64_t>(), c->buf[B_WORK].p};
}

int hj_prj_join_dev(hj_ctx* c, const uint64_t* dR, uint64_t rSize, const uint64_t* dS, uint64_t sSize)
{
    HJ_ENTER(c, dR && rSize);
    if (sSize == 0) dS = nullptr;                    // an empty S is no S (the join kernel clamps its loads to nS - 1)
    if (c->params.algo != HJ_ALGO_PRJ && c->params.algo != HJ_ALGO_AUTO)
        return fail(c, HJ_ERR_STATE, "hj_prj_join_dev: context not reserved for PRJ");
    const uint64_t nmax = rSize > sSize ? rSize : sSize;
    if ((nmax + 2) * sizeof(uint64_t) > c->buf[B_TMP].bytes || (rSize + 2) * sizeof(uint64_t) > c->buf[B_PART_R].bytes ||
        (dS && (sSize + 2) * sizeof(uint64_t) > c->buf[B_PART_S].bytes))
        return fail(c, HJ_ERR_STATE, "hj_prj_join_dev: hj_reserve() not called for these sizes");
    // the plan depends on the sizes (chunking); re-plan with the reserved bit count
    const PrjPlan pl = prj_plan(rSize, dS ? sSize : 0, c->plan.radixBits, c->params.prjMode);
    if (pl.workspaceBytes > c->buf[B_WORK].bytes) return fail(c, HJ_ERR_STATE, "hj_prj_join_dev: workspace too small");
    int rc;
    if ((rc = begin_operation(c, rSize, dS ? sSize : 0, 0))) return rc;
    if ((rc = record(c, EV_PRJ0))) return rc;
    const PrjBuffers buf = prj_buffers(c);
    HJ_HIP(c, launch_prj(pl, buf, dR, rSize, dS, dS ? sSize : 0, c->nCU, c->dCtr(), c->ev[EV_PRJ_PART], c->ev[EV_PRJ_S0],
                         c->ev[EV_PRJ_S1], c->stream));
    c->evSet[EV_PRJ_PART] = c->evSet[EV_PRJ_S0] = c->evSet[EV_PRJ_S1] = true;
    if ((rc = record(c, EV_PRJ1))) return rc;
    HJ_HIP(c, hipGetLastError());
    c->prjRan = true;
    c->prjOptimistic = pl.optimistic;
    c->algoUsed = HJ_ALGO_PRJ;
    return HJ_OK;
}

int hj_prj_build_dev(hj_ctx* c, const uint64_t* dR, uint64_t rSize)
{
    HJ_ENTER(c, dR && rSize);
    if (c->params.algo != HJ_ALGO_PRJ && c->params.algo != HJ_ALGO_AUTO)
        return fail(c, HJ_ERR_STATE, "hj_prj_build_dev: context not reserved for PRJ");
    if ((rSize + 2) * sizeof(uint64_t) > c->buf[B_TMP].bytes || (rSize + 2) * sizeof(uint64_t) > c->buf[B_PART_R].bytes ||
        !c->buf[B_PRJ_RES].p || prj_resident_bytes(c->plan.radixBits, 0) > c->buf[B_PRJ_RES].bytes)
        return fail(c, HJ_ERR_STATE, "hj_prj_build_dev: hj_reserve() not called for this rSize");
    HJ_HIP(c, hipSetDevice(c->device));
    // HJ_FLAG_KEEP_ROW_IDS: R stays resident as {key, row} elements, which only the exact passes carry (mode 1)
    const bool rows = (c->params.flags & HJ_FLAG_KEEP_ROW_IDS) != 0;
    const PrjPlan pl = prj_plan(rSize, 0, c->plan.radixBits, rows ? 1u : c->params.prjMode);    // R's side alone
    int rc;
    // the scratch workspace of the passes holds nothing resident: a relation (here) or a slice (hj_prj_probe_dev) whose plan
    // needs more than hj_reserve's (the chunk count is not monotone in the size, see prj_plan) gets a larger one
    if ((rc = c->buf[B_WORK].reserve(c, pl.workspaceBytes))) return rc;
    if ((rc = marks_begin(c, "hj_prj_build_dev", rSize))) return rc;
    if ((rc = begin_operation(c, rSize, 0, 0))) return rc;
    if ((rc = record(c, EV_PRJ0))) return rc;
    const PrjBuffers buf = prj_buffers(c);
    if (rows) HJ_HIP(c, launch_prj_build_rows(pl, buf, prj_resident_carve(c->buf[B_PRJ_RES].p, pl.radixBits, 0), dR, rSize, c->nCU, c->dCtr(),
                                              c->ev[EV_PRJ_PART], c->ev[EV_PRJ_S0], c->ev[EV_PRJ_S1], c->stream));
    else HJ_HIP(c, launch_prj_build(pl, buf, prj_resident_carve(c->buf[B_PRJ_RES].p, pl.radixBits, 0), dR, rSize, c->nCU, c->dCtr(),
                               c->ev[EV_PRJ_PART], c->ev[EV_PRJ_S0], c->ev[EV_PRJ_S1], c->stream));
    c->evSet[EV_PRJ_PART] = c->evSet[EV_PRJ_S0] = c->evSet[EV_PRJ_S1] = true;
    if ((rc = record(c, EV_PRJ1))) return rc;
    c->prjRan = true;
    c->prjOptimistic = pl.optimistic;
    c->algoUsed = HJ_ALGO_PRJ;
    c->resident = true; c->resPlan = pl; c->resR = rSize; c->resRows = rows;
    c->resProbed = false; c->resProbeOpt = false;
    marks_built(c, rSize, 0);
    return HJ_OK;
}

// whether a slice fits what hj_reserve sized for the probes of a resident R
static bool prj_slice_fits(const hj_ctx* c, uint64_t sSize)
{
    return sSize <= c->prjMaxSlice && (sSize + 2) * sizeof(uint64_t) <= c->buf[B_PART_S].bytes && (sSize + 2) * sizeof(uint64_t) <= c->buf[B_TMP].bytes &&
           prj_resident_bytes(c->resPlan.radixBits, sSize) <= c->buf[B_PRJ_RES].bytes;
}

// One probe of a resident R of {key, row} elements: the slice's row-id passes and the pairs join, timed as a probe
// (EV_RP*); pairsCall: also as a pairs call (EV_PAIRS*), the facts hj_pairs_info reports
static int prj_probe_rows(hj_ctx* c, uint32_t kind, const uint64_t* dS, uint64_t sSize, uint64_t sIdxBase, const PairsOut& out, bool pairsCall)
{
    HJ_HIP(c, hipSetDevice(c->device));
    const PrjPlan pl = prj_plan(sSize, sSize, c->resPlan.radixBits, 1u);     // exact passes only: they carry the rows
    int rc;
    if ((rc = c->buf[B_WORK].reserve(c, pl.workspaceBytes))) return rc;      // R stays resident: see hj_prj_build_dev
    if ((rc = record(c, EV_RP0))) return rc;
    if (pairsCall && (rc = record(c, EV_PAIRS0))) return rc;
    // only a pairs call marks R rows: the counting probe of a rows context keeps the kernel it ran before there were marks
    RMarks mk;
    const RMarks* const marks = pairsCall && marks_for(c, kind, &mk) ? &mk : nullptr;
    HJ_HIP(c, launch_prj_probe_rows(kind, c->resPlan, pl, prj_buffers(c), prj_resident_carve(c->buf[B_PRJ_RES].p, c->resPlan.radixBits, sSize),
                                    dS, sSize, sIdxBase, out, c->nCU, c->dCtr(), c->ev[EV_RP_PART], c->ev[EV_RP_JOIN0], c->stream, marks));
    c->evSet[EV_RP_PART] = c->evSet[EV_RP_JOIN0] = true;
    if (pairsCall && (rc = record(c, EV_PAIRS1))) return rc;
    if ((rc = record(c, EV_RP1))) return rc;
    c->sSize += sSize;
    c->resProbed = true; c->resProbeOpt = false;
    return HJ_OK;
}

int hj_prj_probe_dev(hj_ctx* c, const uint64_t* dS, uint64_t sSize)
{
    HJ_ENTER(c, dS || !sSize);
    if (!c->resident) return fail(c, HJ_ERR_STATE, "hj_prj_probe_dev: no resident R (call hj_prj_build_dev first)");
    if (!prj_slice_fits(c, sSize)) return fail(c, HJ_ERR_STATE, "hj_prj_probe_dev: slice larger than the sSize given to hj_reserve()");
    if (sSize == 0) return HJ_OK;
    if (c->resRows) {
        // R holds {key, row} elements, which the counting kernels cannot read: the pairs join with capacity 0, counting into
        // a word of its own (stats[4]: past the four the work items use) so that hj_pairs_info keeps the last pairs call
        const PrjResident res = prj_resident_carve(c->buf[B_PRJ_RES].p, c->resPlan.radixBits, sSize);
        // (and the word behind it, which HJ_JOIN_INNER leaves at zero)
        return prj_probe_rows(c, HJ_JOIN_INNER, dS, sSize, 0, PairsOut{nullptr, nullptr, 0, res.stats + 4}, false);
    }
    HJ_HIP(c, hipSetDevice(c->device));
    const PrjPlan pl = prj_plan(sSize, sSize, c->resPlan.radixBits, c->params.prjMode);   // fragS: the slice's own geometry
    int rc;
    if ((rc = c->buf[B_WORK].reserve(c, pl.workspaceBytes))) return rc;      // R stays resident: see hj_prj_build_dev
    if ((rc = record(c, EV_RP0))) return rc;
    const PrjBuffers buf = prj_buffers(c);
    HJ_HIP(c, launch_prj_probe(c->resPlan, c->resR, pl, buf, prj_resident_carve(c->buf[B_PRJ_RES].p, c->resPlan.radixBits, sSize), dS, sSize,
                               c->nCU, c->dCtr(), c->ev[EV_RP_PART], c->ev[EV_RP_JOIN0], c->stream));
    c->evSet[EV_RP_PART] = c->evSet[EV_RP_JOIN0] = true;
    if ((rc = record(c, EV_RP1))) return rc;
    c->sSize += sSize;
    c->resProbed = true; c->resProbeOpt = pl.optimistic;
    return HJ_OK;
}

// The one host sequence of the materialising radix probe; fn: the entry point's name, for the error texts
static int prj_probe_join(hj_ctx* c, const char* fn, uint32_t kind, const uint64_t* dS, uint64_t sSize, uint64_t sIdxBase, uint32_t* dOutS,
                          uint32_t* dOutR, uint64_t capacity)
{
    HJ_ENTER(c, dS || !sSize);
    const std::string f(fn);
    if (kind > HJ_JOIN_ANTI) return fail(c, HJ_ERR_INVALID, (f + ": kind must be an hj_join_kind").c_str());
    const bool planeR = kind <= HJ_JOIN_LEFT;            // SEMI and ANTI write S rows only: dOutR is ignored
    if (!c->resident) return fail(c, HJ_ERR_STATE, (f + ": no resident R (call hj_prj_build_dev first)").c_str());
    if (!c->resRows) return fail(c, HJ_ERR_STATE, (f + ": R was built without HJ_FLAG_KEEP_ROW_IDS").c_str());
    if (!prj_slice_fits(c, sSize)) return fail(c, HJ_ERR_STATE, (f + ": slice larger than the sSize given to hj_reserve()").c_str());
    if (capacity && (!dOutS || (planeR && !dOutR))) return fail(c, HJ_ERR_INVALID, (f + ": output pointer NULL with capacity > 0").c_str());
    if (sIdxBase > 0xFFFFFFFFull || sIdxBase + sSize > 0xFFFFFFFFull)
        return fail(c, HJ_ERR_INVALID, (f + ": S row range exceeds 2^32 - 1").c_str());
    if (sSize == 0) return HJ_OK;
    const PairsOut out{dOutS, planeR ? dOutR : nullptr, capacity, c->buf[B_PAIRS_CURSOR].as<unsigned long long>()};
    const int rc = prj_probe_rows(c, kind, dS, sSize, sIdxBase, out, true);
    if (rc == HJ_OK) { c->pairsCapacity = capacity; c->pairsKind = kind; c->pairsS = sSize; }
    return rc;
}

// (No R row is HJ_NO_ROW: hj_reserve refuses rSize >= 2^32 - 1 for PRJ and hj_prj_build_dev takes no more than was reserved,
// so the largest row is 2^32 - 3 and HJ_JOIN_LEFT needs no check of its own.)
int hj_prj_probe_join_dev(hj_ctx* c, uint32_t kind, const uint64_t* dS, uint64_t sSize, uint64_t sIdxBase, uint32_t* dOutS, uint32_t* dOutR,
                          uint64_t capacity)
{
    return prj_probe_join(c, "hj_prj_probe_join_dev", kind, dS, sSize, sIdxBase, dOutS, dOutR, capacity);
}

int hj_prj_probe_pairs_dev(hj_ctx* c, const uint64_t* dS, uint64_t sSize, uint64_t sIdxBase, uint32_t* dOutS, uint32_t* dOutR,
                           uint64_t capacity)
{
    return prj_probe_join(c, "hj_prj_probe_pairs_dev", HJ_JOIN_INNER, dS, sSize, sIdxBase, dOutS, dOutR, capacity);
}

int hj_prj_resident_info(hj_ctx* c, uint64_t out[8])
{
    HJ_ENTER(c, out);
    if (!c->resident) return fail(c, HJ_ERR_STATE, "hj_prj_resident_info: no resident R");
    HJ_HIP(c, hipSetDevice(c->device));
    const PrjResident res = prj_resident_carve(c->buf[B_PRJ_RES].p, c->resPlan.radixBits, 0);
    unsigned long long st[4];
    HJ_HIP(c, hipMemcpyAsync(st, res.stats, sizeof st, hipMemcpyDeviceToHost, c->stream));
    if (const int rc = read_counters(c, false)) return rc;
    const PrjPlan& pl = c->resPlan;
    const bool fragR = pl.optimistic && c->hCtr->prjFallbackR == 0;
    const uint64_t P = 1ull << pl.radixBits;
    out[0] = !pl.optimistic ? 0u : (c->hCtr->prjFallbackR ? 2u : 1u);
    out[1] = (!c->resProbed || !c->resProbeOpt) ? 0u : (c->hCtr->prjFallback ? 2u : 1u);
    out[2] = st[1]; out[3] = st[2]; out[4] = st[3];
    // R's keys (the fragments with their slack, or one dense run) + its offsets and fragment counts
    // (reserved with HJ_FLAG_KEEP_ROW_IDS: one dense run of 8-byte {key, row} elements)
    out[5] = (c->resRows ? 8 * c->resR : 4 * (fragR ? P * pl.fragR.C2 * pl.fragR.cap2 : c->resR)) + 4 * (P + 1) + 4 * P * 16;
    out[6] = out[7] = 0;
    return HJ_OK;
}

int hj_join_dev(hj_ctx* c, const uint64_t* dR, uint64_t rSize, const uint64_t* dS, uint64_t sSize)
{
    if (!c || !dR || rSize == 0) return HJ_ERR_INVALID;
    if (!dS) sSize = 0;
    if (sSize == 0) dS = nullptr;
    int rc;
    bool prj = c->params.algo == HJ_ALGO_PRJ;
    uint32_t force = 0;
    if (c->params.algo == HJ_ALGO_AUTO) {
        // the same question the build asks itself for buildVariant 0, asked once here: with locality the
        // LDS-window build + linear probe wins, without it both of them turn into random HBM accesses
        // and two radix passes are cheaper
        HJ_HIP(c, hipSetDevice(c->device));
        if (!is_pow2(rSize) || rSize > (1ull << 31)) return hj_prj_join_dev(c, dR, rSize, dS, sSize);   // see hj_reserve
        if ((2 * rSize + kTableSlack) * sizeof(uint64_t) > c->buf[B_TABLE].bytes)
            return fail(c, HJ_ERR_STATE, "hj_join_dev: hj_reserve() not called for this rSize");
        const BuildCaps can = build_caps(c, rSize, 2 * rSize);
        uint32_t v = 1;
        if ((can.own || can.wave) && c->params.buildVariant != 1 &&
            (rc = sample_variant(c, dR, false, rSize, 2 * rSize, 0, can, &v))) return rc;
        // no locality: both table phases would be random HBM accesses. Loose locality (variant 2) pays for every tuple
        // that leaves its window with global atomics: at 2^27, local_shuffle W=2^11 (3.8 % deferred) the table join
        // takes 1.09 ms against the radix join's 1.81 ms, at W=2^12 (36 % deferred) 2.79 against 1.83 (round 3, deferred
        // queue sliced per workgroup; 2.06 / 1.89 at W=2^11 before): the radix join from 1/8 of the sample outside the window.
        prj = v == 1 || (v == 2 && (uint64_t)c->hFit[0] * 8u > c->hFit[1]);
        force = v;
    }
    if (prj) return hj_prj_join_dev(c, dR, rSize, dS, sSize);
    c->forceVariant = force;
    rc = hj_build_dev(c, dR, rSize, 0);
    c->forceVariant = 0;
    if (rc) return rc;
    return hj_probe_dev(c, dS, sSize);
}

int hj_checksums_dev(hj_ctx* c)
{
    HJ_ENTER(c, true);
    if (!c->built) return fail(c, HJ_ERR_STATE, "hj_checksums_dev: no table");
    HJ_HIP(c, hipSetDevice(c->device));
    // zero the two sums so the call is idempotent
    HJ_HIP(c, hipMemsetAsync(&c->dCtr()->tableSumHalf, 0, 2 * sizeof(unsigned long long), c->stream));
    if (c->htmBuilt) {
        HJ_HIP(c, hipMemsetAsync(&c->dCtr()->htmOverflowSum, 0, sizeof(unsigned long long), c->stream));
        launch_htm_sums(c->buf[B_TABLE].as<uint64_t>(), c->htmBuckets, c->buf[B_HTM_OVERFLOW].as<uint64_t>(), c->dCtr(), c->stream);
        HJ_HIP(c, hipGetLastError());
        return HJ_OK;
    }
    launch_table_sums(c->buf[B_TABLE].as<uint64_t>(), c->tableSize, c->tableSize / 2, c->dCtr(), c->stream);
    HJ_HIP(c, hipGetLastError());
    return HJ_OK;
}

int hj_fetch_result(hj_ctx* c, hj_result* out)
{
    HJ_ENTER(c, out);
    HJ_HIP(c, hipSetDevice(c->device));
    if (const int rc = read_counters(c, true)) return rc;
    memset(out, 0, sizeof(*out));
    const Counters& k = *c->hCtr;
    out->rSize = c->rSize; out->sSize = c->sSize; out->tableSize = c->tableSize;
    out->inputSum = k.inputSum;
    if (c->prjRan) {
        out->totalMatches = k.prjMatches;
        out->prjChecksum = k.prjChecksum;
        out->prjPartitions = 1ull << c->plan.radixBits;
        out->radixBits = c->plan.radixBits;
        out->partition_us = elapsed_us(c, EV_PRJ0, EV_PRJ_PART);
        out->join_us = elapsed_us(c, EV_PRJ_PART, EV_PRJ1);
        out->total_us = elapsed_us(c, EV_PRJ0, EV_PRJ1);
        out->prjScatterPass1R_us = elapsed_us(c, EV_PRJ_S0, EV_PRJ_S1);
        out->prjPath = !c->prjOptimistic ? 0u : (k.prjFallback ? 2u : 1u);
        if (c->resident) {
            // resident R: the build's passes (partition_us, build_us = passes + R's checksum), the last probe (probe_us = S's
            // passes + work items + join, join_us = the join kernel alone); prjPath = R's path
            out->build_us = elapsed_us(c, EV_PRJ0, EV_PRJ1);
            out->probe_us = elapsed_us(c, EV_RP0, EV_RP1);
            out->join_us = elapsed_us(c, EV_RP_JOIN0, EV_RP1);
            out->total_us = out->build_us + out->probe_us;
            out->prjPath = !c->prjOptimistic ? 0u : (k.prjFallbackR ? 2u : 1u);
        }
    } else {
        out->conflicts = k.conflicts;
        out->conflictSum = k.conflictSum;
        out->totalMatches = k.matches;
        out->tableSumHalf = k.tableSumHalf;
        out->tableSumFull = k.tableSumFull;
        out->outputSum = (c->params.algo == HJ_ALGO_NOCC ? k.tableSumHalf : k.tableSumFull) + k.conflictSum;
        if (c->htmBuilt) {
            // every conflict sits in an overflow bucket of its own bucket's chain: tuples in buckets + tuples in
            // chains = input (HTMHashBuild.hpp:452 adds conflictSum on top of the chains, counting them twice)
            out->htmBuckets = c->htmBuckets; out->htmOverflowBuckets = k.htmOverflowBuckets; out->htmOverflowSum = k.htmOverflowSum;
            out->outputSum = k.tableSumFull + k.htmOverflowSum;
        }
        out->buildVariant = c->variantUsed ? c->variantUsed : (uint32_t)k.variant;   // 0: the device chose
        out->compactFallback = k.compactFail | ((c->htmBuilt && c->htmChainsFellBack) ? 0x100ull : 0ull);
        out->buildDeferred = k.deferred;
        // the dominant build kernel ALONE: the launch of the LDS build that ran is bracketed by its own pair of events (the
        // launches of the variants the device did not pick return at once: microseconds; the largest bracket is the kernel).
        // After a hand-over more than one build kernel ran. compact -> classic: the sum of their brackets. planar -> packed:
        // the packed redo has no bracket of its own (two more event records on every step, for a road `uniform` never takes),
        // so the whole build group stands for it: never flattering.
        out->buildPhaseA_us = 0.0;
        static const Ev kBrackets[3][2] = {{EV_KW0, EV_KW1}, {EV_KC0, EV_KC1}, {EV_KO0, EV_KO1}};
        for (const auto& pr : kBrackets) {
            const double us = elapsed_us(c, pr[0], pr[1]);
            if (k.compactFail != 0) out->buildPhaseA_us += us;
            else if (us > out->buildPhaseA_us) out->buildPhaseA_us = us;
        }
        out->clear_us = elapsed_us(c, EV_CLEAR0, EV_BUILD0);
        out->build_us = elapsed_us(c, EV_BUILD0, EV_BUILD1);
        if (k.planarFail != 0) out->buildPhaseA_us = out->build_us;
        out->probe_us = elapsed_us(c, c->probeStartsAtBuildEnd ? EV_BUILD1 : EV_PROBE0, EV_PROBE1);
        // the reference's timed region is build+probe, table zeroing excluded
        // (NoCCHashBuild.hpp:24-34,83); clear_us is reported beside it
        out->total_us = out->build_us + out->probe_us;
    }
    out->h2d_us = c->h2d_us;
    out->algoUsed = c->algoUsed;
    out->foreignTuples = k.foreign;
    if (k.badKeys) return fail(c, HJ_ERR_KEY_RANGE, "input holds tuples with payload bits set or value 0");
    return HJ_OK;
}

int hj_export_table(hj_ctx* c, uint64_t* host_table, uint64_t tableSize)
{
    HJ_ENTER(c, host_table);
    if (!c->built || c->htmBuilt || tableSize != c->tableSize) return fail(c, HJ_ERR_STATE, "hj_export_table: no open-addressing table of that size");
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    Counters k;
    HJ_HIP(c, hipMemcpy(&k, c->dCtr(), sizeof(k), hipMemcpyDeviceToHost));
    // only [validLo, validHiEx + 512) holds defined values (hj_device.h); the rest is empty by definition
    const uint64_t lo = k.validLo, hi = k.validHiEx + 512 < tableSize ? k.validHiEx + 512 : tableSize;
    if (k.tableFormat == kFormatKeys4) {
        // compact device format (4-byte keys, 0xFFFFFFFF = empty) -> reference format (key, 0 = empty): the keys land in
        // the upper half of the caller's buffer and are widened from the front (the write position never passes the read one)
        uint32_t* keys = reinterpret_cast<uint32_t*>(host_table) + tableSize;
        HJ_HIP(c, hipMemcpy(keys, c->buf[B_TABLE].p, tableSize * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < tableSize; ++i) {
            const uint32_t v = keys[i];
            host_table[i] = (i < lo || i >= hi || v == 0xFFFFFFFFu) ? 0 : v;
        }
        return HJ_OK;
    }
    HJ_HIP(c, hipMemcpy(host_table, c->buf[B_TABLE].p, tableSize * sizeof(uint64_t), hipMemcpyDeviceToHost));
    // device format (index << 32 | key, all ones = empty) -> reference format (key, 0 = empty)
    for (uint64_t i = 0; i < tableSize; ++i)
        host_table[i] = (i < lo || i >= hi || host_table[i] == kEmpty) ? 0 : (uint32_t)host_table[i];
    return HJ_OK;
}

int hj_export_buckets(hj_ctx* c, void* host_buckets, uint64_t numBuckets, void* host_overflows, uint64_t overflowCap,
                      uint64_t* nOverflow)
{
    HJ_ENTER(c, host_buckets);
    if (!c->htmBuilt || numBuckets != c->htmBuckets) return fail(c, HJ_ERR_STATE, "hj_export_buckets: no htm table of that many buckets");
    HJ_HIP(c, hipSetDevice(c->device));
    if (const int rc = read_counters(c, true)) return rc;
    const uint64_t used = c->hCtr->htmOverflowBuckets;
    if (nOverflow) *nOverflow = used;
    if (used && (!host_overflows || overflowCap < used + 1)) return fail(c, HJ_ERR_INVALID, "hj_export_buckets: overflow buffer too small");
    // device format (index << 32 | key, all ones = empty; slot 3 = next << 32 | count, or all ones = "no chain") ->
    // struct Bucket {tuples[3], count, nextIndex}; buckets [lo, hi) are the ones the build defined, the rest are empty
    auto convert = [](uint64_t* b, uint64_t n, uint64_t lo, uint64_t hi) {
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t* p = b + 4 * i;
            if (i < lo || i >= hi) { p[0] = p[1] = p[2] = p[3] = 0; continue; }
            uint32_t count = 0;
            for (int j = 0; j < 3; ++j) { count += p[j] != kEmpty; p[j] = (p[j] == kEmpty) ? 0 : (uint32_t)p[j]; }
            // a bucket with a link word carries its count there: that stored word is what is exported, not a recount
            if (p[3] != kEmpty) count = (uint32_t)p[3];
            const uint32_t next = p[3] == kEmpty ? 0u : (uint32_t)(p[3] >> 32);
            p[3] = (uint64_t)count | ((uint64_t)next << 32);     // little-endian {uint32 count; uint32 nextIndex}
        }
    };
    const uint64_t defLo = c->hCtr->validLo >> 2;
    uint64_t defHi = (c->hCtr->validHiEx + 512) >> 2;
    defHi = defHi < numBuckets ? defHi : numBuckets;
    HJ_HIP(c, hipMemcpy(host_buckets, c->buf[B_TABLE].p, numBuckets * 32, hipMemcpyDeviceToHost));
    convert(static_cast<uint64_t*>(host_buckets), numBuckets, defLo, defHi);
    if (host_overflows) {
        memset(host_overflows, 0, 32);                           // index 0 is unused (as in the reference)
        if (used) {
            HJ_HIP(c, hipMemcpy(static_cast<char*>(host_overflows) + 32, c->buf[B_HTM_OVERFLOW].as<uint64_t>() + 4, used * 32, hipMemcpyDeviceToHost));
            convert(static_cast<uint64_t*>(host_overflows) + 4, used, 0, used);
        }
    }
    return HJ_OK;
}

int hj_run(hj_ctx* c, const hj_params* params, const uint64_t* relR, uint64_t rSize,
           const uint64_t* relS, uint64_t sSize, hj_result* out)
{
    if (!c || !params || !relR || !out) return HJ_ERR_INVALID;
    if (!relS) sSize = 0;
    int rc;
    if ((rc = hj_reserve(c, params, rSize, sSize))) return rc;
    if ((rc = c->buf[B_STAGE_R].reserve(c, (rSize + 2) * sizeof(uint64_t)))) return rc;
    if (sSize && (rc = c->buf[B_STAGE_S].reserve(c, (sSize + 2) * sizeof(uint64_t)))) return rc;
    uint64_t* const stageR = c->buf[B_STAGE_R].as<uint64_t>();
    uint64_t* const stageS = c->buf[B_STAGE_S].as<uint64_t>();
    const auto t0 = std::chrono::steady_clock::now();
    HJ_HIP(c, hipMemcpyAsync(stageR, relR, rSize * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    if (sSize) HJ_HIP(c, hipMemcpyAsync(stageS, relS, sSize * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    c->h2d_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if ((rc = hj_join_dev(c, stageR, rSize, sSize ? stageS : nullptr, sSize))) return rc;
    if (!c->prjRan && (rc = hj_checksums_dev(c))) return rc;
    return hj_fetch_result(c, out);
}

int hj_prj_fragment_info(uint64_t rSize, uint64_t sSize, uint32_t radixBits, uint32_t prjMode, uint64_t out[13])
{
    if (!out || radixBits > 16 || prjMode > 2) return HJ_ERR_INVALID;
    const uint32_t bits = radixBits ? radixBits : auto_radix_bits(rSize);
    const PrjPlan pl = prj_plan(rSize, sSize, bits, prjMode);
    out[0] = pl.optimistic ? 1 : 0;
    const PrjFrag* g[2] = {&pl.fragR, &pl.fragS};
    for (int k = 0; k < 2; ++k) {
        uint64_t* o = out + 1 + 5 * k;
        o[0] = g[k]->C1; o[1] = g[k]->cap1; o[2] = g[k]->chunkLen1; o[3] = g[k]->C2; o[4] = g[k]->cap2;
    }
    out[11] = pl.bits1; out[12] = pl.bits2;
    return HJ_OK;
}

int hj_wave_layout_info(const hj_ctx* c, uint32_t computeUnits, uint64_t n, uint64_t out[16])
{
    if (!out || (!c && (computeUnits == 0 || computeUnits > 65536)) || n > 0xFFFFFFFFull) return HJ_ERR_INVALID;
    const int nCU = c ? c->nCU : (int)computeUnits;
    const WaveLayout w = wave_layout(n, nCU);
    const uint64_t v[16] = {w.chunkLen, w.nChunks, w.sliceLen, w.tileTuples, w.granSlots, w.ringGran, w.look, w.overlap,
                            w.shadow, w.tail, w.predCap, w.compactMaxProbe, (uint64_t)nCU, 0, 0, 0};
    memcpy(out, v, sizeof v);
    return HJ_OK;
}

int hj_wave_seams(hj_ctx* c, uint32_t* starts, uint32_t* bounds, uint32_t* pcounts, uint64_t capacity, uint64_t* nChunks)
{
    HJ_ENTER(c, starts && bounds && nChunks);
    if (!c->built || !c->wavePreN) return fail(c, HJ_ERR_STATE, "hj_wave_seams: the last build did not run the ring pre-pass");
    HJ_HIP(c, hipSetDevice(c->device));
    if (const int rc = read_counters(c, false)) return rc;
    // buildVariant 0: the pre-pass was enqueued behind the device's pick and ran only if that pick was the rings
    if (c->wavePreGated && c->hCtr->variant != 3 && c->hCtr->variant != 4)
        return fail(c, HJ_ERR_STATE, "hj_wave_seams: the last build did not run the ring pre-pass");
    const uint64_t chunks = wave_layout(c->wavePreN, c->nCU).nChunks;
    *nChunks = chunks;
    if (capacity < chunks + 1) return fail(c, HJ_ERR_INVALID, "hj_wave_seams: capacity below the number of chunks + 1");
    const WaveScratch w(c->nCU, c->buf[B_BOUNDS].p);
    HJ_HIP(c, hipMemcpy(starts, w.starts, (chunks + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HJ_HIP(c, hipMemcpy(bounds, w.bounds, (chunks + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (pcounts) HJ_HIP(c, hipMemcpy(pcounts, w.pcounts, chunks * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return HJ_OK;
}

int hj_htm_chain_layout_info(const hj_ctx* c, uint32_t computeUnits, uint64_t n, uint64_t out[8])
{
    if (!out || (!c && (computeUnits == 0 || computeUnits > 65536)) || n == 0 || n > 0xFFFFFFFFull) return HJ_ERR_INVALID;
    const int nCU = c ? c->nCU : (int)computeUnits;
    const WaveLayout w = wave_layout(n, nCU);
    const uint64_t v[8] = {w.nChunks, w.sliceLen, htm_chain_parts((uint32_t)w.sliceLen), kChainCountCap, kChainCap, kChainMaxParts,
                           kChainPartTuples,
                           // build_htm's rule for a request for the rings: they must take the table at all (wave_supported), and
                           // the phase's scratch must fit (htm_chain_tries -- which every table the rings take satisfies)
                           (wave_supported(4ull * htm_num_buckets(n)) &&
                            htm_chain_tries((uint32_t)w.nChunks, (uint32_t)w.sliceLen, htm_num_buckets(n))) ? 1u : 0u};
    memcpy(out, v, sizeof v);
    return HJ_OK;
}

int hj_htm_chain_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    if (!c->built || !c->htmBuilt) return fail(c, HJ_ERR_STATE, "hj_htm_chain_info: no htm table (call hj_build_dev on a context reserved for HJ_ALGO_HTM)");
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    out[0] = c->htmChainState; out[1] = c->htmChainCause; out[2] = c->htmChainGroups; out[3] = 0;
    return HJ_OK;
}

int hj_wave_planar_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    if (!c->built || c->htmBuilt) return fail(c, HJ_ERR_STATE, "hj_wave_planar_info: no open-addressing table");
    HJ_HIP(c, hipSetDevice(c->device));
    if (const int rc = read_counters(c, false)) return rc;
    const Counters& k = *c->hCtr;
    const uint32_t variant = c->variantUsed ? c->variantUsed : (uint32_t)k.variant;
    out[0] = (variant == 3 && k.tableFormat == kFormatKeys4) ? 1 : 0;
    out[1] = k.planarFail;
    out[2] = k.tableFormat;
    out[3] = 0;
    return HJ_OK;
}

int hj_table_debug(hj_ctx* c, uint64_t out[6])
{
    HJ_ENTER(c, out);
    if (!c->built) return fail(c, HJ_ERR_STATE, "hj_table_debug: no table (call hj_build_dev first)");
    HJ_HIP(c, hipSetDevice(c->device));
    if (const int rc = read_counters(c, false)) return rc;
    const Counters& k = *c->hCtr;
    out[0] = k.validLo; out[1] = k.validHiEx;
    out[2] = k.tableFormat;
    out[3] = c->tableSize;                                   // htm: 4 slots per bucket
    out[4] = (uint64_t)reinterpret_cast<uintptr_t>(c->buf[B_TABLE].p);
    out[5] = c->buf[B_TABLE].bytes;
    return HJ_OK;
}

int hj_prj_workspace_info(uint64_t rSize, uint64_t sSize, uint32_t radixBits, uint64_t out[4])
{
    if (!out || radixBits > 16) return HJ_ERR_INVALID;
    const uint32_t bits = radixBits ? radixBits : auto_radix_bits(rSize);
    const PrjPlan pl = prj_plan(rSize, sSize, bits);
    out[0] = pl.workspaceBytes; out[1] = pl.histEntries;
    out[2] = prj_hist_entries_needed(rSize, bits); out[3] = prj_hist_entries_needed(sSize, bits);
    return HJ_OK;
}

// ---- streaming Zipf generator ---------------------------------------------------
int hj_zipf_open(hj_ctx* c, uint64_t alphabetSize, double theta, unsigned seed)
{
    if (!c) return HJ_ERR_INVALID;
    if (alphabetSize == 0 || alphabetSize > 0xFFFFFFFFull || !(theta >= 0.0)) return fail(c, HJ_ERR_INVALID, "hj_zipf_open: alphabet in [1, 2^32), theta >= 0");
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    zipf_release(c);
    c->zipfRng = new (std::nothrow) hjhost::GlibcRand(seed);
    if (!c->zipfRng) return HJ_ERR_OOM;
    std::vector<uint32_t> alphabet;
    std::vector<double> lut;
    hjhost::zipf_tables(*c->zipfRng, (uint32_t)alphabetSize, theta, alphabet, lut);       // consumes alphabetSize - 1 draws
    HJ_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->zipfLut), alphabetSize * sizeof(double)));
    HJ_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->zipfAlphabet), alphabetSize * sizeof(uint32_t)));
    HJ_HIP(c, hipMemcpy(c->zipfLut, lut.data(), alphabetSize * sizeof(double), hipMemcpyHostToDevice));
    HJ_HIP(c, hipMemcpy(c->zipfAlphabet, alphabet.data(), alphabetSize * sizeof(uint32_t), hipMemcpyHostToDevice));
    c->zipfAlphabetSize = (uint32_t)alphabetSize;
    for (int i = 0; i < 2; ++i) HJ_HIP(c, hipEventCreateWithFlags(&c->zipfDone[i], hipEventDisableTiming));
    return HJ_OK;
}

int hj_zipf_next_dev(hj_ctx* c, uint64_t n, uint64_t* dOut)
{
    HJ_ENTER(c, dOut || !n);
    if (!c->zipfRng) return fail(c, HJ_ERR_STATE, "hj_zipf_next_dev: hj_zipf_open() first");
    HJ_HIP(c, hipSetDevice(c->device));
    // pieces of at most 2^26 draws through two pinned buffers: the host draws piece k + 1 of the serial rand() stream
    // while the device still copies and searches piece k
    const uint64_t piece = 1ull << 26;
    if (c->zipfRawCap == 0) {
        for (int i = 0; i < 2; ++i) {
            HJ_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&c->zipfRawHost[i]), piece * sizeof(int)));
            HJ_HIP(c, hipMalloc(reinterpret_cast<void**>(&c->zipfRawDev[i]), piece * sizeof(int)));
        }
        c->zipfRawCap = piece;
    }
    for (uint64_t off = 0; off < n; off += piece) {
        const uint64_t m = n - off < piece ? n - off : piece;
        const int b = c->zipfFlip;
        c->zipfFlip ^= 1;
        HJ_HIP(c, hipEventSynchronize(c->zipfDone[b]));          // the previous use of this buffer pair has been consumed
        int* h = c->zipfRawHost[b];
        for (uint64_t i = 0; i < m; ++i) h[i] = c->zipfRng->next();
        HJ_HIP(c, hipMemcpyAsync(c->zipfRawDev[b], h, m * sizeof(int), hipMemcpyHostToDevice, c->stream));
        launch_zipf_lookup(c->zipfRawDev[b], m, c->zipfLut, c->zipfAlphabet, c->zipfAlphabetSize, dOut + off, c->stream);
        HJ_HIP(c, hipGetLastError());
        HJ_HIP(c, hipEventRecord(c->zipfDone[b], c->stream));
    }
    return HJ_OK;
}

int hj_zipf_close(hj_ctx* c)
{
    if (!c) return HJ_ERR_INVALID;
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    zipf_release(c);
    return HJ_OK;
}

// ---- shard helpers -----------------------------------------------------------
int hj_set_shard_check(hj_ctx* c, uint32_t nShards, uint32_t mode, uint32_t shardId)
{
    if (!c) return HJ_ERR_INVALID;
    if (nShards == 0) { c->sc = ShardCheck{0, 0, 0, 0}; return HJ_OK; }
    if (!is_pow2(nShards) || nShards > 64 || shardId >= nShards || (mode & 0xFFu) > 31 || (mode >> 9) != 0)
        return fail(c, HJ_ERR_INVALID, "hj_set_shard_check: nShards a power of two <= 64, shardId < nShards, mode as for hj_shard_histogram_dev");
    c->sc = ShardCheck{nShards - 1, mode & 0xFFu, (mode >> 8) & 1u, shardId};
    return HJ_OK;
}

static int shard_check(hj_ctx* c, const char* who, uint64_t n, uint32_t nShards, uint32_t mode)
{
    if (!is_pow2(nShards) || nShards > 64) return fail(c, HJ_ERR_INVALID, who);
    if ((mode & 0xFFu) > 31 || (mode >> 9) != 0)
        return fail(c, HJ_ERR_INVALID, "shard helpers: mode = digit position (0..31), optionally | HJ_SHARD_ONE_BASED");
    if (n >= 0xFFFFFFFFull) return fail(c, HJ_ERR_INVALID, "shard helpers: n must be < 2^32");
    return HJ_OK;
}

int hj_shard_histogram_dev(hj_ctx* c, const uint64_t* dIn, uint64_t n, uint32_t nShards, uint32_t mode,
                           uint64_t* dCounts)
{
    HJ_ENTER(c, (dIn || !n) && dCounts);
    int rc = shard_check(c, "hj_shard_histogram_dev: nShards must be a power of two <= 64", n, nShards, mode);
    if (rc) return rc;
    HJ_HIP(c, hipSetDevice(c->device));
    // reuse the slot of the same input, else the least recently used one
    hj_ctx::ShardPlan* slot = &c->shard[0];
    for (auto& sp : c->shard) if (sp.in == dIn && sp.n == n) { slot = &sp; break; } else if (sp.stamp < slot->stamp) slot = &sp;
    DevBuf& work = c->buf[B_SHARD0 + (slot - c->shard)];
    if ((rc = work.reserve(c, shard_work_bytes(n, nShards)))) return rc;
    slot->in = dIn; slot->n = n; slot->nShards = nShards; slot->mode = mode; slot->stamp = ++c->shardStamp;
    HJ_HIP(c, launch_shard_hist(dIn, n, nShards, mode, work.p, reinterpret_cast<unsigned long long*>(dCounts), c->stream));
    return HJ_OK;
}

int hj_shard_scatter_dev(hj_ctx* c, const uint64_t* dIn, uint64_t n, uint32_t nShards, uint32_t mode,
                         const uint64_t* dCounts, uint32_t* dOutKeys)
{
    HJ_ENTER(c, (dIn || !n) && dCounts && (dOutKeys || !n));
    int rc = shard_check(c, "hj_shard_scatter_dev: nShards must be a power of two <= 64", n, nShards, mode);
    if (rc) return rc;
    hj_ctx::ShardPlan* slot = nullptr;
    for (auto& sp : c->shard) if (sp.in == dIn && sp.n == n && sp.nShards == nShards && sp.mode == mode && c->buf[B_SHARD0 + (&sp - c->shard)].p) slot = &sp;
    if (!slot) return fail(c, HJ_ERR_STATE, "hj_shard_scatter_dev: call hj_shard_histogram_dev on this input (same nShards and mode) first");
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, launch_shard_scatter_ordered(dIn, n, nShards, mode, c->buf[B_SHARD0 + (slot - c->shard)].p, dOutKeys, c->stream));
    slot->in = nullptr;   // consumed
    return HJ_OK;
}

// ---- raw device memory ---------------------------------------------------------
int hj_dev_alloc(hj_ctx* c, uint64_t bytes, void** dptr)
{
    if (!c || !dptr) return HJ_ERR_INVALID;
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipMalloc(dptr, bytes ? bytes : 16));
    return HJ_OK;
}

int hj_dev_free(hj_ctx* c, void* dptr)
{
    if (!c) return HJ_ERR_INVALID;
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    if (dptr) HJ_HIP(c, hipFree(dptr));
    return HJ_OK;
}

int hj_copy_h2d(hj_ctx* c, void* dst_dev, const void* src_host, uint64_t bytes)
{
    HJ_ENTER(c, dst_dev && src_host);
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, c->stream));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    return HJ_OK;
}

int hj_copy_d2h(hj_ctx* c, void* dst_host, const void* src_dev, uint64_t bytes)
{
    HJ_ENTER(c, dst_host && src_dev);
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    return HJ_OK;
}

}  // extern "C"
