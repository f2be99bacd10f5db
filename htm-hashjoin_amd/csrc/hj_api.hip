// hj_api.hip -- implementation of the C ABI in include/htm_hashjoin.h: the context's life cycle, hj_reserve, the whole
// joins (hj_join_dev, hj_run), hj_fetch_result, error strings and raw device memory. The other entry points, by use:
// hj_api_table.hip (table builds and probes), hj_api_prj.hip (radix join), hj_api_rows.hip (marks, row maps, key columns,
// every call's *_info) and hj_api_tools.hip (Zipf stream, shard helpers); hj_host.h is what they share. Host-side glue
// only: argument checks, device memory, stream order, HIP-event timing; the kernel files do all arithmetic on tuples.
// There is no CPU fallback in here: every operator needs a gfx950 device.
#include "hj_host.h"

#include <chrono>
#include <cstring>
#include <new>

using namespace hjapi;

static int create_common(int device, void* stream, bool own, hj_ctx** out)
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
              hipHostMalloc(reinterpret_cast<void**>(&c->pin), sizeof(Pinned)) == hipSuccess &&
              hipHostMalloc(reinterpret_cast<void**>(&c->hPreferred), sizeof(unsigned long long), hipHostMallocMapped) == hipSuccess &&
              hipHostGetDevicePointer(reinterpret_cast<void**>(&c->dPreferred), c->hPreferred, 0) == hipSuccess &&
              c->buf[B_BOUNDS].reserve(c, wave_bounds_bytes(c->nCU)) == HJ_OK &&
              c->buf[B_CALL_WORDS].reserve(c, CALL_COUNT * kCallWords * sizeof(unsigned long long)) == HJ_OK &&
              hipMemset(c->buf[B_CALL_WORDS].p, 0, CALL_COUNT * kCallWords * sizeof(unsigned long long)) == hipSuccess;
    for (int i = 0; ok && i < EV_COUNT; ++i) ok = hipEventCreate(&c->time.ev[i]) == hipSuccess;
    for (CallRecord& r : c->call) ok = ok && hipEventCreate(&r.ev[0]) == hipSuccess && hipEventCreate(&r.ev[1]) == hipSuccess;
    if (!ok) { hj_destroy(c); return HJ_ERR_HIP; }
    hipMemset(c->dCtr(), 0, sizeof(Counters));
    memset(c->hCtr, 0, sizeof(Counters));
    *c->hPreferred = 0;
    *out = c;
    return HJ_OK;
}

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

void hj_destroy(hj_ctx* c)
{
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream || !c->ownStream) hipStreamSynchronize(c->stream);
    zipf_release(c);
    if (c->stream || !c->ownStream) hipStreamSynchronize(c->stream);
    for (const DevBuf& b : c->buf) if (b.p) hipFree(b.p);
    for (void* pinned : {(void*)c->hCtr, (void*)c->pin, (void*)c->hPreferred}) if (pinned) hipHostFree(pinned);
    for (int i = 0; i < EV_COUNT; ++i) if (c->time.ev[i]) hipEventDestroy(c->time.ev[i]);
    for (const CallRecord& r : c->call) for (hipEvent_t e : r.ev) if (e) hipEventDestroy(e);
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

// every buffer of the list at its size (0: not needed); *replaced: as DevBuf::reserve
struct Need { Buf b; size_t bytes; };
static int reserve_all(hj_ctx* c, std::initializer_list<Need> needs, bool* replaced = nullptr)
{
    for (const Need& n : needs) if (const int rc = c->buf[n.b].reserve(c, n.bytes, replaced)) return rc;
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
    if (params->flags & HJ_FLAG_SLOT_CODES) {
        if (params->flags & HJ_FLAG_KEEP_ROW_IDS)
            return fail(c, HJ_ERR_INVALID, "hj_reserve: HJ_FLAG_SLOT_CODES excludes HJ_FLAG_KEEP_ROW_IDS (a code byte holds no row)");
        if (params->algo != HJ_ALGO_NOCC && params->algo != HJ_ALGO_ATOMIC)
            return fail(c, HJ_ERR_INVALID, "hj_reserve: HJ_FLAG_SLOT_CODES needs an open-addressing algo");
        if (probe_len(*params) > 128) return fail(c, HJ_ERR_INVALID, "hj_reserve: HJ_FLAG_SLOT_CODES needs probeLength <= 128");
    }
    HJ_HIP(c, hipSetDevice(c->device));
    c->params = *params;
    HJ_HIP(c, hipStreamSynchronize(c->stream));          // buffers may be replaced below; and a new workload starts without an expectation
    *c->hPreferred = 0;
    if (track) {
        // one bit per R row in 32-bit words (the sweep reads whole words: rounded up to 16 bytes), and the sweep's workspace
        bool replaced = false;
        int rc = c->buf[B_R_MARKS].reserve(c, (((rSize + 31) / 32 + 3) & ~3ull) * sizeof(uint32_t), &replaced);
        if (!rc) rc = c->buf[B_R_SWEEP].reserve(c, r_sweep_count_words(rSize) * sizeof(uint32_t));
        if (replaced) forget_marks(c);                              // the plane of the last build is gone
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
        const int rc = reserve_all(c, {{B_TMP, (nmax + 2) * sizeof(uint64_t)}, {B_PART_R, (rSize + 2) * sizeof(uint64_t)},
                                       {B_PART_S, sSize ? (sSize + 2) * sizeof(uint64_t) : 0}, {B_WORK, c->plan.workspaceBytes},
                                       {B_PRJ_RES, prj_resident_bytes(bits, sSize)}}, &replaced);
        if (replaced) { c->res = {}; c->agg = {}; }
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
        // rings (variant 3), workgroup window (2) or global atomics (1): buffers for the larger need of the first two
        const bool own = own_supported(4 * nb);
        size_t qb = wave_queue_bytes(rSize, c->nCU), cb = wave_conflict_bytes(rSize, c->nCU);
        if (own && own_queue_bytes(rSize) > qb) qb = own_queue_bytes(rSize);
        if (own && own_conflict_bytes(rSize, c->nCU) > cb) cb = own_conflict_bytes(rSize, c->nCU);
        bool ownerReplaced = false;                 // hj_own_info: the owner words of the last window build are gone
        int rc = c->buf[B_OWNER].reserve(c, own ? own_owner_bytes(4 * nb) : 0, &ownerReplaced);
        if (ownerReplaced) c->op.ownN = 0;
        if (rc) return rc;
        return reserve_all(c, {{B_TABLE, (4 * nb + kTableSlack) * sizeof(uint64_t)},
                               {B_HTM_OWN_COUNTS, own ? own_conflict_count_bytes(rSize, c->nCU) : 0}, {B_QUEUE, qb}, {B_HTM_CONFLICTS, cb},
                               {B_HTM_OVF_COUNT, nb * sizeof(unsigned int)}, {B_HTM_OVF_BASE, nb * sizeof(uint32_t)},
                               {B_HTM_SCAN, scan_workspace_words(nb) * sizeof(uint32_t)}});
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
        bool ownerReplaced = false;                 // hj_own_info: the owner words of the last window build are gone
        if (own_supported(2 * rSize)) rc = c->buf[B_OWNER].reserve(c, own_owner_bytes(2 * rSize), &ownerReplaced);
        if (ownerReplaced) c->op.ownN = 0;
        if (rc) return rc;
        if ((rc = c->buf[B_QUEUE].reserve(c, qb))) return rc;
    }
    return HJ_OK;
}

int hj_join_dev(hj_ctx* c, const uint64_t* dR, uint64_t rSize, const uint64_t* dS, uint64_t sSize)
{
    if (!c || !dR || rSize == 0) return HJ_ERR_INVALID;
    if (!dS) sSize = 0;
    if (sSize == 0) dS = nullptr;
    int rc;
    bool prj = c->params.algo == HJ_ALGO_PRJ;
    uint32_t variant = 0;                           // of the table build: 0 = hj_params.buildVariant decides
    if (c->params.algo == HJ_ALGO_AUTO) {
        // the same question the build asks itself for buildVariant 0, asked once here: with locality the
        // LDS-window build + linear probe wins, without it both of them turn into random HBM accesses
        // and two radix passes are cheaper
        HJ_HIP(c, hipSetDevice(c->device));
        if (!is_pow2(rSize) || rSize > (1ull << 31)) return hj_prj_join_dev(c, dR, rSize, dS, sSize);   // see hj_reserve
        if ((2 * rSize + kTableSlack) * sizeof(uint64_t) > c->buf[B_TABLE].bytes)
            return fail(c, HJ_ERR_STATE, "hj_join_dev: hj_reserve() not called for this rSize");
        const BuildCaps can = build_caps(c, rSize, 2 * rSize);
        variant = 1;
        if ((can.own || can.wave) && c->params.buildVariant != 1 &&
            (rc = sample_variant(c, dR, false, rSize, 2 * rSize, 0, can, &variant))) return rc;
        // no locality: both table phases would be random HBM accesses. Loose locality (variant 2) pays for every tuple
        // that leaves its window with global atomics: at 2^27, local_shuffle W=2^11 (3.8 % deferred) the table join
        // takes 1.09 ms against the radix join's 1.81 ms, at W=2^12 (36 % deferred) 2.79 against 1.83 (round 3, deferred
        // queue sliced per workgroup; 2.06 / 1.89 at W=2^11 before): the radix join from 1/8 of the sample outside the window.
        // (fit[] is the sampler's alone: nothing between sample_variant and here writes it, and no build does)
        prj = variant == 1 || (variant == 2 && (uint64_t)c->pin->fit[0] * 8u > c->pin->fit[1]);
    }
    if (prj) return hj_prj_join_dev(c, dR, rSize, dS, sSize);
    if ((rc = build_table(c, dR, rSize, 0, variant))) return rc;
    return hj_probe_dev(c, dS, sSize);
}

int hj_fetch_result(hj_ctx* c, hj_result* out)
{
    HJ_ENTER(c, out);
    if (const int rc = read_counters(c, true)) return rc;
    memset(out, 0, sizeof(*out));
    const Counters& k = *c->hCtr;
    out->rSize = c->op.rSize; out->sSize = c->op.sSize; out->tableSize = c->op.tableSize;
    out->inputSum = k.inputSum;
    if (c->prj.ran) {
        out->totalMatches = k.prjMatches;
        out->prjChecksum = k.prjChecksum;
        out->prjPartitions = 1ull << c->plan.radixBits;
        out->radixBits = c->plan.radixBits;
        out->partition_us = elapsed_us(c, EV_PRJ0, EV_PRJ_PART);
        out->join_us = elapsed_us(c, EV_PRJ_PART, EV_PRJ1);
        out->total_us = elapsed_us(c, EV_PRJ0, EV_PRJ1);
        out->prjScatterPass1R_us = elapsed_us(c, EV_PRJ_S0, EV_PRJ_S1);
        out->prjPath = !c->prj.optimistic ? 0u : (k.prjFallback ? 2u : 1u);
        if (c->res.on) {
            // resident R: the build's passes (partition_us, build_us = passes + R's checksum), the last probe (probe_us = S's
            // passes + work items + join, join_us = the join kernel alone); prjPath = R's path
            out->build_us = elapsed_us(c, EV_PRJ0, EV_PRJ1);
            out->probe_us = elapsed_us(c, EV_RP0, EV_RP1);
            out->join_us = elapsed_us(c, EV_RP_JOIN0, EV_RP1);
            out->total_us = out->build_us + out->probe_us;
            out->prjPath = !c->prj.optimistic ? 0u : (k.prjFallbackR ? 2u : 1u);
        }
    } else {
        out->conflicts = k.conflicts;
        out->conflictSum = k.conflictSum;
        out->totalMatches = k.matches;
        out->tableSumHalf = k.tableSumHalf;
        out->tableSumFull = k.tableSumFull;
        out->outputSum = (c->params.algo == HJ_ALGO_NOCC ? k.tableSumHalf : k.tableSumFull) + k.conflictSum;
        if (c->htm.built) {
            // every conflict sits in an overflow bucket of its own bucket's chain: tuples in buckets + tuples in
            // chains = input (HTMHashBuild.hpp:452 adds conflictSum on top of the chains, counting them twice)
            out->htmBuckets = c->htm.buckets; out->htmOverflowBuckets = k.htmOverflowBuckets; out->htmOverflowSum = k.htmOverflowSum;
            out->outputSum = k.tableSumFull + k.htmOverflowSum;
        }
        out->buildVariant = c->op.variantUsed ? c->op.variantUsed : (uint32_t)k.variant;   // 0: the device chose
        out->compactFallback = k.compactFail | ((c->htm.built && c->htm.chainsFellBack) ? 0x100ull : 0ull);
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
        out->probe_us = elapsed_us(c, c->op.probeStartsAtBuildEnd ? EV_BUILD1 : EV_PROBE0, EV_PROBE1);
        // the reference's timed region is build+probe, table zeroing excluded
        // (NoCCHashBuild.hpp:24-34,83); clear_us is reported beside it
        out->total_us = out->build_us + out->probe_us;
    }
    out->h2d_us = c->time.h2d_us;
    out->algoUsed = c->op.algoUsed;
    out->foreignTuples = k.foreign;
    if (k.badKeys) return fail(c, HJ_ERR_KEY_RANGE, "input holds tuples with payload bits set or value 0");
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
    c->time.h2d_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if ((rc = hj_join_dev(c, stageR, rSize, sSize ? stageS : nullptr, sSize))) return rc;
    if (!c->prj.ran && (rc = hj_checksums_dev(c))) return rc;
    return hj_fetch_result(c, out);
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

// a copy in the context's stream order that has arrived when the call returns
static int copy_sync(hj_ctx* c, void* dst, const void* src, uint64_t bytes, hipMemcpyKind kind)
{
    HJ_ENTER(c, dst && src);
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipMemcpyAsync(dst, src, bytes, kind, c->stream));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    return HJ_OK;
}

int hj_copy_h2d(hj_ctx* c, void* dst_dev, const void* src_host, uint64_t bytes) { return copy_sync(c, dst_dev, src_host, bytes, hipMemcpyHostToDevice); }

int hj_copy_d2h(hj_ctx* c, void* dst_host, const void* src_dev, uint64_t bytes) { return copy_sync(c, dst_host, src_dev, bytes, hipMemcpyDeviceToHost); }

}  // extern "C"
