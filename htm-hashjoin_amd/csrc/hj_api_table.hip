// hj_api_table.hip -- the C ABI's table joins: the builds (open addressing and the bucketised table of --algo htm), the
// counting and the materialising probes, checksums, exports, and the wave / htm / table info calls. Host-side glue only.
#include "hj_host.h"

#include <cstring>

using namespace hjapi;

// One build as its launchers see it (hj_table.h): the context's table, counters and stream around the caller's input
static BuildJob build_job(hj_ctx* c, const void* R, bool key32, uint64_t n, uint32_t hshift, uint64_t tableSize, uint32_t probeLen,
                          uint64_t idxBase, ShardCheck sc)
{
    BuildJob job{};
    job.R = R; job.key32 = key32; job.n = n; job.idxBase = idxBase;
    job.table = c->buf[B_TABLE].as<uint64_t>(); job.tableSize = tableSize; job.hshift = hshift; job.probeLen = probeLen; job.sc = sc;
    job.nCU = c->nCU; job.ctr = c->dCtr(); job.s = c->stream;
    return job;
}

// Locality pre-round, host-side form (hj_join_dev with HJ_ALGO_AUTO only: the choice between table join and radix join
// changes which buffers and kernels are used at all, so it is read back; hj_build_dev decides on the device, see
// build_common). 256 sample tiles of R. Answer = the build kernel worth taking:
//   3  the wavefront-private rings (hj_build_wave.hip) if at most 1/128 of the sampled tuples would fall outside
//      their ring (tight locality: the reference's default shuffle window of 16, anything up to ~100 positions);
//   2  the workgroup window (hj_build_own.hip) if it would have to defer at most 3/4 of the tuples (variant_for_sample,
//      hj_table.h: what it defers costs about what global atomics cost for every tuple);
//   1  global atomics otherwise (no locality: hj_join_dev(AUTO) then takes the radix join instead).
int hjapi::sample_variant(hj_ctx* c, const void* d, bool key32, uint64_t n, uint64_t tableSize, uint32_t hshift,
                          const BuildCaps& can, uint32_t* variant, bool htm)
{
    const uint32_t nSample = 256;
    unsigned int* const fit = c->buf[B_FIT].as<unsigned int>();
    HJ_HIP(c, launch_sample_locality(d, key32, n, tableSize, hshift, nSample, fit, c->stream, htm));
    HJ_HIP(c, hipMemcpyAsync(c->pin->fit, fit, 8 * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    *variant = variant_for_sample(c->pin->fit[0], c->pin->fit[1], c->pin->fit[2], can.own, can.wave, can.compact, c->pin->fit[3], c->pin->fit[4]);
    return HJ_OK;
}

// Shared by build_table (DataGen tuples) and hj_build_keys_dev (bare keys of a radix shard). forceVariant: the build kernel
// hj_join_dev(AUTO) has already sampled for, 0: hj_params.buildVariant
static int build_common(hj_ctx* c, const void* d, bool key32, uint64_t n, uint32_t hshift,
                        uint64_t tableSize, uint64_t idxBase, uint32_t forceVariant)
{
    int rc;
    if ((rc = begin_operation(c, n, 0, tableSize))) return rc;
    c->op.hshift = hshift;
    if ((rc = record(c, EV_CLEAR0))) return rc;
    const BuildCaps can = build_caps(c, n, tableSize);
    const uint32_t variant = settle_variant(forceVariant ? forceVariant : c->params.buildVariant, can);
    c->op.variantUsed = (variant == 4) ? 0 : variant;     // 0: decided on the device (4 may fall back to 3), reported from Counters::variant
    c->op.algoUsed = c->params.algo == HJ_ALGO_AUTO ? (uint32_t)HJ_ALGO_ATOMIC : c->params.algo;
    const BuildJob job = build_job(c, d, key32, n, hshift, tableSize, probe_len(c->params), idxBase, c->sc);
    const WaveBufs wave{c->buf[B_BOUNDS].p, c->buf[B_QUEUE].p};
    const OwnBufs own{c->buf[B_OWNER].p, c->buf[B_QUEUE].p, c->buf[B_QUEUE_COUNT].as<uint32_t>()};
    const unsigned long long* word = &job.ctr->variant;
    c->op.wavePreGated = variant == 0;
    // The classic rings (3) of a context that keeps no row ids retire planar: 4-byte keys for the probe, the index words in a
    // plane of their own that only the deferred walks read. Behind them the packed classic build stays enqueued, gated on the
    // word k_wave_fixup sets when the planar build had to give up (Counters::planarFail); not needed, its launches return at once.
    // Slot codes instead of the key plane (kWaveCodes): tuple builds only, and by itself only where a
    // code byte holds ANY 32-bit key -- tables of 2^27 slots and more at probeLength 4, where the probe's bytes are what
    // the step costs. Below that everything stays as it was unless HJ_FLAG_SLOT_CODES forces the road (then a key without a
    // code hands over to the packed build like the planar build's own causes).
    const SlotCode code = slot_code(tableSize, job.probeLen);
    const bool codesCan = !(c->params.flags & HJ_FLAG_KEEP_ROW_IDS) && !key32 && hshift == 0 && code.dbits <= kCodeBits &&
                          wave_codes_supported(n, job.nCU, tableSize);
    c->op.codesRoad = !codesCan ? 0u : code.fits_all() ? 1u : (c->params.flags & HJ_FLAG_SLOT_CODES) ? 2u : 0u;
    const int classicMode = (c->params.flags & HJ_FLAG_KEEP_ROW_IDS) ? kWaveClassic : c->op.codesRoad ? kWaveCodes : kWavePlanar;
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
            c->op.wavePreN = n;
            HJ_HIP(c, launch_build_wave(job, wave, Gate{word, 3, 4}, kWavePre));
            if (enqCompact)
                HJ_HIP(c, launch_build_wave(job, wave, Gate{word, 4}, kWaveMain, kWaveCompact, bracket(c, EV_KC0)));
            HJ_HIP(c, launch_build_wave(job, wave, Gate{word, 3}, kWaveMain, classicMode, bracket(c, EV_KW0)));
        }
        if (enqOwn) {
            c->op.ownN = n; c->op.ownGated = true;
            HJ_HIP(c, launch_build_own(job, own, Gate{word, 2}, 1, bracket(c, EV_KO0)));
        }
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
        c->op.wavePreN = n;
        if ((rc = record(c, EV_BUILD0))) return rc;
        HJ_HIP(c, launch_build_wave(job, wave, Gate{word, 4}, kWavePre | kWaveMain, kWaveCompact, bracket(c, EV_KC0)));
        HJ_HIP(c, launch_build_wave(job, wave, Gate{word, 3}, kWaveMain, classicMode, bracket(c, EV_KW0)));
        HJ_HIP(c, launch_build_wave(job, wave, Gate{word, 4}, kWaveTail, kWaveCompact));
        HJ_HIP(c, classic_tail(Gate{word, 3}));
    } else if (variant == 3) {
        c->op.wavePreN = n;
        if ((rc = record(c, EV_BUILD0))) return rc;
        HJ_HIP(c, launch_build_wave(job, wave, Gate{nullptr, 0}, kWavePre | kWaveMain, classicMode, bracket(c, EV_KW0)));
        HJ_HIP(c, classic_tail(Gate{nullptr, 0}));
    } else if (variant == 2) {
        c->op.ownN = n;
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
    c->op.built = true;
    c->op.streamAtBuildEnd = c->ownStream; c->op.probeStartsAtBuildEnd = false;
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
// genericChains: the second attempt on a relation the LDS chain phase gave up on -- no routing, generic chain kernels
static int build_htm(hj_ctx* c, const uint64_t* dR, uint64_t rSize, uint64_t idxBase, bool genericChains = false)
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
    c->op.hshift = 0; c->htm.buckets = nb;
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
    c->op.variantUsed = variant; c->op.algoUsed = HJ_ALGO_HTM;
    const WaveSlices sl = variant == 2 ? own_conflict_layout(rSize, c->nCU, ownCounts) : wave_conflict_layout(rSize, c->nCU, bounds);
    // the rings: chains in LDS (hj_htm.hip) unless an earlier attempt on this relation had to give up
    const uint32_t nParts = sl.nChunks * htm_chain_parts(sl.sliceLen);
    const bool ldsChains = variant == 3 && !genericChains && htm_chain_tries(sl.nChunks, sl.sliceLen, nb);
    if (variant == 2) {
        c->op.ownN = rSize;
        if ((rc = record(c, EV_BUILD0))) return rc;
        const OwnBufs own{c->buf[B_OWNER].p, c->buf[B_QUEUE].p, c->buf[B_QUEUE_COUNT].as<uint32_t>(), htmConflicts, ownCounts};
        HJ_HIP(c, launch_build_own(job, own, Gate{nullptr, 0}, 3, bracket(c, EV_KO0)));
    } else if (variant == 3) {
        c->op.wavePreN = rSize; c->op.wavePreGated = false;
        if ((rc = record(c, EV_BUILD0))) return rc;
        const WaveBufs wave{bounds, c->buf[B_QUEUE].p, htmConflicts, ldsChains};
        HJ_HIP(c, launch_build_wave(job, wave, Gate{nullptr, 0}, kWaveAll, kWaveClassic, bracket(c, EV_KW0)));
        if (ldsChains) {
            // the chain phase in LDS, first half: overflow buckets per part of a slice, scanned (one word more: the total)
            HJ_HIP(c, hipMemsetAsync(ovfBase + nParts, 0, sizeof(uint32_t), c->stream));
            HJ_HIP(c, launch_htm_chain_count(htmConflicts, sl.counts, WaveScratch(c->nCU, bounds).bounds, sl.nChunks, sl.sliceLen, nb,
                                             ovfBase, ovfCount, job.ctr, c->stream));
            HJ_HIP(c, launch_exclusive_scan_u32(ovfBase, (uint64_t)nParts + 1, scan, c->stream));
            HJ_HIP(c, hipMemcpyAsync(&c->pin->chainGroups, ovfBase + nParts, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
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
    if (ldsChains && c->hCtr->htmChainBail) {
        // an input the LDS chain phase cannot take (hj_htm.hip): once more, unrouted, with the generic chain kernels
        const uint64_t cause = c->hCtr->htmChainBail;           // kept here: the second attempt zeroes the counters and c->htm
        rc = build_htm(c, dR, rSize, idxBase, true);
        c->htm.chainsFellBack = true; c->htm.chainState = 2; c->htm.chainCause = cause;
        return rc;
    }
    if (ldsChains) {
        const uint64_t groups = c->pin->chainGroups;                    // overflow buckets the parts need, exactly
        c->htm.chainState = 1; c->htm.chainGroups = groups;
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
    c->op.built = true; c->htm.built = true;
    c->op.streamAtBuildEnd = c->ownStream; c->op.probeStartsAtBuildEnd = false;
    return HJ_OK;
}

int hjapi::build_table(hj_ctx* c, const uint64_t* dR, uint64_t rSize, uint64_t idxBase, uint32_t forceVariant)
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
    rc = htm ? build_htm(c, dR, rSize, idxBase) : build_common(c, dR, false, rSize, 0, 2 * rSize, idxBase, forceVariant);
    if (rc == HJ_OK) marks_built(c, rSize, idxBase);
    return rc;
}

extern "C" {

int hj_build_dev(hj_ctx* c, const uint64_t* dR, uint64_t rSize, uint64_t idxBase) { return build_table(c, dR, rSize, idxBase, 0); }

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
    return build_common(c, dKeys, true, n, homeShift, tableSize, 0, 0);
}

// The counting probe behind hj_probe_dev (tuples) and hj_probe_keys_dev (bare keys). fromBuildEnd: the very next thing behind the
// build on the library's own stream, so the build's end event is the probe's start (one event record less per step)
static int probe_count(hj_ctx* c, const void* S, bool key32, uint64_t n, bool fromBuildEnd)
{
    HJ_HIP(c, hipSetDevice(c->device));
    int rc;
    c->op.probeStartsAtBuildEnd = fromBuildEnd;
    c->op.streamAtBuildEnd = false;
    if (!fromBuildEnd && (rc = record(c, EV_PROBE0))) return rc;
    const uint64_t* const table = c->buf[B_TABLE].as<uint64_t>();
    if (n && c->htm.built) launch_htm_probe(static_cast<const uint64_t*>(S), n, table, c->htm.buckets, c->buf[B_HTM_OVERFLOW].as<uint64_t>(), c->dCtr(), c->stream);
    else if (n) launch_probe(S, key32, n, table, c->op.tableSize, c->op.hshift, probe_len(c->params), c->sc, c->dCtr(), c->stream);
    if ((rc = record(c, EV_PROBE1))) return rc;
    HJ_HIP(c, hipGetLastError());
    c->op.sSize += n;
    return HJ_OK;
}

int hj_probe_dev(hj_ctx* c, const uint64_t* dS, uint64_t sSize)
{
    if (!c || (!dS && sSize)) return HJ_ERR_INVALID;
    if (!c->op.built) return fail(c, HJ_ERR_STATE, "hj_probe_dev: no table (call hj_build_dev first)");
    return probe_count(c, dS, false, sSize, c->op.streamAtBuildEnd);
}

int hj_probe_keys_dev(hj_ctx* c, const uint32_t* dKeys, uint64_t n)
{
    HJ_ENTER(c, dKeys || !n);
    if (!c->op.built || c->htm.built) return fail(c, HJ_ERR_STATE, "hj_probe_keys_dev: no open-addressing table (build first)");
    return probe_count(c, dKeys, true, n, false);
}

// The one host sequence of the materialising table probe; fn: the entry point's name, for the error texts
static int probe_join(hj_ctx* c, const char* fn, uint32_t kind, const uint64_t* dS, uint64_t sSize, uint64_t sIdxBase, uint32_t* dOutS,
                      uint32_t* dOutR, uint64_t capacity)
{
    if (!c || (!dS && sSize)) return HJ_ERR_INVALID;
    // decided on the host: whether the table keeps its index words is chosen on the device (Counters::tableFormat), so
    // the call keys on what hj_reserve was promised
    const char* const state = c->params.algo == HJ_ALGO_PRJ ? "a PRJ context keeps no row ids"
                            : !c->op.built ? "no table (call hj_build_dev first)"
                            : !c->htm.built && !(c->params.flags & HJ_FLAG_KEEP_ROW_IDS) ? "open-addressing context reserved without HJ_FLAG_KEEP_ROW_IDS"
                            : nullptr;
    bool planeR;
    if (const int bad = pairs_args(c, fn, kind, state, sSize, sIdxBase, dOutS, dOutR, capacity, &planeR)) return bad;
    if (!c->htm.built && probe_len(c->params) > pairs_max_probe_len()) return fail(c, HJ_ERR_INVALID, fn, "probeLength above 8");
    if (sSize == 0) return HJ_OK;
    HJ_HIP(c, hipSetDevice(c->device));
    c->op.streamAtBuildEnd = false;
    int rc;
    const PairsOut out{dOutS, planeR ? dOutR : nullptr, capacity, call_words(c, CALL_PAIRS)};
    HJ_HIP(c, hipMemsetAsync(out.cursor, 0, 2 * sizeof(unsigned long long), c->stream));
    HJ_HIP(c, hipEventRecord(c->call[CALL_PAIRS].ev[0], c->stream));
    const uint64_t* const table = c->buf[B_TABLE].as<uint64_t>();
    RMarks mk;
    const RMarks* const marks = marks_for(c, kind, &mk) ? &mk : nullptr;
    if (c->htm.built) launch_htm_probe_pairs(kind, dS, sSize, sIdxBase, table, c->htm.buckets, c->buf[B_HTM_OVERFLOW].as<uint64_t>(), out, c->nCU, c->dCtr(), c->stream, marks);
    else launch_probe_pairs(kind, dS, sSize, sIdxBase, table, c->op.tableSize, c->op.hshift, probe_len(c->params), c->sc, out, c->nCU, c->dCtr(), c->stream, marks);
    if ((rc = call_end(c, CALL_PAIRS, capacity, sSize, kind))) return rc;
    HJ_HIP(c, hipGetLastError());
    c->op.sSize += sSize;
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

int hj_checksums_dev(hj_ctx* c)
{
    HJ_ENTER(c, true);
    if (!c->op.built) return fail(c, HJ_ERR_STATE, "hj_checksums_dev: no table");
    HJ_HIP(c, hipSetDevice(c->device));
    // zero the two sums so the call is idempotent
    HJ_HIP(c, hipMemsetAsync(&c->dCtr()->tableSumHalf, 0, 2 * sizeof(unsigned long long), c->stream));
    if (c->htm.built) {
        HJ_HIP(c, hipMemsetAsync(&c->dCtr()->htmOverflowSum, 0, sizeof(unsigned long long), c->stream));
        launch_htm_sums(c->buf[B_TABLE].as<uint64_t>(), c->htm.buckets, c->buf[B_HTM_OVERFLOW].as<uint64_t>(), c->dCtr(), c->stream);
    } else launch_table_sums(c->buf[B_TABLE].as<uint64_t>(), c->op.tableSize, c->op.tableSize / 2, probe_len(c->params), c->dCtr(), c->stream);
    HJ_HIP(c, hipGetLastError());
    return HJ_OK;
}

int hj_export_table(hj_ctx* c, uint64_t* host_table, uint64_t tableSize)
{
    HJ_ENTER(c, host_table);
    if (!c->op.built || c->htm.built || tableSize != c->op.tableSize) return fail(c, HJ_ERR_STATE, "hj_export_table: no open-addressing table of that size");
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    Counters k;
    HJ_HIP(c, hipMemcpy(&k, c->dCtr(), sizeof(k), hipMemcpyDeviceToHost));
    // only [validLo, validHiEx + 512) holds defined values (hj_table.h); the rest is empty by definition
    const uint64_t lo = k.validLo, hi = k.validHiEx + 512 < tableSize ? k.validHiEx + 512 : tableSize;
    if (k.tableFormat == kFormatCodes1) {
        // slot codes (one byte per slot, 0xFF = empty) -> reference format: the codes land at the end of the caller's buffer
        // and are decoded from the front (slot i is written at byte 8 i, its code sits at byte 7 tableSize + i: never behind)
        const SlotCode code = slot_code(tableSize, probe_len(c->params));
        const uint8_t* codes = reinterpret_cast<const uint8_t*>(host_table) + 7 * tableSize;
        HJ_HIP(c, hipMemcpy(const_cast<uint8_t*>(codes), c->buf[B_TABLE].p, tableSize, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < tableSize; ++i) {
            const uint32_t v = codes[i];
            host_table[i] = (i < lo || i >= hi || v == kCodeEmpty) ? 0 : code.decode(v, (uint32_t)i, (uint32_t)(tableSize - 1));
        }
        return HJ_OK;
    }
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
    if (!c->htm.built || numBuckets != c->htm.buckets) return fail(c, HJ_ERR_STATE, "hj_export_buckets: no htm table of that many buckets");
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
    if (!c->op.built || !c->op.wavePreN) return fail(c, HJ_ERR_STATE, "hj_wave_seams: the last build did not run the ring pre-pass");
    if (const int rc = read_counters(c, false)) return rc;
    // buildVariant 0: the pre-pass was enqueued behind the device's pick and ran only if that pick was the rings
    if (c->op.wavePreGated && c->hCtr->variant != 3 && c->hCtr->variant != 4)
        return fail(c, HJ_ERR_STATE, "hj_wave_seams: the last build did not run the ring pre-pass");
    const uint64_t chunks = wave_layout(c->op.wavePreN, c->nCU).nChunks;
    *nChunks = chunks;
    if (capacity < chunks + 1) return fail(c, HJ_ERR_INVALID, "hj_wave_seams: capacity below the number of chunks + 1");
    const WaveScratch w(c->nCU, c->buf[B_BOUNDS].p);
    HJ_HIP(c, hipMemcpy(starts, w.starts, (chunks + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HJ_HIP(c, hipMemcpy(bounds, w.bounds, (chunks + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (pcounts) HJ_HIP(c, hipMemcpy(pcounts, w.pcounts, chunks * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return HJ_OK;
}

int hj_own_layout_info(const hj_ctx* c, uint32_t computeUnits, uint64_t n, uint64_t out[16])
{
    if (!out || (!c && (computeUnits == 0 || computeUnits > 65536)) || n == 0 || n > 0xFFFFFFFFull) return HJ_ERR_INVALID;
    const int nCU = c ? c->nCU : (int)computeUnits;
    const OwnLayout w = own_layout(n, nCU);
    const uint64_t v[16] = {w.chunkLen, w.nChunks, w.tileTuples, w.blockSlots, w.winBlocks, w.backBlocks, w.seamDivisor, w.minTableSlots,
                            w.deferredParts, w.maxProbeLen, (uint64_t)nCU, 0, 0, 0, 0, 0};
    memcpy(out, v, sizeof v);
    return HJ_OK;
}

int hj_own_info(hj_ctx* c, uint32_t* owner, uint64_t ownerCapacity, uint32_t* deferCounts, uint64_t countsCapacity, uint64_t out[4])
{
    HJ_ENTER(c, owner && deferCounts && out);
    const char* const notRun = "hj_own_info: the last build did not run the workgroup-window build";
    if (!c->op.built || !c->op.ownN) return fail(c, HJ_ERR_STATE, notRun);
    if (const int rc = read_counters(c, false)) return rc;
    // buildVariant 0: its kernels were enqueued behind the device's pick and ran only if that pick was the window
    if (c->op.ownGated && c->hCtr->variant != 2) return fail(c, HJ_ERR_STATE, notRun);
    const OwnLayout w = own_layout(c->op.ownN, c->nCU);
    const uint64_t blocks = c->op.tableSize / w.blockSlots, chunks = w.nChunks;
    out[0] = blocks; out[1] = chunks; out[2] = 0; out[3] = 0;
    if (ownerCapacity < blocks || countsCapacity < chunks) return fail(c, HJ_ERR_INVALID, "hj_own_info: capacity below the number of blocks / chunks");
    HJ_HIP(c, hipMemcpy(owner, c->buf[B_OWNER].p, blocks * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HJ_HIP(c, hipMemcpy(deferCounts, c->buf[B_QUEUE_COUNT].p, chunks * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < chunks; ++i) out[2] += deferCounts[i];
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
    if (!c->op.built || !c->htm.built) return fail(c, HJ_ERR_STATE, "hj_htm_chain_info: no htm table (call hj_build_dev on a context reserved for HJ_ALGO_HTM)");
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    out[0] = c->htm.chainState; out[1] = c->htm.chainCause; out[2] = c->htm.chainGroups; out[3] = 0;
    return HJ_OK;
}

int hj_wave_planar_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    if (!c->op.built || c->htm.built) return fail(c, HJ_ERR_STATE, "hj_wave_planar_info: no open-addressing table");
    if (const int rc = read_counters(c, false)) return rc;
    const Counters& k = *c->hCtr;
    const uint32_t variant = c->op.variantUsed ? c->op.variantUsed : (uint32_t)k.variant;
    out[0] = (variant == 3 && k.tableFormat == kFormatKeys4) ? 1 : 0;
    out[1] = k.planarFail; out[2] = k.tableFormat; out[3] = 0;
    return HJ_OK;
}

int hj_slot_codes_info(hj_ctx* c, uint64_t tableSize, uint32_t probeLength, uint64_t out[8])
{
    if (!out) return HJ_ERR_INVALID;
    if (c && tableSize == 0) {
        // the table of the last build
        if (!c->op.built || c->htm.built) return fail(c, HJ_ERR_STATE, "hj_slot_codes_info: no open-addressing table");
        tableSize = c->op.tableSize; probeLength = probe_len(c->params);
    }
    if (!is_pow2(tableSize) || tableSize > (1ull << 32) || probeLength == 0) return HJ_ERR_INVALID;
    const SlotCode code = slot_code(tableSize, probeLength);
    out[0] = code.fits_all() ? 1 : 0; out[1] = code.dbits; out[2] = code.hiCap; out[3] = code.tbits;
    out[4] = out[5] = out[6] = out[7] = 0;
    if (!c || !c->op.built || c->htm.built || tableSize != c->op.tableSize) return HJ_OK;
    if (const int rc = read_counters(c, false)) return rc;
    const Counters& k = *c->hCtr;
    const uint32_t variant = c->op.variantUsed ? c->op.variantUsed : (uint32_t)k.variant;
    out[4] = (variant == 3 && k.tableFormat == kFormatCodes1) ? 1 : 0;      // the table is in slot codes
    out[5] = (variant == 3 && c->op.codesRoad) ? k.planarFail : 0;          // why the road handed over (0: it did not, or was not taken)
    out[6] = c->op.codesRoad; out[7] = k.tableFormat;
    return HJ_OK;
}

int hj_ring_word_layout_info(uint64_t tableSize, uint32_t probeLength, uint32_t rel, uint32_t key, uint32_t steps, uint64_t out[8])
{
    if (!out || !is_pow2(tableSize) || tableSize > (1ull << 32) || probeLength == 0) return HJ_ERR_INVALID;
    const SlotCode code = slot_code(tableSize, probeLength);
    out[5] = RingWord::kRelCap; out[6] = RingWord::kEmpty; out[0] = out[1] = out[2] = out[3] = out[4] = out[7] = 0;
    // what the road never makes: no code at this probeLength, a key without a code, a tuple past the layout rule, a step
    // past the budget
    if (code.dbits > kCodeBits || code.overflows(key) || !RingWord::holds((uint64_t)rel + 1) || steps >= probeLength) return HJ_ERR_INVALID;
    const RingWord rw = ring_word(code);
    const uint32_t mask32 = (uint32_t)(tableSize - 1);
    uint32_t word = rw.at_home(rel, key), pos = key & mask32;
    for (uint32_t k = 0; k < steps; ++k) { word = RingWord::step(word); pos = (pos + 1) & mask32; }
    out[0] = word; out[1] = rw.key(word, pos, mask32); out[2] = rw.tries_left(word, probeLength);
    out[3] = RingWord::rel(word); out[4] = RingWord::code(word); out[7] = pos;
    return HJ_OK;
}

int hj_table_debug(hj_ctx* c, uint64_t out[6])
{
    HJ_ENTER(c, out);
    if (!c->op.built) return fail(c, HJ_ERR_STATE, "hj_table_debug: no table (call hj_build_dev first)");
    if (const int rc = read_counters(c, false)) return rc;
    const Counters& k = *c->hCtr;
    out[0] = k.validLo; out[1] = k.validHiEx; out[2] = k.tableFormat;
    out[3] = c->op.tableSize;                                   // htm: 4 slots per bucket
    out[4] = (uint64_t)reinterpret_cast<uintptr_t>(c->buf[B_TABLE].p);
    out[5] = c->buf[B_TABLE].bytes;
    return HJ_OK;
}

}  // extern "C"
