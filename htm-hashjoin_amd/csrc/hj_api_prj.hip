// hj_api_prj.hip -- the C ABI's radix join: the whole join, the resident R with its counting and materialising probes,
// and the plan / workspace info calls. Host-side glue only.
#include "hj_host.h"

using namespace hjapi;

static PrjBuffers prj_buffers(const hj_ctx* c)
{
    return PrjBuffers{c->buf[B_TMP].as<uint64_t>(), c->buf[B_PART_R].as<uint64_t>(), c->buf[B_PART_S].as<uint64_t>(), c->buf[B_WORK].p};
}

// a radix join, or the build of a resident R, is enqueued with `pl`: its launcher recorded the three inner events
static void prj_ran(hj_ctx* c, const PrjPlan& pl)
{
    c->time.set[EV_PRJ_PART] = c->time.set[EV_PRJ_S0] = c->time.set[EV_PRJ_S1] = true;
    c->prj.ran = true; c->prj.optimistic = pl.optimistic;
    c->op.algoUsed = HJ_ALGO_PRJ;
}

extern "C" {

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
    HJ_HIP(c, launch_prj(pl, prj_buffers(c), dR, rSize, dS, dS ? sSize : 0, c->nCU, c->dCtr(), c->time.ev[EV_PRJ_PART], c->time.ev[EV_PRJ_S0],
                         c->time.ev[EV_PRJ_S1], c->stream));
    if ((rc = record(c, EV_PRJ1))) return rc;
    HJ_HIP(c, hipGetLastError());
    prj_ran(c, pl);
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
    HJ_HIP(c, (rows ? launch_prj_build_rows : launch_prj_build)(pl, prj_buffers(c), prj_resident_carve(c->buf[B_PRJ_RES].p, pl.radixBits, 0), dR, rSize, c->nCU,
                                                               c->dCtr(), c->time.ev[EV_PRJ_PART], c->time.ev[EV_PRJ_S0], c->time.ev[EV_PRJ_S1], c->stream));
    if ((rc = record(c, EV_PRJ1))) return rc;
    prj_ran(c, pl);
    c->res.on = true; c->res.plan = pl; c->res.nR = rSize; c->res.rows = rows;
    marks_built(c, rSize, 0);
    return HJ_OK;
}

// whether a slice fits what hj_reserve sized for the probes of a resident R
static bool prj_slice_fits(const hj_ctx* c, uint64_t sSize)
{
    return sSize <= c->prjMaxSlice && (sSize + 2) * sizeof(uint64_t) <= c->buf[B_PART_S].bytes && (sSize + 2) * sizeof(uint64_t) <= c->buf[B_TMP].bytes &&
           prj_resident_bytes(c->res.plan.radixBits, sSize) <= c->buf[B_PRJ_RES].bytes;
}

// One probe of the resident R, timed as a probe (EV_RP*, which bracket a pairs call's own events). out: R holds {key, row} elements
// -- the slice's row-id passes and the pairs join; nullptr: bare keys and the counting kernels. pairsCall: also a pairs call (what
// hj_pairs_info reports); only such a call marks R rows: the counting probe of a rows context keeps the kernel it ran before there were marks
static int prj_probe(hj_ctx* c, uint32_t kind, const uint64_t* dS, uint64_t sSize, uint64_t sIdxBase, const PairsOut* out, bool pairsCall)
{
    HJ_HIP(c, hipSetDevice(c->device));
    // the slice's own geometry (fragS); with rows the exact passes only: they carry the rows
    const PrjPlan pl = prj_plan(sSize, sSize, c->res.plan.radixBits, out ? 1u : c->params.prjMode);
    int rc;
    if ((rc = c->buf[B_WORK].reserve(c, pl.workspaceBytes))) return rc;      // R stays resident: see hj_prj_build_dev
    if ((rc = record(c, EV_RP0))) return rc;
    if (pairsCall) HJ_HIP(c, hipEventRecord(c->call[CALL_PAIRS].ev[0], c->stream));
    const PrjResident res = prj_resident_carve(c->buf[B_PRJ_RES].p, c->res.plan.radixBits, sSize);
    RMarks mk;
    const RMarks* const marks = pairsCall && marks_for(c, kind, &mk) ? &mk : nullptr;
    if (out) HJ_HIP(c, launch_prj_probe_rows(kind, c->res.plan, pl, prj_buffers(c), res, dS, sSize, sIdxBase, *out, c->nCU, c->dCtr(),
                                             c->time.ev[EV_RP_PART], c->time.ev[EV_RP_JOIN0], c->stream, marks));
    else HJ_HIP(c, launch_prj_probe(c->res.plan, c->res.nR, pl, prj_buffers(c), res, dS, sSize, c->nCU, c->dCtr(), c->time.ev[EV_RP_PART],
                                    c->time.ev[EV_RP_JOIN0], c->stream));
    if (pairsCall && (rc = call_end(c, CALL_PAIRS, out->capacity, sSize, kind))) return rc;
    if ((rc = record(c, EV_RP1))) return rc;
    c->time.set[EV_RP_PART] = c->time.set[EV_RP_JOIN0] = true;      // the launcher recorded them
    c->op.sSize += sSize;
    c->res.probeOpt = !out && pl.optimistic;
    return HJ_OK;
}

int hj_prj_probe_dev(hj_ctx* c, const uint64_t* dS, uint64_t sSize)
{
    HJ_ENTER(c, dS || !sSize);
    if (!c->res.on) return fail(c, HJ_ERR_STATE, "hj_prj_probe_dev: no resident R (call hj_prj_build_dev first)");
    if (!prj_slice_fits(c, sSize)) return fail(c, HJ_ERR_STATE, "hj_prj_probe_dev: slice larger than the sSize given to hj_reserve()");
    if (sSize == 0) return HJ_OK;
    if (!c->res.rows) return prj_probe(c, HJ_JOIN_INNER, dS, sSize, 0, nullptr, false);
    // R holds {key, row} elements, which the counting kernels cannot read: the pairs join with capacity 0, counting into
    // a word of its own (stats[4]: past the four the work items use; and the word behind it, which HJ_JOIN_INNER leaves
    // at zero) so that hj_pairs_info keeps the last pairs call
    const PairsOut count{nullptr, nullptr, 0, prj_resident_carve(c->buf[B_PRJ_RES].p, c->res.plan.radixBits, sSize).stats + 4};
    return prj_probe(c, HJ_JOIN_INNER, dS, sSize, 0, &count, false);
}

// The one host sequence of the materialising radix probe; fn: the entry point's name, for the error texts
static int prj_probe_join(hj_ctx* c, const char* fn, uint32_t kind, const uint64_t* dS, uint64_t sSize, uint64_t sIdxBase, uint32_t* dOutS,
                          uint32_t* dOutR, uint64_t capacity)
{
    HJ_ENTER(c, dS || !sSize);
    const char* const state = !c->res.on ? "no resident R (call hj_prj_build_dev first)"
                            : !c->res.rows ? "R was built without HJ_FLAG_KEEP_ROW_IDS"
                            : !prj_slice_fits(c, sSize) ? "slice larger than the sSize given to hj_reserve()"
                            : nullptr;
    bool planeR;
    if (const int bad = pairs_args(c, fn, kind, state, sSize, sIdxBase, dOutS, dOutR, capacity, &planeR)) return bad;
    if (sSize == 0) return HJ_OK;
    const PairsOut out{dOutS, planeR ? dOutR : nullptr, capacity, call_words(c, CALL_PAIRS)};
    return prj_probe(c, kind, dS, sSize, sIdxBase, &out, true);
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

// ---- aggregating joins on the resident R (hj_prj_agg.hip) -------------------
// what the three calls behind the begin need (fn: the entry point's name): an aggregation that no build has ended
static int agg_state(hj_ctx* c, const char* fn)
{
    if (!c->res.on) return fail(c, HJ_ERR_STATE, fn, "no resident R (call hj_prj_build_dev first)");
    if (!c->agg.on) return fail(c, HJ_ERR_STATE, fn, "no aggregation (call hj_prj_agg_begin first)");
    return HJ_OK;
}

int hj_prj_agg_begin(hj_ctx* c, const hj_agg_spec* specs, uint32_t nCols)
{
    HJ_ENTER(c, true);
    const char* const fn = "hj_prj_agg_begin";
    if (!c->res.on) return fail(c, HJ_ERR_STATE, fn, "no resident R (call hj_prj_build_dev first)");
    if (!c->res.rows) return fail(c, HJ_ERR_STATE, fn, "R was built without HJ_FLAG_KEEP_ROW_IDS");
    if (nCols == 0 || nCols > HJ_AGG_MAX_COLS) return fail(c, HJ_ERR_INVALID, fn, "nCols must be 1 .. HJ_AGG_MAX_COLS");
    if (!specs) return fail(c, HJ_ERR_INVALID, fn, "specs NULL");
    AggOps ops{};
    for (uint32_t i = 0; i < nCols; ++i) {
        const hj_agg_spec& sp = specs[i];
        if (sp.op > HJ_AGG_MAX) return fail(c, HJ_ERR_INVALID, fn, "op must be an hj_agg_op");
        if (sp.op == HJ_AGG_COUNT ? sp.width != 0 : (sp.width != 4 && sp.width != 8))
            return fail(c, HJ_ERR_INVALID, fn, "a width that is not 4 or 8 (HJ_AGG_COUNT: 0)");
        if (sp.flags & ~HJ_AGG_SIGNED) return fail(c, HJ_ERR_INVALID, fn, "hj_agg_spec.flags has bits other than HJ_AGG_SIGNED");
        if (sp.reserved) return fail(c, HJ_ERR_INVALID, fn, "hj_agg_spec.reserved must be 0");
        ops.op[i] = sp.op; ops.width[i] = sp.width; ops.sgn[i] = sp.flags & HJ_AGG_SIGNED;
    }
    HJ_HIP(c, hipSetDevice(c->device));
    c->agg = {};
    if (const int rc = c->buf[B_AGG].reserve(c, agg_bytes(c->res.nR, nCols))) return rc;
    c->agg.nCols = nCols; c->agg.nR = c->res.nR; c->agg.ops = ops;
    HJ_HIP(c, hipMemsetAsync(c->buf[B_AGG].p, 0, 256, c->stream));
    HJ_HIP(c, launch_agg_fill(agg_planes(c), ops, nCols, c->agg.nR, c->nCU, c->stream));
    c->agg.on = true;
    c->call[CALL_PRJ_AGG].called = false;
    return HJ_OK;
}

int hj_prj_probe_agg_dev(hj_ctx* c, const uint64_t* dS, uint64_t sSize, const hj_agg_src* srcs, uint32_t nCols)
{
    HJ_ENTER(c, dS || !sSize);
    const char* const fn = "hj_prj_probe_agg_dev";
    if (const int rc = agg_state(c, fn)) return rc;
    if (!prj_slice_fits(c, sSize)) return fail(c, HJ_ERR_STATE, fn, "slice larger than the sSize given to hj_reserve()");
    if (nCols != c->agg.nCols) return fail(c, HJ_ERR_INVALID, fn, "nCols differs from hj_prj_agg_begin's");
    if (!srcs) return fail(c, HJ_ERR_INVALID, fn, "srcs NULL");
    AggSrc src{};
    for (uint32_t i = 0; i < nCols; ++i) {
        const uint32_t width = c->agg.ops.width[i];
        if (reinterpret_cast<uintptr_t>(srcs[i].srcValid) & 3u) return fail(c, HJ_ERR_INVALID, fn, "a srcValid that is not 4-byte aligned");
        if (width && (!srcs[i].src || (reinterpret_cast<uintptr_t>(srcs[i].src) & (width - 1))))
            return fail(c, HJ_ERR_INVALID, fn, "a src that is NULL or not aligned to its width");
        src.p[i] = srcs[i].src; src.valid[i] = srcs[i].srcValid;
    }
    if (sSize == 0) return HJ_OK;
    HJ_HIP(c, hipSetDevice(c->device));
    // the probe's own sequence is prj_probe's: the slice's geometry with the exact passes (they carry the rows), timed as a probe
    const PrjPlan pl = prj_plan(sSize, sSize, c->res.plan.radixBits, 1u);
    int rc;
    if ((rc = c->buf[B_WORK].reserve(c, pl.workspaceBytes))) return rc;
    if ((rc = record(c, EV_RP0))) return rc;
    HJ_HIP(c, hipEventRecord(c->call[CALL_PRJ_AGG].ev[0], c->stream));
    const PrjResident res = prj_resident_carve(c->buf[B_PRJ_RES].p, c->res.plan.radixBits, sSize);
    HJ_HIP(c, launch_prj_probe_agg(c->res.plan, pl, prj_buffers(c), res, dS, sSize, src, c->agg.ops, nCols, agg_planes(c),
                                   c->buf[B_AGG].as<unsigned long long>(), c->nCU, c->dCtr(), c->time.ev[EV_RP_PART], c->time.ev[EV_RP_JOIN0],
                                   c->stream));
    if ((rc = call_end(c, CALL_PRJ_AGG, 0, sSize))) return rc;
    if ((rc = record(c, EV_RP1))) return rc;
    c->time.set[EV_RP_PART] = c->time.set[EV_RP_JOIN0] = true;      // the launcher recorded them
    c->op.sSize += sSize;
    c->res.probeOpt = false;
    c->agg.probes += 1;
    return HJ_OK;
}

int hj_prj_agg_rows_dev(hj_ctx* c, void* const* dOut, uint64_t* dOutCount)
{
    HJ_ENTER(c, true);
    const char* const fn = "hj_prj_agg_rows_dev";
    if (const int rc = agg_state(c, fn)) return rc;
    if (!dOut) return fail(c, HJ_ERR_INVALID, fn, "dOut NULL");
    AggRowsOut out{};
    for (uint32_t i = 0; i < c->agg.nCols; ++i) {
        if (!dOut[i] || (reinterpret_cast<uintptr_t>(dOut[i]) & 7u)) return fail(c, HJ_ERR_INVALID, fn, "an output plane that is NULL or not 8-byte aligned");
        out.col[i] = static_cast<unsigned long long*>(dOut[i]);
    }
    if (reinterpret_cast<uintptr_t>(dOutCount) & 7u) return fail(c, HJ_ERR_INVALID, fn, "dOutCount not 8-byte aligned");
    out.count = reinterpret_cast<unsigned long long*>(dOutCount);
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, launch_agg_rows(c->buf[B_PART_R].as<uint64_t>(), agg_planes(c), out, c->agg.nCols, c->agg.nR, c->nCU, c->stream));
    return HJ_OK;
}

int hj_prj_agg_info(hj_ctx* c, uint64_t out[8])
{
    HJ_ENTER(c, out);
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (!c->res.on || !c->agg.on) return HJ_OK;
    const CallRecord& r = c->call[CALL_PRJ_AGG];
    if (r.called) {
        unsigned long long last = 0;
        HJ_HIP(c, hipMemcpy(&last, c->buf[B_AGG].p, sizeof last, hipMemcpyDeviceToHost));
        float ms = 0;
        if (!r.timed || hipEventElapsedTime(&ms, r.ev[0], r.ev[1]) != hipSuccess) ms = 0;
        out[0] = last; out[1] = (uint64_t)((double)ms * 1000.0 + 0.5);
    }
    out[2] = c->agg.nCols; out[3] = c->agg.probes; out[4] = c->agg.nR;
    return HJ_OK;
}

int hj_prj_agg_layout_info(uint32_t nCols, uint64_t out[4])
{
    if (!out || nCols == 0 || nCols > HJ_AGG_MAX_COLS) return HJ_ERR_INVALID;
    for (uint32_t i = 0; i < 4; ++i) out[i] = agg_layout(nCols, i);
    return HJ_OK;
}

int hj_prj_resident_info(hj_ctx* c, uint64_t out[8])
{
    HJ_ENTER(c, out);
    if (!c->res.on) return fail(c, HJ_ERR_STATE, "hj_prj_resident_info: no resident R");
    HJ_HIP(c, hipSetDevice(c->device));
    const PrjResident res = prj_resident_carve(c->buf[B_PRJ_RES].p, c->res.plan.radixBits, 0);
    unsigned long long st[4];
    HJ_HIP(c, hipMemcpyAsync(st, res.stats, sizeof st, hipMemcpyDeviceToHost, c->stream));
    if (const int rc = read_counters(c, false)) return rc;
    const PrjPlan& pl = c->res.plan;
    const bool fragR = pl.optimistic && c->hCtr->prjFallbackR == 0;
    const uint64_t P = 1ull << pl.radixBits;
    out[0] = !pl.optimistic ? 0u : (c->hCtr->prjFallbackR ? 2u : 1u);
    out[1] = !c->res.probeOpt ? 0u : (c->hCtr->prjFallback ? 2u : 1u);
    out[2] = st[1]; out[3] = st[2]; out[4] = st[3];
    // R's keys (the fragments with their slack, or one dense run) + its offsets and fragment counts
    // (reserved with HJ_FLAG_KEEP_ROW_IDS: one dense run of 8-byte {key, row} elements)
    out[5] = (c->res.rows ? 8 * c->res.nR : 4 * (fragR ? P * pl.fragR.C2 * pl.fragR.cap2 : c->res.nR)) + 4 * (P + 1) + 4 * P * 16;
    out[6] = out[7] = 0;
    return HJ_OK;
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

int hj_prj_workspace_info(uint64_t rSize, uint64_t sSize, uint32_t radixBits, uint64_t out[4])
{
    if (!out || radixBits > 16) return HJ_ERR_INVALID;
    const uint32_t bits = radixBits ? radixBits : auto_radix_bits(rSize);
    const PrjPlan pl = prj_plan(rSize, sSize, bits);
    out[0] = pl.workspaceBytes; out[1] = pl.histEntries;
    out[2] = prj_hist_entries_needed(rSize, bits); out[3] = prj_hist_entries_needed(sSize, bits);
    return HJ_OK;
}

}  // extern "C"
