// hj_prj.h -- the radix join as the host layer sees it: the plans and buffers of the partition passes, the resident R,
// the row-id (materialising) and the aggregating forms of the resident join, and the multi-GPU shard split.
#pragma once

#include "hj_common.h"
#include "hj_pairs.h"
#include "hj_columns.h"

namespace hj {

// ---- PRJ (defined in hj_prj.hip) -------------------------------------------
// Fragment geometry of the histogram-free partitioning of ONE relation (hj_prj.hip, "histogram-free partitioning"):
// pass 1 cuts the relation into C1 chunks and writes bin b of chunk c to the fragment (b * C1 + c) of cap1 key slots;
// pass 2 cuts every pass-1 partition (C1 fragments) into C2 chunks and writes to fragments of cap2 slots; a final
// partition is C2 fragments. C = 0: the relation takes the exact path only.
struct PrjFrag {
    uint32_t C1, cap1, chunkLen1;
    uint32_t C2, cap2, log2C2;
};
struct PrjPlan {
    uint32_t radixBits;   // total
    uint32_t bits1, bits2;
    bool     optimistic;               // try the histogram-free path first (both relations qualify)
    PrjFrag  fragR, fragS;
    uint64_t cnt1Entries, cnt2EntriesR, cnt2EntriesS;   // fragment counters in the workspace
    uint64_t maxChunks1, maxChunks2;   // chunk descriptors per pass (upper bounds over both relations)
    uint64_t histEntries, scanBlocks;  // histogram / block-sum entries: the larger need of R's and S's layouts in
                                       // either pass (the chunk length, hence the chunk count, is NOT monotone in
                                       // the relation size: the smaller relation can need the larger histogram)
    size_t   workspaceBytes;           // everything below, excluding tuple buffers
};
// Sizes the workspace for (nR, nS): each relation is laid out with its own chunk length (run_pass), so every
// region is the maximum over the two relations' layouts.
// mode (hj_params.prjMode): 0 = histogram-free path for large relations, 1 = exact path only, 2 = histogram-free path
// at any size it can be laid out for (tests)
PrjPlan prj_plan(uint64_t nR, uint64_t nS, uint32_t radixBits, uint32_t mode = 0);
// histogram entries the passes over ONE relation of n tuples write (what run_pass memsets and scans)
uint64_t prj_hist_entries_needed(uint64_t n, uint32_t radixBits);
struct PrjBuffers {
    uint64_t* tmpA;      // max(nR,nS) tuples
    uint64_t* partR;     // nR tuples (final partitioned R)
    uint64_t* partS;     // nS tuples
    void*     work;      // plan.workspaceBytes
};
// Enqueues partition(R), partition(S) and the per-partition LDS join.
// evPartDone (may be null) is recorded between partitioning and join.
hipError_t launch_prj(const PrjPlan& plan, const PrjBuffers& buf,
                      const uint64_t* R, uint64_t nR, const uint64_t* S, uint64_t nS, int nCU,
                      Counters* ctr, hipEvent_t evPartDone, hipEvent_t evScatter0, hipEvent_t evScatter1, hipStream_t s);
// evScatter0/1 (may be null): recorded around the pass-1 scatter of R, PRJ's dominant kernel
hipError_t prj_set_attributes();          // per device, at hj_create

// ---- PRJ with a resident R (hj_prj_build_dev / hj_prj_probe_dev, defined in hj_prj.hip) ----
// Everything of R's partitioning that must outlive the scratch workspace (whose layout every slice plan re-carves) and
// the per-probe work-item list, in one buffer of prj_resident_bytes(radixBits, maxSlice) sized at hj_reserve.
struct PrjResident {
    uint32_t* offR;                 // [P + 1] R's partition offsets (exact passes)
    uint32_t* cnt2R;                // [P * 16] R's pass-2 fragment counts (histogram-free passes)
    uint32_t* itemCnt;              // [2P + 1] items per partition: split partitions first, then the rest; scanned in place
    uint32_t* scanSums;             // scan workspace of itemCnt
    uint2* items;                   // [P + maxSlice / kPrjItemS + 1] (partition, S chunk)
    unsigned long long* stats;      // [4] next item ticket, items, split partitions, largest S partition;
                                    // [4]: the pair count of a counting probe against a {key, row} R (hj_prj_probe_dev)
};
constexpr uint32_t kPrjItemS = 1u << 16;  // S tuples per join work item at most (hj_prj.hip, k_prj_probe_items)
size_t prj_resident_bytes(uint32_t radixBits, uint64_t maxSlice);
PrjResident prj_resident_carve(void* base, uint32_t radixBits, uint64_t maxSlice);
// R's passes into buf.partR / res (plan = prj_plan(nR, 0, ...)), then R's checksum (k_prj_join without S);
// Counters::prjFallbackR = R's fallback. evPartDone: between the passes and the checksum.
hipError_t launch_prj_build(const PrjPlan& plan, const PrjBuffers& buf, const PrjResident& res, const uint64_t* R, uint64_t nR,
                            int nCU, Counters* ctr, hipEvent_t evPartDone, hipEvent_t evScatter0, hipEvent_t evScatter1, hipStream_t s);
// S's passes into buf.partS (planS = prj_plan(nS, nS, ...)), the work-item list, the skew-split join against the resident R
// (planR = the build's plan). evPartDone: after S's passes; evJoin0: right before the join kernel.
hipError_t launch_prj_probe(const PrjPlan& planR, uint64_t nR, const PrjPlan& planS, const PrjBuffers& buf, const PrjResident& res,
                            const uint64_t* S, uint64_t nS, int nCU, Counters* ctr, hipEvent_t evPartDone, hipEvent_t evJoin0,
                            hipStream_t s);

// ---- row-id form of the resident radix join (HJ_FLAG_KEEP_ROW_IDS; defined in hj_prj_pairs.hip) ----
// buf.partR / partS / tmpA hold 8-byte {key, row} elements; exact passes only (plan = prj_plan(.., mode 1)).
// R's passes (row = position in R) into buf.partR / res.offR, then R's checksum.
hipError_t launch_prj_build_rows(const PrjPlan& plan, const PrjBuffers& buf, const PrjResident& res, const uint64_t* R, uint64_t nR,
                                 int nCU, Counters* ctr, hipEvent_t evPartDone, hipEvent_t evScatter0, hipEvent_t evScatter1, hipStream_t s);
// S's passes (row = sIdxBase + position in S), the work-item list, the join that emits (S row, R row) pairs to `out`
// (out.cursor is zeroed on the stream first; out.capacity 0: the pairs are counted only). Adds to Counters::prjMatches.
// kind: hj_join_kind. HJ_JOIN_LEFT and HJ_JOIN_ANTI give partitions with S tuples and no R tuple a work item of their own.
// marks != nullptr (kinds INNER and LEFT only): the join's MARK instantiation (RMarks above; base 0, the row is the position in R)
hipError_t launch_prj_probe_rows(uint32_t kind, const PrjPlan& planR, const PrjPlan& planS, const PrjBuffers& buf, const PrjResident& res,
                                 const uint64_t* S, uint64_t nS, uint64_t sIdxBase, PairsOut out, int nCU, Counters* ctr,
                                 hipEvent_t evPartDone, hipEvent_t evJoin0, hipStream_t s, const RMarks* marks = nullptr);

// ---- aggregating form of the resident radix join (defined in hj_prj_agg.hip) ----

// The resident radix join's planes hold n = rSize entries each, indexed by resident position (the index into partR).
// what: 0 slots, 1 R tuples per LDS build, 2 S elements per round of a workgroup, 3 kPrjItemS (hj_prj_agg_layout_info)
uint32_t agg_layout(uint32_t nCols, uint32_t what);
hipError_t launch_agg_fill(const AggPlanes& pl, const AggOps& ops, uint32_t nCols, uint64_t n, int nCU, hipStream_t s);
// out.col[c][partR[pos].y] = pl.acc[c][pos], out.count likewise (may be null); plain stores, the planes are only read
hipError_t launch_agg_rows(const uint64_t* partR, const AggPlanes& pl, const AggRowsOut& out, uint32_t nCols, uint64_t n, int nCU, hipStream_t s);
// launch_prj_probe_rows with the accumulators in place of the pairs: S's row-id passes (rows from 0: src is indexed by the
// position in S), the work-item list, k_prj_join_agg. Adds to Counters::prjMatches and to *last, which is zeroed here first.
hipError_t launch_prj_probe_agg(const PrjPlan& planR, const PrjPlan& planS, const PrjBuffers& buf, const PrjResident& res,
                                const uint64_t* S, uint64_t nS, const AggSrc& src, const AggOps& ops, uint32_t nCols, const AggPlanes& pl,
                                unsigned long long* last, int nCU, Counters* ctr, hipEvent_t evPartDone, hipEvent_t evJoin0, hipStream_t s);

// ---- multi-GPU destination split (defined in hj_shard.hip) ----

// one order-preserving radix pass, tuples in, keys out;
// destination = (key >> digitShift) & (nShards - 1)
size_t shard_work_bytes(uint64_t n, uint32_t nShards);
hipError_t launch_shard_hist(const uint64_t* in, uint64_t n, uint32_t nShards, uint32_t digitShift, void* work,
                             unsigned long long* counts, hipStream_t s);
hipError_t launch_shard_scatter_ordered(const uint64_t* in, uint64_t n, uint32_t nShards, uint32_t digitShift, void* work,
                                        uint32_t* outKeys, hipStream_t s);

}  // namespace hj
