// hj_prj_agg.hip -- the aggregating form of the resident radix join for gfx950 (MI355X): hj_prj_agg_begin,
// hj_prj_probe_agg_dev, hj_prj_agg_rows_dev. COUNT / SUM / MIN / MAX of S values per R row, without the pairs.
//
// It uses the row-id passes (partition_relation_rows) and the work-item list (enqueue_prj_items, rless = false) of
// hj_prj.hip unchanged, as hj_prj_pairs.hip does; both through hj_prj_impl.h.
//
//   accumulators       one 64-bit match-count plane and nCols 64-bit planes of rSize entries in global memory, indexed by
//                      RESIDENT POSITION -- the index into partR -- so that the entries of one R partition, hence of one
//                      work item, are one contiguous range (AggPlanes)
//   k_agg_fill         the planes at their identities (hj_prj_agg_begin)
//   k_prj_join_agg<NC> k_prj_join_pairs without its pair stage: per work item the R partition's LDS table holds
//                      (key >> radixBits, position in the block) entries, duplicates of a key as separate entries; the block's
//                      tuples have one 32-bit match count and NC 64-bit accumulators in LDS, at their identities. A
//                      matching S element fetches its values src[c][row] once -- a scattered read, only of valid elements
//                      -- and walks its run to the first empty slot, updating EVERY equal entry with LDS atomics. At the
//                      end of a block the entries that were hit leave for the global planes at rb + blk + i: contiguous
//                      addresses, 64-bit global atomics of the column's op, because the items of a split S partition
//                      run at the same time and flush into the same entries.
//   k_agg_rows         resident order -> R rows: out[c][partR[pos].y] = acc[c][pos], plain stores (hj_prj_agg_rows_dev)
//
// LDS per NC (agg_slots / agg_block_tuples): a slot is a 4-byte key remainder and a 2-byte position, a block tuple a 4-byte
// count and NC 8-byte accumulators; the table's load is 0.75, so a slot costs 6 + 0.75 * (4 + 8 NC) = 9 + 6 NC bytes:
//   NC  slots   block tuples  bytes
//   1   10752   8064          161280
//   2    7680   5760          161280
//   3    5888   4416          158976
//   4    4864   3648          160512
// The walk is per lane. A variant that walked in step and let a wavefront whose lanes all name one entry reduce in registers
// and issue one LDS atomic was measured under Zipf and did not pay (profiles/join_aggregate.md).
// All integer work, bound by the scattered value reads and the LDS atomics; no MFMA. Exact: every op is associative and
// commutative on 64-bit integers (SUM wraps), so no result depends on the order of the adds.

#include "hj_prj_impl.h"

namespace hj {

constexpr uint32_t kAggLdsBudget = 160 * 1024 - 1024;         // the CU's LDS less the kernel's few static words
constexpr int kAggElems = 2;                                  // S elements per thread and round
constexpr uint32_t agg_slots(uint32_t nc) { return kAggLdsBudget / (9u + 6u * nc) / 256u * 256u; }
constexpr uint32_t agg_block_tuples(uint32_t nc) { return agg_slots(nc) / 4u * 3u; }
constexpr size_t agg_lds_bytes(uint32_t nc)
{
    return (size_t)agg_block_tuples(nc) * (8u * nc + 4u) + (size_t)agg_slots(nc) * 6u;
}
uint32_t agg_layout(uint32_t nCols, uint32_t what)
{
    return what == 0 ? agg_slots(nCols) : what == 1 ? agg_block_tuples(nCols) : what == 2 ? (uint32_t)kAggElems * kJoinThreads : kPrjItemS;
}

__global__ void __launch_bounds__(kBlock)
k_agg_fill(AggPlanes pl, AggOps ops, uint32_t nCols, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
        pl.count[i] = 0ull;
        for (uint32_t c = 0; c < nCols; ++c) pl.acc[c][i] = agg_identity(ops.op[c], ops.sgn[c]);
    }
}

__global__ void __launch_bounds__(kBlock)
k_agg_rows(const uint2* __restrict__ partR, AggPlanes pl, AggRowsOut out, uint32_t nCols, uint32_t n)
{
    for (uint32_t pos = blockIdx.x * kBlock + threadIdx.x; pos < n; pos += gridDim.x * kBlock) {
        const uint32_t row = partR[pos].y;
        if (row >= n) continue;                        // (no row of the build: its rows are the positions in dR)
        for (uint32_t c = 0; c < nCols; ++c) out.col[c][row] = pl.acc[c][pos];
        if (out.count) out.count[row] = pl.count[pos];
    }
}

// items, ticket and both relations as in k_prj_join_pairs. src.p / src.valid are indexed by the S element's row (sIdxBase 0:
// its position in the slice). last: the matches of this call alone, next to Counters::prjMatches.
template <int NC>
__global__ void __launch_bounds__(kJoinThreads)
k_prj_join_agg(const uint2* __restrict__ partR, const uint32_t* __restrict__ offR,
               const uint2* __restrict__ partS, const uint32_t* __restrict__ offS,
               const uint2* __restrict__ items, const uint32_t* __restrict__ nItemsAt, unsigned long long* __restrict__ ticket,
               uint32_t radixBits, AggSrc src, AggOps ops, AggPlanes pl, unsigned long long* __restrict__ last, Counters* __restrict__ ctr)
{
    constexpr uint32_t kSlots = agg_slots(NC), kTuples = agg_block_tuples(NC);
    static_assert(agg_lds_bytes(NC) <= kAggLdsBudget, "accumulators, counts and table must fit one CU's LDS");
    static_assert(kTuples * 4 <= kSlots * 3, "a probe's walk ends at an empty slot: the table is never full");
    static_assert(kTuples <= 65536, "the position of a block tuple fits the 16-bit plane");
    static_assert(kTuples % 2 == 0 && kSlots % 2 == 0, "the planes behind the 8-byte accumulators stay aligned");
    extern __shared__ unsigned long long aggLds[];
    unsigned long long* const accL = aggLds;                           // [NC][kTuples]
    uint32_t* const cntL = reinterpret_cast<uint32_t*>(accL + NC * kTuples);     // [kTuples] matches of the block tuple
    uint32_t* const tabK = cntL + kTuples;                             // [kSlots] key remainders, kEmpty32 = free
    uint16_t* const tabP = reinterpret_cast<uint16_t*>(tabK + kSlots); // [kSlots] the entry's position in the block
    __shared__ uint32_t sNext;

    const auto hash = [](uint32_t k) { return __umulhi(k * 0x9E3779B1u, kSlots); };
    const auto next = [](uint32_t h) { return h + 1 == kSlots ? 0u : h + 1; };
    const uint32_t nItems = *nItemsAt;
    unsigned long long matches = 0;

    for (;;) {
        if (threadIdx.x == 0) sNext = (uint32_t)atomicAdd(ticket, 1ull);
        __syncthreads();
        const uint32_t cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)sNext);
        if (cur >= nItems) break;                      // workgroup-uniform
        // (sNext is written again only behind the barriers of this item: nRp >= 1, so the block loop runs at least once)
        const uint2 it = items[cur];
        const uint32_t rb = offR[it.x], nRp = offR[it.x + 1] - rb;
        const uint32_t sb0 = offS[it.x], lo = it.y * kPrjItemS, rest = offS[it.x + 1] - sb0 - lo;
        const uint32_t sb = sb0 + lo, nSi = rest < kPrjItemS ? rest : kPrjItemS;      // >= 1: k_prj_items_count
        auto load_s = [&](uint32_t j0, uint2 (&e)[kAggElems]) {        // clamped: every lane loads a valid address
#pragma unroll
            for (int u = 0; u < kAggElems; ++u) {
                const uint32_t j = j0 + (uint32_t)u * kJoinThreads + threadIdx.x;
                e[u] = partS[sb + (j < nSi ? j : nSi - 1)];
            }
        };
        // an R partition larger than one table: several builds, the item's S probed against each; an entry lives in one block
        for (uint32_t blk = 0; blk < nRp; blk += kTuples) {
            const uint32_t bn = nRp - blk > kTuples ? kTuples : nRp - blk;
            uint2 nxt[kAggElems];
            load_s(0u, nxt);                                           // in flight while the table is built
            for (uint32_t i = threadIdx.x; i < kSlots; i += kJoinThreads) tabK[i] = kEmpty32;
            for (uint32_t i = threadIdx.x; i < bn; i += kJoinThreads) {
                cntL[i] = 0u;
#pragma unroll
                for (int c = 0; c < NC; ++c) accL[c * kTuples + i] = agg_identity(ops.op[c], ops.sgn[c]);
            }
            __syncthreads();
            for (uint32_t i0 = threadIdx.x; i0 < bn; i0 += 4u * kJoinThreads) {        // four key loads in flight
                uint32_t key[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t i = i0 + (uint32_t)u * kJoinThreads;
                    key[u] = partR[rb + blk + (i < bn ? i : bn - 1)].x;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t i = i0 + (uint32_t)u * kJoinThreads;
                    if (i >= bn) continue;
                    const uint32_t k = key[u] >> radixBits;
                    uint32_t h = hash(k);
                    while (atomicCAS(&tabK[h], kEmpty32, k) != kEmpty32) h = next(h);   // an equal key is one more entry
                    tabP[h] = (uint16_t)i;
                }
            }
            __syncthreads();
            // rounds of kAggElems S elements per thread; a padding lane holds a clamped COPY of the item's last element and adds nothing
            for (uint32_t j0 = 0; j0 < nSi; j0 += kAggElems * kJoinThreads) {
                uint2 e[kAggElems];
#pragma unroll
                for (int u = 0; u < kAggElems; ++u) e[u] = nxt[u];
                load_s(j0 + kAggElems * kJoinThreads < nSi ? j0 + kAggElems * kJoinThreads : j0, nxt);
#pragma unroll
                for (int u = 0; u < kAggElems; ++u) {
                    if (j0 + (uint32_t)u * kJoinThreads + threadIdx.x >= nSi) continue;          // a padding lane adds nothing
                    const uint32_t k = e[u].x >> radixBits;
                    uint32_t h = hash(k);
                    bool have = false;                 // the element's values are fetched at its first match
                    bool ok[NC];
                    unsigned long long v[NC];
                    for (;;) {
                        const uint32_t t = tabK[h];
                        if (t == kEmpty32) break;
                        if (t == k) {
                            if (!have) {
                                have = true;
#pragma unroll
                                for (int c = 0; c < NC; ++c) {
                                    const uint32_t* const valid = src.valid[c];
                                    ok[c] = !valid || valid_bit(valid, e[u].y);
                                    v[c] = ok[c] ? agg_value(src.p[c], ops.op[c], ops.width[c], ops.sgn[c], e[u].y) : 0ull;
                                }
                            }
                            const uint32_t p = tabP[h];
                            __hip_atomic_fetch_add(&cntL[p], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
                            for (int c = 0; c < NC; ++c)
                                if (ok[c]) agg_apply<__HIP_MEMORY_SCOPE_WORKGROUP>(&accL[c * kTuples + p], ops.op[c], ops.sgn[c], v[c]);
                            ++matches;
                        }
                        h = next(h);
                    }
                }
            }
            __syncthreads();                                           // every update of the block is in LDS
            for (uint32_t i = threadIdx.x; i < bn; i += kJoinThreads) {
                const uint32_t m = cntL[i];
                if (m == 0) continue;                                  // never hit: the global entry keeps what it has
                const uint32_t g = rb + blk + i;
                __hip_atomic_fetch_add(&pl.count[g], (unsigned long long)m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const unsigned long long a = accL[c * kTuples + i];
                    if (a != agg_identity(ops.op[c], ops.sgn[c])) agg_apply<__HIP_MEMORY_SCOPE_AGENT>(&pl.acc[c][g], ops.op[c], ops.sgn[c], a);
                }
            }
            __syncthreads();                                           // table and accumulators are read no more
        }
    }
    matches = wave_sum(matches);
    if ((threadIdx.x & (kWave - 1)) == 0 && matches) {
        atomicAdd(&counter_shard(ctr)->prjMatches, matches);
        atomicAdd(last, matches);
    }
}

template <class F>
static void with_agg_cols(uint32_t nCols, F&& f)
{
    using std::integral_constant;
    if (nCols == 1) f(integral_constant<int, 1>{});
    else if (nCols == 2) f(integral_constant<int, 2>{});
    else if (nCols == 3) f(integral_constant<int, 3>{});
    else f(integral_constant<int, 4>{});
}

hipError_t prj_agg_set_attributes()
{
    hipError_t e = hipSuccess;
    for (uint32_t nc = 1; nc <= kAggMaxCols; ++nc)
        with_agg_cols(nc, [&](auto n) {
            constexpr int NC = decltype(n)::value;
            if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_prj_join_agg<NC>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)agg_lds_bytes(NC));
        });
    return e;
}

hipError_t launch_agg_fill(const AggPlanes& pl, const AggOps& ops, uint32_t nCols, uint64_t n, int nCU, hipStream_t s)
{
    const uint64_t blocks = (n + kBlock - 1) / kBlock, want = 8ull * (uint64_t)nCU;
    hipLaunchKernelGGL(k_agg_fill, dim3((unsigned)(blocks < want ? blocks : want)), dim3(kBlock), 0, s, pl, ops, nCols, n);
    return hipGetLastError();
}

hipError_t launch_agg_rows(const uint64_t* partR, const AggPlanes& pl, const AggRowsOut& out, uint32_t nCols, uint64_t n, int nCU, hipStream_t s)
{
    const uint64_t blocks = (n + kBlock - 1) / kBlock, want = 8ull * (uint64_t)nCU;
    hipLaunchKernelGGL(k_agg_rows, dim3((unsigned)(blocks < want ? blocks : want)), dim3(kBlock), 0, s,
                       reinterpret_cast<const uint2*>(partR), pl, out, nCols, (uint32_t)n);
    return hipGetLastError();
}

// S's row-id passes into buf.partS (rows from 0), the work-item list of the counting probe, k_prj_join_agg against the resident R.
// *last is zeroed here.
hipError_t launch_prj_probe_agg(const PrjPlan& planR, const PrjPlan& planS, const PrjBuffers& buf, const PrjResident& res,
                                const uint64_t* S, uint64_t nS, const AggSrc& src, const AggOps& ops, uint32_t nCols, const AggPlanes& pl,
                                unsigned long long* last, int nCU, Counters* ctr, hipEvent_t evPartDone, hipEvent_t evJoin0, hipStream_t s)
{
    const Work w = carve(planS, buf.work);
    hipError_t e;
    if ((e = hipMemsetAsync(&ctr->prjFallback, 0, sizeof(unsigned long long), s)) != hipSuccess) return e;
    if ((e = partition_relation_rows(planS, w, S, nS, 0u, buf.tmpA, buf.partS, w.offS, s)) != hipSuccess) return e;
    if (evPartDone && (e = hipEventRecord(evPartDone, s)) != hipSuccess) return e;
    const uint32_t P = 1u << planR.radixBits;
    if ((e = hipMemsetAsync(last, 0, sizeof(unsigned long long), s)) != hipSuccess) return e;
    if ((e = enqueue_prj_items(res, res.offR, nullptr, 0u, w.offS, nullptr, 0u, P, ctr, s, false)) != hipSuccess) return e;
    if (evJoin0 && (e = hipEventRecord(evJoin0, s)) != hipSuccess) return e;
    with_agg_cols(nCols, [&](auto n) {
        constexpr int NC = decltype(n)::value;
        hipLaunchKernelGGL((k_prj_join_agg<NC>), dim3((unsigned)nCU), dim3(kJoinThreads), agg_lds_bytes(NC), s,
                           reinterpret_cast<const uint2*>(buf.partR), res.offR, reinterpret_cast<const uint2*>(buf.partS), w.offS,
                           res.items, res.itemCnt + 2ull * P, res.stats, planR.radixBits, src, ops, pl, last, ctr);
    });
    return hipGetLastError();
}

}  // namespace hj
