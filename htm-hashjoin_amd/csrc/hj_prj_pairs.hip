// hj_prj_pairs.hip -- the materialising form of the resident radix join for gfx950 (MI355X): hj_prj_build_dev on a
// context reserved with HJ_FLAG_KEEP_ROW_IDS, hj_prj_probe_pairs_dev.
//
// It runs the passes of hj_prj.hip in their row-id form (partition_relation_rows) and walks the work-item list its kernels
// build (enqueue_prj_items: k_prj_items_count / k_prj_items_fill, unchanged); both through hj_prj_impl.h.
//
//   row-id passes      the exact passes of hj_prj.hip over 8-byte {key, row} elements (partition_relation_rows there): the
//                      first histogram stamps the row -- idxBase + position in the input -- over each tuple's upper word
//                      (k_radix_hist_rows), the scatters move the elements whole (k_radix_scatter<false, false>).
//                      No histogram-free form: its fragments hold bare keys.
//   k_prj_rows_checksum  prjChecksum of a resident R in this format (k_prj_join reads bare keys)
//   k_prj_join_pairs   k_prj_probe_items with its result kept: per work item the R partition's LDS table holds
//                      (key >> radixBits, R row) entries, duplicates of a key as separate entries; a probe walks its run to the
//                      first empty slot and emits one (S row, R row) pair per equal entry
//
// Pair output through the stage of hj_pairs.hip (PairStage, hj_pairs.h): pairs are staged in LDS, a full stage claims its run of the two output
// planes with ONE 64-bit atomicAdd on the cursor and leaves as 16-byte stores; pairs at or beyond `capacity` are counted and not written.
// LDS: table 15360 slots x (4 B key + 4 B row) = 120 KiB, stage 4096 pairs x 8 B = 32 KiB, 152 KiB of the CU's 160.
//
// Join kinds (hj_prj_probe_join_dev): the kind K is a template parameter of k_prj_join_pairs; K = INNER is the kernel as it
// was. An item's S range is probed once per LDS build of its R partition, so "has matched" must survive the block loop:
// a thread meets the same <= kPrjItemS / kJoinThreads = 64 S elements in every block, and one 64-bit register holds their
// flags. LEFT writes the inner pairs per block and the (S row, kNoRow) row in the LAST block for flags still clear; SEMI
// the S row in the first block that matches it; ANTI the S row in the last block. A padding lane holds a clamped COPY of
// the item's last element (load_s): j < nSi gates every row of these kinds, not only the walk. LEFT and ANTI also take
// items of partitions without R tuples (k_prj_items_count, rless): no build, every element unmatched.

#include "hj_prj_impl.h"

namespace hj {

constexpr uint32_t kPairSlots = 15360;            // table slots: a key plane and a row plane of 60 KiB each
constexpr uint32_t kPairBlockTuples = 11520;      // R tuples per LDS build (load <= 0.75)
constexpr int kPairElems = 2;                     // S elements per thread and round: on unique R keys a round fits half a stage
constexpr size_t kPairLdsBytes = sizeof(uint32_t) * (2 * kPairSlots + 2 * kStagePairs);
static_assert(kPairLdsBytes + 1024 <= 160 * 1024, "table, stage and the few static words must fit one CU's LDS");
static_assert(kPairBlockTuples * 4 <= kPairSlots * 3, "a probe's walk ends at an empty slot: the table is never full");
static_assert((uint32_t)kPairElems * kJoinThreads <= kStagePairs, "a round of single matches fits an empty stage");
static_assert(kPrjItemS / kJoinThreads <= 64, "the matched flags of a thread's S elements of one item fit one 64-bit register");

// Slot of key-remainder k: the Fibonacci hash of join_hash, scaled to a slot count that is no power of two
__device__ __forceinline__ uint32_t pair_hash(uint32_t k) { return __umulhi(k * 0x9E3779B1u, kPairSlots); }
__device__ __forceinline__ uint32_t pair_next(uint32_t h) { return h + 1 == kPairSlots ? 0u : h + 1; }

// prjChecksum of a resident R of {key, row} elements, as k_prj_join sums it: (key >> radixBits) & (nextpow2(|partition|) - 1)
__global__ void __launch_bounds__(kBlock)
k_prj_rows_checksum(const uint2* __restrict__ partR, const uint32_t* __restrict__ offR, uint32_t radixBits, uint32_t nParts,
                    Counters* __restrict__ ctr)
{
    unsigned long long checksum = 0;
    for (uint32_t pid = blockIdx.x; pid < nParts; pid += gridDim.x) {
        const uint32_t rb = offR[pid], re = offR[pid + 1];
        if (re == rb) continue;
        const uint32_t idxMask = next_pow2_u32(re - rb) - 1;
        for (uint32_t i = rb + threadIdx.x; i < re; i += kBlock) checksum += (partR[i].x >> radixBits) & idxMask;
    }
    for (int off = 32; off > 0; off >>= 1) checksum += __shfl_down(checksum, off, 64);
    if ((threadIdx.x & 63) == 0 && checksum) atomicAdd(&counter_shard(ctr)->prjChecksum, checksum);
}

// items[0 .. *nItemsAt) taken through *ticket (zeroed by the host), as in k_prj_probe_items; both relations in the exact
// layout: partition pid = part[off[pid] .. off[pid + 1]), elements {x = key, y = row}. The arrays are separate __restrict__
// parameters (k_prj_join: members of a struct became vector loads), and what an item reads is looked up before its LDS work.
// K: hj_join_kind. out.cursor[1]: LEFT's unmatched S elements.
// MARK (INNER and LEFT only): `out` also carries the R-side match marks (RMarks, hj_pairs.h; base 0: an R row is its
// position in the relation given to the build). Every produced R row sets its bit in one of two places: where the staged
// R plane is read at a flush (stage_flush, whatever the capacity lets out), and in the `put` of the direct-write round,
// which bypasses the stage.
template <int K, bool MARK>
__global__ void __launch_bounds__(kJoinThreads)
k_prj_join_pairs(const uint2* __restrict__ partR, const uint32_t* __restrict__ offR,
                 const uint2* __restrict__ partS, const uint32_t* __restrict__ offS,
                 const uint2* __restrict__ items, const uint32_t* __restrict__ nItemsAt, unsigned long long* __restrict__ ticket,
                 uint32_t radixBits, PairsOutOf<MARK> out, Counters* __restrict__ ctr)
{
    static_assert(!MARK || K <= kLeft, "only the kinds that produce R rows mark them");
    extern __shared__ uint32_t pairLds[];
    uint32_t* const tabK = pairLds;                    // key remainders, kEmpty32 = free
    uint32_t* const tabR = tabK + kPairSlots;          // the R row of the slot's entry
    __shared__ uint32_t wtot[2 * (kJoinThreads / kWave)];      // the stage's words (PairStage::wtot, base)
    __shared__ unsigned long long sBase;
    __shared__ uint32_t sNext;
    // the stage behind the table: S rows, R rows
    PairStage<kJoinThreads> st{tabR + kPairSlots, tabR + kPairSlots + kStagePairs, wtot, &sBase, 0u, 0u, 0ull, 0ull, 0u};

    const uint32_t nItems = *nItemsAt;
    constexpr bool kRless = K == kLeft || K == kAnti;  // items of partitions without R tuples are in the list
    // the matches of one S element: their number, the R row of the first
    auto walk = [&](uint32_t key, bool ok, uint32_t& first) {
        uint32_t m = 0;
        if (ok) {
            const uint32_t k = key >> radixBits;
            uint32_t h = pair_hash(k);
            for (;;) {
                const uint32_t v = tabK[h];
                if (v == kEmpty32) break;
                if (v == k) {
                    if constexpr (K <= kLeft) { if (m == 0) first = tabR[h]; }       // SEMI and ANTI never read the row plane
                    ++m;
                }
                h = pair_next(h);
            }
        }
        return m;
    };
    // put(S row, R row) for each of the m matches: the first from the register, further ones (duplicate keys in R) by a second walk
    // rows: the element's rows of the kind in this block (INNER: m); LEFT's unmatched row is rows > m
    auto emit = [&](uint2 e, uint32_t m, uint32_t first, uint32_t rows, auto&& put) {
        if constexpr (K >= kSemi) { if (rows) put(e.y, 0u); return; }
        if constexpr (K == kLeft) if (rows > m) put(e.y, kNoRow);
        if (m == 0) return;
        put(e.y, first);
        if (m == 1) return;
        const uint32_t k = e.x >> radixBits;
        uint32_t h = pair_hash(k), seen = 0;
        for (;;) {
            const uint32_t v = tabK[h];
            if (v == kEmpty32) break;
            if (v == k && seen++) put(e.y, tabR[h]);
            h = pair_next(h);
        }
    };

    for (;;) {
        if (threadIdx.x == 0) sNext = (uint32_t)atomicAdd(ticket, 1ull);
        __syncthreads();
        const uint32_t cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)sNext);
        if (cur >= nItems) break;                      // workgroup-uniform
        // (sNext is written again only behind the barriers of this item: every item runs the block loop at least once, and
        // a pass through it ends at a barrier whether it built a table or, for an item without R tuples, did not)
        const uint2 it = items[cur];
        const uint32_t rb = offR[it.x], nRp = offR[it.x + 1] - rb;
        const uint32_t sb0 = offS[it.x], lo = it.y * kPrjItemS, rest = offS[it.x + 1] - sb0 - lo;
        const uint32_t sb = sb0 + lo, nSi = rest < kPrjItemS ? rest : kPrjItemS;      // >= 1: k_prj_items_count
        auto load_s = [&](uint32_t j0, uint2 (&e)[kPairElems]) {       // clamped: every lane loads a valid address
#pragma unroll
            for (int u = 0; u < kPairElems; ++u) {
                const uint32_t j = j0 + (uint32_t)u * kJoinThreads + threadIdx.x;
                e[u] = partS[sb + (j < nSi ? j : nSi - 1)];
            }
        };
        // an R partition larger than one table: several builds, the item's S probed against each
        unsigned long long seen = 0;                   // bit (round * kPairElems + u): that S element matched in some block
        // (an item without R tuples -- kRless only -- takes one pass without a build: every valid element is unmatched)
        for (uint32_t blk = 0; blk < nRp || (kRless && blk == 0); blk += kPairBlockTuples) {
            const uint32_t bn = nRp - blk > kPairBlockTuples ? kPairBlockTuples : nRp - blk;
            const bool last = nRp - blk <= kPairBlockTuples;           // (nRp == 0: the only pass is the last)
            const bool built = !kRless || nRp != 0;                    // workgroup-uniform
            uint2 nxt[kPairElems];
            load_s(0u, nxt);                                           // in flight while the table is built
            if (built) {
                for (uint32_t i = threadIdx.x; i < kPairSlots; i += kJoinThreads) tabK[i] = kEmpty32;
                __syncthreads();
                for_run(partR, rb + blk, 0u, bn, [&](uint2 e) {
                    const uint32_t k = e.x >> radixBits;
                    uint32_t h = pair_hash(k);
                    while (atomicCAS(&tabK[h], kEmpty32, k) != kEmpty32) h = pair_next(h);    // an equal key is one more entry
                    tabR[h] = e.y;
                });
                __syncthreads();
            }
            // rounds of kPairElems S elements per thread; every thread runs the same number of them (they meet at barriers)
            for (uint32_t j0 = 0; j0 < nSi; j0 += kPairElems * kJoinThreads) {
                uint2 e[kPairElems];
#pragma unroll
                for (int u = 0; u < kPairElems; ++u) e[u] = nxt[u];
                load_s(j0 + kPairElems * kJoinThreads < nSi ? j0 + kPairElems * kJoinThreads : j0, nxt);
                uint32_t m[kPairElems], first[kPairElems], rows[kPairElems], mine = 0;
#pragma unroll
                for (int u = 0; u < kPairElems; ++u) {
                    first[u] = 0;
                    const bool valid = j0 + (uint32_t)u * kJoinThreads + threadIdx.x < nSi;
                    m[u] = walk(e[u].x, valid && built, first[u]);
                    if constexpr (K == kInner) {
                        rows[u] = m[u];
                    } else {
                        // the element's flag; a padding lane (a clamped copy of the last element) writes no row of any kind
                        const unsigned long long bit = 1ull << (j0 / kJoinThreads + (uint32_t)u);
                        const bool none = valid && last && m[u] == 0 && !(seen & bit);
                        st.inner += m[u];
                        if constexpr (K == kLeft) { rows[u] = m[u] + (uint32_t)none; st.unmatched += (uint32_t)none; }
                        if constexpr (K == kSemi) rows[u] = (uint32_t)(m[u] != 0 && !(seen & bit));
                        if constexpr (K == kAnti) rows[u] = (uint32_t)none;
                        if (m[u]) seen |= bit;
                    }
                    mine += rows[u];
                }
                bool any;
                uint32_t tot;
                const uint32_t before = stage_scan(st, mine, false, any, tot);     // rows of the round in front of this lane's
                if (tot > kStagePairs) {
                    // Duplicate keys on both sides: more pairs than a stage holds (one S tuple alone can match a whole
                    // table). The round claims its run itself and every lane writes its pairs straight to the planes.
                    if (st.fill) stage_flush<K>(st, out);
                    if (threadIdx.x == 0) sBase = atomicAdd(out.cursor, (unsigned long long)tot);
                    __syncthreads();
                    // (sBase is written again only behind the next round's barrier)
                    uint64_t g = sBase + before;
                    auto put = [&](uint32_t s, uint32_t r) {
                        if (g < out.capacity) {
                            out.s[g] = s;
                            if constexpr (K <= kLeft) out.r[g] = r;
                        }
                        if constexpr (MARK) mark_r_row(out.marks, r);      // written or not
                        ++g;
                    };
#pragma unroll
                    for (int u = 0; u < kPairElems; ++u) emit(e[u], m[u], first[u], rows[u], put);
                    st.found += tot;
                } else {
                    uint32_t pos = stage_place<K>(st, out, tot) + before;
                    auto put = [&](uint32_t s, uint32_t r) {
                        st.s[pos] = s;
                        if constexpr (K <= kLeft) st.r[pos] = r;
                        ++pos;
                    };
#pragma unroll
                    for (int u = 0; u < kPairElems; ++u) emit(e[u], m[u], first[u], rows[u], put);
                }
            }
            __syncthreads();                                           // the table is read no more
        }
    }
    stage_finish<K>(st, out, ctr, &Counters::Shard::prjMatches);
}

hipError_t prj_pairs_set_attributes()
{
    hipError_t e = hipSuccess;
    for (uint32_t kind = 0; kind <= (uint32_t)kAnti; ++kind)
        for (const bool marks : {false, true})          // (a kind that marks nothing comes by twice)
            with_kind(kind, marks, [&](auto k, auto mark) {
                const auto kernel = k_prj_join_pairs<decltype(k)::value, decltype(mark)::value>;
                if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPairLdsBytes);
            });
    return e;
}

// R's row-id passes into buf.partR / res.offR (plan: exact passes only), then R's checksum
hipError_t launch_prj_build_rows(const PrjPlan& pl, const PrjBuffers& buf, const PrjResident& res, const uint64_t* R, uint64_t nR,
                                 int nCU, Counters* ctr, hipEvent_t evPartDone, hipEvent_t evScatter0, hipEvent_t evScatter1, hipStream_t s)
{
    const Work w = carve(pl, buf.work);
    hipError_t e;
    if ((e = partition_relation_rows(pl, w, R, nR, 0u, buf.tmpA, buf.partR, res.offR, s, evScatter0, evScatter1)) != hipSuccess) return e;
    if (evPartDone && (e = hipEventRecord(evPartDone, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(res.stats, 0, 4 * sizeof(unsigned long long), s)) != hipSuccess) return e;
    const uint32_t P = 1u << pl.radixBits;
    const unsigned want = 4u * (unsigned)nCU;
    hipLaunchKernelGGL(k_prj_rows_checksum, dim3(P < want ? P : want), dim3(kBlock), 0, s,
                       reinterpret_cast<const uint2*>(buf.partR), res.offR, pl.radixBits, P, ctr);
    return hipGetLastError();
}

// S's row-id passes into buf.partS (rows from sIdxBase), the work-item list, k_prj_join_pairs against the resident R.
// out.cursor and the word behind it are zeroed here; out.capacity 0 counts only. kind: hj_join_kind. marks: the MARK
// instantiation (INNER and LEFT); nullptr -- every caller that only counts, hj_prj_probe_dev among them -- the kernels as they were.
hipError_t launch_prj_probe_rows(uint32_t kind, const PrjPlan& planR, const PrjPlan& planS, const PrjBuffers& buf, const PrjResident& res,
                                 const uint64_t* S, uint64_t nS, uint64_t sIdxBase, PairsOut out, int nCU, Counters* ctr,
                                 hipEvent_t evPartDone, hipEvent_t evJoin0, hipStream_t s, const RMarks* marks)
{
    const Work w = carve(planS, buf.work);
    hipError_t e;
    if ((e = hipMemsetAsync(&ctr->prjFallback, 0, sizeof(unsigned long long), s)) != hipSuccess) return e;
    if ((e = partition_relation_rows(planS, w, S, nS, (uint32_t)sIdxBase, buf.tmpA, buf.partS, w.offS, s)) != hipSuccess) return e;
    if (evPartDone && (e = hipEventRecord(evPartDone, s)) != hipSuccess) return e;
    // the work items of the counting probe: the exact layout's offsets are the same whatever the element width
    const uint32_t P = 1u << planR.radixBits;
    if ((e = hipMemsetAsync(out.cursor, 0, 2 * sizeof(unsigned long long), s)) != hipSuccess) return e;
    // LEFT and ANTI: the S tuples of a partition without R tuples are rows too, so such a partition gets its items
    const bool rless = kind == (uint32_t)kLeft || kind == (uint32_t)kAnti;
    if ((e = enqueue_prj_items(res, res.offR, nullptr, 0u, w.offS, nullptr, 0u, P, ctr, s, rless)) != hipSuccess) return e;
    if (evJoin0 && (e = hipEventRecord(evJoin0, s)) != hipSuccess) return e;
    with_kind(kind, marks != nullptr, [&](auto k, auto mark) {
        hipLaunchKernelGGL((k_prj_join_pairs<decltype(k)::value, decltype(mark)::value>), dim3((unsigned)nCU), dim3(kJoinThreads), kPairLdsBytes, s,
                           reinterpret_cast<const uint2*>(buf.partR), res.offR, reinterpret_cast<const uint2*>(buf.partS), w.offS,
                           res.items, res.itemCnt + 2ull * P, res.stats, planR.radixBits, pairs_out_of<decltype(mark)::value>(out, marks), ctr);
    });
    return hipGetLastError();
}

}  // namespace hj
