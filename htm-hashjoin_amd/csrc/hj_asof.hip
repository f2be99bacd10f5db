// hj_asof.hip -- as-of joins for gfx950 (MI355X): hj_pairs_asof_dev and hj_pairs_asof_host.
//
// "The latest R row of the same key at or before S.ts": of the pairs that agree on the key, per S row the ONE pair whose R
// value is nearest on the permitted side of the S value. That is no filter on a pair -- whether a pair survives depends on
// the other pairs of its S row -- but an arg-max per S row, so the step takes three passes over the pair list and two
// planes with one entry per S row, which the call initialises itself:
//
//   k_asof_best   bestVal[s] = max over the ELIGIBLE pairs (s, r) -- s[s] OP r[r] holds as a term of the condition step
//                 does -- of asof_key(r[r]) (hj_columns.h: an unsigned word that orders as the values do; the forward ops
//                 complement it, so every pass takes a maximum). 64-bit atomic max at agent scope.
//   k_asof_row    bestRow[s] = min over the eligible pairs whose key EQUALS bestVal[s] of their R row: ties on the value --
//                 -0.0 and 0.0 among them -- go to the lowest R row, the library's index-priority rule. 32-bit atomic min.
//   k_asof_keep   the pair-filter frame (hj_pairs.h) a third time: a live pair is kept iff its R row is bestRow[s]; staged,
//                 claimed, flushed and marked on both sides as k_pairs_where does it.
//
// Both planes hold a maximum / minimum over a SET of pairs, so the result does not depend on the order of the list or on
// scheduling. bestVal starts at 0, which is also a key an element can have (unsigned 0 under >=): that is no conflict,
// because pass 2 looks at eligible pairs only -- where no pair of an S row is eligible nobody touches its bestRow, and
// where one is, a bestVal of 0 is the true maximum.
//
// Passes 1 and 2 share asof_pairs: the frame's shape (1024 pairs per workgroup, four per lane, 64 apart), map loads, drop
// rule and spare rows, and where_load, the term loads of k_pairs_where -- both elements of all four pairs, with validity
// planes the eight words beside them, in pass 2 also the four bestVal words, in flight before the first compare.
// Runs: the probes of this library write the matches of one S tuple side by side (k_prj_join_pairs and k_probe_pairs: a
// lane stages all pairs of its S element at consecutive positions), so a list straight out of a probe holds the pairs of
// an S row as neighbours; behind a verify or condition step the frame's staging has dealt a wavefront's 256 pairs out
// lane by lane, and a run survives only in parts. k_asof_best therefore combines, per step of 64 neighbouring pairs, the
// keys of a run of equal S rows with k_pairs_agg's segmented scan (shuffles) and lets the run's last lane issue one
// atomic: a hot S row with 2^16 versions costs 2^10 atomic requests on its address instead of 2^16. It is an economy
// only -- runs are whatever the list happens to hold. Pass 2 issues one atomic per tied pair: ties are as rare as
// duplicate timestamps of one key.
// What it does NOT do: no packed single pass for narrow values, no "nearest" of both sides, no tolerance window, no as-of
// without an equality key; all pairs of an S row must be in ONE call (the planes are reset per call).

#include "hj_columns.h"

namespace hj {

namespace {

// The lane's four pairs of passes 1 and 2, settled: live (not dropped), si / ri (the rows, S's base off; a dropped pair's are
// spare rows, which exist), ok (live and eligible) and key (asof_key of the R element). Only called with sRows and rRows
// above 0. kBest: the four bestVal words of the S rows are loaded with the elements.
template <bool kValid, bool kBest>
__device__ __forceinline__ void asof_pairs(const uint32_t* __restrict__ mapS, const uint32_t* __restrict__ mapR, uint64_t nPairs,
                                           uint32_t sRowBase, uint32_t sRows, uint32_t rRows, const AsofTerm& t,
                                           const unsigned long long* __restrict__ bestVal,
                                           uint32_t (&si)[kFilterLanePairs], uint32_t (&ri)[kFilterLanePairs], bool (&live)[kFilterLanePairs],
                                           bool (&ok)[kFilterLanePairs], uint64_t (&key)[kFilterLanePairs],
                                           unsigned long long (&best)[kFilterLanePairs])
{
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const uint64_t k0 = (uint64_t)blockIdx.x * kFilterBlockPairs + w * kFilterWavePairs + lane;     // the lane's first pair
    uint32_t es[kFilterLanePairs], er[kFilterLanePairs];
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) {
        const uint64_t k = k0 + j * kFilterStepPairs;
        es[j] = er[j] = kNoRow;
        if (k < nPairs) { es[j] = __builtin_nontemporal_load(mapS + k); er[j] = __builtin_nontemporal_load(mapR + k); }
    }
    // a dropped pair reads, and ignores, one of the first rows
    const uint32_t spareS = threadIdx.x < sRows ? threadIdx.x : sRows - 1u, spareR = threadIdx.x < rRows ? threadIdx.x : rRows - 1u;
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) {
        si[j] = es[j] - sRowBase; ri[j] = er[j];
        live[j] = es[j] != kNoRow && er[j] != kNoRow && si[j] < sRows && ri[j] < rRows;             // past nPairs: both kNoRow
        si[j] = live[j] ? si[j] : spareS; ri[j] = live[j] ? ri[j] : spareR;
    }
    if constexpr (kBest) {
#pragma unroll
        for (uint32_t j = 0; j < kFilterLanePairs; ++j) best[j] = bestVal[si[j]];
    }
    const uint32_t *pvs = kValid ? t.sValid : nullptr, *pvr = kValid ? t.rValid : nullptr;
    uint64_t a[kFilterLanePairs], b[kFilterLanePairs];
    uint32_t vs[kFilterLanePairs], vr[kFilterLanePairs];
    switch (t.width) {
        case 1: where_load<uint8_t, kValid>(t.s, t.r, pvs, pvr, si, ri, a, b, vs, vr); break;
        case 2: where_load<uint16_t, kValid>(t.s, t.r, pvs, pvr, si, ri, a, b, vs, vr); break;
        case 4: where_load<uint32_t, kValid>(t.s, t.r, pvs, pvr, si, ri, a, b, vs, vr); break;
        default: where_load<uint64_t, kValid>(t.s, t.r, pvs, pvr, si, ri, a, b, vs, vr); break;
    }
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) {
        bool e = where_holds(t.type, t.width, t.op, a[j], b[j]);
        if constexpr (kValid) e = e && ((vs[j] >> (si[j] & 31u)) & (vr[j] >> (ri[j] & 31u)) & 1u);
        ok[j] = live[j] && e;
        key[j] = asof_key(t.type, t.width, t.op, b[j]);
    }
}

}  // namespace

// pass 1: bestVal[s] = the largest key among the eligible pairs of s. bestVal is 0 everywhere before it.
template <bool kValid>
__global__ void __launch_bounds__(kBlock)
k_asof_best(const uint32_t* __restrict__ mapS, const uint32_t* __restrict__ mapR, uint64_t nPairs, uint32_t sRowBase, uint32_t sRows,
            uint32_t rRows, AsofTerm term, unsigned long long* __restrict__ bestVal)
{
    uint32_t si[kFilterLanePairs], ri[kFilterLanePairs];
    bool live[kFilterLanePairs], ok[kFilterLanePairs];
    uint64_t key[kFilterLanePairs];
    unsigned long long unused[kFilterLanePairs];
    asof_pairs<kValid, false>(mapS, mapR, nPairs, sRowBase, sRows, rRows, term, nullptr, si, ri, live, ok, key, unused);
    const uint32_t lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) {
        // runs: neighbouring lanes hold neighbouring pairs of the list; the live pairs of one S row among them combine their
        // keys (k_pairs_agg's segmented scan; every lane of the wavefront is here) and the run's last lane issues the atomic.
        // A pair that is not eligible brings 0, which a maximum over unsigned words ignores -- as the plane does, which starts at 0.
        const uint32_t run = live[j] ? si[j] : kNoRow;
        const uint32_t before = __shfl_up(run, 1, kWave);
        const bool head = lane == 0 || before != run;
        const unsigned long long heads = __ballot(head);
        const uint32_t start = 63u - (uint32_t)__clzll(heads & (~0ull >> (63u - lane)));            // the head of this lane's run
        const bool tail = lane == kWave - 1 || ((heads >> (lane + 1)) & 1ull);
        unsigned long long x = ok[j] ? key[j] : 0ull;
#pragma unroll
        for (uint32_t off = 1; off < (uint32_t)kWave; off <<= 1) {
            const unsigned long long below = __shfl_up(x, off, kWave);
            if (lane >= start + off) x = x > below ? x : below;
        }
        if (live[j] && tail && x) __hip_atomic_fetch_max(&bestVal[si[j]], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// pass 2: bestRow[s] = the lowest R row among the eligible pairs of s whose key is bestVal[s]. bestRow is kNoRow everywhere
// before it, bestVal as pass 1 left it.
template <bool kValid>
__global__ void __launch_bounds__(kBlock)
k_asof_row(const uint32_t* __restrict__ mapS, const uint32_t* __restrict__ mapR, uint64_t nPairs, uint32_t sRowBase, uint32_t sRows,
           uint32_t rRows, AsofTerm term, const unsigned long long* __restrict__ bestVal, uint32_t* __restrict__ bestRow)
{
    uint32_t si[kFilterLanePairs], ri[kFilterLanePairs];
    bool live[kFilterLanePairs], ok[kFilterLanePairs];
    uint64_t key[kFilterLanePairs];
    unsigned long long best[kFilterLanePairs];
    asof_pairs<kValid, true>(mapS, mapR, nPairs, sRowBase, sRows, rRows, term, bestVal, si, ri, live, ok, key, best);
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j)
        if (ok[j] && key[j] == best[j]) __hip_atomic_fetch_min(&bestRow[si[j]], ri[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// pass 3: out, sMarks as k_pairs_where takes them (cursor[0]: kept pairs; cursor[1]: dropped pairs). The pair-filter frame
// (hj_pairs.h) around one load of the bestRow plane per pair; nCols is the launch's and unused.
__global__ void __launch_bounds__(kBlock)
k_asof_keep(const uint32_t* __restrict__ mapS, const uint32_t* __restrict__ mapR, uint64_t nPairs, uint32_t sRowBase, uint32_t sRows,
            uint32_t rRows, const uint32_t* __restrict__ bestRow, uint32_t nCols, PairsOutMarked out, RMarks sMarks)
{
    __shared__ uint32_t ldsS[kFilterBlockPairs], ldsR[kFilterBlockPairs], ldsTot[2 * kFilterWaves], ldsDrop[kFilterWaves];
    __shared__ unsigned long long ldsBase;
    PairStage<kBlock> st{ldsS, ldsR, ldsTot, &ldsBase, 0u, 0u, 0ull, 0ull, 0u};
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const uint64_t k0 = (uint64_t)blockIdx.x * kFilterBlockPairs + w * kFilterWavePairs + lane;     // the lane's first pair

    // the map entries of the lane's four pairs, all in flight before the first is looked at
    uint32_t es[kFilterLanePairs], er[kFilterLanePairs];
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) {
        const uint64_t k = k0 + j * kFilterStepPairs;
        es[j] = er[j] = kNoRow;
        if (k < nPairs) { es[j] = __builtin_nontemporal_load(mapS + k); er[j] = __builtin_nontemporal_load(mapR + k); }
    }

    uint32_t si[kFilterLanePairs], ri[kFilterLanePairs];
    bool live[kFilterLanePairs];
    uint32_t nDrop = 0;                                               // of this wavefront (ballots: the same in every lane)
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) {
        const bool in = k0 + j * kFilterStepPairs < nPairs;
        si[j] = es[j] - sRowBase; ri[j] = er[j];
        live[j] = in && es[j] != kNoRow && er[j] != kNoRow && si[j] < sRows && ri[j] < rRows;       // the raw entries: whatever the base
        nDrop += (uint32_t)__popcll(__ballot(in && !live[j]));
    }
    if (lane == 0) ldsDrop[w] = nDrop;                                // read behind stage_reserve's barrier

    // sRows or rRows 0: every pair is dropped, and there is no row to read
    if (sRows && rRows) {
        // a dropped pair reads, and ignores, the plane's entry of one of the first rows
        const uint32_t spareS = threadIdx.x < sRows ? threadIdx.x : sRows - 1u;
        uint32_t best[kFilterLanePairs];
#pragma unroll
        for (uint32_t j = 0; j < kFilterLanePairs; ++j) best[j] = bestRow[live[j] ? si[j] : spareS];
#pragma unroll
        for (uint32_t j = 0; j < kFilterLanePairs; ++j) live[j] = live[j] && best[j] == ri[j];
    }

    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) m += (uint32_t)live[j];
    bool any;
    uint32_t pos = stage_reserve<kInner>(st, out, m, false, any);     // never flushes: the stage was empty and takes every pair
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j)
        if (live[j]) { st.s[pos] = es[j]; st.r[pos] = er[j]; ++pos; }
    if (threadIdx.x == 0) {
        uint32_t d = 0;
#pragma unroll
        for (uint32_t i = 0; i < kFilterWaves; ++i) d += ldsDrop[i];
        if (d) atomicAdd(out.cursor + 1, (unsigned long long)d);
    }
    const uint32_t kept = st.fill;                                    // the same in every thread
    if (kept == 0) return;                                            // workgroup-uniform
    stage_flush<kInner>(st, out);                                     // the claim, both planes, R's marks
    mark_plane<kBlock>(st.s, kept, sMarks);                           // the stage is still as it was flushed
}

hipError_t launch_pairs_asof(const PairList& in, const AsofTerm& term, unsigned long long* bestVal, uint32_t* bestRow, const PairSink& to,
                             hipStream_t s)
{
    hipError_t e;
    if (in.sRows) {
        if ((e = hipMemsetAsync(bestVal, 0, (size_t)in.sRows * sizeof(unsigned long long), s)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(bestRow, 0xFF, (size_t)in.sRows * sizeof(uint32_t), s)) != hipSuccess) return e;
    }
    if (in.n == 0) return hipSuccess;
    if (in.sRows && in.rRows) {       // else every pair is dropped: pass 3 counts them
        const dim3 grid((uint32_t)((in.n + kFilterBlockPairs - 1) / kFilterBlockPairs));
        const bool valid = term.sValid || term.rValid;
        hipLaunchKernelGGL(valid ? k_asof_best<true> : k_asof_best<false>, grid, dim3(kBlock), 0, s, in.mapS, in.mapR, in.n, in.sRowBase, in.sRows,
                           in.rRows, term, bestVal);
        hipLaunchKernelGGL(valid ? k_asof_row<true> : k_asof_row<false>, grid, dim3(kBlock), 0, s, in.mapS, in.mapR, in.n, in.sRowBase, in.sRows,
                           in.rRows, term, static_cast<const unsigned long long*>(bestVal), bestRow);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return launch_pair_filter(k_asof_keep, in, static_cast<const uint32_t*>(bestRow), 0u, to, s);
}

void pairs_asof_host(const PairList& in, const AsofTerm& t, uint64_t* bestVal, uint32_t* bestRow, const PairSink& to, uint64_t* info)
{
    for (uint32_t i = 0; i < in.sRows; ++i) { bestVal[i] = 0; bestRow[i] = kNoRow; }
    for (uint64_t k = 0; k < in.n; ++k) {
        if (dropped_pair(in.mapS[k], in.mapR[k], in.sRowBase, in.sRows, in.rRows)) continue;
        const uint32_t si = in.mapS[k] - in.sRowBase, ri = in.mapR[k];
        const bool okS = !t.sValid || valid_bit(t.sValid, si), okR = !t.rValid || valid_bit(t.rValid, ri);
        const uint64_t b = col_elem(t.r, t.width, ri);
        if (!okS || !okR || !where_holds(t.type, t.width, t.op, col_elem(t.s, t.width, si), b)) continue;
        const uint64_t key = asof_key(t.type, t.width, t.op, b);
        if (bestRow[si] == kNoRow || key > bestVal[si] || (key == bestVal[si] && ri < bestRow[si])) { bestVal[si] = key; bestRow[si] = ri; }
    }
    pairs_keep_host(in, to, info, [&](uint32_t si, uint32_t ri) { return bestRow[si] == ri; });
}

}  // namespace hj
