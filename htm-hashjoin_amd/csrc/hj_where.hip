// hj_where.hip -- join conditions beyond equality for gfx950 (MI355X): hj_pairs_where_dev and hj_pairs_where_host.
//
// ON S.k = R.k AND S.ts >= R.valid_from AND S.ts < R.valid_to is an equi-join plus a condition on the matched pair. The
// joins of this library give the pairs that agree on the key; k_pairs_where takes such pairs, keeps those for which every
// term  s[si] OP r[ri]  holds and marks their S and R rows in two caller-owned planes, so that all eight kinds follow from
// the kept pairs and two sweeps -- the flow of hj_pairs_verify_dev (hj_keys.hip) with typed comparisons in place of bytes.
//
// k_pairs_where. Shape and flow: the pair-filter frame (hj_pairs.h) as k_pairs_verify2 (hj_keys.hip) has it, because
// profiles/join_on.md measured that shape -- 1024 pairs per workgroup, four per lane, dropped pairs counted and never
// dereferenced, one LDS stage flushed once, both sides marked from it; the flow is written out in both kernels. What is this
// kernel's own is the loop in the middle. The terms are evaluated one after the other: the S and the R element of the
// term for all four pairs of the lane -- eight element-granular random loads, and with validity planes the eight words
// beside them -- are in flight before the first compare; a pair that an earlier term has rejected is read again and a
// dropped one reads a spare row, instead of branching around their loads (a branch would make every load wait for the
// one before it).
// Width, type and op of a term are kernel arguments, so scalar branches select among them; the 6 x 10 x 4 combinations
// are not instantiated. The switch on the width holds the loads alone, every element zero-extended to 64 bits. The compare
// is where_holds (hj_columns.h), ONE __host__ __device__ body that hj_pairs_where_host runs in a host loop: the two raw words are widened
// to one of two domains -- a 64-bit integer, sign-extended from the width and its sign bit flipped for HJ_VAL_INT so that
// one unsigned compare serves both, or a double, to which a float widens exactly --, `lt`, `eq` and `unordered` are derived
// once, and the op picks from those three bits.
// Two instances: the launch picks kValid = false when no term has a validity plane, so that plain columns do not carry the
// eight validity words of a term.
// What it does NOT do: the pairs are taken in the order the join left them, so both elements of a term are random
// element-granular reads; a term's loads wait for those of the term before (the wait counters cannot tell the arms of the
// width switch apart); no constants, no arithmetic, no OR; the terms are not fused into the verify kernel.

#include "hj_columns.h"

namespace hj {

// out, sMarks: as k_pairs_verify2 takes them (cursor[0]: kept pairs; cursor[1]: dropped pairs). The pair-filter frame
// (hj_pairs.h) around the terms
template <bool kValid>
__global__ void __launch_bounds__(kBlock)
k_pairs_where(const uint32_t* __restrict__ mapS, const uint32_t* __restrict__ mapR, uint64_t nPairs, uint32_t sRowBase, uint32_t sRows,
              uint32_t rRows, WhereTerms terms, uint32_t nTerms, PairsOutMarked out, RMarks sMarks)
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
        // a dropped pair reads, and ignores, one of the first rows (its validity word too: it exists)
        const uint32_t spareS = threadIdx.x < sRows ? threadIdx.x : sRows - 1u, spareR = threadIdx.x < rRows ? threadIdx.x : rRows - 1u;
#pragma unroll
        for (uint32_t j = 0; j < kFilterLanePairs; ++j) { si[j] = live[j] ? si[j] : spareS; ri[j] = live[j] ? ri[j] : spareR; }
#pragma unroll
        for (uint32_t t = 0; t < kWhereMaxTerms; ++t) {
            if (t >= nTerms) continue;                                // kernel arguments: uniform
            const uint32_t *pvs = kValid ? terms.sValid[t] : nullptr, *pvr = kValid ? terms.rValid[t] : nullptr;
            uint64_t a[kFilterLanePairs], b[kFilterLanePairs];
            uint32_t vs[kFilterLanePairs], vr[kFilterLanePairs];
            switch (terms.width[t]) {
                case 1: where_load<uint8_t, kValid>(terms.s[t], terms.r[t], pvs, pvr, si, ri, a, b, vs, vr); break;
                case 2: where_load<uint16_t, kValid>(terms.s[t], terms.r[t], pvs, pvr, si, ri, a, b, vs, vr); break;
                case 4: where_load<uint32_t, kValid>(terms.s[t], terms.r[t], pvs, pvr, si, ri, a, b, vs, vr); break;
                default: where_load<uint64_t, kValid>(terms.s[t], terms.r[t], pvs, pvr, si, ri, a, b, vs, vr); break;
            }
#pragma unroll
            for (uint32_t j = 0; j < kFilterLanePairs; ++j) {
                bool ok = where_holds(terms.type[t], terms.width[t], terms.op[t], a[j], b[j]);
                if constexpr (kValid) ok = ok && ((vs[j] >> (si[j] & 31u)) & (vr[j] >> (ri[j] & 31u)) & 1u);
                live[j] = live[j] && ok;
            }
        }
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

hipError_t launch_pairs_where(const PairList& in, const WhereTerms& terms, uint32_t nTerms, const PairSink& to, hipStream_t s)
{
    bool valid = false;
    for (uint32_t t = 0; t < nTerms; ++t) valid = valid || terms.sValid[t] || terms.rValid[t];
    const auto kernel = valid ? k_pairs_where<true> : k_pairs_where<false>;
    return launch_pair_filter(kernel, in, terms, nTerms, to, s);
}

void pairs_where_host(const PairList& in, const WhereTerms& terms, uint32_t nTerms, const PairSink& to, uint64_t* info)
{
    pairs_keep_host(in, to, info, [&](uint32_t si, uint32_t ri) {
        bool live = true;
        for (uint32_t t = 0; live && t < nTerms; ++t) {
            const bool okS = !terms.sValid[t] || valid_bit(terms.sValid[t], si);
            const bool okR = !terms.rValid[t] || valid_bit(terms.rValid[t], ri);
            live = okS && okR && where_holds(terms.type[t], terms.width[t], terms.op[t], col_elem(terms.s[t], terms.width[t], si),
                                             col_elem(terms.r[t], terms.width[t], ri));
        }
        return live;
    });
}

}  // namespace hj
