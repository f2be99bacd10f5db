// hj_keys.hip -- joins on real key columns for gfx950 (MI355X): hj_key_hash_dev / hj_key_hash2_dev and
// hj_pairs_verify_dev / hj_pairs_verify2_dev. The hash and the element compare are in hj_keys_impl.h: hj_groups.hip
// (hj_key_groups_dev) groups the rows of ONE table with the same ones.
//
// The joins of this library match on one 32-bit word. A key of 64 bits, of several columns, of 16 bytes, with NULLs or of
// variable length is joined as hash -> candidate join -> verify: k_key_hash2 turns the key columns of a row into a 32-bit
// join word (the header's MurmurHash3_x86_32, include/htm_hashjoin.h), the resident radix join produces the pairs that
// agree on that word, and k_pairs_verify2 compares the real keys of every candidate, keeps the equal ones and marks
// their S and R rows. There is ONE such pair of kernels, on key columns in the Arrow layout (hj_key_col2: a validity plane
// and 32-bit offsets per side, both optional). A plain column (hj_key_col) is that descriptor with null planes, null
// offsets and flags 0, and the launchers give it the narrow instances (kVar = false, kForm = 0), which do per row
// nothing that a kernel written for plain columns alone would not do (profiles/join_on_columns.md, (a) and (e)).
//
// k_key_hash2. Shape: one workgroup of kBlock lanes per kHashBlockRows = 1024 consecutive rows; a wavefront owns 256 of
// them and a lane kHashLaneRows = 4, one per step of 64, so a wave-instruction reads 64 * width contiguous bytes of a
// column and stores 512 contiguous bytes of tuples. The hash runs over the columns in order, so the lane carries four
// running hashes through them column by column: the four loads of a column are issued straight, then its words are
// mixed. The width of a column is picked by a switch on a kernel argument (uniform: a scalar branch) rather than by a
// template parameter per column -- 5^4 width lists are too many to instantiate. The price, seen in the ISA: the wait
// counters cannot tell the arms of a switch apart, so a column's loads wait for those of the column before; inside an
// arm the four loads are in flight together, and the other wavefronts of the CU cover the rest (no LDS, 8 per SIMD).
// A row behind the end reads the last row instead of branching around its loads. Loads are nontemporal: every column is
// read once. key_hash2_rows is ONE __host__ __device__ body: hj_key_hash_host and hj_key_hash2_host run it in a host
// loop, a row at a time. What a validity plane and offsets add is described where the kernel is defined below.
// What it does NOT do: no atomics, no LDS.
//
// k_pairs_verify2. Shape and flow: the pair-filter frame (hj_pairs.h), which k_pairs_where (hj_where.hip) repeats -- 1024
// candidates per workgroup, four per lane, dropped candidates counted and never dereferenced, one LDS stage flushed once,
// both sides marked from it. What is this kernel's own is the loop in the middle: the keys are compared column by column,
// the S and the R element of the column for all four candidates of the lane -- eight element-granular random loads, with
// their validity words beside them -- in flight before the first compare; a candidate that an earlier column has rejected
// is read again and a dropped one reads a spare row, instead of branching around their loads (a branch would make every
// load wait for the one before it). (All columns at once would be 4 x 2 x 4 sixteen-byte cells per lane; by column it is
// 32 registers.)
// What it does NOT do: the candidates are taken in the order the radix join left them, which is by partition; the S side
// is near-sequential only if that order happens to be, and the R side is a random element read per column.

#include "hj_keys_impl.h"

namespace hj {

namespace {

// One key column of fixed width of the lane's candidates: both elements of every candidate, and beside them the validity
// words of both sides (null plane: all valid), everything before the first compare. The loads are unconditional -- a load
// under a per-lane condition is a branch around it, and the wait counters in front of the next one would then wait for
// it. So a candidate that an earlier column has rejected is read again, and a dropped one (its caller's doing) reads a row
// that exists. Either element NULL: equal iff both are and nullsEqual.
template <int W>
__device__ __forceinline__ void verify_col2(const void* sCol, const void* rCol, const uint32_t* sValid, const uint32_t* rValid, bool nullsEqual,
                                            const uint32_t (&si)[kFilterLanePairs], const uint32_t (&ri)[kFilterLanePairs],
                                            bool (&live)[kFilterLanePairs])
{
    using E = KeyElem<W>;
    E a[kFilterLanePairs], b[kFilterLanePairs];
    uint32_t vs[kFilterLanePairs], vr[kFilterLanePairs];
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) { vs[j] = sValid ? sValid[si[j] >> 5] : ~0u; vr[j] = rValid ? rValid[ri[j] >> 5] : ~0u; }
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) { a[j] = static_cast<const E*>(sCol)[si[j]]; b[j] = static_cast<const E*>(rCol)[ri[j]]; }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) {
        const bool okS = (vs[j] >> (si[j] & 31u)) & 1u, okR = (vr[j] >> (ri[j] & 31u)) & 1u;
        live[j] = live[j] && ((okS && okR) ? same_bytes<E>(a[j], b[j]) : (!okS && !okR && nullsEqual));
    }
}

// A variable-length column of the lane's candidates. The lengths go first: four offsets and two validity words per
// candidate, all in flight together; NULLs and a length mismatch are settled from them without touching a byte. Then the
// words, while the candidate is live and words remain: per step one aligned word per side and live candidate, all loaded
// before the first compare. A candidate that is dropped, rejected or NULL has no words and reads no byte.
__device__ __forceinline__ void verify_varlen(const void* sBytes, const void* rBytes, const uint32_t* sOff, const uint32_t* rOff,
                                              const uint32_t* sValid, const uint32_t* rValid, bool nullsEqual,
                                              const uint32_t (&si)[kFilterLanePairs], const uint32_t (&ri)[kFilterLanePairs],
                                              bool (&live)[kFilterLanePairs])
{
    uint32_t so0[kFilterLanePairs], so1[kFilterLanePairs], ro0[kFilterLanePairs], ro1[kFilterLanePairs];
    uint32_t vs[kFilterLanePairs], vr[kFilterLanePairs], len[kFilterLanePairs], nW[kFilterLanePairs];
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) {
        so0[j] = sOff[si[j]]; so1[j] = sOff[si[j] + 1u]; ro0[j] = rOff[ri[j]]; ro1[j] = rOff[ri[j] + 1u];
        vs[j] = sValid ? sValid[si[j] >> 5] : ~0u; vr[j] = rValid ? rValid[ri[j] >> 5] : ~0u;
    }
    __builtin_amdgcn_sched_barrier(0);
    VarWords a[kFilterLanePairs], b[kFilterLanePairs];
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) {
        const bool okS = (vs[j] >> (si[j] & 31u)) & 1u, okR = (vr[j] >> (ri[j] & 31u)) & 1u, both = okS && okR;
        const uint32_t ls = so1[j] - so0[j], lr = ro1[j] - ro0[j];
        live[j] = live[j] && (both ? ls == lr : (!okS && !okR && nullsEqual));
        len[j] = live[j] && both ? ls : 0u;
        nW[j] = var_words_of(len[j]);
    }
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) { a[j] = var_begin<false>(sBytes, so0[j], len[j]); b[j] = var_begin<false>(rBytes, ro0[j], len[j]); }
    for (uint32_t w = 0;; ++w) {
        bool go[kFilterLanePairs], any = false;
#pragma unroll
        for (uint32_t j = 0; j < kFilterLanePairs; ++j) { go[j] = live[j] && w < nW[j]; any = any || go[j]; }
        if (!any) break;
        uint32_t na[kFilterLanePairs], nb[kFilterLanePairs];
#pragma unroll
        for (uint32_t j = 0; j < kFilterLanePairs; ++j) { na[j] = var_fetch<false>(a[j], w, go[j]); nb[j] = var_fetch<false>(b[j], w, go[j]); }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (uint32_t j = 0; j < kFilterLanePairs; ++j)
            if (go[j]) live[j] = var_word(a[j], na[j], len[j], w) == var_word(b[j], nb[j], len[j], w);
    }
}

}  // namespace

// What Arrow columns add to the hash per column: with a validity plane, one load of the wavefront's eight words and a
// shuffle; with offsets, the lane's four offset pairs and a word loop over aligned words to the lane's own longest
// element (key_mix_varlen). No LDS allocation, no atomics.
// What it does NOT do: the word loop waits for a step's loads before it mixes them (the other wavefronts cover that),
// and a wavefront runs as long as its longest element. Two instances: the launch picks kVar = false when no column has
// offsets, so that fixed-width columns do not pay for the word loop's registers.
template <bool kVar>
__global__ void __launch_bounds__(kBlock)
k_key_hash2(KeyCols2 cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint64_t* __restrict__ out)
{
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * kHashBlockRows + w * (kHashLaneRows * kWave) + lane;     // the lane's first row
    uint64_t row[kHashLaneRows], at[kHashLaneRows];
    uint32_t word[kHashLaneRows];
#pragma unroll
    for (uint32_t j = 0; j < kHashLaneRows; ++j) {
        at[j] = i0 + j * kWave;
        row[j] = at[j] < nRows ? at[j] : nRows - 1;                   // a row behind the end reads the last one and stores nothing
    }
    key_hash2_rows<(int)kHashLaneRows, kVar>(cols, nCols, row, at, nRows, mask, word);
#pragma unroll
    for (uint32_t j = 0; j < kHashLaneRows; ++j)
        if (at[j] < nRows) out[at[j]] = (uint64_t)word[j];
}

// The pair-filter frame (hj_pairs.h: its flow, written out here and in k_pairs_where) around the key columns, which go
// through verify_col2 / verify_varlen. out: the planes, their capacity and the cursor (cursor[0]: kept pairs; cursor[1]:
// dropped candidates); out.marks: R's plane. sMarks: S's plane, its base the sRowBase of the maps. A plane that is not
// wanted has rows = 0 and marks nothing. sValid and sOff are indexed by the S row with the base off, like the column. Three instances, so that a call pays in registers
// only for what its columns have; the launch looks and picks kForm: 0 = fixed columns without a validity plane (every
// hj_key_col call), 1 = fixed columns, some with a plane, 2 = some variable-length column (the word loop and its cursors).
template <int kForm>
__global__ void __launch_bounds__(kBlock)
k_pairs_verify2(const uint32_t* __restrict__ mapS, const uint32_t* __restrict__ mapR, uint64_t nPairs, uint32_t sRowBase, uint32_t sRows,
                uint32_t rRows, KeyCols2SR cols, uint32_t nCols, PairsOutMarked out, RMarks sMarks)
{
    __shared__ uint32_t ldsS[kFilterBlockPairs], ldsR[kFilterBlockPairs], ldsTot[2 * kFilterWaves], ldsDrop[kFilterWaves];
    __shared__ unsigned long long ldsBase;
    PairStage<kBlock> st{ldsS, ldsR, ldsTot, &ldsBase, 0u, 0u, 0ull, 0ull, 0u};
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const uint64_t k0 = (uint64_t)blockIdx.x * kFilterBlockPairs + w * kFilterWavePairs + lane;   // the lane's first candidate

    // the map entries of the lane's four candidates, all in flight before the first is looked at
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
        live[j] = in && es[j] != kNoRow && er[j] != kNoRow && si[j] < sRows && ri[j] < rRows;     // the raw entries: whatever the base
        nDrop += (uint32_t)__popcll(__ballot(in && !live[j]));
    }
    if (lane == 0) ldsDrop[w] = nDrop;                                // read behind stage_reserve's barrier

    // sRows or rRows 0: every candidate is dropped, and there is no row to read
    if (sRows && rRows) {
        // a dropped candidate reads, and ignores, one of the first rows (its offsets and validity too: they exist)
        const uint32_t spareS = threadIdx.x < sRows ? threadIdx.x : sRows - 1u, spareR = threadIdx.x < rRows ? threadIdx.x : rRows - 1u;
#pragma unroll
        for (uint32_t j = 0; j < kFilterLanePairs; ++j) { si[j] = live[j] ? si[j] : spareS; ri[j] = live[j] ? ri[j] : spareR; }
#pragma unroll
        for (uint32_t c = 0; c < kKeyMaxCols; ++c) {
            if (c >= nCols) continue;                                 // kernel arguments: uniform
            const bool ne = (cols.flags[c] & kKeyNullsEqual) != 0u;
            const uint32_t *vs = kForm ? cols.sValid[c] : nullptr, *vr = kForm ? cols.rValid[c] : nullptr;
            switch (cols.width[c]) {
                case 0: if constexpr (kForm == 2) verify_varlen(cols.s[c], cols.r[c], cols.sOff[c], cols.rOff[c], vs, vr, ne, si, ri, live); break;
                case 1: verify_col2<1>(cols.s[c], cols.r[c], vs, vr, ne, si, ri, live); break;
                case 2: verify_col2<2>(cols.s[c], cols.r[c], vs, vr, ne, si, ri, live); break;
                case 4: verify_col2<4>(cols.s[c], cols.r[c], vs, vr, ne, si, ri, live); break;
                case 8: verify_col2<8>(cols.s[c], cols.r[c], vs, vr, ne, si, ri, live); break;
                default: verify_col2<16>(cols.s[c], cols.r[c], vs, vr, ne, si, ri, live); break;
            }
        }
    }

    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) m += (uint32_t)live[j];
    bool any;
    uint32_t pos = stage_reserve<kInner>(st, out, m, false, any);     // never flushes: the stage was empty and takes every candidate
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

hipError_t launch_key_hash2(const KeyCols2& cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint64_t* out, hipStream_t s)
{
    if (nRows == 0) return hipSuccess;
    const dim3 grid((uint32_t)((nRows + kHashBlockRows - 1) / kHashBlockRows));               // nRows <= 2^32 - 1: <= 2^22 workgroups
    bool var = false;
    for (uint32_t c = 0; c < nCols; ++c) var = var || cols.off[c];
    if (var) hipLaunchKernelGGL(k_key_hash2<true>, grid, dim3(kBlock), 0, s, cols, nCols, nRows, mask, out);
    else hipLaunchKernelGGL(k_key_hash2<false>, grid, dim3(kBlock), 0, s, cols, nCols, nRows, mask, out);
    return hipGetLastError();
}

void key_hash2_host(const KeyCols2& cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint64_t* out)
{
    for (uint64_t i = 0; i < nRows; ++i) {
        const uint64_t row[1] = {i};
        uint32_t word[1];
        key_hash2_rows<1, true>(cols, nCols, row, row, nRows, mask, word);
        out[i] = (uint64_t)word[0];
    }
}

hipError_t launch_pairs_verify2(const PairList& in, const KeyCols2SR& cols, uint32_t nCols, const PairSink& to, hipStream_t s)
{
    int form = 0;
    for (uint32_t c = 0; c < nCols; ++c) form = cols.width[c] == 0u ? 2 : form ? form : (cols.sValid[c] || cols.rValid[c]) ? 1 : 0;
    const auto kernel = form == 2 ? k_pairs_verify2<2> : form == 1 ? k_pairs_verify2<1> : k_pairs_verify2<0>;
    return launch_pair_filter(kernel, in, cols, nCols, to, s);
}

}  // namespace hj
