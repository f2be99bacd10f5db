// hj_pairs.hip -- the materialising probe for gfx950 (MI355X): HOT LOOP 2 with its result kept.
//
//   k_probe_pairs      the walk of k_probe (NoCCHashBuild.hpp:70-79) over the 8-byte slot table, one (S row, R row) pair
//                      per match it counts; the R row is the index word the slot carries (index << 32 | key)
//   k_htm_probe_pairs  the walk of k_htm_probe (HTMHashBuild.hpp:291-305): bucket, then the whole chain
//
// Output: two 4-byte planes (gather maps), filled from 0 without holes in no particular order. How a workgroup gets its
// stretch of them is the whole design ("Materialising probe"): one returning atomic on one word serves about
// 88 requests per microsecond chip-wide, so output space is claimed per STAGE, not per wavefront iteration. Every
// workgroup collects its pairs in an LDS stage of kStagePairs pairs; a round (1024 S tuples, or one bucket of every
// live chain) first agrees on its pair count -- wavefront scan, four totals exchanged through LDS, one barrier -- and
// when the stage cannot take the round, the workgroup claims [base, base + fill) with ONE 64-bit atomicAdd and the stage
// leaves LDS as 16-byte nontemporal stores over the aligned body of the run. That is the spill rule as well: a Zipf-hot
// key whose chain has thousands of buckets just flushes more often; no lane ever buffers more than one bucket.
// Pairs at or beyond `capacity` are counted (the cursor runs on) and not written: the check is per element.
//
//
// Join kinds (hj_probe_join_dev): the kind K is a template parameter of both kernels. A kind is a different ROW count per
// S element and a different thing written, not another pass: INNER one row per match (the code as it was), LEFT the same
// plus one (S row, kNoRow) row for an element without a match, SEMI the S row once if it has a match, ANTI the S row if
// it has none. SEMI and ANTI stage and write the S plane only. Lanes without an element (load_vecs pads, the head/tail
// round leaves 255 threads idle) carry valid = false and never produce an unmatched row. Counters::matches grows by the
// INNER matches whatever the kind.
//
// R-side match marks (HJ_FLAG_TRACK_R_MATCHES): `bool MARK` next to K on both kernels, instantiated for INNER and LEFT. A MARK
// instantiation takes PairsOutMarked where the others take PairsOut, and stage_flush also sets the bit of every staged R
// row (mark_plane, hj_pairs.h).
//
// The stage itself (PairStage, stage_reserve, stage_flush, stage_finish), the kinds' constants and the dispatch over
// (kind, marks) are in hj_pairs.h: k_prj_join_pairs (hj_prj_pairs.hip) stages its rows through the same code.
//
// All integer work, bound by HBM and the table gather; no MFMA.

#include "hj_pairs.h"
#include "hj_table.h"

namespace hj {

namespace {

constexpr uint32_t kWaves = kBlock / kWave;
// A round must fit an empty stage (asserted where the rounds are shaped): 1024 S tuples x 4 slots at probeLength 4,
// 512 x kMaxProbeLen at any other length, 1024 buckets x 3 tuples for htm
constexpr uint32_t kMaxProbeLen = 8;
using Stage = PairStage<kBlock>;

// ---------------------------------------------------------------------------
// the S read of both kernels
// ---------------------------------------------------------------------------
// As probe_body of hj_kernels.hip: 16-byte nontemporal loads over the aligned body (two tuples each), the element before
// and after it by one thread of workgroup 0. A round takes V such loads per lane (lane t of the workgroup: vectors
// v0 + t, v0 + kBlock + t, ...), and the loads of the NEXT round are issued before this round's table lines are waited
// for: a workgroup meets at a barrier every round, so what is not in flight before the barrier is latency paid per round.
constexpr uint64_t kNoElement = ~0ull;          // payload bits set: matches nothing anywhere (a lane without an element)

struct SBody { const u4* S4; uint64_t head, nv, tail; };

__device__ __forceinline__ SBody s_body(const uint64_t* S, uint64_t n)
{
    SBody b;
    b.head = ((16 - (reinterpret_cast<uintptr_t>(S) & 15)) & 15) / sizeof(uint64_t);
    if (b.head > n) b.head = n;
    b.S4 = reinterpret_cast<const u4*>(S + b.head);
    b.nv = (n - b.head) >> 1;
    b.tail = b.head + 2 * b.nv;
    return b;
}

template <int V>
__device__ __forceinline__ void load_vecs(const SBody& b, uint64_t v0, u4 (&t)[V])
{
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const uint64_t v = v0 + (uint64_t)k * kBlock + threadIdx.x;
        t[k].x = 0u; t[k].y = ~0u; t[k].z = 0u; t[k].w = ~0u;            // two times "no element"
        if (v < b.nv) t[k] = __builtin_nontemporal_load(b.S4 + v);
    }
}

// The S rounds of a workgroup: V vectors (2 V elements) per lane and round by grid stride, then the element before and
// after the aligned body in one round of two elements for thread 0 of workgroup 0. round(sk, row, valid) takes a round's
// elements (E = 2 V or 2, the arrays' length); key(k) sees the key word of every element that exists (the foreign-tuple
// count of k_probe_pairs). Every thread of the workgroup runs the same number of rounds (they meet at barriers).
template <int V, class Key, class Round>
__device__ __forceinline__ void for_s_rounds(const uint64_t* __restrict__ S, uint64_t n, uint64_t sIdxBase, Key&& key, Round&& round)
{
    const SBody b = s_body(S, n);
    const uint64_t stride = (uint64_t)gridDim.x * kBlock * V;
    uint64_t v0 = (uint64_t)blockIdx.x * kBlock * V;
    u4 cur[V];
    load_vecs<V>(b, v0, cur);
    for (; v0 < b.nv; v0 += stride) {
        u4 nxt[V];
        load_vecs<V>(b, v0 + stride, nxt);
        uint64_t sk[2 * V], row[2 * V];
        bool valid[2 * V];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const uint64_t v = v0 + (uint64_t)k * kBlock + threadIdx.x;
            sk[2 * k] = ((uint64_t)cur[k].y << 32) | cur[k].x; sk[2 * k + 1] = ((uint64_t)cur[k].w << 32) | cur[k].z;
            row[2 * k] = sIdxBase + b.head + 2 * v; row[2 * k + 1] = row[2 * k] + 1;
            valid[2 * k] = valid[2 * k + 1] = v < b.nv;
            if (v < b.nv) { key(cur[k].x); key(cur[k].z); }
        }
        round(sk, row, valid);
#pragma unroll
        for (int k = 0; k < V; ++k) cur[k] = nxt[k];
    }
    if (blockIdx.x == 0 && (b.head || b.tail < n)) {
        uint64_t sk[2] = {kNoElement, kNoElement};
        const uint64_t row[2] = {sIdxBase, sIdxBase + b.tail};
        const bool valid[2] = {threadIdx.x == 0 && b.head != 0, threadIdx.x == 0 && b.tail < n};     // 255 threads bring nothing
        if (threadIdx.x == 0) {
            if (b.head) { sk[0] = S[0]; key((uint32_t)sk[0]); }
            if (b.tail < n) { sk[1] = S[b.tail]; key((uint32_t)sk[1]); }
        }
        round(sk, row, valid);
    }
}

// ---------------------------------------------------------------------------
// open addressing
// ---------------------------------------------------------------------------
// What the walk of one S element matched: bit j = slot home + j holds the key and no slot before it is empty;
// first = the R row of the lowest such slot (the only one on unique keys; further ones are read again when written)
struct Hit { uint32_t mask, first; const uint64_t* p; };

// probe_one of hj_kernels.hip, remembering where it counted. sk with payload bits set matches nothing.
// FOUR (probeLength 4): the window is loaded unconditionally (slack slots past the table end; an element that cannot
// match reads the window at `dummy`), so that the windows of all of a lane's elements are in flight together.
template <bool FOUR>
__device__ __forceinline__ Hit walk(uint64_t sk, const uint64_t* __restrict__ table, uint64_t mask, uint32_t hshift,
                                    uint32_t probeLen, uint64_t validLo, uint64_t validHiEx, uint64_t dummy)
{
    const uint32_t key = (uint32_t)sk;
    const uint64_t home = home_slot(key, hshift, mask);
    const bool ok = (sk >> 32) == 0 && home >= validLo && home < validHiEx;
    Hit h;
    h.mask = 0; h.first = 0;
    h.p = table + (ok ? home : dummy);
    if constexpr (FOUR) {
        const uint64_t a = h.p[0], b = h.p[1], c = h.p[2], d = h.p[3];
        const bool ea = a != kEmpty, eb = ea && b != kEmpty, ec = eb && c != kEmpty, ed = ec && d != kEmpty;
        const uint32_t m = (uint32_t)(ea && (uint32_t)a == key) | ((uint32_t)(eb && (uint32_t)b == key) << 1) |
                           ((uint32_t)(ec && (uint32_t)c == key) << 2) | ((uint32_t)(ed && (uint32_t)d == key) << 3);
        h.mask = ok ? m : 0u;
        const uint64_t f = (m & 1u) ? a : (m & 2u) ? b : (m & 4u) ? c : d;
        h.first = (uint32_t)(f >> 32);
    } else if (ok) {
        for (uint32_t j = 0; j < probeLen; ++j) {
            const uint64_t v = h.p[j];
            if (v == kEmpty) break;
            if ((uint32_t)v == key) {
                if (h.mask == 0) h.first = (uint32_t)(v >> 32);
                h.mask |= 1u << j;
            }
        }
    }
    return h;
}

// valid: the lane holds an element (only the kinds that write unmatched rows ask)
template <int K>
__device__ __forceinline__ void emit(Stage& st, uint32_t& pos, uint32_t sRow, const Hit& h, bool valid)
{
    if constexpr (K == kSemi) { if (h.mask != 0) { st.s[pos] = sRow; ++pos; } return; }
    if constexpr (K == kAnti) { if (valid && h.mask == 0) { st.s[pos] = sRow; ++pos; } return; }
    if constexpr (K == kLeft) if (valid && h.mask == 0) { st.s[pos] = sRow; st.r[pos] = kNoRow; ++pos; }
    if (h.mask == 0) return;
    st.s[pos] = sRow; st.r[pos] = h.first; ++pos;
    for (uint32_t rest = h.mask & (h.mask - 1u); rest; rest &= rest - 1u) {      // duplicate keys in R
        const uint32_t j = (uint32_t)__builtin_ctz(rest);
        st.s[pos] = sRow; st.r[pos] = (uint32_t)(h.p[j] >> 32); ++pos;
    }
}

struct OaTable { const uint64_t* table; uint64_t mask; uint32_t hshift, probeLen; uint64_t validLo, validHiEx, dummy; };

// E elements per lane: walk them all, agree on the round's pair count, write the pairs into the stage
// Rows per element: INNER popc(mask); LEFT max(popc(mask), 1), SEMI mask != 0, ANTI mask == 0 -- the latter three for a
// valid lane only (a lane without an element has mask 0 and is no unmatched row)
template <int K, bool FOUR, int E, class Out>
__device__ __forceinline__ void oa_round(Stage& st, const Out& out, const OaTable& T, const uint64_t (&sk)[E], const uint64_t (&row)[E],
                                         const bool (&valid)[E])
{
    Hit h[E];
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        h[e] = walk<FOUR>(sk[e], T.table, T.mask, T.hshift, T.probeLen, T.validLo, T.validHiEx, T.dummy);
        const uint32_t hits = (uint32_t)__popc(h[e].mask);
        if constexpr (K == kInner) {
            m += hits;
        } else {
            const uint32_t none = (uint32_t)(valid[e] && h[e].mask == 0);
            st.inner += hits;
            if constexpr (K == kLeft) { m += hits + none; st.unmatched += none; }
            if constexpr (K == kSemi) m += (uint32_t)(h[e].mask != 0);
            if constexpr (K == kAnti) m += none;
        }
    }
    bool any;
    uint32_t pos = stage_reserve<K>(st, out, m, false, any);
#pragma unroll
    for (int e = 0; e < E; ++e) emit<K>(st, pos, (uint32_t)row[e], h[e], valid[e]);
}

template <int K, int V, bool FOUR, class Out>
__device__ __forceinline__ void probe_pairs_body(Stage& st, const uint64_t* __restrict__ S, uint64_t n, uint64_t sIdxBase, const OaTable& T,
                                                 const ShardCheck& sc, const Out& out, Counters* __restrict__ ctr)
{
    static_assert(2 * V * kBlock * (FOUR ? 4 : kMaxProbeLen) <= kStagePairs, "a round must fit an empty stage");
    uint32_t foreign = 0;
    for_s_rounds<V>(S, n, sIdxBase, [&](uint32_t key) { foreign += (uint32_t)is_foreign(key, sc); },
                    [&](const auto& sk, const auto& row, const auto& valid) { oa_round<K, FOUR>(st, out, T, sk, row, valid); });
    stage_finish<K>(st, out, ctr, &Counters::Shard::matches);
    foreign = wave_sum(foreign);
    if ((threadIdx.x & (kWave - 1)) == 0 && foreign) atomicAdd(&counter_shard(ctr)->foreign, (unsigned long long)foreign);
}

}  // namespace

// probeLength 4 (the reference's default): four elements per lane and round, all sixteen window loads in flight;
// any other length: two elements, the walk with its early exit
// K: hj_join_kind. SEMI and ANTI keep no R plane in LDS
// MARK (INNER and LEFT only): `out` also carries the R-side match marks, set at every flush of the stage (stage_flush)
template <int K, bool MARK>
__global__ void __launch_bounds__(kBlock)
k_probe_pairs(const uint64_t* __restrict__ S, uint64_t n, uint64_t sIdxBase, const uint64_t* __restrict__ table, uint64_t mask,
              uint32_t hshift, uint32_t probeLen, ShardCheck sc, PairsOutOf<MARK> out, Counters* __restrict__ ctr)
{
    static_assert(!MARK || K <= kLeft, "only the kinds that produce R rows mark them");
    __shared__ uint32_t ldsS[kStagePairs], ldsR[K <= kLeft ? kStagePairs : 1], ldsTot[2 * kWaves];
    __shared__ unsigned long long ldsBase;
    Stage st{ldsS, ldsR, ldsTot, &ldsBase, 0u, 0u, 0ull, 0ull, 0u};
    OaTable T{table, mask, hshift, probeLen, ctr->validLo, ctr->validHiEx, 0};
    T.dummy = T.validLo < mask ? T.validLo : 0;          // any in-table slot; this one is in cache
    if (probeLen == 4) probe_pairs_body<K, 2, true>(st, S, n, sIdxBase, T, sc, out, ctr);
    else probe_pairs_body<K, 1, false>(st, S, n, sIdxBase, T, sc, out, ctr);
}

namespace {

// ---------------------------------------------------------------------------
// --algo htm: bucket, then the whole chain, one bucket per element and round
// ---------------------------------------------------------------------------
// the bucket a walk stands at (nullptr: done), and what the last bucket read matched
struct ChainWalk { const ulonglong2* p; uint32_t key, sRow, m, r0, r1, r2; };
// what a walk carries besides for the kinds other than INNER: seen = an earlier bucket of the chain matched; done = the
// element's last row decision is taken (its chain has ended, or the lane never held an element); rows = what this step writes
struct ChainKind { bool seen, done; uint32_t rows; };

__device__ __forceinline__ void chain_step(ChainWalk& c, const uint64_t* __restrict__ overflow)
{
    c.m = 0;
    if (c.p == nullptr) return;
    const ulonglong2 a = c.p[0], b = c.p[1];
    const bool h0 = a.x != kEmpty && (uint32_t)a.x == c.key, h1 = a.y != kEmpty && (uint32_t)a.y == c.key,
               h2 = b.x != kEmpty && (uint32_t)b.x == c.key;
    const uint32_t v0 = (uint32_t)(a.x >> 32), v1 = (uint32_t)(a.y >> 32), v2 = (uint32_t)(b.x >> 32);
    // the matching R rows, packed to the front (r0 .. r[m - 1])
    c.m = (uint32_t)h0 + (uint32_t)h1 + (uint32_t)h2;
    c.r0 = h0 ? v0 : h1 ? v1 : v2;
    c.r1 = (h0 && h1) ? v1 : v2;
    c.r2 = v2;
    const uint32_t next = b.y == kEmpty ? 0u : (uint32_t)(b.y >> 32);      // slot 3 = next << 32 | count, all ones = no chain
    c.p = next ? reinterpret_cast<const ulonglong2*>(overflow + ((uint64_t)next << 2)) : nullptr;
}

// The step's rows of the kind K. An element is unmatched only once its chain has ended (c.p == nullptr after the step)
// and no bucket matched: that row, like SEMI's, is written once, never once per bucket. At most 3 rows per step: the
// unmatched row comes with m == 0.
template <int K>
__device__ __forceinline__ void chain_rows(const ChainWalk& c, ChainKind& k, Stage& st)
{
    const bool ends = !k.done && c.p == nullptr;
    const bool none = ends && !k.seen && c.m == 0;
    st.inner += c.m;
    if constexpr (K == kLeft) { k.rows = c.m + (uint32_t)none; st.unmatched += (uint32_t)none; }
    if constexpr (K == kSemi) k.rows = (uint32_t)(c.m != 0 && !k.seen);
    if constexpr (K == kAnti) k.rows = (uint32_t)none;
    k.seen = k.seen || c.m != 0;
    k.done = k.done || ends;
}

template <int K>
__device__ __forceinline__ void chain_emit(Stage& st, uint32_t& pos, const ChainWalk& c, const ChainKind& k)
{
    if constexpr (K >= kSemi) { if (k.rows) { st.s[pos] = c.sRow; ++pos; } return; }
    if constexpr (K == kLeft) if (k.rows > c.m) { st.s[pos] = c.sRow; st.r[pos] = kNoRow; ++pos; }
    if (c.m > 0) { st.s[pos] = c.sRow; st.r[pos] = c.r0; ++pos; }
    if (c.m > 1) { st.s[pos] = c.sRow; st.r[pos] = c.r1; ++pos; }
    if (c.m > 2) { st.s[pos] = c.sRow; st.r[pos] = c.r2; ++pos; }
}

struct HtmTable { const uint64_t* table; const uint64_t* overflow; uint32_t bucketMask; uint64_t defLo, defHi; };

// E elements per lane: bucket rounds until the longest chain of the workgroup's elements has ended; lanes whose chains
// have ended idle through them
template <int K, int E, class Out>
__device__ __forceinline__ void htm_rounds(Stage& st, const Out& out, const HtmTable& T, const uint64_t (&sk)[E], const uint64_t (&row)[E],
                                           const bool (&valid)[E])
{
    ChainWalk c[E];
    ChainKind k[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        c[e].key = (uint32_t)sk[e]; c[e].sRow = (uint32_t)row[e]; c[e].m = 0; c[e].r0 = c[e].r1 = c[e].r2 = 0;
        const uint64_t slot = (uint64_t)((c[e].key / 3u) & T.bucketMask) << 2;
        const bool ok = (sk[e] >> 32) == 0 && sk[e] != 0 && slot >= T.defLo && slot + 3 < T.defHi;      // else: equals no stored tuple
        c[e].p = ok ? reinterpret_cast<const ulonglong2*>(T.table + slot) : nullptr;
        k[e] = ChainKind{false, !valid[e], 0u};
    }
    bool any;
    do {
        uint32_t m = 0;
        bool more = false;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            chain_step(c[e], T.overflow);
            if constexpr (K == kInner) m += c[e].m;
            else { chain_rows<K>(c[e], k[e], st); m += k[e].rows; }
            more = more || c[e].p != nullptr;
        }
        uint32_t pos = stage_reserve<K>(st, out, m, more, any);
#pragma unroll
        for (int e = 0; e < E; ++e) chain_emit<K>(st, pos, c[e], k[e]);
    } while (any);
}

constexpr int kHtmVecs = 2;       // four elements per lane and round: at most 12 pairs per lane, 3072 per round
static_assert(2 * kHtmVecs * kBlock * 3 <= kStagePairs, "a round must fit an empty stage");

}  // namespace

template <int K, bool MARK>
__global__ void __launch_bounds__(kBlock)
k_htm_probe_pairs(const uint64_t* __restrict__ S, uint64_t n, uint64_t sIdxBase, const uint64_t* __restrict__ table, uint32_t bucketMask,
                  const uint64_t* __restrict__ overflow, PairsOutOf<MARK> out, Counters* __restrict__ ctr)
{
    static_assert(!MARK || K <= kLeft, "only the kinds that produce R rows mark them");
    constexpr int V = kHtmVecs;
    __shared__ uint32_t ldsS[kStagePairs], ldsR[K <= kLeft ? kStagePairs : 1], ldsTot[2 * kWaves];
    __shared__ unsigned long long ldsBase;
    Stage st{ldsS, ldsR, ldsTot, &ldsBase, 0u, 0u, 0ull, 0ull, 0u};
    // buckets outside the slots the build defined were never written and hold no tuple (hj_common.h, Counters)
    const HtmTable T{table, overflow, bucketMask, ctr->validLo, ctr->validHiEx + 512};
    for_s_rounds<V>(S, n, sIdxBase, [](uint32_t) {},
                    [&](const auto& sk, const auto& row, const auto& valid) { htm_rounds<K>(st, out, T, sk, row, valid); });
    stage_finish<K>(st, out, ctr, &Counters::Shard::matches);
}

namespace {

// four workgroups of 32 KiB of LDS per CU, the rest of S by grid stride; vecs = 16-byte loads per lane and round
unsigned pairs_grid(uint64_t n, int nCU, int vecs)
{
    const uint64_t perBlock = 2ull * kBlock * (uint64_t)vecs;
    uint64_t blocks = (n + perBlock - 1) / perBlock;
    const uint64_t most = (uint64_t)(nCU > 0 ? nCU : 256) * 4u;
    if (blocks > most) blocks = most;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

}  // namespace

uint32_t pairs_max_probe_len() { return kMaxProbeLen; }

void launch_probe_pairs(uint32_t kind, const uint64_t* S, uint64_t n, uint64_t sIdxBase, const uint64_t* table, uint64_t tableSize, uint32_t hshift,
                        uint32_t probeLen, ShardCheck sc, PairsOut out, int nCU, Counters* ctr, hipStream_t s, const RMarks* marks)
{
    const dim3 grid(pairs_grid(n, nCU, probeLen == 4 ? 2 : 1));
    with_kind(kind, marks != nullptr, [&](auto k, auto mark) {
        hipLaunchKernelGGL((k_probe_pairs<decltype(k)::value, decltype(mark)::value>), grid, dim3(kBlock), 0, s, S, n, sIdxBase, table,
                           tableSize - 1, hshift, probeLen, sc, pairs_out_of<decltype(mark)::value>(out, marks), ctr);
    });
}

void launch_htm_probe_pairs(uint32_t kind, const uint64_t* S, uint64_t n, uint64_t sIdxBase, const uint64_t* table, uint32_t numBuckets,
                            const uint64_t* overflow, PairsOut out, int nCU, Counters* ctr, hipStream_t s, const RMarks* marks)
{
    const dim3 grid(pairs_grid(n, nCU, kHtmVecs));
    with_kind(kind, marks != nullptr, [&](auto k, auto mark) {
        hipLaunchKernelGGL((k_htm_probe_pairs<decltype(k)::value, decltype(mark)::value>), grid, dim3(kBlock), 0, s, S, n, sIdxBase, table,
                           numBuckets - 1, overflow, pairs_out_of<decltype(mark)::value>(out, marks), ctr);
    });
}

}  // namespace hj
