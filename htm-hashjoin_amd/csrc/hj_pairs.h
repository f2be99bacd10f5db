// hj_pairs.h -- how matches leave a kernel as (S row, R row) pairs: the output planes and their cursor, the R-side match
// marks and their sweep, the LDS pair stage, the pair-filter frame, and the launchers of the materialising probes.
#pragma once

#include "hj_common.h"

namespace hj {

// ---- materialising probe (defined in hj_pairs.hip) --------------------------
// where hj_probe_pairs_dev writes: the two gather-map planes, their length, and the 64-bit cursor the workgroups claim
// their runs from (zeroed before the launch; its final value = pairs found, written or not)
// Join kinds (hj_join_kind): `kind` picks the kernels' instantiation. cursor[1] (zeroed with the cursor) collects the S
// elements without a match under HJ_JOIN_LEFT and is touched by no other kind; HJ_JOIN_SEMI / ANTI never touch plane r.
struct PairsOut { uint32_t* s; uint32_t* r; uint64_t capacity; unsigned long long* cursor; };

// A staged plane leaves LDS, by a workgroup of NT threads: lds[0 .. cnt) -> out[base .. base + cnt), cut at capacity. The
// elements before the first 16-byte boundary of the destination and after the last one by one lane each, the body as
// 16-byte stores. Written once, read by nobody here.
template <int NT>
__device__ __forceinline__ void flush_plane(const uint32_t* lds, uint32_t cnt, uint32_t* __restrict__ out, uint64_t base, uint64_t capacity)
{
    if (base >= capacity) return;
    const uint64_t room = capacity - base;
    const uint32_t lim = room < cnt ? (uint32_t)room : cnt;           // elements of the run that exist in the output
    uint32_t* const dst = out + base;
    uint32_t lead = (uint32_t)(((16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) >> 2);
    if (lead > lim) lead = lim;
    if (threadIdx.x < lead) __builtin_nontemporal_store(lds[threadIdx.x], dst + threadIdx.x);
    const uint32_t nv = (lim - lead) >> 2;
    for (uint32_t v = threadIdx.x; v < nv; v += NT) {
        const uint32_t i = lead + 4u * v;
        u4 x;
        x.x = lds[i]; x.y = lds[i + 1]; x.z = lds[i + 2]; x.w = lds[i + 3];
        __builtin_nontemporal_store(x, reinterpret_cast<u4*>(dst + i));
    }
    const uint32_t tail = lead + 4u * nv;
    if (threadIdx.x < lim - tail) __builtin_nontemporal_store(lds[tail + threadIdx.x], dst + tail + threadIdx.x);
}
// R-side match marks (HJ_FLAG_TRACK_R_MATCHES): one bit per R row of the last build, bit (row - base) of words[]; rows =
// the build's rSize. Set by the MARK instantiations of the three pairs kernels for every R row of a row they produce
// (written or cut by the capacity alike), read by the sweep of hj_r_marks.hip. Bits only go 0 -> 1 between clears.
struct RMarks { uint32_t* words; uint32_t base, rows; };
// what a MARK instantiation takes where the others take PairsOut: the same planes and cursor, and the marks behind them
struct PairsOutMarked : PairsOut { RMarks marks; };
template <bool MARK> using PairsOutOf = std::conditional_t<MARK, PairsOutMarked, PairsOut>;
template <bool MARK>
inline PairsOutOf<MARK> pairs_out_of(const PairsOut& out, const RMarks* marks)
{
    PairsOutOf<MARK> o;
    static_cast<PairsOut&>(o) = out;
    if constexpr (MARK) o.marks = *marks;
    return o;
}
// One produced R row -> its bit. First a relaxed agent-scope LOAD of the word, which L2 serves: a Zipf-hot R row is
// produced millions of times from every CU, and one word takes a limited number of atomics per microsecond chip-wide.
// The atomic OR (no value returned) is issued only while the bit reads clear; a stale "clear" costs one redundant OR and
// is never wrong, because nothing clears a bit while probes run. HJ_NO_ROW (a LEFT row without a match) marks nothing:
// it is no row of the build, like anything else outside [base, base + rows).
__device__ __forceinline__ void mark_r_row(const RMarks& mk, uint32_t row)
{
    const uint32_t i = row - mk.base;
    if (i >= mk.rows) return;
    uint32_t* const w = mk.words + (i >> 5);
    const uint32_t bit = 1u << (i & 31u);
    if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) return;
    __hip_atomic_fetch_or(w, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the R rows of a stage, as it is read at a flush: neighbouring lanes hold neighbouring pairs
template <int NT>
__device__ __forceinline__ void mark_plane(const uint32_t* lds, uint32_t cnt, const RMarks& mk)
{
    for (uint32_t i = threadIdx.x; i < cnt; i += NT) mark_r_row(mk, lds[i]);
}

// ---- the pair stage of the three pairs kernels (k_probe_pairs, k_htm_probe_pairs, k_prj_join_pairs) ----
// How a workgroup gets its place in the output ("Materialising probe"): it collects its rows in an LDS stage of
// kStagePairs pairs; a round first agrees on its row count -- wavefront scan, the wavefronts' totals exchanged through
// LDS, one barrier -- and when the stage cannot take the round, the workgroup claims [base, base + fill) with ONE 64-bit
// atomicAdd on the cursor and the stage leaves LDS through flush_plane.
constexpr uint32_t kStagePairs = 4096;          // pairs per stage: 2 planes x 16 KiB of LDS

// hj_join_kind; kinds above LEFT write S rows only
constexpr int kInner = 0, kLeft = 1, kSemi = 2, kAnti = 3;

// A runtime (kind, marks wanted) becomes f(integral_constant<int, K>, bool_constant<MARK>): the instantiations of the
// pairs kernels that exist, in this one place. Only the kinds that produce R rows mark them.
template <class F>
inline void with_kind(uint32_t kind, bool marks, F&& f)
{
    using std::integral_constant;
    if (marks && kind == (uint32_t)kLeft) f(integral_constant<int, kLeft>{}, std::true_type{});
    else if (marks && kind == (uint32_t)kInner) f(integral_constant<int, kInner>{}, std::true_type{});
    else if (kind == (uint32_t)kLeft) f(integral_constant<int, kLeft>{}, std::false_type{});
    else if (kind == (uint32_t)kSemi) f(integral_constant<int, kSemi>{}, std::false_type{});
    else if (kind == (uint32_t)kAnti) f(integral_constant<int, kAnti>{}, std::false_type{});
    else f(integral_constant<int, kInner>{}, std::false_type{});
}

template <int NT>                 // threads of the workgroup
struct PairStage {
    uint32_t* s;                  // LDS [kStagePairs]: S rows of the staged pairs
    uint32_t* r;                  // LDS [kStagePairs]: R rows (kinds above LEFT: unused)
    uint32_t* wtot;               // LDS [2][NT / 64]: the wavefronts' row counts of a round (bit 31: a lane has more to walk)
    unsigned long long* base;     // LDS: where the run being written starts in the output
    uint32_t fill;                // pairs staged (the same value in every thread)
    uint32_t round;
    unsigned long long found;     // rows of this workgroup so far (the same value in every thread)
    // kinds other than INNER, per lane: the inner matches of its elements, its elements without a match
    unsigned long long inner;
    uint32_t unmatched;
};

// Claims the output run of everything staged and writes it. Called by all threads of the workgroup together.
// Out = PairsOutMarked (the MARK instantiations): every staged R row also sets its mark. Here, because the stage holds every
// row the workgroup produced since its last flush whether the capacity lets it out or not (flush_plane cuts per element and
// returns early behind the capacity; the marks must not), and because neighbouring lanes read neighbouring pairs.
template <int K, int NT, class Out>
__device__ __forceinline__ void stage_flush(PairStage<NT>& st, const Out& out)
{
    if (threadIdx.x == 0) *st.base = atomicAdd(out.cursor, (unsigned long long)st.fill);
    __syncthreads();                                  // the base is there, and so is every pair of the rounds before
    const uint64_t base = *st.base;
    flush_plane<NT>(st.s, st.fill, out.s, base, out.capacity);
    if constexpr (K <= kLeft) flush_plane<NT>(st.r, st.fill, out.r, base, out.capacity);
    if constexpr (std::is_same_v<Out, PairsOutMarked>) mark_plane<NT>(st.r, st.fill, out.marks);
    __syncthreads();                                  // nobody refills the stage (or claims again) while it is being read
    st.fill = 0;
}

// One round: every lane brings m rows of its kind (more: it has further buckets to walk). Returns the rows of the round in
// front of the lane's own; tot: the round's rows, anyMore: some lane of the workgroup has more. One barrier. The totals
// are double-buffered by round parity: a wavefront writes round k + 2's only after the barrier of round k + 1, which
// every wavefront reaches after reading round k's.
template <int NT>
__device__ __forceinline__ uint32_t stage_scan(PairStage<NT>& st, uint32_t m, bool more, bool& anyMore, uint32_t& tot)
{
    constexpr uint32_t kWaves = NT / kWave;
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    uint32_t inc = m;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t below = __shfl_up(inc, off, kWave);
        if (lane >= (uint32_t)off) inc += below;
    }
    const bool waveMore = __ballot(more) != 0ull;
    uint32_t* const wt = st.wtot + (st.round & 1u) * kWaves;
    if (lane == kWave - 1) wt[w] = inc | (waveMore ? 0x80000000u : 0u);
    __syncthreads();
    uint32_t wbase = 0, any = 0;
    tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < kWaves; ++k) {
        const uint32_t v = wt[k], c = v & 0x7FFFFFFFu;
        if (k < w) wbase += c;
        tot += c;
        any |= v >> 31;
    }
    st.round += 1;
    anyMore = any != 0;
    return wbase + inc - m;
}

// The stage takes a round of tot <= kStagePairs rows, flushed first when they do not fit (a second barrier). Returns the
// fill before the round: the lane writes its rows from there + what stage_scan returned.
template <int K, int NT, class Out>
__device__ __forceinline__ uint32_t stage_place(PairStage<NT>& st, const Out& out, uint32_t tot)
{
    if (st.fill + tot > kStagePairs) stage_flush<K>(st, out);         // workgroup-uniform
    const uint32_t before = st.fill;
    st.fill += tot;
    st.found += tot;
    return before;
}

// stage_scan, then stage_place: the lane's position in the stage, for kernels whose rounds always fit an empty stage
template <int K, int NT, class Out>
__device__ __forceinline__ uint32_t stage_reserve(PairStage<NT>& st, const Out& out, uint32_t m, bool more, bool& anyMore)
{
    uint32_t tot;
    const uint32_t before = stage_scan(st, m, more, anyMore, tot);
    return stage_place<K>(st, out, tot) + before;
}

// The end of a pairs kernel: the last stage, then the workgroup's share of the counters. word: the counter of the INNER
// matches (matches / prjMatches), which grows by them whatever the kind. INNER: the rows are the matches, found is the same
// in every thread, one atomic per workgroup. Other kinds: the lanes' inner matches are summed instead, and LEFT also leaves
// its unmatched elements in the word behind the cursor (hj_pairs_info; SEMI and ANTI derive theirs on the host).
template <int K, int NT, class Out>
__device__ __forceinline__ void stage_finish(PairStage<NT>& st, const Out& out, Counters* __restrict__ ctr,
                                             unsigned long long Counters::Shard::* word)
{
    if (st.fill) stage_flush<K>(st, out);
    if constexpr (K == kInner) {
        if (threadIdx.x == 0 && st.found) atomicAdd(&(counter_shard(ctr)->*word), st.found);
    } else {
        const unsigned long long inner = wave_sum(st.inner);
        if ((threadIdx.x & (kWave - 1)) == 0 && inner) atomicAdd(&(counter_shard(ctr)->*word), inner);
        if constexpr (K == kLeft) {
            const uint32_t unmatched = wave_sum(st.unmatched);
            if ((threadIdx.x & (kWave - 1)) == 0 && unmatched) atomicAdd(out.cursor + 1, (unsigned long long)unmatched);
        }
    }
}

// ---- the pair-filter frame of the kernels that take a pair list and keep part of it (k_pairs_verify2, k_pairs_where,
// k_asof_keep of hj_asof.hip, which repeats the text a third time with one plane load as its loop) ----
// What the two kernels have in common around their column / term loop: the shape and its names, the flow below, and the
// launch. The flow is written out in each kernel, the same text twice, NOT shared as device code: as one function that
// takes the loop as a callable the compiler copies the kernel's by-value column struct into scalar registers up front
// (the callable captures it by reference) and the variable-length verify instance spills; as two inlined halves around the
// kernel's own loop the registers are the same but the code is not, and the calls without mark planes measured 3 to 7 %
// slower (profiles/join_on_columns.md, (e)). A change to the flow is made in both kernels and in k_asof_keep; tools/asm_diff.py
// and tests/test_gpu_pair_filter_frame.py hold the two together, tests/test_gpu_asof.py the third to the same contract.
// Shape: one workgroup of kBlock lanes per kFilterBlockPairs = 1024 consecutive pairs, so the stage is flushed exactly
// once; a wavefront owns 256 consecutive pairs and takes them as kFilterLanePairs = 4 steps of 64, the map reads coalesced
// and nontemporal, all eight in flight before the first is looked at. A pair with an HJ_NO_ROW entry, or with a row outside
// its relation, is dropped before anything is dereferenced, and counted (ballots) into cursor[1]. The kernel's own loop
// settles the lane's four pairs: si / ri are the rows with S's base off, live comes in as "not dropped" and goes out as
// "kept". Its loads are to be unconditional (a load under a per-lane condition is a branch around it, and the wait
// counters in front of the next one would then wait for it), so a dropped pair brings a spare row, which exists --
// neighbouring lanes neighbouring rows, not all one address; with sRows or rRows 0 there is no row to read, every pair is
// dropped and the loop is not run. The kept count is agreed on by stage_reserve (wavefront scan + LDS totals, one barrier),
// the kept pairs are staged, the run is claimed with one atomicAdd on the 64-bit cursor and leaves through flush_plane
// (stage_flush, R's marks with it); S's marks are set from the stage too: neighbouring lanes hold neighbouring pairs, and
// a pair the capacity cuts marks like any other.
constexpr uint32_t kFilterStepPairs = kWave;
constexpr uint32_t kFilterLanePairs = 4;                              // pairs in flight per lane, kFilterStepPairs apart
constexpr uint32_t kFilterWavePairs = kFilterStepPairs * kFilterLanePairs;
constexpr uint32_t kFilterWaves = kBlock / kWave;
constexpr uint32_t kFilterBlockPairs = kFilterWavePairs * kFilterWaves;      // 1024
static_assert(kFilterBlockPairs <= kStagePairs, "a workgroup's pairs fit one stage: it is flushed exactly once");

// What the calls on a pair list take and leave (verify, where, as-of; their host twins too). The list: pair k is
// (mapS[k] - sRowBase, mapR[k]), sRows / rRows the rows of the two relations. The sink: the planes and the cursor of the
// kept pairs (the host twins have no cursor: null) and the two mark planes in RMarks' layout, either may be null.
struct PairList { const uint32_t* mapS; const uint32_t* mapR; uint64_t n; uint32_t sRowBase, sRows, rRows; };
struct PairSink { PairsOut out; uint32_t* sMarks; uint32_t* rMarks; };

// The launch of either kernel: k(mapS, mapR, nPairs, sRowBase, sRows, rRows, cols, nCols, out, S's marks).
template <class Kernel, class Cols>
inline hipError_t launch_pair_filter(Kernel kernel, const PairList& in, const Cols& cols, uint32_t nCols, const PairSink& to, hipStream_t s)
{
    if (in.n == 0) return hipSuccess;
    const RMarks mkS{to.sMarks, in.sRowBase, to.sMarks ? in.sRows : 0u}, mkR{to.rMarks, 0u, to.rMarks ? in.rRows : 0u};
    const PairsOutMarked o = pairs_out_of<true>(to.out, &mkR);
    const dim3 grid((uint32_t)((in.n + kFilterBlockPairs - 1) / kFilterBlockPairs));          // n <= 2^32 - 1: <= 2^22 workgroups
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, in.mapS, in.mapR, in.n, in.sRowBase, in.sRows, in.rRows, cols, nCols, o, mkS);
    return hipGetLastError();
}

uint32_t pairs_max_probe_len();          // longest walk a round of k_probe_pairs can stage
// the table must be in the 8-byte slot format (kFormatSlots8): the R row is the index word of the slot
// marks != nullptr (kinds INNER and LEFT only): the MARK instantiation, which also sets the bit of every R row it produces
void launch_probe_pairs(uint32_t kind, const uint64_t* S, uint64_t n, uint64_t sIdxBase, const uint64_t* table, uint64_t tableSize, uint32_t hshift,
                        uint32_t probeLen, ShardCheck sc, PairsOut out, int nCU, Counters* ctr, hipStream_t s, const RMarks* marks = nullptr);
void launch_htm_probe_pairs(uint32_t kind, const uint64_t* S, uint64_t n, uint64_t sIdxBase, const uint64_t* table, uint32_t numBuckets,
                            const uint64_t* overflow, PairsOut out, int nCU, Counters* ctr, hipStream_t s, const RMarks* marks = nullptr);

// ---- sweep of the R-side match marks (defined in hj_r_marks.hip) ------------
// The ordered compaction of a mark plane: the rows base + i, i in [0, rows), whose bit equals `set`, ascending, to
// out[0 ..) without holes; rows at or beyond capacity are counted and not written. counts: r_sweep_count_words(rows) words
// of workspace -- one count per block and the total behind them (counts[r_sweep_blocks(rows)] after the call), then the
// scan's own words.
uint32_t r_sweep_blocks(uint64_t rows);
size_t r_sweep_count_words(uint64_t rows);
hipError_t launch_r_sweep(const RMarks& marks, bool set, uint32_t* out, uint64_t capacity, uint32_t* counts, hipStream_t s);

}  // namespace hj
