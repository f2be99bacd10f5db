// hj_range.hip -- range joins without an equality key for gfx950 (MI355X): hj_range_index_* and hj_range_pairs_*
// (... ON R.y BETWEEN S.lo AND S.hi, one bound, the keyless as-of). R's column is sorted once into an index the caller
// owns -- the sort's permutation, the plane of sort_key words along it, four head words -- and every S row becomes the
// half-open run of positions [a, b) of that plane whose keys lie in its interval.
//
// The range call, in launches that order each other and nothing else:
//   (pivots)  k_range_pivots: every stride-th key of the indexed prefix, packed into the workspace (range_layout).
//   (bounds)  k_range_bounds: one workgroup per chunk of kRangeChunkRows S rows, one lane per row. The pivots go to LDS once;
//             a lane searches there first and finishes in the stride - 1 keys between two pivots in global memory, both
//             of its searches in one loop so that their loads are in flight together, no branch on a comparison. Writes
//             a[i], b[i], S's marks (plain word ORs: a wavefront owns the two words of its 64 rows) and the chunk's 64-bit
//             total and counts. With R marks wanted: +1 at a, -1 at b in a difference plane (HJ_RANGE_ALL), or the bit of
//             the one picked row (FIRST / LAST).
//   (R marks) the library's scan over the difference plane, then k_range_rmarks: position q is covered when the scanned
//             sum behind it is not 0 -> bit perm[q]. O(|S| + |R|) whatever the pairs.
//   (chunks)  k_range_chunks: one workgroup, the 64-bit exclusive scan of the chunk totals and the call's counter words.
//   (expand)  k_range_expand: driven by the output. A workgroup owns kRangeTile output positions, finds the chunks that
//             cross them in the chunk offsets, redoes the 64-bit scan inside such a chunk, drops one word per S row that
//             starts in the tile into LDS and spreads it with a max-scan; position j then knows its S row and its
//             position in the key plane, and both planes are written coalesced.
// No workgroup waits for another, every loop is bounded (by the pivots, the stride, the chunks), the only atomics are the
// difference plane's adds and the ORs of mark bits, and integer adds and ORs make the result independent of scheduling.
#include "hj_columns.h"

#include <algorithm>
#include <vector>

namespace hj {
namespace {

constexpr int kRangeThreads = 256;
constexpr uint32_t kRangeChunkRows = 4096;                             // S rows of one bounds workgroup
constexpr uint32_t kRangeRowsPer = kRangeChunkRows / kRangeThreads;    // 16
constexpr uint32_t kRangeMaxPivots = 4096;                             // 32 KiB of LDS as 8-byte keys
constexpr uint32_t kRangeMinStride = 16;
constexpr uint32_t kRangeTile = 2048;                                  // output positions of one expansion workgroup
constexpr uint32_t kRangeTilePer = kRangeTile / kRangeThreads;         // 8
constexpr uint32_t kPickAll = 0, kPickFirst = 1, kPickLast = 2;        // hj_range_pick
constexpr uint32_t kLoOpen = 1u, kHiOpen = 2u;                         // HJ_RANGE_LO_OPEN, HJ_RANGE_HI_OPEN

size_t up256(uint64_t b) { return (size_t)((b + 255) & ~255ull); }

// the workspace of a call, carved
struct RangeWork {
    void* pivots; uint32_t *a, *b; unsigned long long* chunkTot; uint32_t* chunkCnt; unsigned long long* chunkOff; uint32_t *diff, *sums;
};
RangeWork range_carve(void* work, const RangeLayout& l)
{
    char* p = static_cast<char*>(work);
    RangeWork w{};
    w.pivots = p; p += l.pivotBytes;
    w.a = reinterpret_cast<uint32_t*>(p); p += l.boundBytes;
    w.b = reinterpret_cast<uint32_t*>(p); p += l.boundBytes;
    w.chunkTot = reinterpret_cast<unsigned long long*>(p); p += l.chunkBytes;
    w.chunkOff = reinterpret_cast<unsigned long long*>(p); p += l.chunkBytes;
    w.chunkCnt = reinterpret_cast<uint32_t*>(p); p += l.chunkBytes;
    w.diff = reinterpret_cast<uint32_t*>(p); p += l.diffBytes;
    w.sums = reinterpret_cast<uint32_t*>(p);
    return w;
}

// exclusive scan of 64-bit values over the workgroup; wsum: kRangeThreads / 64 words of LDS. Two barriers.
__device__ __forceinline__ unsigned long long block_exclusive_scan_u64(unsigned long long v, unsigned long long* wsum, unsigned long long& total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long n = __shfl_up(inc, off, 64);
        if (lane >= off) inc += n;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned long long wbase = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kRangeThreads / 64; ++k) {
        const unsigned long long s = wsum[k];
        if (k < w) wbase += s;
        tot += s;
    }
    total = tot;
    __syncthreads();
    return wbase + inc - v;
}

// ---- the index: the key plane along the permutation, and the head ----------------
// keys[q] = sort_key of the element of row perm[q]; head[1] += the NULL rows, head[2] += the NaN rows (zeroed before)
template <class K>
__global__ void __launch_bounds__(kRangeThreads)
k_range_keys(const void* __restrict__ col, const uint32_t* __restrict__ valid, uint32_t width, uint32_t type, const uint32_t* __restrict__ perm,
             K* __restrict__ keys, uint64_t n, uint32_t* __restrict__ head)
{
    const uint64_t q = (uint64_t)blockIdx.x * kRangeThreads + threadIdx.x;
    bool isNull = false, isNan = false;
    if (q < n) {
        const uint32_t row = perm[q];
        const uint64_t key = sort_key(type, width, 0u, col_elem(col, width, row));     // read under a NULL too: the bytes exist
        isNull = valid && !valid_bit(valid, row);
        isNan = !isNull && type == kValFloat && key == (width == 4u ? 0xFFFFFFFFull : ~0ull);
        keys[q] = isNull ? (K)0 : (K)key;
    }
    const uint32_t nulls = (uint32_t)__popcll(__ballot(isNull)), nans = (uint32_t)__popcll(__ballot(isNan));
    if ((threadIdx.x & 63) == 0) {
        if (nulls) atomicAdd(head + 1, nulls);
        if (nans) atomicAdd(head + 2, nans);
    }
}
__global__ void k_range_head(uint32_t* __restrict__ head, uint32_t nRows, uint32_t keyBytes)
{
    head[0] = nRows - head[1] - head[2];
    head[3] = keyBytes;
}

// the indexed rows as a range call takes them: none for an index of the other key width, never more than the caller's rRows
template <class K>
__device__ __forceinline__ uint32_t range_indexed(const uint32_t* __restrict__ head, uint32_t rRows)
{
    if (!head || !rRows || head[3] != sizeof(K)) return 0u;
    const uint32_t n = head[0];
    return n < rRows ? n : rRows;
}

template <class K>
__global__ void __launch_bounds__(kRangeThreads)
k_range_pivots(const K* __restrict__ keys, const uint32_t* __restrict__ head, uint32_t rRows, uint32_t stride, K* __restrict__ pivots)
{
    const uint32_t n = range_indexed<K>(head, rRows);
    const uint64_t at = ((uint64_t)blockIdx.x * kRangeThreads + threadIdx.x) * stride;
    if (at < n) pivots[blockIdx.x * kRangeThreads + threadIdx.x] = keys[at];
}

// Two searches of one lane, step by step together. Search X counts the keys of the indexed prefix for which
//   key < tX || (eqX && key == tX)
// holds -- a prefix of the plane, so the count is std::lower_bound's (eqX false) or std::upper_bound's (eqX true) position.
// First the pivots in LDS: c of them hold -> the answer lies in ((c - 1) stride, c stride], and the stride - 1 keys behind
// pivot c - 1 are searched in global memory; c == 0 -> 0. Every step adds its width or nothing: no branch on a key.
template <class K>
__device__ __forceinline__ void range_search2(const K* __restrict__ keys, const K* piv, uint32_t n, uint32_t np, uint32_t stride,
                                              K tA, bool eqA, K tB, bool eqB, uint32_t& a, uint32_t& b)
{
    uint32_t ca = 0, cb = 0;
#pragma unroll
    for (uint32_t step = kRangeMaxPivots; step; step >>= 1) {
        const uint32_t ia = ca + step - 1u, ib = cb + step - 1u;
        const K ka = piv[ia < np ? ia : 0u], kb = piv[ib < np ? ib : 0u];
        const bool ra = ia < np && (ka < tA || (eqA && ka == tA)), rb = ib < np && (kb < tB || (eqB && kb == tB));
        ca += ra ? step : 0u; cb += rb ? step : 0u;
    }
    const uint32_t baseA = ca ? (ca - 1u) * stride + 1u : 0u, baseB = cb ? (cb - 1u) * stride + 1u : 0u;
    const uint32_t lenA = ca ? (n - baseA < stride - 1u ? n - baseA : stride - 1u) : 0u;
    const uint32_t lenB = cb ? (n - baseB < stride - 1u ? n - baseB : stride - 1u) : 0u;
    uint32_t pa = 0, pb = 0;
    for (uint32_t step = stride >> 1; step; step >>= 1) {
        const uint32_t ia = pa + step - 1u, ib = pb + step - 1u;
        const K ka = keys[ia < lenA ? baseA + ia : 0u], kb = keys[ib < lenB ? baseB + ib : 0u];      // both loads, then both compares
        const bool ra = ia < lenA && (ka < tA || (eqA && ka == tA)), rb = ib < lenB && (kb < tB || (eqB && kb == tB));
        pa += ra ? step : 0u; pb += rb ? step : 0u;
    }
    a = baseA + pa; b = baseB + pb;
}

template <class K>
__global__ void __launch_bounds__(kRangeThreads)
k_range_bounds(const K* __restrict__ keys, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ head, uint32_t rRows, uint32_t stride,
               const K* __restrict__ pivots, RangeTerm t, uint32_t sRows, uint32_t* __restrict__ outA, uint32_t* __restrict__ outB,
               unsigned long long* __restrict__ chunkTot, uint32_t* __restrict__ chunkCnt, uint32_t* sMarks, uint32_t* diff, uint32_t* rMarks)
{
    __shared__ K piv[kRangeMaxPivots];
    __shared__ unsigned long long wtot[kRangeThreads / 64];
    __shared__ uint32_t wcnt[2][kRangeThreads / 64];
    const uint32_t n = range_indexed<K>(head, rRows);
    const uint32_t np = (uint32_t)(((uint64_t)n + stride - 1u) / stride);                  // <= kRangeMaxPivots: stride is rRows' own
    for (uint32_t j = threadIdx.x; j < np; j += kRangeThreads) piv[j] = pivots[j];
    __syncthreads();

    const uint64_t nanKey = t.width == 4u ? 0xFFFFFFFFull : ~0ull;
    const RMarks mkR{rMarks, 0u, rMarks ? rRows : 0u};
    unsigned long long tot = 0;
    uint32_t matched = 0, bad = 0;
    const uint64_t chunkBase = (uint64_t)blockIdx.x * kRangeChunkRows;
    for (uint32_t it = 0; it < kRangeRowsPer; ++it) {
        const uint64_t i64 = chunkBase + (uint64_t)it * kRangeThreads + threadIdx.x;
        const bool live = i64 < sRows;
        const uint32_t i = live ? (uint32_t)i64 : sRows - 1u;                              // a spare row that exists: the loads stay unconditional
        bool ok = live;
        K tA = (K)0, tB = (K)~(K)0;
        bool eqA = false, eqB = true;                                                      // no bound: count nothing / count everything
        if (t.lo) {
            const uint64_t key = sort_key(t.type, t.width, 0u, col_elem(t.lo, t.width, i));
            ok = ok && !(t.loValid && !valid_bit(t.loValid, i)) && !(t.type == kValFloat && key == nanKey);
            tA = (K)key; eqA = (t.flags & kLoOpen) != 0u;
        }
        if (t.hi) {
            const uint64_t key = sort_key(t.type, t.width, 0u, col_elem(t.hi, t.width, i));
            ok = ok && !(t.hiValid && !valid_bit(t.hiValid, i)) && !(t.type == kValFloat && key == nanKey);
            tB = (K)key; eqB = (t.flags & kHiOpen) == 0u;
        }
        uint32_t a = 0, b = 0;
        if (n) range_search2<K>(keys, piv, n, np, stride, tA, eqA, tB, eqB, a, b);          // uniform
        uint32_t cnt = ok && b > a ? b - a : 0u;
        if (t.pick == kPickFirst) cnt = cnt ? 1u : 0u;
        if (t.pick == kPickLast && n) {                                                    // uniform
            // the largest value in the range is the key at b - 1; ties go to the lowest row: the first position of its run
            const K top = keys[cnt ? b - 1u : 0u];
            uint32_t p, unused;
            range_search2<K>(keys, piv, n, np, stride, top, false, top, false, p, unused);
            a = p; cnt = cnt ? 1u : 0u;
        }
        if (!cnt) a = 0u;
        b = a + cnt;
        if (live) { outA[i] = a; outB[i] = b; }
        tot += cnt; matched += cnt ? 1u : 0u; bad += live && !ok ? 1u : 0u;
        if (cnt && diff) {
            __hip_atomic_fetch_add(diff + a, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(diff + b, 0xFFFFFFFFu, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (cnt && rMarks && t.pick != kPickAll) mark_r_row(mkR, perm[a]);
        if (sMarks) {
            // the wavefront's 64 rows are the bits of two whole words that no other wavefront touches
            const unsigned long long m = __ballot(cnt != 0u);
            const uint32_t lane = threadIdx.x & 63u;
            const uint32_t half = lane == 0u ? (uint32_t)m : (uint32_t)(m >> 32);
            if ((lane == 0u || lane == 32u) && half) sMarks[i64 >> 5] |= half;
        }
    }
    wave_sum_all(tot, matched, bad);
    if ((threadIdx.x & 63) == 0) { wtot[threadIdx.x >> 6] = tot; wcnt[0][threadIdx.x >> 6] = matched; wcnt[1][threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0; uint32_t m = 0, x = 0;
        for (int k = 0; k < kRangeThreads / 64; ++k) { s += wtot[k]; m += wcnt[0][k]; x += wcnt[1][k]; }
        chunkTot[blockIdx.x] = s; chunkCnt[2 * blockIdx.x] = m; chunkCnt[2 * blockIdx.x + 1] = x;
    }
}

// scanned: the difference plane after the exclusive scan; position q is covered by scanned[q + 1] ranges (modulo 2^32,
// and no call has 2^32 S rows)
template <class K>
__global__ void __launch_bounds__(kRangeThreads)
k_range_rmarks(const uint32_t* __restrict__ scanned, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ head, uint32_t rRows,
               uint32_t* rMarks)
{
    const uint32_t n = range_indexed<K>(head, rRows);
    const uint64_t q = (uint64_t)blockIdx.x * kRangeThreads + threadIdx.x;
    if (q < n && scanned[q + 1] != 0u) mark_r_row(RMarks{rMarks, 0u, rRows}, perm[q]);
}

// one workgroup: chunkOff[c] = the pairs of the chunks below c, chunkOff[chunks] = the total; words: the total, the S rows
// with a pair, the S rows with a NULL or NaN bound, the rows indexed
template <class K>
__global__ void __launch_bounds__(kRangeThreads)
k_range_chunks(const unsigned long long* __restrict__ chunkTot, const uint32_t* __restrict__ chunkCnt, uint32_t chunks,
               unsigned long long* __restrict__ chunkOff, const uint32_t* __restrict__ head, uint32_t rRows, unsigned long long* __restrict__ words)
{
    __shared__ unsigned long long wsum[kRangeThreads / 64];
    __shared__ unsigned long long wm[2][kRangeThreads / 64];
    unsigned long long carry = 0, matched = 0, bad = 0;
    for (uint32_t base = 0; base < chunks; base += kRangeThreads) {
        const uint32_t c = base + threadIdx.x;
        const unsigned long long v = c < chunks ? chunkTot[c] : 0ull;
        unsigned long long total;
        const unsigned long long ex = block_exclusive_scan_u64(v, wsum, total);
        if (c < chunks) { chunkOff[c] = carry + ex; matched += chunkCnt[2 * c]; bad += chunkCnt[2 * c + 1]; }
        carry += total;
    }
    wave_sum_all(matched, bad);
    if ((threadIdx.x & 63) == 0) { wm[0][threadIdx.x >> 6] = matched; wm[1][threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = 0, x = 0;
        for (int k = 0; k < kRangeThreads / 64; ++k) { m += wm[0][k]; x += wm[1][k]; }
        chunkOff[chunks] = carry;
        words[0] = carry; words[1] = m; words[2] = x; words[3] = range_indexed<K>(head, rRows);
    }
}

// See the head of the file. An LDS word of the tile: (S row + 1) << 32 | (position in the key plane of the row's pair at
// tile position 0, modulo 2^32); 0: no row starts here. Rows ascend with the output, so a maximum spreads the latest start.
__global__ void __launch_bounds__(kRangeThreads)
k_range_expand(const uint32_t* __restrict__ inA, const uint32_t* __restrict__ inB, const unsigned long long* __restrict__ chunkOff,
               uint32_t chunks, uint32_t sRows, uint32_t sRowBase, const uint32_t* __restrict__ perm, uint32_t* __restrict__ outS,
               uint32_t* __restrict__ outR, uint64_t capacity)
{
    __shared__ unsigned long long mark[kRangeTile];
    __shared__ unsigned long long wsum[kRangeThreads / 64];
    const unsigned long long total = chunkOff[chunks];
    const unsigned long long lim = total < capacity ? total : capacity;
    const unsigned long long T0 = (unsigned long long)blockIdx.x * kRangeTile;
    if (T0 >= lim) return;                                                                 // uniform
    const unsigned long long T1 = T0 + kRangeTile < lim ? T0 + kRangeTile : lim;
    for (uint32_t p = threadIdx.x; p < kRangeTile; p += kRangeThreads) mark[p] = 0ull;
    __syncthreads();

    unsigned long long pos = T0;
    while (pos < T1) {                                                                     // every round takes a chunk that holds position pos: pos grows
        uint32_t lo = 0, hi = chunks;                                                      // chunkOff[lo] <= pos < chunkOff[hi]
        while (hi - lo > 1u) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (chunkOff[mid] <= pos) lo = mid; else hi = mid;
        }
        const unsigned long long cOff = chunkOff[lo], cEnd = chunkOff[lo + 1u];
        const uint64_t rowBase = (uint64_t)lo * kRangeChunkRows + (uint64_t)threadIdx.x * kRangeRowsPer;
        uint32_t a[kRangeRowsPer], cnt[kRangeRowsPer];
        unsigned long long local = 0;
#pragma unroll
        for (uint32_t k = 0; k < kRangeRowsPer; ++k) {
            const bool in = rowBase + k < sRows;
            a[k] = in ? inA[rowBase + k] : 0u;
            cnt[k] = in ? inB[rowBase + k] - a[k] : 0u;
            local += cnt[k];
        }
        unsigned long long chunkTotal;
        unsigned long long o = cOff + block_exclusive_scan_u64(local, wsum, chunkTotal);
#pragma unroll
        for (uint32_t k = 0; k < kRangeRowsPer; ++k) {
            const unsigned long long start = o, end = o + cnt[k];
            if (cnt[k] && end > T0 && start < T1) {
                const uint32_t p = start > T0 ? (uint32_t)(start - T0) : 0u;
                const uint32_t base = a[k] + (start > T0 ? 0u : (uint32_t)(T0 - start)) - p;
                mark[p] = ((unsigned long long)((uint32_t)(rowBase + k) + 1u) << 32) | base;
            }
            o = end;
        }
        pos = cEnd;
    }
    __syncthreads();

    // inclusive max-scan over the tile, kRangeTilePer consecutive words per thread
    unsigned long long m[kRangeTilePer], run = 0;
#pragma unroll
    for (uint32_t k = 0; k < kRangeTilePer; ++k) {
        const unsigned long long v = mark[threadIdx.x * kRangeTilePer + k];
        run = v > run ? v : run;
        m[k] = run;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned long long inc = run;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long x = __shfl_up(inc, off, 64);
        if (lane >= off) inc = x > inc ? x : inc;
    }
    if (lane == 63) wsum[w] = inc;
    unsigned long long before = __shfl_up(inc, 1, 64);
    if (lane == 0) before = 0ull;
    __syncthreads();
    for (int k = 0; k < w; ++k) before = wsum[k] > before ? wsum[k] : before;
#pragma unroll
    for (uint32_t k = 0; k < kRangeTilePer; ++k) mark[threadIdx.x * kRangeTilePer + k] = m[k] > before ? m[k] : before;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kRangeTilePer; ++k) {
        const uint32_t p = k * kRangeThreads + threadIdx.x;
        if (T0 + p < T1) {
            const unsigned long long v = mark[p];
            outS[T0 + p] = sRowBase + ((uint32_t)(v >> 32) - 1u);
            outR[T0 + p] = perm[(uint32_t)v + p];
        }
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// layout, workspace, launches
// ---------------------------------------------------------------------------
RangeLayout range_layout(uint64_t nRows, uint64_t sRows)
{
    RangeLayout l{};
    uint64_t stride = kRangeMinStride;
    while ((nRows + stride - 1) / stride > kRangeMaxPivots) stride <<= 1;                  // 2^32 rows: 2^20
    l.stride = (uint32_t)stride;
    l.pivots = (uint32_t)((nRows + stride - 1) / stride);
    l.tilePairs = kRangeTile; l.chunkRows = kRangeChunkRows;
    l.chunks = (uint32_t)((sRows + kRangeChunkRows - 1) / kRangeChunkRows);
    l.ldsBytes = kRangeMaxPivots * 8u;
    l.pivotBytes = up256((uint64_t)kRangeMaxPivots * 8u);                                  // whatever the rows: the workspace grows with them
    l.boundBytes = up256(sRows * sizeof(uint32_t));
    l.chunkBytes = up256(((uint64_t)l.chunks + 1) * sizeof(unsigned long long));
    l.diffBytes = up256((nRows + 1) * sizeof(uint32_t));
    l.bytes = l.pivotBytes + 2 * l.boundBytes + 3 * l.chunkBytes + l.diffBytes + up256(scan_workspace_words(nRows + 1) * sizeof(uint32_t));
    return l;
}

hipError_t launch_range_index(const SortCols& col, uint64_t nRows, uint32_t* perm, void* keys, uint32_t* head, void* work, hipStream_t s)
{
    const uint32_t kb = col.width[0] == 8 ? 8u : 4u;
    hipError_t e = hipMemsetAsync(head, 0, 4 * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    if (nRows) {
        e = launch_sort_rows(col, 1, nRows, perm, work, s);
        if (e != hipSuccess) return e;
        const dim3 grid((uint32_t)((nRows + kRangeThreads - 1) / kRangeThreads));
        if (kb == 8)
            hipLaunchKernelGGL(k_range_keys<unsigned long long>, grid, dim3(kRangeThreads), 0, s, col.p[0], col.valid[0], col.width[0], col.type[0], perm,
                               static_cast<unsigned long long*>(keys), nRows, head);
        else
            hipLaunchKernelGGL(k_range_keys<uint32_t>, grid, dim3(kRangeThreads), 0, s, col.p[0], col.valid[0], col.width[0], col.type[0], perm,
                               static_cast<uint32_t*>(keys), nRows, head);
    }
    hipLaunchKernelGGL(k_range_head, dim3(1), dim3(1), 0, s, head, (uint32_t)nRows, kb);
    return hipGetLastError();
}

namespace {
template <class K>
hipError_t range_pairs(const K* keys, const uint32_t* perm, const uint32_t* head, uint32_t rRows, const RangeTerm& t, uint32_t sRows,
                       uint32_t sRowBase, const PairSink& to, void* work, unsigned long long* words, hipStream_t s)
{
    const RangeLayout l = range_layout(rRows, sRows);
    const RangeWork w = range_carve(work, l);
    K* const pivots = static_cast<K*>(w.pivots);
    uint32_t* const diff = to.rMarks && t.pick == kPickAll && rRows && sRows ? w.diff : nullptr;
    if (diff) {
        const hipError_t e = hipMemsetAsync(diff, 0, ((size_t)rRows + 1) * sizeof(uint32_t), s);
        if (e != hipSuccess) return e;
    }
    if (l.pivots && sRows)
        hipLaunchKernelGGL(k_range_pivots<K>, dim3((l.pivots + kRangeThreads - 1) / kRangeThreads), dim3(kRangeThreads), 0, s, keys, head, rRows,
                           l.stride, pivots);
    if (l.chunks)
        hipLaunchKernelGGL(k_range_bounds<K>, dim3(l.chunks), dim3(kRangeThreads), 0, s, keys, perm, head, rRows, l.stride, pivots, t, sRows, w.a, w.b,
                           w.chunkTot, w.chunkCnt, to.sMarks, diff, to.rMarks);
    if (diff) {
        const hipError_t e = launch_exclusive_scan_u32(diff, (uint64_t)rRows + 1, w.sums, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_range_rmarks<K>, dim3((rRows + kRangeThreads - 1) / kRangeThreads), dim3(kRangeThreads), 0, s, diff, perm, head, rRows,
                           to.rMarks);
    }
    hipLaunchKernelGGL(k_range_chunks<K>, dim3(1), dim3(kRangeThreads), 0, s, w.chunkTot, w.chunkCnt, l.chunks, w.chunkOff, head, rRows, words);
    // no tile lies behind the capacity, nor behind the most pairs the call can have
    const uint64_t most = t.pick == kPickAll ? (uint64_t)sRows * rRows : sRows;
    const uint64_t room = to.out.capacity < most ? to.out.capacity : most;
    if (room)
        hipLaunchKernelGGL(k_range_expand, dim3((uint32_t)((room + kRangeTile - 1) / kRangeTile)), dim3(kRangeThreads), 0, s, w.a, w.b, w.chunkOff,
                           l.chunks, sRows, sRowBase, perm, to.out.s, to.out.r, to.out.capacity);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_range_pairs(const void* keys, const uint32_t* perm, const uint32_t* head, uint32_t rRows, const RangeTerm& t, uint32_t sRows,
                              uint32_t sRowBase, const PairSink& to, void* work, unsigned long long* words, hipStream_t s)
{
    if (t.width == 8)
        return range_pairs(static_cast<const unsigned long long*>(keys), perm, head, rRows, t, sRows, sRowBase, to, work, words, s);
    return range_pairs(static_cast<const uint32_t*>(keys), perm, head, rRows, t, sRows, sRowBase, to, work, words, s);
}

// ---- the host twins: sort_key and the sort's order around std::lower_bound / std::upper_bound --------------------
void range_index_host(const SortCols& col, uint64_t nRows, uint32_t* perm, void* keys, uint32_t head[4])
{
    const uint32_t kb = col.width[0] == 8 ? 8u : 4u;
    sort_rows_host(col, 1, nRows, perm);
    uint32_t nulls = 0, nans = 0;
    for (uint64_t q = 0; q < nRows; ++q) {
        const uint32_t row = perm[q];
        const uint64_t key = sort_key(col.type[0], col.width[0], 0u, col_elem(col.p[0], col.width[0], row));
        const bool isNull = col.valid[0] && !valid_bit(col.valid[0], row);
        const bool isNan = !isNull && col.type[0] == kValFloat && key == (col.width[0] == 4u ? 0xFFFFFFFFull : ~0ull);
        nulls += isNull; nans += isNan;
        if (kb == 8) static_cast<unsigned long long*>(keys)[q] = isNull ? 0ull : key;
        else static_cast<uint32_t*>(keys)[q] = isNull ? 0u : (uint32_t)key;
    }
    head[0] = (uint32_t)nRows - nulls - nans; head[1] = nulls; head[2] = nans; head[3] = kb;
}

namespace {
template <class K>
void range_pairs_on_host(const K* keys, const uint32_t* perm, uint32_t n, const RangeTerm& t, uint32_t sRows, uint32_t sRowBase, const PairSink& to,
                         uint64_t info[8])
{
    const uint64_t nanKey = t.width == 4u ? 0xFFFFFFFFull : ~0ull;
    uint64_t total = 0, matched = 0, bad = 0;
    for (uint32_t i = 0; i < sRows; ++i) {
        bool ok = true;
        uint32_t a = 0, b = n;
        if (t.lo) {
            const uint64_t key = sort_key(t.type, t.width, 0u, col_elem(t.lo, t.width, i));
            ok = ok && !(t.loValid && !valid_bit(t.loValid, i)) && !(t.type == kValFloat && key == nanKey);
            a = (uint32_t)(((t.flags & kLoOpen) ? std::upper_bound(keys, keys + n, (K)key) : std::lower_bound(keys, keys + n, (K)key)) - keys);
        }
        if (t.hi) {
            const uint64_t key = sort_key(t.type, t.width, 0u, col_elem(t.hi, t.width, i));
            ok = ok && !(t.hiValid && !valid_bit(t.hiValid, i)) && !(t.type == kValFloat && key == nanKey);
            b = (uint32_t)(((t.flags & kHiOpen) ? std::lower_bound(keys, keys + n, (K)key) : std::upper_bound(keys, keys + n, (K)key)) - keys);
        }
        if (!ok) { ++bad; continue; }
        if (b <= a) continue;
        if (t.pick == kPickFirst) b = a + 1;
        if (t.pick == kPickLast) { a = (uint32_t)(std::lower_bound(keys, keys + n, keys[b - 1]) - keys); b = a + 1; }
        ++matched;
        if (to.sMarks) set_mark_bit(to.sMarks, i);
        for (uint32_t q = a; q < b; ++q) {
            if (to.rMarks) set_mark_bit(to.rMarks, perm[q]);
            if (total < to.out.capacity) { to.out.s[total] = sRowBase + i; to.out.r[total] = perm[q]; }
            ++total;
        }
    }
    if (info) {
        for (int k = 0; k < 8; ++k) info[k] = 0;
        info[0] = total; info[1] = total < to.out.capacity ? total : to.out.capacity; info[3] = matched; info[4] = bad; info[5] = n;
    }
}
}  // namespace

void range_pairs_host(const void* keys, const uint32_t* perm, const uint32_t* head, uint32_t rRows, const RangeTerm& t, uint32_t sRows,
                      uint32_t sRowBase, const PairSink& to, uint64_t info[8])
{
    const uint32_t n = head && rRows ? std::min(head[0], rRows) : 0u;
    if (t.width == 8) range_pairs_on_host(static_cast<const unsigned long long*>(keys), perm, n, t, sRows, sRowBase, to, info);
    else range_pairs_on_host(static_cast<const uint32_t*>(keys), perm, n, t, sRows, sRowBase, to, info);
}

}  // namespace hj
