// hj_frames.hip -- sliding window frames over the runs along a permutation for gfx950 (MI355X): hj_window_frames_dev /
// hj_window_frames_host. COUNT / SUM / MIN / MAX over ROWS BETWEEN lo AND hi around every position, either side unbounded,
// clamped to the position's partition: the moving sum, the rolling maximum, the centred window, the partition's total.
// A sliding MIN / MAX is no difference of prefixes, and a loop over the frame is O(W) with W up to 2^32. Instead every op
// is TWO segmented scans of hj_window.hip's kind and one combine (both sides bounded, W = hi - lo + 1; positions cut into
// blocks of W from position 0):
//   G[q] = op over [max(start(q), block start), q]     forward, heads = partition heads and every q with q mod W == 0
//   H[q] = op over [q, min(end(q), block end)]         backward, tails = partition tails and every q with q mod W == W - 1
// The clamped frame [L, R] of p is at most W long, so it touches at most two adjacent blocks:
//   L > R                  the identity
//   L / W == R / W         G[R] if L == start or L mod W == 0, else H[L] (then R is the partition's end)
//   otherwise              op(H[L], G[R])
// lo unbounded: no block heads, G[R]. hi unbounded: no block tails, H[L]. Both: G[end]. One code path for the four ops; COUNT
// and SUM take no prefix differences (not measured against this path). A scan that the flags make unnecessary is not run.
// Launches, all in stream order; no workgroup waits for another, no look-back, no flag, no atomic, plain vector stores:
//   once per call      k_win_heads (hj_window.hip) -> the head bytes; k_frm_summary: per chunk the last head, the first tail,
//                      the counts; k_frm_carry0: ONE workgroup scans them; k_frm_ends: end(p) to a plane, from the back
//   once per function  k_frm_values: the values gathered through dPerm into a position-indexed plane V (the ONLY scattered
//                      read), and per chunk the reduction behind its last head of G and in front of its first tail of H;
//                      k_frm_carry: ONE workgroup scans the two; k_frm_scan<false>: V -> G; k_frm_scan<true>: V -> H IN PLACE
//                      (a tile is read whole before it is written, by the one workgroup that owns it); k_frm_combine: start(p)
//                      scanned in registers, end(p) loaded, H[L] and G[R] loaded -- p shifted by a constant and clamped, so
//                      coalesced --, one scattered 8-byte store to out[row(p)].
// The functions of a call share V / H and G one after another: the workspace is 21 bytes per position whatever nFuncs.
// Tile geometry and scans: hj_window_impl.h.
#include "hj_window_impl.h"

#include <algorithm>
#include <vector>

namespace hj {
namespace {

// The chunk summaries, kWinMaxChunks entries each. Once per call:
//   head1   last partition head + 1, 0: none (as the chunk has it)      headIn  the same scanned: what comes into the chunk
//   tail    first tail, kNone: none (as the chunk has it)               tailIn  the same scanned from the back
//   parts, skips: the chunk's counts for the totals
// and per function, overwritten by the next:
//   flagF   the chunk holds a head of G (a partition's or a block's)    runF   the reduction behind its last one -> what comes in
//   flagB   the chunk holds a tail of H                                 runB   the reduction in front of its first one -> what comes in
struct FrmSums { uint32_t *head1, *headIn, *tail, *tailIn, *parts, *skips, *flagF, *flagB; unsigned long long *runF, *runB; };
constexpr size_t kFrmSumBytes = win_up((size_t)kWinMaxChunks * (8 * sizeof(uint32_t) + 2 * sizeof(unsigned long long)));

// a function as the kernels take it; block: W clamped to 2^32 - 1 (above every position: one block), 0: no blocks
struct FrmFn { const void* src; const uint32_t* valid; unsigned long long* out; long long lo, hi; uint32_t op, width, sgn, unbLo, unbHi, block; };

__global__ void __launch_bounds__(kWinThreads)
k_frm_summary(uint64_t nPos, const uint8_t* __restrict__ heads, uint32_t chunkPos, FrmSums sums)
{
    __shared__ uint32_t lds32[kWinWaves];
    const uint64_t begin = (uint64_t)blockIdx.x * chunkPos;
    const uint64_t end = nPos - begin < chunkPos ? nPos : begin + chunkPos;
    uint32_t parts = 0, skips = 0, head1 = 0, tail = kNone;
    for (uint64_t p = begin + threadIdx.x; p < end; p += kWinThreads) {
        const uint32_t hb = heads[p];
        const bool in = !(hb & kHeadSkip);
        skips += !in;
        parts += in && (hb & kHeadPart);
        if (hb & kHeadPart) head1 = (uint32_t)p + 1;                   // p rises: the last one stays
        if (tail == kNone && win_tail(heads, p, nPos)) tail = (uint32_t)p;
    }
    const auto add = [](uint32_t a, uint32_t b) { return a + b; };
    const auto hi = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    const auto lo = [](uint32_t a, uint32_t b) { return a < b ? a : b; };
    parts = block_reduce(parts, add, lds32);
    skips = block_reduce(skips, add, lds32);
    head1 = block_reduce(head1, hi, lds32);
    tail = block_reduce(tail, lo, lds32);
    if (threadIdx.x == 0) {
        sums.parts[blockIdx.x] = parts; sums.skips[blockIdx.x] = skips;
        sums.head1[blockIdx.x] = sums.headIn[blockIdx.x] = head1;
        sums.tail[blockIdx.x] = sums.tailIn[blockIdx.x] = tail;
    }
}

__global__ void __launch_bounds__(kWinThreads)
k_frm_carry0(FrmSums sums, uint32_t chunks, unsigned long long* __restrict__ totals)
{
    __shared__ unsigned long long ldsV[kWinWaves];
    __shared__ uint32_t ldsF[kWinWaves];
    unsigned long long parts = 0, skips = 0;
    for (uint32_t c = threadIdx.x; c < chunks; c += kWinThreads) { parts += sums.parts[c]; skips += sums.skips[c]; }
    const auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
    parts = block_reduce(parts, add, ldsV);
    skips = block_reduce(skips, add, ldsV);
    if (threadIdx.x == 0) { totals[0] = parts; totals[1] = 0; totals[2] = skips; }
    carry_scan<uint32_t, false>(sums.headIn, nullptr, chunks, kAggMax, 0u, ldsV, ldsF);
    carry_scan<uint32_t, true>(sums.tailIn, nullptr, chunks, kAggMin, 0u, ldsV, ldsF);
}

// ends[p] = end(p): the chunk's tiles from the last down, position begin + len - 1 - j at scan index j (k_win_ends' shape)
__global__ void __launch_bounds__(kWinThreads)
k_frm_ends(const uint8_t* __restrict__ heads, uint64_t nPos, uint32_t chunkPos, FrmSums sums, uint32_t* __restrict__ ends)
{
    __shared__ unsigned long long ldsV[kWinWaves];
    __shared__ uint32_t ldsF[kWinWaves];
    const uint64_t begin = (uint64_t)blockIdx.x * chunkPos;
    const uint32_t len = nPos - begin < chunkPos ? (uint32_t)(nPos - begin) : chunkPos;
    const uint32_t at = (threadIdx.x >> 6) * kWinWaveSpan + (threadIdx.x & 63);
    uint32_t carry = sums.tailIn[blockIdx.x];
    for (uint32_t tb = 0; tb < len; tb += kWinTile) {
        uint32_t f[kWinPer], v[kWinPer];
#pragma unroll
        for (int k = 0; k < kWinPer; ++k) {
            const uint32_t j = tb + at + (uint32_t)k * 64;
            const uint64_t p = begin + (len - 1 - (j < len ? j : len - 1));
            v[k] = (uint32_t)p;
            f[k] = j < len && win_tail(heads, p, nPos);
        }
        tile_seg_scan<uint32_t>(kAggMax, 0u, f, v, carry, ldsV, ldsF);
#pragma unroll
        for (int k = 0; k < kWinPer; ++k) {
            const uint32_t j = tb + at + (uint32_t)k * 64;
            if (j < len) ends[begin + (len - 1 - j)] = v[k];
        }
    }
}

// vals[p] = what row(p) brings to the op (the identity for a skipped entry), and the chunk's two reductions
__global__ void __launch_bounds__(kWinThreads)
k_frm_values(const uint32_t* __restrict__ perm, uint64_t nPos, uint32_t nRows, FrmFn fn, uint32_t chunkPos, FrmSums sums,
             unsigned long long* __restrict__ vals)
{
    __shared__ unsigned long long lds64[kWinWaves];
    const uint64_t begin = (uint64_t)blockIdx.x * chunkPos;
    const uint64_t end = nPos - begin < chunkPos ? nPos : begin + chunkPos;
    const uint32_t head1 = sums.head1[blockIdx.x], tail = sums.tail[blockIdx.x], W = fn.block;
    // G's last head in the chunk (none: the whole chunk reaches into the next), H's first tail (none: the whole chunk
    // reaches into the one in front)
    uint64_t from = head1 ? (uint64_t)head1 - 1 : begin, to = tail != kNone ? (uint64_t)tail : end - 1;
    uint32_t hasF = head1 != 0, hasB = tail != kNone;
    if (W) {
        const uint64_t lastHead = (end - 1) / W * W, firstTail = begin / W * W + (W - 1);
        if (lastHead >= begin) { hasF = 1; from = lastHead > from ? lastHead : from; }
        if (firstTail < end) { hasB = 1; to = firstTail < to ? firstTail : to; }
    }
    const uint32_t op = fn.op, sgn = fn.sgn, width = fn.width;
    const unsigned long long id = agg_identity<unsigned long long>(op, sgn);
    unsigned long long accF = id, accB = id;
    // four positions a turn: their rows first, then their values -- four scattered loads in flight per lane
    for (uint64_t p0 = begin + threadIdx.x; p0 < end; p0 += 4 * kWinThreads) {
        uint32_t row[4];
        unsigned long long v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t p = p0 + (uint64_t)k * kWinThreads;
            row[k] = p >= end ? kNoRow : perm ? perm[p] : (uint32_t)p;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = row[k] < nRows ? win_value(fn.src, fn.valid, op, width, sgn, row[k]) : id;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t p = p0 + (uint64_t)k * kWinThreads;
            if (p >= end) continue;
            vals[p] = v[k];
            if (p >= from) accF = win_op<unsigned long long>(op, sgn, accF, v[k]);
            if (p <= to) accB = win_op<unsigned long long>(op, sgn, accB, v[k]);
        }
    }
    const auto comb = [=](unsigned long long a, unsigned long long b) { return win_op<unsigned long long>(op, sgn, a, b); };
    accF = block_reduce(accF, comb, lds64);
    accB = block_reduce(accB, comb, lds64);
    if (threadIdx.x == 0) {
        sums.runF[blockIdx.x] = accF; sums.runB[blockIdx.x] = accB;
        sums.flagF[blockIdx.x] = hasF; sums.flagB[blockIdx.x] = hasB;
    }
}

__global__ void __launch_bounds__(kWinThreads)
k_frm_carry(FrmSums sums, uint32_t chunks, uint32_t op, uint32_t sgn)
{
    __shared__ unsigned long long ldsV[kWinWaves];
    __shared__ uint32_t ldsF[kWinWaves];
    carry_scan<unsigned long long, false>(sums.runF, sums.flagF, chunks, op, sgn, ldsV, ldsF);
    carry_scan<unsigned long long, true>(sums.runB, sums.flagB, chunks, op, sgn, ldsV, ldsF);
}

// out[p] = G[p] (REV false: the chunk's tiles upwards) or H[p] (REV true: from the last tile down, position begin + len - 1
// - j at scan index j). in == out is allowed: a tile is loaded whole before its first store. W: the block, 0 for none.
template <bool REV>
__global__ void __launch_bounds__(kWinThreads)
k_frm_scan(const uint8_t* __restrict__ heads, uint64_t nPos, uint32_t chunkPos, uint32_t W, uint32_t op, uint32_t sgn,
           const unsigned long long* __restrict__ carryIn, const unsigned long long* in, unsigned long long* out)
{
    __shared__ unsigned long long ldsV[kWinWaves];
    __shared__ uint32_t ldsF[kWinWaves];
    const uint64_t begin = (uint64_t)blockIdx.x * chunkPos;
    const uint32_t len = nPos - begin < chunkPos ? (uint32_t)(nPos - begin) : chunkPos;
    const uint32_t at = (threadIdx.x >> 6) * kWinWaveSpan + (threadIdx.x & 63);
    const unsigned long long id = agg_identity<unsigned long long>(op, sgn);
    unsigned long long carry = carryIn[blockIdx.x];
    for (uint32_t tb = 0; tb < len; tb += kWinTile) {
        uint32_t f[kWinPer];
        unsigned long long v[kWinPer];
#pragma unroll
        for (int k = 0; k < kWinPer; ++k) {
            const uint32_t j = tb + at + (uint32_t)k * 64;
            const bool live = j < len;
            const uint64_t p = begin + (REV ? len - 1 - (live ? j : len - 1) : (live ? j : 0u));
            const uint32_t p32 = (uint32_t)p;
            v[k] = live ? in[p] : id;
            bool h = REV ? win_tail(heads, p, nPos) : (heads[p] & kHeadPart) != 0;
            if (W) h = h || p32 % W == (REV ? W - 1 : 0u);
            f[k] = live && h;
        }
        tile_seg_scan<unsigned long long>(op, sgn, f, v, carry, ldsV, ldsF);    // its first barrier stands behind every load
#pragma unroll
        for (int k = 0; k < kWinPer; ++k) {
            const uint32_t j = tb + at + (uint32_t)k * 64;
            if (j < len) out[begin + (REV ? len - 1 - j : j)] = v[k];
        }
    }
}

__global__ void __launch_bounds__(kWinThreads)
k_frm_combine(const uint32_t* __restrict__ perm, uint64_t nPos, uint32_t nRows, const uint8_t* __restrict__ heads, const uint32_t* __restrict__ ends,
              FrmFn fn, uint32_t chunkPos, FrmSums sums, const unsigned long long* __restrict__ G, const unsigned long long* __restrict__ H)
{
    __shared__ unsigned long long ldsV[kWinWaves];
    __shared__ uint32_t ldsF[kWinWaves];
    const uint64_t begin = (uint64_t)blockIdx.x * chunkPos;
    const uint32_t len = nPos - begin < chunkPos ? (uint32_t)(nPos - begin) : chunkPos;
    const uint32_t at = (threadIdx.x >> 6) * kWinWaveSpan + (threadIdx.x & 63);
    const uint32_t op = fn.op, sgn = fn.sgn, W = fn.block;
    const bool unbLo = fn.unbLo, unbHi = fn.unbHi;
    const long long lo = fn.lo, hi = fn.hi, last = (long long)nPos - 1;
    const unsigned long long id = agg_identity<unsigned long long>(op, sgn);
    uint32_t cStart = sums.headIn[blockIdx.x] - 1u;                     // chunk 0: 0 - 1 = the identity of MIN
    for (uint32_t tb = 0; tb < len; tb += kWinTile) {
        uint32_t row[kWinPer], st[kWinPer], en[kWinPer], f[kWinPer];
        bool ok[kWinPer];                                               // a position of the call whose entry is a row
#pragma unroll
        for (int k = 0; k < kWinPer; ++k) {
            const uint32_t q = tb + at + (uint32_t)k * 64;
            const bool live = q < len;
            const uint64_t p = begin + q;
            const uint32_t hb = live ? heads[p] : 0u;
            row[k] = !live ? kNoRow : perm ? perm[p] : (uint32_t)p;
            ok[k] = live && !(hb & kHeadSkip);
            st[k] = (uint32_t)p;
            en[k] = ok[k] ? ends[p] : (uint32_t)p;
            f[k] = hb & kHeadPart;
        }
        tile_seg_scan<uint32_t>(kAggMin, 0u, f, st, cStart, ldsV, ldsF);
#pragma unroll
        for (int k = 0; k < kWinPer; ++k) {
            if (!ok[k]) continue;
            const long long p = (long long)(begin + tb + at + (uint32_t)k * 64), s = st[k], e = en[k];
            // |lo|, |hi| < 2^32 and p < 2^32: nothing wraps in 64 bits. L and R lie in [start, end] wherever they are used,
            // and no load leaves the planes whatever a scan gave (clamped to [0, nPos - 1])
            long long L = unbLo ? s : (p + lo > s ? p + lo : s), R = unbHi ? e : (p + hi < e ? p + hi : e);
            unsigned long long r = id;
            if (L <= R) {
                L = L < 0 ? 0 : L > last ? last : L;
                R = R < 0 ? 0 : R > last ? last : R;
                if (unbLo) r = G[R];
                else if (unbHi) r = H[L];
                else {
                    const uint32_t l32 = (uint32_t)L, r32 = (uint32_t)R;
                    const uint32_t bl = l32 / W, br = r32 / W;
                    if (bl == br) r = (L == s || l32 - bl * W == 0) ? G[R] : H[L];
                    else r = win_op<unsigned long long>(op, sgn, H[L], G[R]);
                }
            }
            fn.out[row[k]] = r;
        }
    }
}

FrmFn frm_fn(const FrameFunc& f)
{
    FrmFn k{};
    k.src = f.src; k.valid = f.valid; k.out = static_cast<unsigned long long*>(f.out);
    k.lo = f.lo; k.hi = f.hi; k.op = f.op; k.width = f.width; k.sgn = f.sgn; k.unbLo = f.unbLo; k.unbHi = f.unbHi;
    k.block = 0;
    if (!f.unbLo && !f.unbHi) {
        const unsigned long long W = (unsigned long long)(f.hi - f.lo) + 1;                    // 1 .. 2^33 - 1
        k.block = W > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)W;                               // above every position: one block
    }
    return k;
}

}  // namespace

FramesLayout frames_layout(uint64_t nPos)
{
    FramesLayout l{};
    const WindowLayout w = window_layout(nPos);
    l.tilePos = w.tilePos; l.chunkPos = w.chunkPos; l.chunks = w.chunks;
    l.headBytes = win_up(nPos);
    l.endBytes = win_up(nPos * sizeof(uint32_t));
    l.planeBytes = win_up(nPos * sizeof(unsigned long long));
    l.sumBytes = kFrmSumBytes;
    l.bytes = l.headBytes + l.endBytes + 2 * l.planeBytes + l.sumBytes;
    return l;
}

hipError_t launch_window_frames(const uint32_t* perm, uint64_t nPos, uint32_t nRows, const uint32_t* part, const FrameFunc* funcs, uint32_t nFuncs,
                                void* work, unsigned long long* totals, hipStream_t s)
{
    if (nPos == 0) return hipSuccess;
    const FramesLayout l = frames_layout(nPos);
    char* p = static_cast<char*>(work);
    uint8_t* const heads = reinterpret_cast<uint8_t*>(p);
    uint32_t* const ends = reinterpret_cast<uint32_t*>(p + l.headBytes);
    unsigned long long* const V = reinterpret_cast<unsigned long long*>(p + l.headBytes + l.endBytes);     // becomes H
    unsigned long long* const G = reinterpret_cast<unsigned long long*>(p + l.headBytes + l.endBytes + l.planeBytes);
    uint32_t* const w32 = reinterpret_cast<uint32_t*>(p + l.headBytes + l.endBytes + 2 * l.planeBytes);
    FrmSums sums{};
    sums.head1 = w32; sums.headIn = w32 + kWinMaxChunks; sums.tail = w32 + 2 * kWinMaxChunks; sums.tailIn = w32 + 3 * kWinMaxChunks;
    sums.parts = w32 + 4 * kWinMaxChunks; sums.skips = w32 + 5 * kWinMaxChunks; sums.flagF = w32 + 6 * kWinMaxChunks; sums.flagB = w32 + 7 * kWinMaxChunks;
    sums.runF = reinterpret_cast<unsigned long long*>(w32 + 8 * kWinMaxChunks);
    sums.runB = sums.runF + kWinMaxChunks;
    const dim3 grid(l.chunks), block(kWinThreads);
    launch_window_heads(perm, nPos, nRows, part, SortCols{}, 0, heads, s);
    hipLaunchKernelGGL(k_frm_summary, grid, block, 0, s, nPos, heads, l.chunkPos, sums);
    hipLaunchKernelGGL(k_frm_carry0, dim3(1), block, 0, s, sums, l.chunks, totals);
    hipLaunchKernelGGL(k_frm_ends, grid, block, 0, s, heads, nPos, l.chunkPos, sums, ends);
    for (uint32_t i = 0; i < nFuncs; ++i) {
        const FrmFn fn = frm_fn(funcs[i]);
        const bool needH = !fn.unbLo, needG = fn.unbLo || !fn.unbHi;
        hipLaunchKernelGGL(k_frm_values, grid, block, 0, s, perm, nPos, nRows, fn, l.chunkPos, sums, V);
        hipLaunchKernelGGL(k_frm_carry, dim3(1), block, 0, s, sums, l.chunks, fn.op, fn.sgn);
        if (needG) hipLaunchKernelGGL(k_frm_scan<false>, grid, block, 0, s, heads, nPos, l.chunkPos, fn.block, fn.op, fn.sgn, sums.runF, V, G);
        if (needH) hipLaunchKernelGGL(k_frm_scan<true>, grid, block, 0, s, heads, nPos, l.chunkPos, fn.block, fn.op, fn.sgn, sums.runB, V, V);
        hipLaunchKernelGGL(k_frm_combine, grid, block, 0, s, perm, nPos, nRows, heads, ends, fn, l.chunkPos, sums, G, V);
    }
    return hipGetLastError();
}

// Another algorithm on purpose: per function one pass in which both ends of the frame only move up inside a partition.
// COUNT / SUM: a running window -- add the entering element, subtract the leaving one, modulo 2^64. MIN / MAX: a monotonic
// deque of positions whose front is the frame's extreme. O(nPos) per function whatever W; no blocks, no scans.
void window_frames_host(const uint32_t* perm, uint64_t nPos, uint32_t nRows, const uint32_t* part, const FrameFunc* funcs, uint32_t nFuncs,
                        uint64_t totals[3])
{
    totals[0] = totals[1] = totals[2] = 0;
    if (nPos == 0) return;
    std::vector<uint8_t> heads(nPos);
    for (uint64_t p = 0; p < nPos; ++p) {
        const uint32_t hb = heads[p] = (uint8_t)win_head(perm, p, nRows, part, SortCols{}, 0);
        if (hb & kHeadSkip) ++totals[2];
        else totals[0] += (hb & kHeadPart) ? 1 : 0;
    }
    const auto row_at = [&](uint64_t q) { return perm ? perm[q] : (uint32_t)q; };
    std::vector<unsigned long long> vals(nPos);
    std::vector<uint64_t> deque(nPos);                                  // positions; [front, back) is live
    for (uint32_t i = 0; i < nFuncs; ++i) {
        const FrameFunc& f = funcs[i];
        const unsigned long long id = agg_identity<unsigned long long>(f.op, f.sgn);
        const bool sums = f.op <= kAggSum;
        unsigned long long* const out = static_cast<unsigned long long*>(f.out);
        for (uint64_t p = 0; p < nPos; ++p)
            vals[p] = (heads[p] & kHeadSkip) ? id : win_value(f.src, f.valid, f.op, f.width, f.sgn, row_at(p));
        for (uint64_t s = 0; s < nPos;) {
            uint64_t e = s;                                             // the partition [s, e]
            while (e + 1 < nPos && !(heads[e + 1] & kHeadPart)) ++e;
            if (!(heads[s] & kHeadSkip)) {
                const long long ls = (long long)s, le = (long long)e;
                // the frame of p is [a, b): a = clamp(p + lo), b = clamp(p + hi + 1), both into [s, e + 1], both rising with p
                long long a = ls, b = ls;
                unsigned long long acc = 0;
                size_t front = 0, back = 0;
                for (long long p = ls; p <= le; ++p) {
                    const long long wantB = f.unbHi ? le + 1 : std::min(std::max(p + f.hi + 1, ls), le + 1);
                    const long long wantA = f.unbLo ? ls : std::min(std::max(p + f.lo, ls), le + 1);
                    for (; b < wantB; ++b) {                            // b enters, unless a has passed it already (a frame ahead of p)
                        if (sums) { if (b >= a) acc += vals[b]; continue; }
                        while (back > front && win_op<unsigned long long>(f.op, f.sgn, vals[deque[back - 1]], vals[b]) == vals[b]) --back;
                        deque[back++] = (uint64_t)b;
                    }
                    for (; a < wantA; ++a)                              // a leaves, if it ever entered
                        if (sums && a < b) acc -= vals[a];
                    unsigned long long r = id;
                    if (a < b) {
                        if (sums) r = acc;
                        else {
                            while (front < back && (long long)deque[front] < a) ++front;
                            r = vals[deque[front]];
                        }
                    }
                    out[row_at((uint64_t)p)] = r;
                }
            }
            s = e + 1;
        }
    }
}

}  // namespace hj
