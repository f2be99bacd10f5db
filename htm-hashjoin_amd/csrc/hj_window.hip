// hj_window.hip -- window functions over the runs along a permutation for gfx950 (MI355X): hj_window_rows_dev /
// hj_window_rows_host (ROW_NUMBER, RANK, DENSE_RANK, the rows of the partition, LAG / LEAD / first / last row as gather
// maps, running COUNT / SUM / MIN / MAX). Everything is a SEGMENTED SCAN over positions: a pair (head seen, value) under
//   (fa, va) o (fb, vb) = (fa | fb, fb ? vb : op(va, vb)),
// which is associative for every op here (sum, min, max), so positions, tiles and chunks combine in any grouping:
//   start(p)     = segmented MIN of p over the partition heads        peerStart(p) = the same over the peer heads
//   dense(p)     = segmented SUM of the peer-head bits over the partition heads
//   end(p)       = segmented MAX of p over the partition TAILS, scanned from the last position down
//   RUN_*        = segmented op over the partition heads of the 64-bit values gathered through dPerm
// Five launches order the phases; no workgroup waits for another, there is no look-back, no flag and no atomic:
//   (heads)   k_win_heads: one byte per position -- partition head, peer head, skipped entry (win_head, hj_columns.h). The
//             only kernel that reads dPart and the order columns: two scattered rows per position.
//   (summary) k_win_summary: per chunk (window_layout) the last partition head, the last peer head, the first tail, the
//             counts for hj_window_rows_info, and behind the last head -- the only part of a chunk that reaches into the
//             next -- the peer heads and every RUN function's reduction. All ops commute, so this is a plain masked
//             reduction, and a chunk with many partitions reads values of its last one alone.
//   (carry)   k_win_carry: ONE workgroup scans the at most 4096 chunk summaries in place: what comes into each chunk.
//   (ends)    k_win_ends: end(p) to a plane of the workspace, every chunk from its last tile down. Only when PART_ROWS,
//             LEAD or LAST_ROW is asked for.
//   (apply)   k_win_apply: per tile the planes the functions need, scanned in registers, then every function of the call:
//             one scattered 4- or 8-byte store to out[row(p)] per function and position (coalesced with dPerm null).
// The tile geometry and the scans are hj_window_impl.h's, shared with the sliding frames of hj_frames.hip.
// A tile is 2048 positions: lane l of wavefront w holds, for k = 0..7, position 512 w + 64 k + l, so every load is
// coalesced whatever the alignment of dPerm, and scan order is (w, k, l). A wavefront scans its 8 rows with shuffles (DPP)
// one behind the other -- the row's last lane carries into the next --, one LDS step joins the four wavefronts
// (block_exclusive_scan's shape), and the tile's carry stays in a register.
#include "hj_window_impl.h"

#include <algorithm>
#include <vector>

namespace hj {
namespace {

constexpr uint32_t kNeedStart = 1u, kNeedPeer = 2u, kNeedDense = 4u, kNeedEnd = 8u;

// The chunk summaries, then (k_win_carry, in place) what comes into a chunk. kWinMaxChunks entries each.
//   head1  last partition head + 1, 0: none    -> start of the partition that reaches into the chunk (kNone: chunk 0)
//   peer1  the same of the peer heads          -> its peerStart
//   tail   first tail, kNone: none             -> the first tail behind the chunk (kNone: the last chunk)
//   dense  peer heads at and behind head1 - 1  -> the peer heads of the partition that reaches into the chunk so far
//   run[f] function f's reduction there        -> its accumulator so far
//   parts, peers, skips: the chunk's counts for the totals
struct WinSums { uint32_t *head1, *peer1, *tail, *dense, *parts, *peers, *skips; unsigned long long* run; };

__device__ __forceinline__ bool is_run(uint32_t op) { return op >= kWinRunCount; }

__global__ void __launch_bounds__(kWinThreads)
k_win_heads(const uint32_t* __restrict__ perm, uint64_t nPos, uint32_t nRows, const uint32_t* __restrict__ part, SortCols order, uint32_t nOrder,
            uint8_t* __restrict__ heads)
{
    const uint64_t base = (uint64_t)blockIdx.x * (kWinThreads * 4) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint64_t p = base + (uint64_t)k * kWinThreads;
        if (p >= nPos) break;
        heads[p] = (uint8_t)win_head(perm, p, nRows, part, order, nOrder);
    }
}

__global__ void __launch_bounds__(kWinThreads)
k_win_summary(const uint32_t* __restrict__ perm, uint64_t nPos, uint32_t nRows, const uint8_t* __restrict__ heads, WinFuncs fn, uint32_t nFuncs,
              uint32_t need, uint32_t chunkPos, WinSums sums)
{
    __shared__ uint32_t lds32[kWinWaves];
    __shared__ unsigned long long lds64[kWinWaves];
    const uint64_t begin = (uint64_t)blockIdx.x * chunkPos;
    const uint64_t end = nPos - begin < chunkPos ? nPos : begin + chunkPos;
    uint32_t parts = 0, peers = 0, skips = 0, head1 = 0, peer1 = 0, tail = kNone;
    for (uint64_t p = begin + threadIdx.x; p < end; p += kWinThreads) {
        const uint32_t hb = heads[p];
        const bool in = !(hb & kHeadSkip);
        skips += !in;
        parts += in && (hb & kHeadPart);
        peers += in && (hb & kHeadPeer);
        if (hb & kHeadPart) head1 = (uint32_t)p + 1;                   // p rises: the last one stays
        if (hb & kHeadPeer) peer1 = (uint32_t)p + 1;
        if (tail == kNone && win_tail(heads, p, nPos)) tail = (uint32_t)p;
    }
    const auto add = [](uint32_t a, uint32_t b) { return a + b; };
    const auto hi = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    const auto lo = [](uint32_t a, uint32_t b) { return a < b ? a : b; };
    parts = block_reduce(parts, add, lds32);
    peers = block_reduce(peers, add, lds32);
    skips = block_reduce(skips, add, lds32);
    head1 = block_reduce(head1, hi, lds32);
    peer1 = block_reduce(peer1, hi, lds32);
    tail = block_reduce(tail, lo, lds32);
    if (threadIdx.x == 0) {
        sums.parts[blockIdx.x] = parts; sums.peers[blockIdx.x] = peers; sums.skips[blockIdx.x] = skips;
        sums.head1[blockIdx.x] = head1; sums.peer1[blockIdx.x] = peer1; sums.tail[blockIdx.x] = tail;
    }
    // what reaches into the next chunk: the positions at and behind the last head (none: the whole chunk)
    const uint64_t from = head1 ? (uint64_t)head1 - 1 : begin;
    if (need & kNeedDense) {
        uint32_t d = 0;
        for (uint64_t p = from + threadIdx.x; p < end; p += kWinThreads) d += (heads[p] & kHeadPeer) ? 1u : 0u;
        d = block_reduce(d, add, lds32);
        if (threadIdx.x == 0) sums.dense[blockIdx.x] = d;
    }
    for (uint32_t f = 0; f < nFuncs; ++f) {
        if (!is_run(fn.op[f])) continue;
        const uint32_t op = fn.op[f] - kWinRunCount, sgn = fn.sgn[f], width = fn.width[f];
        unsigned long long acc = agg_identity<unsigned long long>(op, sgn);
        // four positions a turn: their rows first, then their values -- four scattered loads in flight per lane
        for (uint64_t p0 = from + threadIdx.x; p0 < end; p0 += 4 * kWinThreads) {
            uint32_t row[4];
            unsigned long long v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint64_t p = p0 + (uint64_t)k * kWinThreads;
                row[k] = p >= end ? kNoRow : perm ? perm[p] : (uint32_t)p;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = row[k] < nRows ? win_value(fn.src[f], fn.valid[f], op, width, sgn, row[k]) : agg_identity<unsigned long long>(op, sgn);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc = win_op<unsigned long long>(op, sgn, acc, v[k]);
        }
        acc = block_reduce(acc, [=](unsigned long long a, unsigned long long b) { return win_op<unsigned long long>(op, sgn, a, b); }, lds64);
        if (threadIdx.x == 0) sums.run[(size_t)f * kWinMaxChunks + blockIdx.x] = acc;
    }
}

__global__ void __launch_bounds__(kWinThreads)
k_win_carry(WinSums sums, uint32_t chunks, WinFuncs fn, uint32_t nFuncs, uint32_t need, unsigned long long* __restrict__ totals)
{
    __shared__ unsigned long long ldsV[kWinWaves];
    __shared__ uint32_t ldsF[kWinWaves];
    unsigned long long parts = 0, peers = 0, skips = 0;
    for (uint32_t c = threadIdx.x; c < chunks; c += kWinThreads) { parts += sums.parts[c]; peers += sums.peers[c]; skips += sums.skips[c]; }
    const auto add = [](unsigned long long a, unsigned long long b) { return a + b; };
    parts = block_reduce(parts, add, ldsV);
    peers = block_reduce(peers, add, ldsV);
    skips = block_reduce(skips, add, ldsV);
    if (threadIdx.x == 0) { totals[0] = parts; totals[1] = peers; totals[2] = skips; }
    if (need & kNeedDense) carry_scan<uint32_t, false>(sums.dense, sums.head1, chunks, kAggSum, 0u, ldsV, ldsF);
    for (uint32_t f = 0; f < nFuncs; ++f)
        if (is_run(fn.op[f]))
            carry_scan<unsigned long long, false>(sums.run + (size_t)f * kWinMaxChunks, sums.head1, chunks, fn.op[f] - kWinRunCount, fn.sgn[f], ldsV, ldsF);
    if (need & kNeedPeer) carry_scan<uint32_t, false>(sums.peer1, nullptr, chunks, kAggMax, 0u, ldsV, ldsF);
    if (need & kNeedEnd) carry_scan<uint32_t, true>(sums.tail, nullptr, chunks, kAggMin, 0u, ldsV, ldsF);
    carry_scan<uint32_t, false>(sums.head1, nullptr, chunks, kAggMax, 0u, ldsV, ldsF);
}

// ends[p] = end(p): the chunk's tiles from the last down, position begin + len - 1 - j at scan index j
__global__ void __launch_bounds__(kWinThreads)
k_win_ends(const uint8_t* __restrict__ heads, uint64_t nPos, uint32_t chunkPos, WinSums sums, uint32_t* __restrict__ ends)
{
    __shared__ unsigned long long ldsV[kWinWaves];
    __shared__ uint32_t ldsF[kWinWaves];
    const uint64_t begin = (uint64_t)blockIdx.x * chunkPos;
    const uint32_t len = nPos - begin < chunkPos ? (uint32_t)(nPos - begin) : chunkPos;
    const uint32_t at = (threadIdx.x >> 6) * kWinWaveSpan + (threadIdx.x & 63);
    uint32_t carry = sums.tail[blockIdx.x];
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

__global__ void __launch_bounds__(kWinThreads)
k_win_apply(const uint32_t* __restrict__ perm, uint64_t nPos, uint32_t nRows, const uint8_t* __restrict__ heads, const uint32_t* __restrict__ ends,
            WinFuncs fn, uint32_t nFuncs, uint32_t need, uint32_t chunkPos, WinSums sums)
{
    __shared__ unsigned long long ldsV[kWinWaves];
    __shared__ uint32_t ldsF[kWinWaves];
    __shared__ unsigned long long runCarry[kWinMaxFuncs];
    const uint64_t begin = (uint64_t)blockIdx.x * chunkPos;
    const uint32_t len = nPos - begin < chunkPos ? (uint32_t)(nPos - begin) : chunkPos;
    const uint32_t at = (threadIdx.x >> 6) * kWinWaveSpan + (threadIdx.x & 63);
    uint32_t cStart = sums.head1[blockIdx.x] - 1u;                      // chunk 0: 0 - 1 = the identity of MIN
    uint32_t cPeer = (need & kNeedPeer) ? sums.peer1[blockIdx.x] - 1u : 0u;
    uint32_t cDense = (need & kNeedDense) ? sums.dense[blockIdx.x] : 0u;
    if (threadIdx.x < nFuncs) runCarry[threadIdx.x] = is_run(fn.op[threadIdx.x]) ? sums.run[(size_t)threadIdx.x * kWinMaxChunks + blockIdx.x] : 0ull;
    __syncthreads();

    for (uint32_t tb = 0; tb < len; tb += kWinTile) {
        uint32_t row[kWinPer], hb[kWinPer], pos[kWinPer];
        bool ok[kWinPer];                                               // a position of the call whose entry is a row
#pragma unroll
        for (int k = 0; k < kWinPer; ++k) {
            const uint32_t q = tb + at + (uint32_t)k * 64;
            const bool live = q < len;
            const uint64_t p = begin + q;
            pos[k] = (uint32_t)p;
            hb[k] = live ? heads[p] : 0u;
            row[k] = !live ? kNoRow : perm ? perm[p] : (uint32_t)p;
            ok[k] = live && !(hb[k] & kHeadSkip);
        }
        uint32_t st[kWinPer], ps[kWinPer], dn[kWinPer], en[kWinPer], f[kWinPer];
#pragma unroll
        for (int k = 0; k < kWinPer; ++k) { st[k] = ps[k] = en[k] = pos[k]; dn[k] = 0; }
        if (need & kNeedStart) {
#pragma unroll
            for (int k = 0; k < kWinPer; ++k) f[k] = hb[k] & kHeadPart;
            tile_seg_scan<uint32_t>(kAggMin, 0u, f, st, cStart, ldsV, ldsF);
        }
        if (need & kNeedPeer) {
#pragma unroll
            for (int k = 0; k < kWinPer; ++k) f[k] = hb[k] & kHeadPeer;
            tile_seg_scan<uint32_t>(kAggMin, 0u, f, ps, cPeer, ldsV, ldsF);
        }
        if (need & kNeedDense) {
#pragma unroll
            for (int k = 0; k < kWinPer; ++k) { f[k] = hb[k] & kHeadPart; dn[k] = (hb[k] & kHeadPeer) ? 1u : 0u; }
            tile_seg_scan<uint32_t>(kAggSum, 0u, f, dn, cDense, ldsV, ldsF);
        }
        if (need & kNeedEnd) {
#pragma unroll
            for (int k = 0; k < kWinPer; ++k) if (ok[k]) en[k] = ends[begin + tb + at + (uint32_t)k * 64];
        }
        for (uint32_t i = 0; i < nFuncs; ++i) {
            const uint32_t op = fn.op[i];
            if (is_run(op)) {
                const uint32_t aop = op - kWinRunCount, sgn = fn.sgn[i], width = fn.width[i];
                unsigned long long v[kWinPer];
#pragma unroll
                for (int k = 0; k < kWinPer; ++k) {
                    f[k] = hb[k] & kHeadPart;
                    v[k] = ok[k] ? win_value(fn.src[i], fn.valid[i], aop, width, sgn, row[k]) : agg_identity<unsigned long long>(aop, sgn);
                }
                unsigned long long carry = runCarry[i];
                tile_seg_scan<unsigned long long>(aop, sgn, f, v, carry, ldsV, ldsF);
                if (threadIdx.x == 0) runCarry[i] = carry;              // read again behind the barrier that ends the tile
                unsigned long long* const out = static_cast<unsigned long long*>(fn.out[i]);
#pragma unroll
                for (int k = 0; k < kWinPer; ++k) if (ok[k]) out[row[k]] = v[k];
                continue;
            }
            const uint32_t off = fn.offset[i];
            uint32_t* const out = static_cast<uint32_t*>(fn.out[i]);
            // the row at position q of the partition; q lies in [start, end], and no load leaves dPerm whatever a scan gave
            const auto at_pos = [&](uint32_t q) { return q >= nPos ? kNoRow : perm ? perm[q] : q; };
#pragma unroll
            for (int k = 0; k < kWinPer; ++k) {
                if (!ok[k]) continue;
                uint32_t r;
                switch (op) {
                    case kWinRowNumber: r = pos[k] - st[k] + 1u; break;
                    case kWinRank: r = ps[k] - st[k] + 1u; break;
                    case kWinDenseRank: r = dn[k]; break;
                    case kWinPartRows: r = en[k] - st[k] + 1u; break;
                    case kWinLag: r = off > pos[k] - st[k] ? kNoRow : at_pos(pos[k] - off); break;
                    case kWinLead: r = off > en[k] - pos[k] ? kNoRow : at_pos(pos[k] + off); break;
                    case kWinFirstRow: r = at_pos(st[k]); break;
                    default: r = at_pos(en[k]); break;                  // kWinLastRow
                }
                out[row[k]] = r;
            }
        }
        __syncthreads();
    }
}

uint32_t window_need(const WinFuncs& fn, uint32_t nFuncs)
{
    uint32_t need = 0;
    for (uint32_t i = 0; i < nFuncs; ++i) {
        switch (fn.op[i]) {
            case kWinRowNumber: case kWinLag: case kWinFirstRow: need |= kNeedStart; break;
            case kWinRank: need |= kNeedStart | kNeedPeer; break;
            case kWinDenseRank: need |= kNeedDense; break;
            case kWinPartRows: need |= kNeedStart | kNeedEnd; break;
            case kWinLead: case kWinLastRow: need |= kNeedEnd; break;
            default: break;
        }
    }
    return need;
}

// seven 32-bit planes and one of padding, so that the 64-bit planes behind them are aligned
constexpr size_t kWinSumBytes = win_up((size_t)kWinMaxChunks * (8 * sizeof(uint32_t) + kWinMaxFuncs * sizeof(unsigned long long)));

}  // namespace

WindowLayout window_layout(uint64_t nPos)
{
    WindowLayout l{};
    const uint64_t tiles = (nPos + kWinTile - 1) / kWinTile;
    const uint64_t perChunk = std::max<uint64_t>(kWinMinTiles, (tiles + kWinMaxChunks - 1) / kWinMaxChunks);
    l.tilePos = kWinTile;
    l.chunkPos = (uint32_t)(perChunk * kWinTile);                  // 2^32 positions: 512 tiles, 2^20 positions
    l.chunks = (uint32_t)((nPos + l.chunkPos - 1) / l.chunkPos);   // <= kWinMaxChunks
    l.headBytes = win_up(nPos);
    l.endBytes = win_up(nPos * sizeof(uint32_t));
    l.sumBytes = kWinSumBytes;
    l.bytes = l.headBytes + l.endBytes + l.sumBytes;
    return l;
}

void launch_window_heads(const uint32_t* perm, uint64_t nPos, uint32_t nRows, const uint32_t* part, const SortCols& order, uint32_t nOrder,
                         uint8_t* heads, hipStream_t s)
{
    const unsigned headBlocks = (unsigned)((nPos + kWinThreads * 4 - 1) / (kWinThreads * 4));
    hipLaunchKernelGGL(k_win_heads, dim3(headBlocks), dim3(kWinThreads), 0, s, perm, nPos, nRows, part, order, nOrder, heads);
}

hipError_t launch_window_rows(const uint32_t* perm, uint64_t nPos, uint32_t nRows, const uint32_t* part, const SortCols& order, uint32_t nOrder,
                              const WinFuncs& funcs, uint32_t nFuncs, void* work, unsigned long long* totals, hipStream_t s)
{
    if (nPos == 0) return hipSuccess;
    const WindowLayout l = window_layout(nPos);
    char* p = static_cast<char*>(work);
    uint8_t* const heads = reinterpret_cast<uint8_t*>(p);
    uint32_t* const ends = reinterpret_cast<uint32_t*>(p + l.headBytes);
    uint32_t* const w32 = reinterpret_cast<uint32_t*>(p + l.headBytes + l.endBytes);
    WinSums sums{};
    sums.head1 = w32; sums.peer1 = w32 + kWinMaxChunks; sums.tail = w32 + 2 * kWinMaxChunks; sums.dense = w32 + 3 * kWinMaxChunks;
    sums.parts = w32 + 4 * kWinMaxChunks; sums.peers = w32 + 5 * kWinMaxChunks; sums.skips = w32 + 6 * kWinMaxChunks;
    sums.run = reinterpret_cast<unsigned long long*>(w32 + 8 * kWinMaxChunks);      // 8-byte aligned: an even number of planes in front
    const uint32_t need = window_need(funcs, nFuncs);
    const unsigned headBlocks = (unsigned)((nPos + kWinThreads * 4 - 1) / (kWinThreads * 4));
    hipLaunchKernelGGL(k_win_heads, dim3(headBlocks), dim3(kWinThreads), 0, s, perm, nPos, nRows, part, order, nOrder, heads);
    hipLaunchKernelGGL(k_win_summary, dim3(l.chunks), dim3(kWinThreads), 0, s, perm, nPos, nRows, heads, funcs, nFuncs, need, l.chunkPos, sums);
    hipLaunchKernelGGL(k_win_carry, dim3(1), dim3(kWinThreads), 0, s, sums, l.chunks, funcs, nFuncs, need, totals);
    if (need & kNeedEnd) hipLaunchKernelGGL(k_win_ends, dim3(l.chunks), dim3(kWinThreads), 0, s, heads, nPos, l.chunkPos, sums, ends);
    hipLaunchKernelGGL(k_win_apply, dim3(l.chunks), dim3(kWinThreads), 0, s, perm, nPos, nRows, heads, ends, funcs, nFuncs, need, l.chunkPos, sums);
    return hipGetLastError();
}

// The same in one sequential loop: win_head, win_value and win_op are the kernels' own. Positions run up for everything
// but end, which a second loop takes from the last position down.
void window_rows_host(const uint32_t* perm, uint64_t nPos, uint32_t nRows, const uint32_t* part, const SortCols& order, uint32_t nOrder,
                      const WinFuncs& fn, uint32_t nFuncs, uint64_t totals[3])
{
    totals[0] = totals[1] = totals[2] = 0;
    if (nPos == 0) return;
    std::vector<uint8_t> heads(nPos);
    std::vector<uint32_t> ends(nPos);
    for (uint64_t p = 0; p < nPos; ++p) {
        const uint32_t hb = heads[p] = (uint8_t)win_head(perm, p, nRows, part, order, nOrder);
        if (hb & kHeadSkip) ++totals[2];
        else { totals[0] += (hb & kHeadPart) ? 1 : 0; totals[1] += (hb & kHeadPeer) ? 1 : 0; }
    }
    uint32_t end = (uint32_t)(nPos - 1);
    for (uint64_t p = nPos; p-- > 0;) {
        if (p + 1 == nPos || (heads[p + 1] & kHeadPart)) end = (uint32_t)p;
        ends[p] = end;
    }
    const auto at = [&](uint32_t q) { return perm ? perm[q] : q; };
    uint32_t start = 0, peerStart = 0, dense = 0;
    unsigned long long acc[kWinMaxFuncs] = {};
    for (uint64_t p64 = 0; p64 < nPos; ++p64) {
        const uint32_t p = (uint32_t)p64, hb = heads[p];
        if (hb & kHeadPart) { start = p; dense = 0; }
        if (hb & kHeadPeer) { peerStart = p; ++dense; }
        const bool ok = !(hb & kHeadSkip);
        const uint32_t row = at(p);
        for (uint32_t i = 0; i < nFuncs; ++i) {
            const uint32_t op = fn.op[i];
            if (op >= kWinRunCount) {
                const uint32_t aop = op - kWinRunCount;
                if (hb & kHeadPart) acc[i] = agg_identity<unsigned long long>(aop, fn.sgn[i]);
                if (!ok) continue;
                acc[i] = win_op<unsigned long long>(aop, fn.sgn[i], acc[i], win_value(fn.src[i], fn.valid[i], aop, fn.width[i], fn.sgn[i], row));
                static_cast<unsigned long long*>(fn.out[i])[row] = acc[i];
                continue;
            }
            if (!ok) continue;
            const uint32_t off = fn.offset[i];
            uint32_t r;
            switch (op) {
                case kWinRowNumber: r = p - start + 1u; break;
                case kWinRank: r = peerStart - start + 1u; break;
                case kWinDenseRank: r = dense; break;
                case kWinPartRows: r = ends[p] - start + 1u; break;
                case kWinLag: r = off > p - start ? kNoRow : at(p - off); break;
                case kWinLead: r = off > ends[p] - p ? kNoRow : at(p + off); break;
                case kWinFirstRow: r = at(start); break;
                default: r = at(ends[p]); break;
            }
            static_cast<uint32_t*>(fn.out[i])[row] = r;
        }
    }
}

}  // namespace hj
