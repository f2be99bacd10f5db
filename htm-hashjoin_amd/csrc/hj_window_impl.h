// hj_window_impl.h -- what the kernels of the window family share (hj_window.hip: hj_window_rows_dev; hj_frames.hip:
// hj_window_frames_dev): the tile geometry, the segmented scans of a wavefront and of a tile, the workgroup's reduction,
// the tail test on the head bytes and the one-workgroup scan of the chunk summaries. Device code in an unnamed namespace:
// every file that includes it compiles its own copy into its own kernels. Private to csrc/.
// A tile is 2048 positions: lane l of wavefront w holds, for k = 0..7, position 512 w + 64 k + l, so every load is
// coalesced whatever the alignment of the plane, and scan order is (w, k, l). A wavefront scans its 8 rows with shuffles
// (DPP) one behind the other -- the row's last lane carries into the next --, one LDS step joins the four wavefronts
// (block_exclusive_scan's shape), and the tile's carry stays in a register.
#pragma once

#include "hj_columns.h"

namespace hj {
namespace {

constexpr int kWinThreads = 256;                               // four wavefronts
constexpr int kWinPer = 8;                                     // positions per thread per tile
constexpr int kWinWaves = kWinThreads / 64;
constexpr uint32_t kWinTile = kWinThreads * kWinPer;           // 2048
constexpr uint32_t kWinWaveSpan = 64 * kWinPer;                // 512: what one wavefront holds of a tile
constexpr uint32_t kWinMinTiles = 2;                           // tiles per chunk at least: the tile loop runs at any size
constexpr uint32_t kWinMaxChunks = 4096;
constexpr uint32_t kNone = 0xFFFFFFFFu;

// inclusive segmented scan over the lanes of a wavefront
template <class T>
__device__ __forceinline__ void wave_seg_scan(uint32_t op, uint32_t sgn, uint32_t& f, T& v)
{
    const uint32_t lane = threadIdx.x & 63;
#pragma unroll
    for (uint32_t off = 1; off < 64; off <<= 1) {
        const uint32_t pf = __shfl_up(f, off, 64);
        const T pv = __shfl_up(v, off, 64);
        if (lane >= off) { if (!f) v = win_op<T>(op, sgn, pv, v); f |= pf; }
    }
}

// Inclusive segmented scan of a tile in place, scan order (wavefront, k, lane). carry: what comes into the tile -> what
// leaves it. ldsV / ldsF: kWinWaves words each. Two barriers; every thread of the workgroup calls it.
template <class T>
__device__ __forceinline__ void tile_seg_scan(uint32_t op, uint32_t sgn, uint32_t (&f)[kWinPer], T (&v)[kWinPer], T& carry,
                                              unsigned long long* ldsV, uint32_t* ldsF)
{
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t wf = 0;
    T wv = 0;
#pragma unroll
    for (int k = 0; k < kWinPer; ++k) {
        wave_seg_scan<T>(op, sgn, f[k], v[k]);
        if (k) { if (!f[k]) v[k] = win_op<T>(op, sgn, wv, v[k]); f[k] |= wf; }
        wf = __shfl(f[k], 63, 64);
        wv = __shfl(v[k], 63, 64);
    }
    if ((threadIdx.x & 63) == 0) { ldsF[wave] = wf; ldsV[wave] = (unsigned long long)wv; }
    __syncthreads();
    T pv = carry, all = carry;
#pragma unroll
    for (uint32_t w = 0; w < (uint32_t)kWinWaves; ++w) {
        const uint32_t sf = ldsF[w];
        const T sv = (T)ldsV[w];
        all = sf ? sv : win_op<T>(op, sgn, all, sv);
        if (w < wave) pv = all;
    }
#pragma unroll
    for (int k = 0; k < kWinPer; ++k) if (!f[k]) v[k] = win_op<T>(op, sgn, pv, v[k]);
    carry = all;
    __syncthreads();
}

// f(v of every thread), in every thread. lds: kWinWaves words. Two barriers.
template <class T, class F>
__device__ __forceinline__ T block_reduce(T v, F f, T* lds)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = f(v, __shfl_down(v, off, 64));       // lane 0 holds the wavefront's
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = lds[0];
#pragma unroll
    for (int w = 1; w < kWinWaves; ++w) r = f(r, lds[w]);
    __syncthreads();
    return r;
}

// tail(p): the partition of p ends at p
__device__ __forceinline__ bool win_tail(const uint8_t* __restrict__ heads, uint64_t p, uint64_t nPos)
{
    return p + 1 == nPos || (heads[p + 1] & kHeadPart);
}

// Exclusive segmented scan of data[0 .. chunks) in place by ONE workgroup: a thread walks its consecutive chunks, the
// threads' reductions are scanned, the thread walks again. head1: where a chunk holds a head (null: nowhere -- a plain
// scan). REV: from the last chunk down.
template <class T, bool REV>
__device__ __forceinline__ void carry_scan(T* __restrict__ data, const uint32_t* __restrict__ head1, uint32_t chunks, uint32_t op, uint32_t sgn,
                                           unsigned long long* ldsV, uint32_t* ldsF)
{
    const uint32_t per = (chunks + kWinThreads - 1) / kWinThreads;
    const uint32_t lo = threadIdx.x * per < chunks ? threadIdx.x * per : chunks, hi = lo + per < chunks ? lo + per : chunks;
    const T id = agg_identity<T>(op, sgn);
    uint32_t f = 0;
    T v = id;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t c = REV ? chunks - 1 - i : i;
        const bool h = head1 && head1[c];
        const T x = data[c];
        v = h ? x : win_op<T>(op, sgn, v, x);
        f |= h;
    }
    wave_seg_scan<T>(op, sgn, f, v);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 63) { ldsF[wave] = f; ldsV[wave] = (unsigned long long)v; }
    uint32_t ef = __shfl_up(f, 1, 64);
    T ev = __shfl_up(v, 1, 64);
    if (lane == 0) { ef = 0; ev = id; }
    __syncthreads();
    T pv = id;
    for (uint32_t w = 0; w < wave; ++w) pv = ldsF[w] ? (T)ldsV[w] : win_op<T>(op, sgn, pv, (T)ldsV[w]);
    T run = ef ? ev : win_op<T>(op, sgn, pv, ev);
    __syncthreads();
    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t c = REV ? chunks - 1 - i : i;
        const bool h = head1 && head1[c];
        const T x = data[c];
        data[c] = run;
        run = h ? x : win_op<T>(op, sgn, run, x);
    }
    __syncthreads();                                                    // head1 itself is scanned last: everybody has read it
}

// a plane's bytes, rounded up so that the plane behind it is aligned
constexpr size_t win_up(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace
}  // namespace hj
