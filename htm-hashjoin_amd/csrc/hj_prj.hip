// hj_prj.hip -- radix-partitioned join (PRJ path) for gfx950 (MI355X).
//
// What this replaces (paths relative to anilshanbhag/HTM-HashJoin, mc/src/):
//   k_radix_hist     the histogram loops of parallel_radix_partition (:586-589) and
//                    radix_cluster (:418-421)
//   (scan)           the prefix / cursor computation (:592-617, :423-430): launch_exclusive_scan_u32, hj_scan.hip
//   k_radix_scatter  the scatter loops (:622-626, :433-437), here staged through LDS so
//                    every partition's tuples leave the CU as contiguous runs
//   k_prj_join       bucket_chaining_join (:231-283) with the probe loop the fork
//                    commented out (:259-276) restored; the table lives in LDS (join_partition, the core it
//                    shares with k_prj_probe_items)
//   k_radix_scatter_frag  the same two passes WITHOUT the histogram loops (the default for large
//                    relations): private fragments per chunk and bin, capacity checked, the exact
//                    kernels above enqueued behind as a gated fallback (see "histogram-free partitioning")
// Orchestration (prj_thread :808-1122: 6 pthread barriers, 2 task queues) becomes
// stream order between kernels.
//
// Partition function: HASH_BIT_MODULO(key, MASK, R) = (key & MASK) >> R on the low
// 32 bits of the tuple (tuple_t.key), pass 1 on bits [0, bits1), pass 2 on
// [bits1, bits1+bits2), bits1 = radixBits/2 as in prj_thread :814-816. The final
// partition id is (pass-1 bin << bits2) | pass-2 bin, the same order the
// reference's task queues visit them in.
//
// Layout: a pass works on "segments" (pass 1: the whole relation; pass 2: each
// pass-1 partition). Segments are cut into chunks of chunkLen tuples; a workgroup
// owns one chunk. Histogram entries are stored [segment][bin][chunk] so that one
// exclusive scan over the whole array yields every chunk's write cursor.
//
// This file: the partition passes (exact and histogram-free), the LDS partition join with the resident-R probe and its
// work items. What the materialising form (hj_prj_pairs.hip), the aggregating form (hj_prj_agg.hip) and the shard split
// (hj_shard.hip) share with it is in hj_prj_impl.h; the pass runners they call are defined here.

#include "hj_prj_impl.h"

#include <cmath>
#include <cstdlib>
#include <type_traits>

namespace hj {

// chunkBase[s] = sum_{t<s} ceil(len_t / chunkLen). nSeg <= 256: one thread.
__global__ void k_chunk_base(const uint32_t* __restrict__ segOff, uint32_t nSeg, uint32_t chunkLen,
                             uint32_t* __restrict__ chunkBase)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        uint32_t acc = 0;
        for (uint32_t s = 0; s < nSeg; ++s) {
            chunkBase[s] = acc;
            const uint32_t len = segOff[s + 1] - segOff[s];
            acc += (len + chunkLen - 1) / chunkLen;
        }
        chunkBase[nSeg] = acc;
    }
}

__global__ void k_init_seg(uint32_t* seg, uint32_t n)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) { seg[0] = 0; seg[1] = n; }
}

void launch_init_seg(uint32_t* seg, uint32_t n, hipStream_t s) { hipLaunchKernelGGL(k_init_seg, dim3(1), dim3(64), 0, s, seg, n); }
void launch_chunk_base(const uint32_t* segOff, uint32_t nSeg, uint32_t chunkLen, uint32_t* chunkBase, hipStream_t s)
{
    hipLaunchKernelGGL(k_chunk_base, dim3(1), dim3(64), 0, s, segOff, nSeg, chunkLen, chunkBase);
}

// ---------------------------------------------------------------------------
// element formats
//   IN32 / OUT32 = false: 8-byte DataGen tuples (value = key, tuple_t{key,payload});
//   = true: bare 32-bit keys. The join consumes keys only (bucket_chaining_join never reads
//   the payload, :247-256 and the commented probe :264-275), so pass 1 of the PRJ path writes
//   the key word alone and everything after it moves 4 bytes per tuple instead of 8.
//   Inputs are read as 16-byte vectors (2 tuples or 4 keys).
// ---------------------------------------------------------------------------
template <bool IN32> struct Fmt { static constexpr uint32_t EPV = IN32 ? 4u : 2u; };   // elements per vector

template <bool IN32, int E>
__device__ __forceinline__ uint32_t vec_key(const uint4& t)
{
    if constexpr (IN32) return E == 0 ? t.x : E == 1 ? t.y : E == 2 ? t.z : t.w;
    else return E == 0 ? t.x : t.z;
}
template <int E>
__device__ __forceinline__ uint64_t vec_tuple(const uint4& t)      // 8-byte formats only
{
    return E == 0 ? (((uint64_t)t.y << 32) | t.x) : (((uint64_t)t.w << 32) | t.z);
}

// ---------------------------------------------------------------------------
// histogram
// ---------------------------------------------------------------------------
template <bool IN32>
__global__ void __launch_bounds__(kBlock)
k_radix_hist(const void* __restrict__ in, PassParams p, uint32_t* __restrict__ hist, Gate gate)
{
    constexpr uint32_t EPV = Fmt<IN32>::EPV;
    __shared__ unsigned int h[kMaxFan];
    if (gate_closed(gate)) return;
    const uint32_t c = blockIdx.x;
    if (c >= p.chunkBase[p.nSeg]) return;
    const ChunkRange r = chunk_range(p, c);
    if (threadIdx.x < kMaxFan) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t fmask = p.fan - 1;
    // 16-byte aligned sweep: start at the vector that holds element `begin`
    const uint4* in4 = reinterpret_cast<const uint4*>(in);
    if (p.fan <= 16) {
        // few bins (the multi-GPU split: fan = number of shards): 64 lanes adding to a handful of LDS words
        // serialise on the address (measured: 2.4 TB/s at fan 1 against 5.8 TB/s at fan 256), so count with
        // ballots into wave-uniform registers instead and add once per wavefront at the end
        uint32_t wc[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) wc[b] = 0;
        bool live = false;
        auto tally = [&](uint32_t key, uint32_t at) {
            const bool ok = live && at >= r.begin && at < r.end;
            const uint32_t bin = ((key - p.bias) >> p.shift) & fmask;
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (b < (int)p.fan) wc[b] += (uint32_t)__popcll(__ballot(ok && bin == (uint32_t)b));
        };
        const uint32_t vEnd = (uint32_t)(((uint64_t)r.end + EPV - 1) / EPV);
        // whole wavefronts iterate together (ballots need every lane): round the trip count up
        // four 16-byte loads in flight per lane before the first ballot (one load per trip left the kernel at 4.0 TB/s:
        // a wavefront had 1 KiB outstanding)
        constexpr int U = 4;
        for (uint32_t v0 = r.begin / EPV; v0 < vEnd; v0 += U * kBlock) {
            uint4 t[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t v = v0 + (uint32_t)u * kBlock + threadIdx.x;
                t[u] = in4[v < vEnd ? v : vEnd - 1];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const uint32_t v = v0 + (uint32_t)u * kBlock + threadIdx.x;
                live = v < vEnd;
                const uint32_t i = v * EPV;
                if constexpr (IN32) {
                    tally(t[u].x, i); tally(t[u].y, i + 1); tally(t[u].z, i + 2); tally(t[u].w, i + 3);
                } else {
                    tally((p.zeroBad && t[u].y) ? 0u : t[u].x, i);
                    tally((p.zeroBad && t[u].w) ? 0u : t[u].z, i + 1);
                }
            }
        }
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int b = 0; b < 16; ++b)
                if (b < (int)p.fan && wc[b]) atomicAdd(&h[b], wc[b]);
        }
        __syncthreads();
        if (threadIdx.x < p.fan) hist[hist_index(p, r, threadIdx.x)] = h[threadIdx.x];
        return;
    }
    for (uint32_t v = r.begin / EPV + threadIdx.x; (uint64_t)v * EPV < r.end; v += kBlock) {
        const uint4 t = in4[v];
        const uint32_t i = v * EPV;
        auto one = [&](uint32_t key, uint32_t at) {
            if (at >= r.begin && at < r.end) atomicAdd(&h[((key - p.bias) >> p.shift) & fmask], 1u);
        };
        if constexpr (IN32) {
            one(t.x, i); one(t.y, i + 1); one(t.z, i + 2); one(t.w, i + 3);
        } else {
            one((p.zeroBad && t.y) ? 0u : t.x, i);
            one((p.zeroBad && t.w) ? 0u : t.z, i + 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < p.fan) hist[hist_index(p, r, threadIdx.x)] = h[threadIdx.x];
}

// The histogram of the row-id passes' first pass (HJ_FLAG_KEEP_ROW_IDS on a resident radix join, hj_prj_pairs.hip): it
// reads every tuple anyway, so it also writes the tuple's {key, row} element -- row = rowBase + position, over the
// input's own upper word -- to `stamped`, which the scatter passes then move whole (k_radix_scatter<false, false>).
// One segment, the dense relation: chunks start at even positions, so the body goes as aligned 16-byte vectors.
__global__ void __launch_bounds__(kBlock)
k_radix_hist_rows(const uint64_t* __restrict__ in, uint64_t* __restrict__ stamped, PassParams p, uint32_t* __restrict__ hist,
                  uint32_t rowBase)
{
    __shared__ unsigned int h[kMaxFan];
    const uint32_t c = blockIdx.x;
    if (c >= p.chunkBase[p.nSeg]) return;
    const ChunkRange r = chunk_range(p, c);
    if (threadIdx.x < kMaxFan) h[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t fmask = p.fan - 1;
    const uint4* in4 = reinterpret_cast<const uint4*>(in);
    uint4* out4 = reinterpret_cast<uint4*>(stamped);
    const uint32_t vEnd = r.end >> 1;                        // r.begin is even (chunkLen is a multiple of kTile)
    for (uint32_t v = (r.begin >> 1) + threadIdx.x; v < vEnd; v += kBlock) {
        const uint4 t = in4[v];
        const uint32_t row = rowBase + 2 * v;
        out4[v] = uint4{t.x, row, t.z, row + 1};
        atomicAdd(&h[(t.x >> p.shift) & fmask], 1u);
        atomicAdd(&h[(t.z >> p.shift) & fmask], 1u);
    }
    if ((r.end & 1u) && threadIdx.x == 0) {                  // the relation's odd last tuple
        const uint32_t key = (uint32_t)in[r.end - 1];
        stamped[r.end - 1] = ((uint64_t)(rowBase + r.end - 1) << 32) | key;
        atomicAdd(&h[(key >> p.shift) & fmask], 1u);
    }
    __syncthreads();
    if (threadIdx.x < p.fan) hist[hist_index(p, r, threadIdx.x)] = h[threadIdx.x];
}

// New segment offsets after a pass: segOut[s*fan + bin] = start of that bin.
__global__ void __launch_bounds__(kBlock)
k_seg_offsets(PassParams p, const uint32_t* __restrict__ scanned, uint32_t nTotal, uint32_t* __restrict__ segOut)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    const uint32_t total = p.nSeg * p.fan;
    if (i == total) segOut[i] = nTotal;
    if (i >= total) return;
    const uint32_t s = i / p.fan, bin = i - s * p.fan;
    const uint32_t nLocal = p.chunkBase[s + 1] - p.chunkBase[s];
    // an empty segment has no histogram entries: all its bins start where it starts
    segOut[i] = nLocal ? scanned[(uint64_t)p.chunkBase[s] * p.fan + (uint64_t)bin * nLocal] : p.segOff[s];
}

// ---------------------------------------------------------------------------
// scatter: tile-local counting sort in LDS, then contiguous runs to HBM
//   NT threads, TV 16-byte loads per thread and tile -> tile = NT * TV * EPV elements.
//   Instances: pass 1 of PRJ   tuples -> keys, 512 x 8 x 2 = 8192 per tile (128-byte runs at fan 256)
//              pass 2 of PRJ   keys -> keys,   512 x 4 x 4 = 8192 per tile
//              shard scatter   the pass-1 instance with fan-out = number of shards
// ---------------------------------------------------------------------------
template <bool IN32, bool OUT32, int NT, int TV, bool PF = true, int WPE = 1>
__global__ void __launch_bounds__(NT, WPE)
k_radix_scatter(const void* __restrict__ in, void* __restrict__ outv, PassParams p,
                const uint32_t* __restrict__ scanned, Gate gate)
{
    static_assert(!(IN32 && !OUT32), "keys cannot become tuples again");
    constexpr uint32_t EPV = Fmt<IN32>::EPV;
    constexpr int E = (int)EPV * TV;                 // elements per thread per tile
    constexpr uint32_t TILE = (uint32_t)NT * E;
    static_assert(!PF || E == 16, "vmcnt immediate below assumes 16 stores per thread per full tile");
    static_assert(TILE <= 65536 && E % 2 == 0, "ranks are kept in 16 bits, two to a register");
    using OutT = typename std::conditional<OUT32, uint32_t, uint64_t>::type;
    OutT* __restrict__ out = static_cast<OutT*>(outv);

    // Staged position q lives at stage[q + (q >> kPadShift)]: one pad element per 32 banks' worth. Without it,
    // equal-sized bins (dense keys: every bin of a tile holds exactly TILE/fan elements) start at the same
    // bank and lanes, whose ranks advance in step, collide (PMC: 80 % of the LDS cycles were bank conflicts).
    constexpr uint32_t kPadShift = OUT32 ? 5 : 4;
    constexpr uint32_t kDump = TILE + (TILE >> kPadShift);    // slot for elements outside the chunk
    __shared__ OutT stage[kDump + 1];
    __shared__ unsigned int tileCnt[kMaxFan];    // per bin: elements of this tile
    __shared__ unsigned int tileOff[kMaxFan];    // exclusive scan of tileCnt
    __shared__ unsigned int delta[kMaxFan];      // write cursor of the bin - tileOff: output index = delta[bin] + staged position
    __shared__ unsigned int cursor[kMaxFan];
    __shared__ unsigned int sValid;

    if (gate_closed(gate)) return;
    const uint32_t c = blockIdx.x;
    if (c >= p.chunkBase[p.nSeg]) return;
    const ChunkRange r = chunk_range(p, c);
    const uint32_t fmask = p.fan - 1;
    const uint32_t len = r.end - r.begin;
    if (threadIdx.x < kMaxFan) {
        tileCnt[threadIdx.x] = 0;
        cursor[threadIdx.x] = threadIdx.x < p.fan ? scanned[hist_index(p, r, threadIdx.x)] : 0;
    }
    __syncthreads();

    const uint4* in4 = reinterpret_cast<const uint4*>(in);
    const uint32_t b0 = r.begin & ~(EPV - 1);
    // Register prefetch of the next tile (one unconditional, clamped load path; waits placed by hand: see
    // hj_build_own.hip). vmcnt counts loads and stores together in issue order: after a full tile every
    // thread has exactly E stores younger than the prefetch loads, so vmcnt(E) waits for the loads only
    // and leaves the stores in flight.
    const uint32_t lastVec = (r.end - 1) / EPV;
    uint4 nxt[TV];
    auto issue = [&](uint64_t tb) {
#pragma unroll
        for (int k = 0; k < TV; ++k) {
            const uint64_t v = tb / EPV + (uint64_t)k * NT + threadIdx.x;
            nxt[k] = in4[v < lastVec ? v : lastVec];
        }
    };
    if (PF) issue(b0);
    bool prevFull = false;
    // Three barriers per tile. The first version of this loop had eight, and a range-check branch around
    // every LDS atomic, which made each of the 16 returning atomics of a thread its own round trip
    // (s_waitcnt lgkmcnt(0) inside every branch): 3.6 ms per 2^30-tuple pass. Now every lane ranks every
    // element unconditionally (one outside the chunk adds 0 and is staged to the dump slot).
    for (uint64_t tb = b0; tb < r.end; tb += TILE) {
        uint4 cur[TV];
        if (PF) {
            if (prevFull) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int k = 0; k < TV; ++k) cur[k] = nxt[k];
            __builtin_amdgcn_sched_barrier(0);
            issue(tb + TILE);
            __builtin_amdgcn_sched_barrier(0);
        } else {
            issue(tb);
#pragma unroll
            for (int k = 0; k < TV; ++k) cur[k] = nxt[k];
        }
        // ---- rank: position of every element inside its (tile, bin) ----
        OutT tv[E];
        uint32_t br[E];      // bin << 16 | rank
        uint32_t okMask = 0;
        // offset from the chunk's first element; wraps below zero (= huge) for the elements before `begin`
        const uint32_t rel0 = (uint32_t)tb - r.begin + EPV * threadIdx.x;
        auto one = [&](int slot, uint32_t key, uint64_t tuple, uint32_t rel) {
            const uint32_t bin = (key >> p.shift) & fmask;
            const bool ok = rel < len;
            if constexpr (OUT32) tv[slot] = key;
            else tv[slot] = tuple;
            okMask |= ok ? (1u << slot) : 0u;
            br[slot] = (bin << 16) | atomicAdd(&tileCnt[bin], ok ? 1u : 0u);
        };
#pragma unroll
        for (int k = 0; k < TV; ++k) {
            const uint32_t rel = rel0 + EPV * (uint32_t)k * NT;
            const uint4 t = cur[k];
            if constexpr (IN32) {
                one(4 * k, t.x, 0, rel); one(4 * k + 1, t.y, 0, rel + 1); one(4 * k + 2, t.z, 0, rel + 2); one(4 * k + 3, t.w, 0, rel + 3);
            } else {
                one(2 * k, t.x, vec_tuple<0>(t), rel); one(2 * k + 1, t.z, vec_tuple<1>(t), rel + 1);
            }
        }
        __syncthreads();
        // ---- one wavefront: exclusive scan of the 256 counters (4 per lane), cursors, reset ----
        if (threadIdx.x < 64) {
            const uint32_t b4 = 4 * threadIdx.x;
            uint32_t cnt[4], sum = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { cnt[j] = tileCnt[b4 + j]; tileCnt[b4 + j] = 0; sum += cnt[j]; }
            uint32_t inc = sum;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t n = __shfl_up(inc, off, 64);
                if ((int)threadIdx.x >= off) inc += n;
            }
            uint32_t ex = inc - sum;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t cu = cursor[b4 + j];
                tileOff[b4 + j] = ex;
                delta[b4 + j] = cu - ex;
                cursor[b4 + j] = cu + cnt[j];
                ex += cnt[j];
            }
            if (threadIdx.x == 63) sValid = inc;
        }
        __syncthreads();
        // ---- stage: tile-local counting sort ----
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const uint32_t at = tileOff[br[k] >> 16] + (br[k] & 0xFFFFu);
            stage[((okMask >> k) & 1u) ? at + (at >> kPadShift) : kDump] = tv[k];
        }
        __syncthreads();
        // ---- contiguous runs to HBM ----
        const uint32_t valid = sValid;
        auto emit = [&](uint32_t q) {
            const OutT t = stage[q + (q >> kPadShift)];
            const uint32_t bin = ((uint32_t)t >> p.shift) & fmask;
            out[delta[bin] + q] = t;
        };
        if (valid == TILE) {
#pragma unroll
            for (int k = 0; k < E; ++k) emit((uint32_t)k * NT + threadIdx.x);
        } else {
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const uint32_t q = (uint32_t)k * NT + threadIdx.x;
                if (q < valid) emit(q);
            }
        }
        prevFull = (valid == TILE);
        // (the next tile's atomics touch only tileCnt, reset above; its scan step, which rewrites
        //  tileOff/delta, runs after a barrier every wavefront reaches only when it has finished this phase)
    }
}

// ---------------------------------------------------------------------------
// histogram-free partitioning
//   The exact passes above read everything twice: once to count, once to move (parallel_radix_partition :586-626 does
//   the same). The counting exists only to make every partition one dense run. Here a pass does not count: chunk c of
//   segment s owns, for every bin b, a private FRAGMENT of `outCap` key slots at ((s * fan + b) * C + c) * outCap and
//   fills it from the front; what it wrote is recorded per fragment (outCnt). A partition is then C fragments with
//   holes between them, which the next pass (reading positions, masking the holes by the counts) and the join (one
//   fragment at a time) walk without ever compacting. outCap = mean + 7 sigma of a Poisson count (host: frag_cap), so
//   DataGen-shaped inputs -- dense or uniformly drawn keys, whose low bits are uniform in every contiguous piece of
//   the relation -- fit; a fragment that would overflow sets Counters::prjFallback, every kernel of this path
//   returns at once when it sees the word set, and the exact passes, gated on the same word, redo the join.
//   No atomics, no scan, no second read: 12 B (pass 1) and 8 B (pass 2) per tuple instead of 20 and 12.
// ---------------------------------------------------------------------------
constexpr uint32_t kMaxInFrags = 1024;     // pass-1 fragments one pass-2 chunk may span (C1 <= 1024)
// workgroup geometry of the two passes: threads, elements per thread and tile, waves per SIMD the registers must allow;
// pass 1 ranks into per-(bin, lane column) counters (LANECOL, k_radix_scatter_frag)
constexpr int kFrag1Threads = 1024, kFrag1Elems = 32, kFrag1Wpe = 4;
constexpr int kFrag2Threads = 512, kFrag2Elems = 16, kFrag2Wpe = 4;

struct FragPass {
    uint32_t C;              // chunks per input segment = fragments per output partition
    uint32_t shift, fan;
    uint32_t outCap;         // key slots per output fragment (multiple of 32: whole 128-byte lines)
    uint32_t* outCnt;        // [nSeg * fan * C] keys written per output fragment
    // pass 1 (tuples in): one segment, the dense relation
    uint32_t n, chunkLen;
    // pass 2 (keys in): segment s = the inFrags * C fragments of pass-1 bin s, chunk c of it = fragments [c * inFrags, ..)
    uint32_t inFrags, inCap;
    const uint32_t* inCnt;
};

// LANECOL (pass 1, tiles of 32768 keys): the ranking counters are kept per (bin, lane & 15) -- 16 columns per bin, so
// the bank of a lane's counter is ((bin & 1) << 4 | lane & 15): whatever bins the 32 lanes of a group hold, at most two of
// them meet on a bank, which a 4-cycle LDS atomic hides (MI355X_MICROARCH.md, LDS). Ranking 64 shuffled keys into one
// counter per bin put 3-5 lanes on the busiest bank and serialised equal bins (r03_prj_pmc_sq.txt: 244 M conflict cycles
// of 416 M LDS-active on the shuffled R against 104 M of 276 M on the sorted S). One word per counter: the count of the
// current tile in the low half (<= 2048: 64 threads x 32 keys share a column), the counter's first staged position --
// the exclusive scan over (bin, column), written by the scan that also resets the count -- in the high half (< 65536).
// The scan is done by all threads (4 counters each) instead of one wavefront over 256 bins.
template <bool IN32, int NT, int E = 16, int WPE = 4, bool LANECOL = false>         // E = elements per thread and tile
__global__ void __launch_bounds__(NT, WPE)
k_radix_scatter_frag(const void* __restrict__ in, uint32_t* __restrict__ out, FragPass p, Counters* __restrict__ ctr)
{
    constexpr uint32_t TILE = (uint32_t)NT * E;
    static_assert(TILE <= 65536 && E % 2 == 0, "ranks are kept in 16 bits, two to a register");
    static_assert(!LANECOL || (NT == 4 * kMaxFan && TILE < 65536), "LANECOL: four counters per thread, positions in 16 bits");
    constexpr uint32_t kPadShift = 5;                         // see k_radix_scatter
    constexpr uint32_t kDump = TILE + (TILE >> kPadShift);
    __shared__ uint32_t stage[kDump + 1];
    __shared__ unsigned int tileCnt[LANECOL ? 1 : kMaxFan], tileOff[LANECOL ? 1 : kMaxFan], delta[kMaxFan], cursor[kMaxFan];
    __shared__ uint4 colCnt[LANECOL ? kMaxFan * 4 : 1];       // LANECOL: [bin][16 columns], as uint4 for the scan
    __shared__ unsigned int sValid, sAbort;
    __shared__ uint32_t prefix[IN32 ? kMaxInFrags + 1 : 1];   // pass 2: keys of this chunk before input fragment i
    __shared__ uint32_t wsum[NT / 64];

    // The fallback word is set by OTHER workgroups of this very launch (below): every wavefront reading it for itself
    // could split a workgroup -- some wavefronts gone, the rest scanning with stale wsum[] entries, and pass 2 would then
    // read through garbage prefixes. One thread reads, the workgroup decides together (round-2 ADVICE).
    if (threadIdx.x == 0) sAbort = *reinterpret_cast<volatile unsigned long long*>(&ctr->prjFallback) != 0;
    __syncthreads();
    if (sAbort) return;
    const uint32_t c = blockIdx.x;
    const uint32_t seg = c / p.C, local = c - seg * p.C;
    const uint32_t fmask = p.fan - 1;
    // first slot of this chunk's fragment of bin b
    auto frag_start = [&](uint32_t b) { return ((seg * p.fan + b) * p.C + local) * p.outCap; };

    // ---- what this chunk reads: `total` elements, element d at ... ----
    uint32_t total;                                            // elements of the chunk
    uint32_t begin = 0;                                        // pass 1: first tuple
    const uint32_t firstFrag = (seg * p.C + local) * p.inFrags;   // pass 2: first input fragment
    if constexpr (!IN32) {
        begin = local * p.chunkLen;
        const uint32_t end = begin + p.chunkLen < p.n ? begin + p.chunkLen : p.n;   // host: n <= 2^31
        total = begin < end ? end - begin : 0u;
    } else {
        // The holes between the input fragments are skipped, not masked: tiles are full (their runs whole 128-byte
        // lines on dense keys), and nothing is read that is not a key. prefix[] = exclusive scan of the counts.
        uint32_t carry = 0;
        for (uint32_t base = 0; base < p.inFrags; base += NT) {
            const uint32_t i = base + threadIdx.x;
            const uint32_t v = i < p.inFrags ? p.inCnt[firstFrag + i] : 0u;
            uint32_t sum;
            const uint32_t ex = block_exclusive_scan<NT>(v, wsum, sum);
            if (i < p.inFrags) prefix[i] = carry + ex;
            carry += sum;
        }
        if (threadIdx.x == 0) prefix[p.inFrags] = carry;
        total = carry;
        // counts that cannot be (more keys than the input fragments hold): never index with them
        if (total > p.inFrags * p.inCap) {
            if (threadIdx.x == 0) atomicExch(&ctr->prjFallback, 1ull);
            return;                                             // workgroup-uniform: carry is the same in every thread
        }
    }
    if (total == 0) {                                           // the last chunks of a short relation
        if (threadIdx.x < p.fan) p.outCnt[(seg * p.fan + threadIdx.x) * p.C + local] = 0;
        return;
    }
    if (threadIdx.x < kMaxFan) {
        if constexpr (!LANECOL) tileCnt[threadIdx.x] = 0;
        cursor[threadIdx.x] = threadIdx.x < p.fan ? frag_start(threadIdx.x) : 0;
    }
    if constexpr (LANECOL) colCnt[threadIdx.x] = uint4{0u, 0u, 0u, 0u};
    if (threadIdx.x == 0) sAbort = 0;
    __syncthreads();

    const uint32_t* in1 = reinterpret_cast<const uint32_t*>(in);
    uint32_t fA = 0;                                            // pass 2: input fragment the tile starts in
    uint32_t tileNo = 0;
    for (uint32_t T = 0; T < total; T += TILE, ++tileNo) {
        // the thread index is made opaque per tile: everything derived from it (16 positions, LDS addresses, offsets) is
        // one add away, and hoisted out of the loop it only fills registers until they spill
        uint32_t tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        unsigned int* const colWord = reinterpret_cast<unsigned int*>(colCnt) + (tid & 15u);   // LANECOL: + 16 * bin
        uint32_t tv[E], okMask = 0;
        if constexpr (!IN32) {
            // one register per element instead of two (the payload word is never looked at, as in mc: the partition
            // function and the join read tuple_t.key only); lanes read every second word of contiguous lines
            // (a chunk is at most 2^21 tuples -- frag_geometry --, so byte offsets from the chunk's base fit 32 bits:
            // scalar base + one offset register per load)
            const char* const base = static_cast<const char*>(in) + 8ull * (begin + T);
            if (T + TILE <= total) {                            // a full tile: scalar base per load, one shared offset register
#pragma unroll
                for (int j = 0; j < E; ++j)
                    tv[j] = *reinterpret_cast<const uint32_t*>(base + (size_t)j * NT * 8 + (tid << 3));
                okMask = E == 32 ? 0xFFFFFFFFu : (1u << (E & 31)) - 1u;
            } else {
                const uint32_t left = total - T;                // >= 1
#pragma unroll
                for (int j = 0; j < E; ++j) {
                    const uint32_t d = (uint32_t)j * NT + tid;
                    const bool ok = d < left;
                    tv[j] = *reinterpret_cast<const uint32_t*>(base + ((ok ? d : left - 1) << 3));
                    okMask |= (ok ? 1u : 0u) << j;
                }
            }
        } else {
            // element d of the chunk lives in input fragment f (prefix[f] <= d < prefix[f+1]) at slot d - prefix[f].
            // A thread's elements d = T + j * NT + thread grow with j, so it walks the fragments once per tile: the
            // current fragment's end and address offset stay in registers, and a step to the next fragment (a tile of
            // 32768 keys meets ~8 fragments of 4096) costs two LDS reads.
            while (fA + 1 < p.inFrags && prefix[fA + 1] <= T) ++fA;
            uint32_t f = fA;
            uint32_t bound = f + 1 < p.inFrags ? prefix[f + 1] : 0xFFFFFFFFu;
            uint32_t off = (firstFrag + f) * p.inCap - prefix[f];
#pragma unroll
            for (int j = 0; j < E; ++j) {
                const uint32_t d = T + (uint32_t)j * NT + tid;
                const bool ok = d < total;
                while (ok && d >= bound) {
                    ++f;
                    bound = f + 1 < p.inFrags ? prefix[f + 1] : 0xFFFFFFFFu;
                    off = (firstFrag + f) * p.inCap - prefix[f];
                }
                tv[j] = in1[ok ? d + off : firstFrag * p.inCap];
                okMask |= (ok ? 1u : 0u) << j;
            }
        }
        // ---- rank ----
        uint32_t rk[E / 2];                                     // two 16-bit ranks per register; the bin is recomputed from the key
#pragma unroll
        for (int j = 0; j < E; ++j) {
            const uint32_t bin = (tv[j] >> p.shift) & fmask;
            uint32_t r;
            if constexpr (LANECOL) r = atomicAdd(&colWord[bin << 4], (okMask >> j) & 1u) & 0xFFFFu;
            else r = atomicAdd(&tileCnt[bin], (okMask >> j) & 1u);
            if (j & 1) rk[j / 2] |= r << 16; else rk[j / 2] = r;
        }
        __syncthreads();
        if constexpr (LANECOL) {
            // ---- all threads: scan of the 4096 counters (thread t: bin t / 4, columns 4 (t % 4) ..), cursors, capacity check ----
            const uint4 w = colCnt[tid];
            const uint32_t c0 = w.x & 0xFFFFu, c1 = w.y & 0xFFFFu, c2 = w.z & 0xFFFFu, c3 = w.w & 0xFFFFu;
            const uint32_t mine = c0 + c1 + c2 + c3;
            uint32_t tot;
            const uint32_t ex = block_exclusive_scan<NT>(mine, wsum, tot);
            colCnt[tid] = uint4{ex << 16, (ex + c0) << 16, (ex + c0 + c1) << 16, (ex + c0 + c1 + c2) << 16};
            const uint32_t endOfBin = (uint32_t)__shfl_down((int)(ex + mine), 3, 64);     // the four threads of a bin share a wavefront
            if ((tid & 3u) == 0) {
                const uint32_t b = tid >> 2, cnt = endOfBin - ex;
                const uint32_t cu = cursor[b];
                delta[b] = cu - ex;
                cursor[b] = cu + cnt;
                if (b < p.fan && cu + cnt - frag_start(b) > p.outCap) { sAbort = 1; atomicExch(&ctr->prjFallback, 1ull); }
            }
            if (tid == 0) {
                sValid = tot;
                // someone else's overflow: looked at every 16th tile
                if ((tileNo & 15u) == 15u && *reinterpret_cast<volatile unsigned long long*>(&ctr->prjFallback) != 0) sAbort = 1;
            }
        } else
        // ---- one wavefront: scan of the counters, cursors, capacity check ----
        if (tid < 64) {
            const uint32_t b4 = 4 * tid;
            uint32_t cnt[4], sum = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { cnt[j] = tileCnt[b4 + j]; tileCnt[b4 + j] = 0; sum += cnt[j]; }
            uint32_t inc = sum;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t n = __shfl_up(inc, off, 64);
                if ((int)tid >= off) inc += n;
            }
            uint32_t ex = inc - sum;
            bool over = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t cu = cursor[b4 + j];
                tileOff[b4 + j] = ex;
                delta[b4 + j] = cu - ex;
                cursor[b4 + j] = cu + cnt[j];
                over |= (b4 + j < p.fan) && (cu + cnt[j] - frag_start(b4 + j) > p.outCap);
                ex += cnt[j];
            }
            // someone else's overflow: looked at every 16th tile (one wave-uniform load of a word nobody writes otherwise)
            bool stop = __any(over);
            if (!stop && (tileNo & 15u) == 15u) stop = *reinterpret_cast<volatile unsigned long long*>(&ctr->prjFallback) != 0;
            if (tid == 63) { sValid = inc; if (stop) sAbort = 1; }
            if (tid == 0 && __any(over)) atomicExch(&ctr->prjFallback, 1ull);
        }
        __syncthreads();
        if (sAbort) return;                                     // nothing of this path is used any more
        // ---- stage ----
#pragma unroll
        for (int k = 0; k < E; ++k) {
            const uint32_t binK = (tv[k] >> p.shift) & fmask;
            const uint32_t at = (LANECOL ? colWord[binK << 4] >> 16 : tileOff[binK]) + ((rk[k / 2] >> (16 * (k & 1))) & 0xFFFFu);
            stage[((okMask >> k) & 1u) ? at + (at >> kPadShift) : kDump] = tv[k];
        }
        __syncthreads();
        // ---- contiguous runs to HBM ----
        const uint32_t valid = sValid;
        // staged position q = k * NT + thread lives at q + (q >> 5) = (thread + (thread >> 5)) + k * (NT + NT / 32): one
        // address register and an immediate per k
        static_assert(NT % 32 == 0, "the pad of a staged position splits into a thread part and a k part");
        const uint32_t* const myStage = stage + (tid + (tid >> kPadShift));
        auto emit = [&](int k) {
            const uint32_t t = myStage[k * (NT + (NT >> kPadShift))];
            out[delta[(t >> p.shift) & fmask] + (uint32_t)k * NT + tid] = t;
        };
        if (valid == TILE) {
#pragma unroll
            for (int k = 0; k < E; ++k) emit(k);
        } else {
#pragma unroll
            for (int k = 0; k < E; ++k)
                if ((uint32_t)k * NT + tid < valid) emit(k);
        }
    }
    __syncthreads();
    if (threadIdx.x < p.fan) p.outCnt[(seg * p.fan + threadIdx.x) * p.C + local] = cursor[threadIdx.x] - frag_start(threadIdx.x);
}

// ---------------------------------------------------------------------------
// per-partition join in LDS
// ---------------------------------------------------------------------------
// Slot of key-remainder k in the LDS table. NOT the identity: inside a partition the remainders of
// dense keys are consecutive integers, which under linear probing form one solid run that every
// probe would have to walk to its end (measured: 2.4 s instead of milliseconds at 2^30). A
// Fibonacci multiplicative hash scatters them; the reference avoids the issue with chained buckets
// (bucket_chaining_join :247-252), whose idx = k & (N-1) is still what prjChecksum sums.
__device__ __forceinline__ uint32_t join_hash(uint32_t k)
{
    return (k * 0x9E3779B1u) >> (32 - 15);   // kJoinSlots = 2^15
}
static_assert(kJoinSlots == (1u << 15), "join_hash assumes 2^15 slots");

// ---------------------------------------------------------------------------
// the partition-join core: one R partition into the LDS table, one run of S keys probed against it. Its two schedulers
// are k_prj_join (whole partitions by a fixed stride) and k_prj_probe_items (work items by ticket); they decide what is
// joined next and when its keys are fetched, the core how a partition is joined.
// ---------------------------------------------------------------------------

// A relation's final partitions as the join sees them. Exact passes (!frag): partition pid = part[off[pid] .. off[pid+1]),
// one dense run (log2C = 0). Histogram-free passes (frag): 2^log2C fragments of `cap` slots from pid << log2C, fragment f
// holding cnt[(pid << log2C) + f] keys at its front. total: slots of `part` that may be read (loads are clamped to
// total - 1). The kernels take the three arrays and the geometry as separate parameters (see k_prj_join), and a view on
// the device holds those parameters themselves, never a choice between one of them and null: a load through a pointer
// the compiler cannot trace to ONE read-only parameter is no scalar load any more.
struct PartGeom { uint32_t log2C, cap, total; };
struct PartView { const uint32_t* part; const uint32_t* off; const uint32_t* cnt; PartGeom g; bool frag; };

inline PartView exact_view(const uint32_t* part, const uint32_t* off, uint64_t n)
{
    return PartView{part, off, nullptr, PartGeom{0u, 0u, (uint32_t)n}, false};
}
inline PartView frag_view(const uint32_t* part, const uint32_t* cnt2, const PrjFrag& g, uint32_t P)
{
    return PartView{part, nullptr, cnt2, PartGeom{g.log2C2, g.cap2, P * g.C2 * g.cap2}, true};
}

// slot j of the 16-deep register prefetch covers element ((j & (spf - 1)) * 1024 + thread) of fragment j >> spfShift,
// spf = 2^spfShift slots per fragment (one dense run: 16 slots of the one fragment; 4 fragments: 4 slots each). A
// fragment longer than spf * 1024 is finished by a loop over the rest.
__device__ __forceinline__ uint32_t spf_shift(const PartView& v) { return 4u - v.g.log2C; }

// The prefetch of the partition whose first slot is `base`. Clamped: every lane always loads a valid address (one
// unconditional load path -- see hj_build_own.hip for why); which slots hold keys is decided at use (Shape).
__device__ __forceinline__ void prefetch_part(const PartView& v, uint32_t base, uint32_t (&buf)[kJoinPre])
{
    const uint32_t spfShift = spf_shift(v);
#pragma unroll
    for (int j = 0; j < kJoinPre; ++j) {
        const uint32_t o = base + ((uint32_t)j >> spfShift) * v.g.cap + ((j & ((1u << spfShift) - 1u)) * kJoinThreads + threadIdx.x);
        buf[j] = v.part[o < v.g.total ? o : v.g.total - 1];
    }
}


// What a partition holds: n keys; mask bit j = prefetch slot j holds a key; tail = some fragment is longer than the
// prefetch covers.
struct Shape { uint32_t n, mask; bool tail; };

// One relation's side of a partition (or work item): the fragments from slot `base`, fragment f holding cnt(f) keys.
// Made BEFORE any LDS work of the partition: the counts come through scalar loads, and waiting for one (lgkmcnt) also
// waits for every LDS atomic in flight -- a count looked up between two atomics serialises them (measured: join
// 1.6 -> 2.5 ms).
template <typename Cnt> struct PartKeys { const PartView& v; uint32_t base; Cnt cnt; Shape sh; };

template <typename Cnt>
__device__ __forceinline__ PartKeys<Cnt> keys_of(const PartView& v, uint32_t base, Cnt cnt)
{
    Shape sh{0u, 0u, false};
    const uint32_t spfShift = spf_shift(v), spf = 1u << spfShift;  // prefetch slots per fragment
    for (uint32_t fr = 0; fr < (1u << v.g.log2C); ++fr) {          // one scalar load per fragment
        const uint32_t n = cnt(fr);
        sh.n += n;
        sh.tail |= n > (kJoinThreads << spfShift);
        // this thread's slots of the fragment hold elements thread, thread + 1024, ...: the first `mine` are keys
        uint32_t mine = n > threadIdx.x ? (n - threadIdx.x + kJoinThreads - 1) / kJoinThreads : 0u;
        mine = mine < spf ? mine : spf;
        sh.mask |= ((1u << mine) - 1u) << (fr << spfShift);
    }
    return PartKeys<Cnt>{v, base, cnt, sh};
}

// f(key) for the keys the prefetch holds / for the keys from element `from` of every fragment on, read from memory
template <typename F>
__device__ __forceinline__ void for_slots(const Shape& sh, const uint32_t (&buf)[kJoinPre], F&& f)
{
#pragma unroll
    for (int j = 0; j < kJoinPre; ++j)
        if ((sh.mask >> j) & 1u) f(buf[j]);
}
template <typename Cnt, typename F>
__device__ __forceinline__ void for_rest(const PartKeys<Cnt>& p, uint32_t from, F&& f)
{
    for (uint32_t fr = 0; fr < (1u << p.v.g.log2C); ++fr) for_run(p.v.part, p.base + fr * p.v.g.cap, from, p.cnt(fr), f);
}
// f(key) for every key of the partition: the prefetched slots out of `buf`, the rest of long fragments from memory
template <typename Cnt, typename F>
__device__ __forceinline__ void for_each(const PartKeys<Cnt>& p, const uint32_t (&buf)[kJoinPre], F&& f)
{
    for_slots(p.sh, buf, f);
    if (p.sh.tail) for_rest(p, kJoinThreads << spf_shift(p.v), f);
}

// The LDS table (kJoinSlots words) in its two forms; a key is told apart inside its partition by k = key >> radixBits.
__device__ __forceinline__ void fill_table(uint32_t* tab, uint32_t v)
{
    for (uint32_t i = threadIdx.x; i < kJoinSlots; i += kJoinThreads) tab[i] = v;
}
// Direct-addressed counters (radixBits >= 16): k has at most 16 bits, so the 128 KiB hold one 16-bit counter for EVERY
// possible k -- tab[k >> 1] holds the counts of k = 2i (low half) and 2i + 1 (high half). Build = one increment, probe =
// one read, no hashing and no probe walks (the hashed table spends 26 VALU instructions per tuple on them, PMC).
// Counters cannot overflow while |R partition| <= 65535; larger ones take the hashed table.
struct DirectCounters {
    uint32_t* tab; uint32_t radixBits;
    __device__ __forceinline__ void clear() const { fill_table(tab, 0u); }
    __device__ __forceinline__ void insert(uint32_t key) const
    {
        const uint32_t k = key >> radixBits;
        atomicAdd(&tab[k >> 1], 1u << (16u * (k & 1u)));
    }
    __device__ __forceinline__ uint32_t probe(uint32_t key) const      // :268-271, all equal keys at once
    {
        const uint32_t k = key >> radixBits;
        return (tab[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu;
    }
};
// Open addressing over join_hash, linear probing, at most kJoinBlockTuples keys (load <= 0.75): equal keys are separate
// entries, a probe walks to the first empty slot.
struct HashedTable {
    uint32_t* tab; uint32_t radixBits;
    __device__ __forceinline__ void clear() const { fill_table(tab, kEmpty32); }
    __device__ __forceinline__ void insert(uint32_t key) const
    {
        const uint32_t k = key >> radixBits;
        uint32_t h = join_hash(k);
        while (atomicCAS(&tab[h], kEmpty32, k) != kEmpty32) h = (h + 1) & (kJoinSlots - 1);
    }
    __device__ __forceinline__ uint32_t probe(uint32_t key) const      // :268-271
    {
        const uint32_t k = key >> radixBits;
        uint32_t h = join_hash(k), m = 0;
        for (;;) {
            const uint32_t v = tab[h];
            if (v == kEmpty32) break;
            m += (v == k);
            h = (h + 1) & (kJoinSlots - 1);
        }
        return m;
    }
};

// Where join_partition calls its scheduler's hook:
//   Built      R's keys are in the table, the barrier behind the build has not been passed (a ticket is published here)
//   Between    behind that barrier: R's prefetch registers are free, S is about to be probed -- the scheduler waits for
//              S's prefetch (vmcnt) and issues the next R prefetch, in flight while S is probed
//   Oversized  instead of both, before the first of several builds
enum class At { Built, Between, Oversized };

// Joins R's partition with S's keys in one LDS table: clear, build from R, hook, probe S; `matches` += the matches.
// insert(table, key) is the scheduler's, so that it can look at R's keys on their way (k_prj_join's checksum).
template <typename Table, typename CntR, typename CntS, typename Insert, typename Hook>
__device__ __forceinline__ void join_one_table(const Table& t, const PartKeys<CntR>& R, const uint32_t (&bufR)[kJoinPre],
                                               const PartKeys<CntS>& S, const uint32_t (&bufS)[kJoinPre], Insert&& insert,
                                               Hook&& hook, unsigned long long& matches)
{
    t.clear();
    __syncthreads();
    for_each(R, bufR, [&](uint32_t key) { insert(t, key); });
    hook(At::Built);
    __syncthreads();
    hook(At::Between);
    uint32_t m32 = 0;                                  // < 2^16 (2^15 hashed) per probe, 16 probes
    for_slots(S.sh, bufS, [&](uint32_t key) { m32 += t.probe(key); });
    matches += m32;
    if (S.sh.tail) for_rest(S, kJoinThreads << spf_shift(S.v), [&](uint32_t key) { matches += t.probe(key); });
    __syncthreads();
}

// The mode is picked from R's partition size: counters (DIRECT, <= 65535 keys), one hashed table (<= kJoinBlockTuples),
// or, for an oversized R partition (skew), several builds of the hashed table with S probed against each. The last one
// meets the exact layout only -- the histogram-free passes are not planned for partitions that could outgrow one
// table (frag_geometry) --, so R is one dense run there.
template <bool DIRECT, typename CntR, typename CntS, typename Insert, typename Hook>
__device__ __forceinline__ void join_partition(uint32_t* tab, uint32_t radixBits, const PartKeys<CntR>& R,
                                               const uint32_t (&bufR)[kJoinPre], const PartKeys<CntS>& S,
                                               const uint32_t (&bufS)[kJoinPre], Insert&& insert, Hook&& hook,
                                               unsigned long long& matches)
{
    const uint32_t nR = R.sh.n;
    if (DIRECT && nR <= 65535u) {
        join_one_table(DirectCounters{tab, radixBits}, R, bufR, S, bufS, insert, hook, matches);
    } else if (nR <= kJoinBlockTuples) {
        join_one_table(HashedTable{tab, radixBits}, R, bufR, S, bufS, insert, hook, matches);
    } else {
        hook(At::Oversized);
        const HashedTable t{tab, radixBits};
        for (uint32_t blk = 0; blk < nR; blk += kJoinBlockTuples) {
            const uint32_t bn = nR - blk > kJoinBlockTuples ? kJoinBlockTuples : nR - blk;
            t.clear();
            __syncthreads();
            for_run(R.v.part, R.base + blk, 0u, bn, [&](uint32_t key) { insert(t, key); });
            __syncthreads();
            for_rest(S, 0u, [&](uint32_t key) { matches += t.probe(key); });
            __syncthreads();
        }
    }
}

// One persistent workgroup per CU walks the partitions pid = blockIdx.x, += gridDim.x. The LDS table takes
// 128 KiB, so only one workgroup fits a CU and nothing else could hide the HBM latency of a partition's
// 2 x 128 KiB: while partition p is built and probed out of registers, the first 16384 R and S tuples of
// the next partition are already in flight into the other register set (explicit vmcnt wait at the top).
// Measured at 2^30: 13.4 ms -> see profiles/.
// S == nullptr: R's checksum alone (hj_prj_build_dev).
// The six arrays are separate __restrict__ parameters, not members of the views: only then does the compiler read the
// offsets and counts (wave-uniform addresses) with scalar loads. As plain struct members they became vector loads
// whose s_waitcnt vmcnt(0) also waited for the register prefetch of the next partition (join 1.6 -> 2.5 ms).
template <bool DIRECT>
__global__ void __launch_bounds__(kJoinThreads)
k_prj_join(const uint32_t* __restrict__ partR, const uint32_t* __restrict__ offR, const uint32_t* __restrict__ cntR, PartGeom gR,
           const uint32_t* __restrict__ partS, const uint32_t* __restrict__ offS, const uint32_t* __restrict__ cntS, PartGeom gS,
           uint32_t radixBits, uint32_t nParts, Counters* __restrict__ ctr, Gate gate)
{
    extern __shared__ uint32_t tab[];  // kJoinSlots
    if (gate_closed(gate)) return;
    const PartView R{partR, offR, cntR, gR, cntR != nullptr}, S{partS, offS, cntS, gS, cntS != nullptr};
    unsigned long long matches = 0, checksum = 0;
    uint32_t overflowParts = 0;
    const bool haveS = S.part != nullptr;
    auto base_of = [](const PartView& v, uint32_t pid) { return v.frag ? (pid << v.g.log2C) * v.g.cap : v.off[pid]; };
    auto cnt_of = [](const PartView& v, uint32_t pid, uint32_t f) {
        return v.frag ? v.cnt[(pid << v.g.log2C) + f] : v.off[pid + 1] - v.off[pid];
    };

    // Register pipeline: S(p) is loaded while R(p) is built, R(p+1) while S(p) is probed; each buffer is
    // refilled only after its last use, so no copy of in-flight registers is ever needed.
    uint32_t bufR[kJoinPre], bufS[kJoinPre];   // partitions hold bare keys (see element formats above)
    auto load_R = [&](uint32_t pid) { prefetch_part(R, base_of(R, pid < nParts ? pid : nParts - 1), bufR); };
    load_R(blockIdx.x);

    for (uint32_t pid = blockIdx.x; pid < nParts; pid += gridDim.x) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // R(pid) has landed
        __builtin_amdgcn_sched_barrier(0);
        if (haveS) prefetch_part(S, base_of(S, pid), bufS);    // in flight while R is built
        __builtin_amdgcn_sched_barrier(0);

        const auto keysR = keys_of(R, base_of(R, pid), [&](uint32_t f) { return cnt_of(R, pid, f); });
        const auto keysS = keys_of(S, haveS ? base_of(S, pid) : 0u, [&](uint32_t f) { return haveS ? cnt_of(S, pid, f) : 0u; });
        const uint32_t nR = keysR.sh.n;
        if (nR == 0) {          // serial_radix_partition :531 queues only non-empty R parts (wave-uniform)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            load_R(pid + gridDim.x);
            continue;
        }
        const uint32_t idxMask = next_pow2_u32(nR) - 1;  // bucket idx mask, :242-245
        join_partition<DIRECT>(tab, radixBits, keysR, bufR, keysS, bufS,
            [&](const auto& t, uint32_t key) {
                checksum += (key >> radixBits) & idxMask;      // :249,256
                t.insert(key);
            },
            [&](At at) {
                if (at == At::Built) return;
                if (at == At::Oversized) overflowParts += 1;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // S(pid) has landed; bufR is free
                __builtin_amdgcn_sched_barrier(0);
                load_R(pid + gridDim.x);                           // in flight while S is probed
                __builtin_amdgcn_sched_barrier(0);
            }, matches);
    }
    // one atomic per wavefront
    for (int off = 32; off > 0; off >>= 1) {
        matches += __shfl_down(matches, off, 64);
        checksum += __shfl_down(checksum, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (matches) atomicAdd(&counter_shard(ctr)->prjMatches, matches);
        if (checksum) atomicAdd(&counter_shard(ctr)->prjChecksum, checksum);
    }
    if (threadIdx.x == 0 && overflowParts) atomicAdd(&ctr->prjOverflowParts, (unsigned long long)overflowParts);
}

// ---------------------------------------------------------------------------
// skew-split join against a resident R (hj_prj_build_dev / hj_prj_probe_dev)
//   k_prj_join hands out whole partitions by a fixed stride, so one Zipf-hot S partition (Zipf(0.9) over 2^28 keys puts
//   ~1.7 % of all draws on one key: ~4.5 M S tuples in one partition of a 2^28 slice, against 4096 on average) is walked
//   by one workgroup while the other CUs idle. Here the unit of work is an ITEM: a partition and at most kPrjItemS of its
//   S tuples. The list is built on the device from S's partition sizes (k_prj_items_count, one scan, k_prj_items_fill),
//   the partitions that are split over several items first, and a persistent grid takes items from a ticket counter:
//   the big partitions are spread over many CUs at the start, the small ones fill in behind them. Every item rebuilds
//   its R partition's LDS image and probes its S range (join_partition, as k_prj_join does for whole partitions).
//   kPrjItemS = 2^16: 64 keys per thread and item (256 KiB of S), against an R partition of ~4096 keys at 2^28 / 16 bits
//   that every item rebuilds (~6 % extra LDS work for the items of a split partition); a 4.5 M hot partition becomes ~70
//   items. A partition of the histogram-free S layout holds at most 65535 keys (frag_geometry), so it is always ONE item
//   and only the exact layout (a dense run per partition) is ever split.
//   No prjChecksum here: the build counts it once per R partition (k_prj_join without S), and probes do not change it.
// ---------------------------------------------------------------------------
static_assert(kPrjItemS > 65535u, "a partition of the histogram-free layout is one item");

// keys of partition pid in one relation's layout (exact: cnt == nullptr)
__device__ __forceinline__ uint32_t part_keys(const uint32_t* __restrict__ off, const uint32_t* __restrict__ cnt,
                                              uint32_t log2C, uint32_t pid)
{
    if (cnt == nullptr) return off[pid + 1] - off[pid];
    uint32_t n = 0;
    for (uint32_t f = 0; f < (1u << log2C); ++f) n += cnt[(pid << log2C) + f];
    return n;
}

// One thread per partition: items of partition p at itemCnt[p] (split over > 1 item) or itemCnt[P + p] (one item), so that
// one exclusive scan over [0, 2P] numbers the split partitions' items first; itemCnt[2P] = 0 becomes the total.
// A partition without R tuples or without S tuples has no item. stats[2] / [3]: split partitions, largest S partition.
// rless (the left-outer and anti joins of hj_prj_pairs.hip): a partition with S tuples has its items also without R tuples,
// one per kPrjItemS S tuples as ever, so the list stays within P + slice / kPrjItemS items.
__global__ void __launch_bounds__(kBlock)
k_prj_items_count(const uint32_t* __restrict__ offR, const uint32_t* __restrict__ cntR, uint32_t log2CR,
                  const uint32_t* __restrict__ offS, const uint32_t* __restrict__ cntS, uint32_t log2CS,
                  uint32_t nParts, const Counters* __restrict__ ctr, uint32_t* __restrict__ itemCnt,
                  unsigned long long* __restrict__ stats, bool rless)
{
    const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
    const bool rFrag = cntR != nullptr && ctr->prjFallbackR == 0;      // the layout each relation's passes ended in
    const bool sFrag = cntS != nullptr && ctr->prjFallback == 0;
    uint32_t nS = 0, split = 0;
    if (p < nParts) {
        const uint32_t nR = part_keys(offR, rFrag ? cntR : nullptr, log2CR, p);
        nS = part_keys(offS, sFrag ? cntS : nullptr, log2CS, p);
        const uint32_t items = ((nR || rless) && nS) ? (nS - 1) / kPrjItemS + 1 : 0u;
        split = items > 1 ? 1u : 0u;
        itemCnt[p] = split ? items : 0u;
        itemCnt[nParts + p] = split ? 0u : items;
    } else if (p == nParts) {
        itemCnt[2 * nParts] = 0;
    }
    // one atomic per wavefront
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_down((int)nS, off, 64);
        nS = o > nS ? o : nS;
        split += (uint32_t)__shfl_down((int)split, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (split) atomicAdd(&stats[2], (unsigned long long)split);
        if (nS) atomicMax(&stats[3], (unsigned long long)nS);
    }
}

// One thread per itemCnt entry: its items (partition, S chunk) at the scanned position. stats[1] = items in all.
__global__ void __launch_bounds__(kBlock)
k_prj_items_fill(const uint32_t* __restrict__ scanned, uint32_t nParts, uint2* __restrict__ items,
                 unsigned long long* __restrict__ stats)
{
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) stats[1] = scanned[2 * nParts];
    if (i >= 2 * nParts) return;
    const uint32_t b = scanned[i], n = scanned[i + 1] - b;
    const uint32_t pid = i < nParts ? i : i - nParts;
    for (uint32_t k = 0; k < n; ++k) items[b + k] = make_uint2(pid, k);
}

// gR / gS: the histogram-free geometry (cntR / cntS == nullptr: that relation took the exact passes only); which layout a
// relation ended in is read from Counters::prjFallbackR / prjFallback, each relation on its own. nR / nS: tuples (the
// exact layout's clamp bound). items[0 .. *nItemsAt), taken through *ticket (zeroed by the host before the launch).
template <bool DIRECT>
__global__ void __launch_bounds__(kJoinThreads)
k_prj_probe_items(const uint32_t* __restrict__ partR, const uint32_t* __restrict__ offR, const uint32_t* __restrict__ cntR, PartGeom gR, uint32_t nR,
                  const uint32_t* __restrict__ partS, const uint32_t* __restrict__ offS, const uint32_t* __restrict__ cntS, PartGeom gS, uint32_t nS,
                  const uint2* __restrict__ items, const uint32_t* __restrict__ nItemsAt, unsigned long long* __restrict__ ticket,
                  uint32_t radixBits, Counters* __restrict__ ctr)
{
    extern __shared__ uint32_t tab[];  // kJoinSlots
    __shared__ uint32_t sNext;
    const bool rFrag = cntR != nullptr && ctr->prjFallbackR == 0;
    const bool sFrag = cntS != nullptr && ctr->prjFallback == 0;
    const PartView R{partR, offR, cntR, rFrag ? gR : PartGeom{0u, 0u, nR}, rFrag};
    const PartView S{partS, offS, cntS, sFrag ? gS : PartGeom{0u, 0u, nS}, sFrag};
    const uint32_t nItems = *nItemsAt;
    unsigned long long matches = 0;

    // What an item reads. R: the whole partition (fragments of R.g.cap slots from `base`, or one run). S: the whole partition
    // in the histogram-free layout, else the run of at most kPrjItemS tuples of chunk it.y (n = its length).
    struct Run { uint32_t base, n; };
    auto r_run = [&](uint32_t pid) { return R.frag ? Run{(pid << R.g.log2C) * R.g.cap, 0u} : Run{R.off[pid], R.off[pid + 1] - R.off[pid]}; };
    auto s_run = [&](uint2 it) {
        if (S.frag) return Run{(it.x << S.g.log2C) * S.g.cap, 0u};
        const uint32_t b = S.off[it.x], lo = it.y * kPrjItemS, len = S.off[it.x + 1] - b - lo;
        return Run{b + lo, len < kPrjItemS ? len : kPrjItemS};
    };

    if (threadIdx.x == 0) sNext = (uint32_t)atomicAdd(ticket, 1ull);
    __syncthreads();
    uint32_t cur = (uint32_t)__builtin_amdgcn_readfirstlane((int)sNext);
    if (cur >= nItems) return;                                 // workgroup-uniform
    uint2 it = items[cur];
    uint32_t bufR[kJoinPre], bufS[kJoinPre];
    prefetch_part(R, r_run(it.x).base, bufR);

    for (;;) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // R(it) has landed
        __builtin_amdgcn_sched_barrier(0);
        // the next ticket: issued before S's loads, so that waiting for it does not wait for them; published to the
        // workgroup at the barrier after R's build
        uint32_t tk = 0;
        if (threadIdx.x == 0) tk = (uint32_t)atomicAdd(ticket, 1ull);
        const Run sr = s_run(it);
        prefetch_part(S, sr.base, bufS);                       // in flight while R is built
        __builtin_amdgcn_sched_barrier(0);
        const uint32_t pid = it.x;
        const Run rr = r_run(pid);
        const auto keysR = keys_of(R, rr.base, [&](uint32_t f) { return R.frag ? R.cnt[(pid << R.g.log2C) + f] : rr.n; });
        const auto keysS = keys_of(S, sr.base, [&](uint32_t f) { return S.frag ? S.cnt[(pid << S.g.log2C) + f] : sr.n; });
        uint2 nxt = it;
        uint32_t nxtIdx = nItems;
        // (an R partition without tuples builds an empty table: nothing matches)
        join_partition<DIRECT>(tab, radixBits, keysR, bufR, keysS, bufS,
            [](const auto& t, uint32_t key) { t.insert(key); },
            [&](At at) {
                if (at == At::Oversized) __syncthreads();      // no barrier yet in this item: the last ticket has been read
                if (at != At::Between && threadIdx.x == 0) sNext = tk;
                if (at == At::Built) return;
                if (at == At::Oversized) __syncthreads();
                // behind the barrier that follows the ticket: the next item, and its R partition in flight while S is probed
                nxtIdx = (uint32_t)__builtin_amdgcn_readfirstlane((int)sNext);
                if (nxtIdx < nItems) nxt = items[nxtIdx];
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // S(it) has landed; bufR is free
                __builtin_amdgcn_sched_barrier(0);
                prefetch_part(R, r_run(nxt.x).base, bufR);
                __builtin_amdgcn_sched_barrier(0);
            }, matches);
        if (nxtIdx >= nItems) break;                           // wave-uniform: every wavefront read the same ticket
        it = nxt;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the last (unused) R prefetch
    // one atomic per wavefront
    for (int off = 32; off > 0; off >>= 1) matches += __shfl_down(matches, off, 64);
    if ((threadIdx.x & 63) == 0 && matches) atomicAdd(&counter_shard(ctr)->prjMatches, matches);
}

// ---------------------------------------------------------------------------
// host-side planning and launch
// ---------------------------------------------------------------------------
// Slots of a fragment that is to hold a Poisson-distributed number of keys of the given mean: mean + 7 sigma (one
// fragment in 10^12 is larger; a run has ~10^6 of them) + a little for tiny means, in whole 16-byte vectors.
static uint32_t frag_cap(double mean)
{
    // whole 128-byte lines: a tile leaves runs of 128 bytes per bin, and with fragments that start inside a line every one
    // of them straddles two (measured at 2^30: 14.8 ms of partitioning with 4580-slot fragments, 12.5 ms with 4576)
    const double c = mean + 7.0 * std::sqrt(mean) + 32.0;
    return ((uint32_t)c + 31u) & ~31u;
}

constexpr uint64_t kFragMinTuples = 1ull << 25;      // below this the exact passes take well under a millisecond
constexpr double kFragMinMean = 256.0;               // smaller fragments are mostly slack

// Fragment geometry of one relation, or C1 = 0 when it has to take the exact passes.
static PrjFrag frag_geometry(uint64_t n, uint32_t radixBits, uint32_t bits1, uint32_t bits2, uint32_t mode)
{
    PrjFrag g{};
    if (n == 0 || bits2 == 0 || mode == 1 || n > (1ull << 31)) return g;
    if (mode == 0 && n < kFragMinTuples) return g;
    const uint32_t F1 = 1u << bits1, F2 = 1u << bits2;
    // pass 1: as many chunks as two rounds of workgroups (2 per CU), fewer while the fragments would get short
    uint32_t C1 = kMaxInFrags;      // 512 .. 4096 measured at 2^30: 11.8 - 11.9 ms throughout
    while (C1 > 256 && (double)n / C1 / F1 < 2048.0) C1 >>= 1;
    while (C1 > 1 && (double)n / C1 / F1 < kFragMinMean) C1 >>= 1;
    const uint64_t chunkLen1 = ((n + C1 - 1) / C1 + kTile - 1) / kTile * kTile;
    const double mean1 = (double)chunkLen1 / F1;
    if (mean1 < kFragMinMean) return g;
    const uint32_t cap1 = frag_cap(mean1);
    // pass 2: ~1024 chunks in all, each a whole number of pass-1 fragments; the join wants <= 16 fragments per partition
    uint32_t C2 = 1024 / F1 ? 1024 / F1 : 1;
    if (C2 > 16) C2 = 16;
    if (C2 > C1) C2 = C1;
    auto mean2_of = [&](uint32_t c2) { return (double)(C1 / c2) * mean1 / F2; };
    while (C2 > 1 && mean2_of(C2) < kFragMinMean) C2 >>= 1;
    const double mean2 = mean2_of(C2);
    if (mean2 < kFragMinMean) return g;
    const uint32_t cap2 = frag_cap(mean2);
    // the buffers hold 8 bytes per tuple (hj_reserve), the positions are 32-bit, and a partition must fit one LDS table
    const uint64_t slots1 = (uint64_t)F1 * C1 * cap1, slots2 = (uint64_t)F1 * F2 * C2 * cap2;
    if (slots1 > 2 * n || slots2 > 2 * n || slots1 >= (1ull << 32) || slots2 >= (1ull << 32)) return g;
    if ((uint64_t)C2 * cap2 > (radixBits >= 16 ? 65535u : kJoinBlockTuples)) return g;
    g.C1 = C1; g.cap1 = cap1; g.chunkLen1 = (uint32_t)chunkLen1;
    g.C2 = C2; g.cap2 = cap2;
    while ((1u << g.log2C2) < C2) ++g.log2C2;
    return g;
}

PrjPlan prj_plan(uint64_t nR, uint64_t nS, uint32_t radixBits, uint32_t mode)
{
    PrjPlan pl{};
    pl.radixBits = radixBits;
    if (radixBits <= 8) { pl.bits1 = radixBits; pl.bits2 = 0; }
    else { pl.bits1 = radixBits / 2; pl.bits2 = radixBits - pl.bits1; }  // prj_thread :814-816
    const uint32_t F1 = 1u << pl.bits1, F2 = 1u << pl.bits2;
    pl.fragR = frag_geometry(nR, radixBits, pl.bits1, pl.bits2, mode);
    pl.fragS = frag_geometry(nS, radixBits, pl.bits1, pl.bits2, mode);
    pl.optimistic = pl.fragR.C1 != 0 && (nS == 0 || pl.fragS.C1 != 0);
    if (pl.optimistic) {
        pl.cnt1Entries = (uint64_t)F1 * (pl.fragR.C1 > pl.fragS.C1 ? pl.fragR.C1 : pl.fragS.C1);
        pl.cnt2EntriesR = (uint64_t)F1 * F2 * pl.fragR.C2;
        pl.cnt2EntriesS = (uint64_t)F1 * F2 * pl.fragS.C2;
    }
    // run_pass lays every relation out with pick_chunk_len of ITS size, and the chunk count is not monotone in
    // the size (chunkLen doubles at the 8192 -> 16384 step: |R| = 40e6 has fewer chunks than |S| = 2^25), so
    // each region takes the larger of the two relations' needs, pass by pass
    for (const uint64_t n : {nR, nS}) {
        if (n == 0) continue;
        const PassLayout l1 = pass_layout(n, 1, F1);
        const PassLayout l2 = pass_layout(n, F1, F2);
        if (l1.maxChunks > pl.maxChunks1) pl.maxChunks1 = l1.maxChunks;
        if (l2.maxChunks > pl.maxChunks2) pl.maxChunks2 = l2.maxChunks;
        for (const PassLayout& l : {l1, l2}) {
            if (l.histEntries > pl.histEntries) pl.histEntries = l.histEntries;
            if (l.scanBlocks > pl.scanBlocks) pl.scanBlocks = l.scanBlocks;
        }
    }
    const uint64_t P = (uint64_t)F1 * F2;
    size_t bytes = 0;
    bytes += align_up(sizeof(uint32_t) * 2, 256);               // seg0
    bytes += align_up(sizeof(uint32_t) * (F1 + 1), 256);        // seg1 (after pass 1)
    bytes += align_up(sizeof(uint32_t) * (F1 + 2), 256);        // chunkBase
    bytes += align_up(sizeof(uint32_t) * pl.histEntries, 256);  // hist / scanned
    bytes += align_up(sizeof(uint32_t) * (pl.scanBlocks + 1), 256);   // block sums
    bytes += 2 * align_up(sizeof(uint32_t) * (P + 1), 256);     // final offsets R, S
    bytes += align_up(sizeof(uint32_t) * pl.cnt1Entries, 256);  // fragment counters: pass 1 (R, then S), pass 2 of R, of S
    bytes += align_up(sizeof(uint32_t) * pl.cnt2EntriesR, 256) + align_up(sizeof(uint32_t) * pl.cnt2EntriesS, 256);
    pl.workspaceBytes = bytes;
    return pl;
}

uint64_t prj_hist_entries_needed(uint64_t n, uint32_t radixBits)
{
    const PrjPlan shape = prj_plan(0, 0, radixBits);            // bit split only
    const uint32_t F1 = 1u << shape.bits1, F2 = 1u << shape.bits2;
    if (n == 0) return 0;
    const uint64_t a = pass_layout(n, 1, F1).histEntries, b = pass_layout(n, F1, F2).histEntries;
    return a > b ? a : b;
}

hipError_t pass_offsets(const void* in, bool in32, const PassRows& rows, const PassParams& p, const PassLayout& l, uint64_t n,
                        uint32_t* hist, uint32_t* sums, uint32_t* segOut, Gate gate, hipStream_t s)
{
    // entries past the live chunks must be zero for the scan to be a prefix of live data only
    hipError_t e = hipMemsetAsync(hist, 0, sizeof(uint32_t) * l.histEntries, s);
    if (e != hipSuccess) return e;
    if (rows.on && rows.stamped)
        hipLaunchKernelGGL(k_radix_hist_rows, dim3((unsigned)l.maxChunks), dim3(kBlock), 0, s, static_cast<const uint64_t*>(in), rows.stamped,
                           p, hist, rows.rowBase);
    else if (in32) hipLaunchKernelGGL(k_radix_hist<true>, dim3((unsigned)l.maxChunks), dim3(kBlock), 0, s, in, p, hist, gate);
    else hipLaunchKernelGGL(k_radix_hist<false>, dim3((unsigned)l.maxChunks), dim3(kBlock), 0, s, in, p, hist, gate);
    if ((e = launch_exclusive_scan_u32(hist, l.histEntries, sums, s, gate)) != hipSuccess) return e;
    const uint32_t nOut = p.nSeg * p.fan + 1;
    hipLaunchKernelGGL(k_seg_offsets, dim3((nOut + kBlock - 1) / kBlock), dim3(kBlock), 0, s, p, hist, (uint32_t)n, segOut);
    return hipGetLastError();
}

// One radix pass: in -> out, segments segIn[nSeg+1] -> segOut[nSeg*fan+1].
// in32: the input already holds bare keys (pass 2); the output always does, unless rows.on.
static hipError_t run_pass(const void* in, bool in32, uint32_t* out, uint64_t n, const uint32_t* segIn, uint32_t nSeg,
                    uint32_t shift, uint32_t bits, uint32_t* segOut, const Work& w, Gate gate, hipStream_t s,
                    hipEvent_t evScatter0 = nullptr, hipEvent_t evScatter1 = nullptr, PassRows rows = PassRows{false, nullptr, 0u})
{
    const uint32_t fan = 1u << bits;
    const PassLayout l = pass_layout(n, nSeg, fan);
    hipLaunchKernelGGL(k_chunk_base, dim3(1), dim3(64), 0, s, segIn, nSeg, l.chunkLen, w.chunkBase);
    const PassParams p{segIn, nSeg, l.chunkLen, w.chunkBase, shift, fan, 0u, 0u};
    const hipError_t e = pass_offsets(in, in32, rows, p, l, n, w.hist, w.sums, segOut, gate, s);
    if (e != hipSuccess) return e;
    if (rows.on && rows.stamped) in = rows.stamped;
    // instance choice measured at 2^30 (profiles/r01_prj_variants.txt): 512 threads x 16
    // elements, no register prefetch, <= 128 VGPRs (2 workgroups per CU); more, smaller workgroups and the
    // prefetching instance were slower or equal
    if (evScatter0) (void)hipEventRecord(evScatter0, s);
    // row-id passes: tiles of 4096 elements of 8 bytes -- the same 128-byte runs at fan 256 and the same 36 KiB of LDS as
    // the key passes (tiles of 8192 spill registers at the 128 that two workgroups per CU leave a thread)
    if (rows.on) hipLaunchKernelGGL((k_radix_scatter<false, false, 512, 4, false, 4>), dim3((unsigned)l.maxChunks), dim3(512), 0, s,
                                    in, static_cast<void*>(out), p, w.hist, gate);
    else if (in32) hipLaunchKernelGGL((k_radix_scatter<true, true, 512, 4, false, 4>), dim3((unsigned)l.maxChunks), dim3(512), 0, s,
                                 in, static_cast<void*>(out), p, w.hist, gate);
    else hipLaunchKernelGGL((k_radix_scatter<false, true, 512, 8, false, 4>), dim3((unsigned)l.maxChunks), dim3(512), 0, s,
                            in, static_cast<void*>(out), p, w.hist, gate);
    if (evScatter1) (void)hipEventRecord(evScatter1, s);
    return hipGetLastError();
}

// The same two passes in the row-id form: tmp and out hold 8-byte {key, row} elements, row = rowBase + position in `in`.
// The stamped copy of the input goes to the buffer pass 1 does not write: out (two passes) or tmp (one).
hipError_t partition_relation_rows(const PrjPlan& pl, const Work& w, const uint64_t* in, uint64_t n, uint32_t rowBase,
                                   uint64_t* tmp, uint64_t* out, uint32_t* finalOff, hipStream_t s, hipEvent_t evS0, hipEvent_t evS1)
{
    uint32_t* const tmp32 = reinterpret_cast<uint32_t*>(tmp);
    uint32_t* const out32 = reinterpret_cast<uint32_t*>(out);
    hipLaunchKernelGGL(k_init_seg, dim3(1), dim3(64), 0, s, w.seg0, (uint32_t)n);
    if (pl.bits2 == 0)
        return run_pass(in, false, out32, n, w.seg0, 1, 0, pl.bits1, finalOff, w, kNoGate, s, evS0, evS1, PassRows{true, tmp, rowBase});
    const hipError_t e = run_pass(in, false, tmp32, n, w.seg0, 1, 0, pl.bits1, w.seg1, w, kNoGate, s, evS0, evS1, PassRows{true, out, rowBase});
    if (e != hipSuccess) return e;
    return run_pass(tmp, false, out32, n, w.seg1, 1u << pl.bits1, pl.bits1, pl.bits2, finalOff, w, kNoGate, s, nullptr, nullptr,
                    PassRows{true, nullptr, 0u});
}

static hipError_t partition_relation(const PrjPlan& pl, const Work& w, const uint64_t* in, uint64_t n,
                              uint32_t* tmp, uint32_t* out, uint32_t* finalOff, Gate gate, hipStream_t s,
                              hipEvent_t evS0 = nullptr, hipEvent_t evS1 = nullptr)
{
    hipLaunchKernelGGL(k_init_seg, dim3(1), dim3(64), 0, s, w.seg0, (uint32_t)n);
    if (pl.bits2 == 0) return run_pass(in, false, out, n, w.seg0, 1, 0, pl.bits1, finalOff, w, gate, s, evS0, evS1);
    const hipError_t e = run_pass(in, false, tmp, n, w.seg0, 1, 0, pl.bits1, w.seg1, w, gate, s, evS0, evS1);   // pass 1, R = 0: tuples -> keys
    if (e != hipSuccess) return e;
    return run_pass(tmp, true, out, n, w.seg1, 1u << pl.bits1, pl.bits1, pl.bits2, finalOff, w, gate, s);    // pass 2, R = bits1
}

// The two histogram-free passes over one relation: tuples -> fragments of tmp -> fragments of out, counts in cnt2.
static hipError_t partition_relation_frag(const PrjPlan& pl, const PrjFrag& g, const Work& w, const uint64_t* in, uint64_t n,
                                   uint32_t* tmp, uint32_t* out, uint32_t* cnt2, Counters* ctr, hipStream_t s,
                                   hipEvent_t evS0 = nullptr, hipEvent_t evS1 = nullptr)
{
    const uint32_t F1 = 1u << pl.bits1, F2 = 1u << pl.bits2;
    const FragPass p1{g.C1, 0u, F1, g.cap1, w.cnt1, (uint32_t)n, g.chunkLen1, 0u, 0u, nullptr};
    if (evS0) (void)hipEventRecord(evS0, s);
    hipLaunchKernelGGL((k_radix_scatter_frag<false, kFrag1Threads, kFrag1Elems, kFrag1Wpe, true>), dim3(g.C1), dim3(kFrag1Threads), 0, s, static_cast<const void*>(in), tmp, p1, ctr);
    if (evS1) (void)hipEventRecord(evS1, s);
    const FragPass p2{g.C2, pl.bits1, F2, g.cap2, cnt2, 0u, 0u, g.C1 / g.C2, g.cap1, w.cnt1};
    hipLaunchKernelGGL((k_radix_scatter_frag<true, kFrag2Threads, kFrag2Elems, kFrag2Wpe>), dim3(F1 * g.C2), dim3(kFrag2Threads), 0, s, static_cast<const void*>(tmp), out, p2, ctr);
    return hipGetLastError();
}

// One relation of a join: its tuples, where its partitions go, and where their description goes -- fragment counts (the
// histogram-free passes, geometry g) and offsets (the exact passes)
struct RelParts { const PrjFrag& g; const uint64_t* in; uint64_t n; uint32_t* out; uint32_t* cnt2; uint32_t* off; };

// Partitions the relations of one join (tmp: scratch of both passes). An optimistic plan runs the histogram-free passes
// (Counters::prjFallback is 0: the caller zeroed it) and enqueues the exact passes behind them, gated on the word a
// fragment that overflows sets: they return at once unless one did. All relations share the word, so the histogram-free
// passes of all of them come first. *exact = the gate of the join over the exact layout.
// ev0 / ev1 (may be null): recorded around the first pass-1 scatter of the first relation.
static hipError_t partition_relations(const PrjPlan& pl, const Work& w, const RelParts* rels, int nRels, uint32_t* tmp, Counters* ctr,
                               hipStream_t s, Gate* exact, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr)
{
    hipError_t e;
    *exact = kNoGate;
    if (pl.optimistic) {
        for (int i = 0; i < nRels; ++i) {
            const RelParts& r = rels[i];
            if ((e = partition_relation_frag(pl, r.g, w, r.in, r.n, tmp, r.out, r.cnt2, ctr, s, ev0, ev1)) != hipSuccess) return e;
            ev0 = ev1 = nullptr;
        }
        *exact = Gate{&ctr->prjFallback, 1ull};
    }
    for (int i = 0; i < nRels; ++i) {
        const RelParts& r = rels[i];
        if ((e = partition_relation(pl, w, r.in, r.n, tmp, r.out, r.off, *exact, s, ev0, ev1)) != hipSuccess) return e;
        ev0 = ev1 = nullptr;
    }
    return hipSuccess;
}

// k_prj_join over one layout of R and S; vs = kNoPart: R's checksum alone. One persistent workgroup per CU.
const PartView kNoPart{nullptr, nullptr, nullptr, PartGeom{0u, 0u, 1u}, false};
static void enqueue_prj_join(const PrjPlan& pl, const PartView& vr, const PartView& vs, int nCU, Counters* ctr, Gate gate, hipStream_t s)
{
    static_assert(kJoinSlots * 2 == 65536, "two 16-bit counters per LDS word cover every 16-bit key remainder");
    const uint32_t P = 1u << pl.radixBits;
    const unsigned grid = P < (unsigned)nCU ? P : (unsigned)nCU;
    const auto kernel = pl.radixBits >= 16 ? k_prj_join<true> : k_prj_join<false>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kJoinThreads), kJoinSlots * sizeof(uint32_t), s,
                       vr.part, vr.off, vr.cnt, vr.g, vs.part, vs.off, vs.cnt, vs.g, pl.radixBits, P, ctr, gate);
}

hipError_t enqueue_prj_items(const PrjResident& res, const uint32_t* offR, const uint32_t* cntR, uint32_t log2CR,
                             const uint32_t* offS, const uint32_t* cntS, uint32_t log2CS, uint32_t P, Counters* ctr, hipStream_t s,
                             bool rless)
{
    hipError_t e;
    if ((e = hipMemsetAsync(res.stats, 0, 4 * sizeof(unsigned long long), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_prj_items_count, dim3((P + kBlock) / kBlock), dim3(kBlock), 0, s, offR, cntR, log2CR,
                       offS, cntS, log2CS, P, ctr, res.itemCnt, res.stats, rless);
    if ((e = launch_exclusive_scan_u32(res.itemCnt, 2ull * P + 1, res.scanSums, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_prj_items_fill, dim3((2 * P + kBlock - 1) / kBlock), dim3(kBlock), 0, s, res.itemCnt, P, res.items, res.stats);
    return hipGetLastError();
}

hipError_t launch_prj(const PrjPlan& pl, const PrjBuffers& buf, const uint64_t* R, uint64_t nR,
                      const uint64_t* S, uint64_t nS, int nCU, Counters* ctr, hipEvent_t evPartDone, hipEvent_t evScatter0,
                      hipEvent_t evScatter1, hipStream_t s)
{
    const Work w = carve(pl, buf.work);
    uint32_t* const tmp = reinterpret_cast<uint32_t*>(buf.tmpA);
    uint32_t* const partR = reinterpret_cast<uint32_t*>(buf.partR);
    uint32_t* const partS = reinterpret_cast<uint32_t*>(buf.partS);
    const RelParts rels[2] = {{pl.fragR, R, nR, partR, w.cnt2R, w.offR}, {pl.fragS, S, nS, partS, w.cnt2S, w.offS}};
    hipError_t e;
    Gate exact;
    if ((e = partition_relations(pl, w, rels, S ? 2 : 1, tmp, ctr, s, &exact, evScatter0, evScatter1)) != hipSuccess) return e;
    if (evPartDone && (e = hipEventRecord(evPartDone, s)) != hipSuccess) return e;
    const uint32_t P = 1u << pl.radixBits;
    if (pl.optimistic)
        enqueue_prj_join(pl, frag_view(partR, w.cnt2R, pl.fragR, P), S ? frag_view(partS, w.cnt2S, pl.fragS, P) : kNoPart, nCU, ctr,
                         Gate{&ctr->prjFallback, 0ull}, s);
    enqueue_prj_join(pl, exact_view(partR, w.offR, nR), S ? exact_view(partS, w.offS, nS) : kNoPart, nCU, ctr, exact, s);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// resident R: hj_prj_build_dev / hj_prj_probe_dev
// ---------------------------------------------------------------------------
namespace {
// everything but the item list depends on the radix bits alone: a later, smaller slice bound never moves R's arrays
struct ResLayout { size_t offR, cnt2R, itemCnt, scanSums, stats, items, end; };
ResLayout res_layout(uint32_t radixBits, uint64_t maxSlice)
{
    const uint64_t P = 1ull << radixBits;
    ResLayout l;
    l.offR = 0;
    l.cnt2R = l.offR + align_up(sizeof(uint32_t) * (P + 1), 256);
    l.itemCnt = l.cnt2R + align_up(sizeof(uint32_t) * P * 16, 256);          // C2 <= 16 (frag_geometry)
    l.scanSums = l.itemCnt + align_up(sizeof(uint32_t) * (2 * P + 1), 256);
    l.stats = l.scanSums + align_up(sizeof(uint32_t) * scan_workspace_words(2 * P + 1), 256);
    l.items = l.stats + 256;
    l.end = l.items + align_up(sizeof(uint2) * (P + maxSlice / kPrjItemS + 2), 256);
    return l;
}
}  // namespace

size_t prj_resident_bytes(uint32_t radixBits, uint64_t maxSlice) { return res_layout(radixBits, maxSlice).end; }

PrjResident prj_resident_carve(void* base, uint32_t radixBits, uint64_t maxSlice)
{
    const ResLayout l = res_layout(radixBits, maxSlice);
    char* p = static_cast<char*>(base);
    return PrjResident{reinterpret_cast<uint32_t*>(p + l.offR), reinterpret_cast<uint32_t*>(p + l.cnt2R),
                       reinterpret_cast<uint32_t*>(p + l.itemCnt), reinterpret_cast<uint32_t*>(p + l.scanSums),
                       reinterpret_cast<uint2*>(p + l.items), reinterpret_cast<unsigned long long*>(p + l.stats)};
}

hipError_t launch_prj_build(const PrjPlan& pl, const PrjBuffers& buf, const PrjResident& res, const uint64_t* R, uint64_t nR,
                            int nCU, Counters* ctr, hipEvent_t evPartDone, hipEvent_t evScatter0, hipEvent_t evScatter1, hipStream_t s)
{
    const Work w = carve(pl, buf.work);
    uint32_t* const tmp = reinterpret_cast<uint32_t*>(buf.tmpA);
    uint32_t* const partR = reinterpret_cast<uint32_t*>(buf.partR);
    hipError_t e;
    // R's side of launch_prj, with the final offsets / fragment counts in the resident buffer instead of the workspace
    Gate exact;
    const RelParts rel{pl.fragR, R, nR, partR, res.cnt2R, res.offR};
    if ((e = partition_relations(pl, w, &rel, 1, tmp, ctr, s, &exact, evScatter0, evScatter1)) != hipSuccess) return e;
    if (evPartDone && (e = hipEventRecord(evPartDone, s)) != hipSuccess) return e;
    // R's decision outlives the probes' S passes, which reuse prjFallback
    if ((e = hipMemcpyAsync(&ctr->prjFallbackR, &ctr->prjFallback, sizeof(unsigned long long), hipMemcpyDeviceToDevice, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(res.stats, 0, 4 * sizeof(unsigned long long), s)) != hipSuccess) return e;
    const uint32_t P = 1u << pl.radixBits;
    if (pl.optimistic) enqueue_prj_join(pl, frag_view(partR, res.cnt2R, pl.fragR, P), kNoPart, nCU, ctr, Gate{&ctr->prjFallback, 0ull}, s);
    enqueue_prj_join(pl, exact_view(partR, res.offR, nR), kNoPart, nCU, ctr, exact, s);
    return hipGetLastError();
}

hipError_t launch_prj_probe(const PrjPlan& planR, uint64_t nR, const PrjPlan& planS, const PrjBuffers& buf, const PrjResident& res,
                            const uint64_t* S, uint64_t nS, int nCU, Counters* ctr, hipEvent_t evPartDone, hipEvent_t evJoin0,
                            hipStream_t s)
{
    const Work w = carve(planS, buf.work);
    uint32_t* const tmp = reinterpret_cast<uint32_t*>(buf.tmpA);
    uint32_t* const partS = reinterpret_cast<uint32_t*>(buf.partS);
    hipError_t e;
    // S's passes: the histogram-free ones when the slice qualifies, the exact ones gated behind them (a Zipf slice falls back)
    if ((e = hipMemsetAsync(&ctr->prjFallback, 0, sizeof(unsigned long long), s)) != hipSuccess) return e;
    const RelParts rel{planS.fragS, S, nS, partS, w.cnt2S, w.offS};
    Gate exact;                                                // not used: the join reads both layouts' words itself
    if ((e = partition_relations(planS, w, &rel, 1, tmp, ctr, s, &exact)) != hipSuccess) return e;
    if (evPartDone && (e = hipEventRecord(evPartDone, s)) != hipSuccess) return e;
    const uint32_t P = 1u << planR.radixBits;
    const uint32_t* const cntR = planR.optimistic ? res.cnt2R : nullptr;
    const uint32_t* const cntS = planS.optimistic ? w.cnt2S : nullptr;
    if ((e = enqueue_prj_items(res, res.offR, cntR, planR.fragR.log2C2, w.offS, cntS, planS.fragS.log2C2, P, ctr, s)) != hipSuccess) return e;
    if (evJoin0 && (e = hipEventRecord(evJoin0, s)) != hipSuccess) return e;
    // one persistent 1024-thread workgroup per CU (the LDS table is 128 KiB of the CU's 160)
    const PartGeom gR = frag_view(nullptr, cntR, planR.fragR, P).g, gS = frag_view(nullptr, cntS, planS.fragS, P).g;
    const auto kernel = planR.radixBits >= 16 ? k_prj_probe_items<true> : k_prj_probe_items<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)nCU), dim3(kJoinThreads), kJoinSlots * sizeof(uint32_t), s,
                       reinterpret_cast<const uint32_t*>(buf.partR), res.offR, cntR, gR, (uint32_t)nR,
                       static_cast<const uint32_t*>(partS), w.offS, cntS, gS, (uint32_t)nS,
                       res.items, res.itemCnt + 2ull * P, res.stats, planR.radixBits, ctr);
    return hipGetLastError();
}

hipError_t prj_set_attributes()
{
    // per device (hj_create calls this with its device current): the LDS join tables, and the stable split's staging through shard_set_attributes
    hipError_t e;
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_prj_join<false>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, kJoinSlots * sizeof(uint32_t))) != hipSuccess) return e;
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_prj_join<true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, kJoinSlots * sizeof(uint32_t))) != hipSuccess) return e;
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_prj_probe_items<false>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, kJoinSlots * sizeof(uint32_t))) != hipSuccess) return e;
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_prj_probe_items<true>),
                                 hipFuncAttributeMaxDynamicSharedMemorySize, kJoinSlots * sizeof(uint32_t))) != hipSuccess) return e;
    if ((e = prj_pairs_set_attributes()) != hipSuccess) return e;
    if ((e = prj_agg_set_attributes()) != hipSuccess) return e;
    return shard_set_attributes();
}

}  // namespace hj
