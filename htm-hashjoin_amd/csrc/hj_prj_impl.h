// hj_prj_impl.h -- internal to the radix-join family (hj_prj.hip, hj_prj_pairs.hip, hj_prj_agg.hip, hj_shard.hip): what
// the materialising and the aggregating form and the shard split share with the partition passes and the LDS join --
// the geometry of a pass, the chunk lookup of its kernels, the tail loop of the join, the workspace, and the pass
// runners, which have one definition in hj_prj.hip. Not for the host layer: that sees hj_prj.h.
#pragma once

#include "hj_prj.h"

namespace hj {

constexpr int kTile = 8192;                       // largest scatter tile (elements); chunk lengths are multiples of it
constexpr int kMaxFan = 256;                      // <= 8 radix bits per pass
constexpr uint32_t kJoinSlots = 32768;            // LDS table slots (uint32) = 128 KiB
constexpr uint32_t kJoinBlockTuples = 24576;      // R tuples per LDS build (load <= 0.75)
constexpr int kJoinThreads = 1024;
constexpr uint32_t kEmpty32 = 0xFFFFFFFFu;

struct PassParams {
    const uint32_t* segOff;     // [nSeg + 1] tuple offsets of the input segments
    uint32_t nSeg;
    uint32_t chunkLen;          // multiple of kTile
    const uint32_t* chunkBase;  // [nSeg + 1] exclusive prefix of chunks per segment
    uint32_t shift, fan;        // bin = ((key - bias) >> shift) & (fan - 1)
    uint32_t bias;              // 0, or 1 for the range split of 1-based DataGen keys (shard split only)
    uint32_t zeroBad;           // shard split only: a tuple with payload bits set counts and travels as key 0, which the
                                // receiving build reports (HJ_ERR_KEY_RANGE); PRJ reads the key word alone, as mc does
};

// Finds the segment of chunk c (largest s with chunkBase[s] <= c). Wave-uniform.
__device__ __forceinline__ uint32_t find_segment(const uint32_t* __restrict__ chunkBase, uint32_t nSeg, uint32_t c)
{
    uint32_t lo = 0, hi = nSeg;  // invariant: chunkBase[lo] <= c < chunkBase[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (chunkBase[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

struct ChunkRange { uint32_t seg, local, nLocal, begin, end; };

__device__ __forceinline__ ChunkRange chunk_range(const PassParams& p, uint32_t c)
{
    ChunkRange r;
    r.seg = find_segment(p.chunkBase, p.nSeg, c);
    r.local = c - p.chunkBase[r.seg];
    r.nLocal = p.chunkBase[r.seg + 1] - p.chunkBase[r.seg];
    const uint32_t sb = p.segOff[r.seg], se = p.segOff[r.seg + 1];
    r.begin = sb + r.local * p.chunkLen;
    const uint64_t e = (uint64_t)r.begin + p.chunkLen;
    r.end = e < se ? (uint32_t)e : se;
    return r;
}

// hist index of (segment, bin, local chunk)
__device__ __forceinline__ uint64_t hist_index(const PassParams& p, const ChunkRange& r, uint32_t bin)
{
    return (uint64_t)p.chunkBase[r.seg] * p.fan + (uint64_t)bin * r.nLocal + r.local;
}

__device__ __forceinline__ uint32_t next_pow2_u32(uint32_t v)
{
    // NEXT_POW_2, parallel_radix_join.c:66-76
    v--; v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16; v++;
    return v;
}

constexpr int kJoinPre = 16;   // keys per thread and relation prefetched in registers (16 x 1024 = 16384)
constexpr int kTailPre = 8;    // loads in flight per thread in the loops past the register prefetch

// f(element) for element i of [from, n) of a run starting at slot `base`, kTailPre loads in flight per thread (a one-load
// loop waits a whole HBM round trip per key: the rest of a 2^16-tuple item is 48 keys per thread)
template <typename T, typename F>
__device__ __forceinline__ void for_run(const T* __restrict__ part, uint32_t base, uint32_t from, uint32_t n, F&& f)
{
    for (uint32_t i0 = from + threadIdx.x; i0 < n; i0 += kTailPre * kJoinThreads) {
        T k[kTailPre];
#pragma unroll
        for (int u = 0; u < kTailPre; ++u) {
            const uint32_t i = i0 + (uint32_t)u * kJoinThreads;
            k[u] = part[base + (i < n ? i : n - 1)];                  // clamped: i0 < n, so n >= 1
        }
#pragma unroll
        for (int u = 0; u < kTailPre; ++u)
            if (i0 + (uint32_t)u * kJoinThreads < n) f(k[u]);
    }
}

// ---- host side: how a pass is cut, the workspace, the pass runners ----
inline uint32_t pick_chunk_len(uint64_t n)
{
    // aim for ~4096 chunks (>= 2 per CU-slot), whole tiles, 4Ki..64Ki tuples
    uint64_t len = n / 4096;
    len = (len + kTile - 1) / kTile * kTile;
    if (len < (uint64_t)kTile) len = kTile;
    if (len > 65536) len = 65536;
    return (uint32_t)len;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct PassLayout { uint32_t chunkLen; uint64_t maxChunks; uint64_t histEntries; uint64_t scanBlocks; };

inline PassLayout pass_layout(uint64_t n, uint32_t nSeg, uint32_t fan)
{
    PassLayout l;
    l.chunkLen = pick_chunk_len(n);
    l.maxChunks = n / l.chunkLen + nSeg + 1;
    l.histEntries = l.maxChunks * fan;
    l.scanBlocks = (l.histEntries + kScanTile - 1) / kScanTile;
    return l;
}

struct Work {
    uint32_t *seg0, *seg1, *chunkBase, *hist, *sums, *offR, *offS, *cnt1, *cnt2R, *cnt2S;
};
// the workspace of a plan (PrjPlan::workspaceBytes, prj_plan) as the passes use it
inline Work carve(const PrjPlan& pl, void* base)
{
    const uint32_t F1 = 1u << pl.bits1, F2 = 1u << pl.bits2;
    const uint64_t P = (uint64_t)F1 * F2;
    char* p = static_cast<char*>(base);
    Work w;
    w.seg0 = reinterpret_cast<uint32_t*>(p); p += align_up(sizeof(uint32_t) * 2, 256);
    w.seg1 = reinterpret_cast<uint32_t*>(p); p += align_up(sizeof(uint32_t) * (F1 + 1), 256);
    w.chunkBase = reinterpret_cast<uint32_t*>(p); p += align_up(sizeof(uint32_t) * (F1 + 2), 256);
    w.hist = reinterpret_cast<uint32_t*>(p); p += align_up(sizeof(uint32_t) * pl.histEntries, 256);
    w.sums = reinterpret_cast<uint32_t*>(p); p += align_up(sizeof(uint32_t) * (pl.scanBlocks + 1), 256);
    w.offR = reinterpret_cast<uint32_t*>(p); p += align_up(sizeof(uint32_t) * (P + 1), 256);
    w.offS = reinterpret_cast<uint32_t*>(p); p += align_up(sizeof(uint32_t) * (P + 1), 256);
    w.cnt1 = reinterpret_cast<uint32_t*>(p); p += align_up(sizeof(uint32_t) * pl.cnt1Entries, 256);
    w.cnt2R = reinterpret_cast<uint32_t*>(p); p += align_up(sizeof(uint32_t) * pl.cnt2EntriesR, 256);
    w.cnt2S = reinterpret_cast<uint32_t*>(p);
    return w;
}

// The row-id form of a pass (HJ_FLAG_KEEP_ROW_IDS): 8-byte {key, row} elements out. stamped != nullptr: the pass that
// reads the tuples -- its histogram writes their elements, row = rowBase + position, to `stamped`, and the scatter moves
// those; nullptr: `in` holds elements already.
struct PassRows { bool on; uint64_t* stamped; uint32_t rowBase; };

// Defined in hj_prj.hip, which holds the kernels they launch.
// seg[0 .. 1] = {0, n}: the one segment a first pass reads; chunkBase[s] = chunks in front of segment s
void launch_init_seg(uint32_t* seg, uint32_t n, hipStream_t s);
void launch_chunk_base(const uint32_t* segOff, uint32_t nSeg, uint32_t chunkLen, uint32_t* chunkBase, hipStream_t s);
// The front half of a pass, behind launch_chunk_base: the histogram of every chunk, its scan (the chunks' write cursors) and
// the offsets of the output segments. rows.stamped: the row-id histogram, which also writes the {key, row} elements.
hipError_t pass_offsets(const void* in, bool in32, const PassRows& rows, const PassParams& p, const PassLayout& l, uint64_t n,
                        uint32_t* hist, uint32_t* sums, uint32_t* segOut, Gate gate, hipStream_t s);
// The two exact passes in the row-id form: tmp and out hold 8-byte {key, row} elements, row = rowBase + position in `in`.
hipError_t partition_relation_rows(const PrjPlan& pl, const Work& w, const uint64_t* in, uint64_t n, uint32_t rowBase,
                                   uint64_t* tmp, uint64_t* out, uint32_t* finalOff, hipStream_t s,
                                   hipEvent_t evS0 = nullptr, hipEvent_t evS1 = nullptr);
// The work items of a probe against the resident R (no host round trip): items per partition, one scan, fill.
// cntR / cntS: the fragment counts of a relation whose plan was optimistic, else nullptr.
hipError_t enqueue_prj_items(const PrjResident& res, const uint32_t* offR, const uint32_t* cntR, uint32_t log2CR,
                             const uint32_t* offS, const uint32_t* cntS, uint32_t log2CS, uint32_t P, Counters* ctr, hipStream_t s,
                             bool rless = false);
// per device, for prj_set_attributes: the dynamic LDS of the kernels of hj_prj_pairs.hip, hj_prj_agg.hip and hj_shard.hip
hipError_t prj_pairs_set_attributes();
hipError_t prj_agg_set_attributes();
hipError_t shard_set_attributes();

}  // namespace hj
