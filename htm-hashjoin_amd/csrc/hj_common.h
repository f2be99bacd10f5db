// hj_common.h -- what every device file of the library uses: the constants, the slot hash, the wavefront and workgroup
// primitives, the counters with their shards and valid range, the gate, and the generic exclusive scan (hj_scan.hip).
// Nothing of one subsystem belongs here. gfx950 only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

namespace hj {

// A table slot holds (inputIndex << 32 | key32). All-ones is "empty" so that a
// 64-bit atomicMin implements index priority (smaller input index wins).
constexpr uint64_t kEmpty = ~0ull;
// Slots past tableSize that always stay empty: the probe walk does not wrap
// (NoCCHashBuild.hpp:74-75 does curSlot++ without & tableMask).
constexpr uint32_t kTableSlack = 16;

// Home slot of a key: (key >> hshift) & (tableSize - 1). hshift = 0 is the reference's hash (NoCCHashBuild.hpp:41);
// a radix shard of a multi-GPU join holds only keys with the same low log2(shards) bits, which therefore carry no
// information inside the shard and are shifted out of the slot number (hshift = log2(shards)). The slot still stores
// the whole key.
__host__ __device__ inline uint64_t home_slot(uint32_t key, uint32_t hshift, uint64_t mask) { return (uint64_t)(key >> hshift) & mask; }

// Home slot in the bucketised table of --algo htm (HTMHashBuild.hpp:41-45,176): a bucket is 4 consecutive 8-byte
// slots (three tuples + one word of count / overflow link = 32 bytes, one HBM sector), bucket = (key / 3) &
// (numBuckets - 1); mask = 4 * numBuckets - 1. The three tuple slots are filled by the same index-priority protocol as
// the open-addressing table with a probe budget of 3: every tuple of a bucket has the same home slot, so the bucket ends
// up holding the three lowest-indexed tuples in index order and the rest run out of budget = the reference's conflicts.
__host__ __device__ inline uint64_t home_slot_htm(uint32_t key, uint64_t mask) { return ((uint64_t)(key / 3u) << 2) & mask; }
template <bool HTM>
__host__ __device__ inline uint32_t home32(uint32_t key, uint32_t hshift, uint32_t mask32)
{
    if constexpr (HTM) return ((key / 3u) << 2) & mask32;
    else return (key >> hshift) & mask32;
}

// A lane's rank among the set lanes of a 64-bit lane mask (a ballot, or a per-lane mask of peers): the number of set bits
// below the lane. v_mbcnt_lo + v_mbcnt_hi -- two instructions, the mask may stay in scalar registers -- instead of two
// ANDs with a "lanes below me" mask and two popcounts.
__device__ __forceinline__ uint32_t lane_rank(unsigned long long m)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
#else
    (void)m; return 0u;         // host pass of hipcc: parsed, never called
#endif
}

// (index << 32 | key): a table slot, a deferred tuple, an entry of a conflict list
__host__ __device__ __forceinline__ uint64_t pack64(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; }
// sums over the wavefront (32- or 64-bit values), valid in lane 0. Several at once, in place: their shuffles interleave,
// one step of every sum after the other, instead of one chain of six dependent shuffles per sum.
template <class... T>
__device__ __forceinline__ void wave_sum_all(T&... v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ((v += __shfl_down(v, off, 64)), ...);
}
template <class T>
__device__ __forceinline__ T wave_sum(T v) { wave_sum_all(v); return v; }
// A runtime flag becomes a compile-time one: f(std::true_type{}) or f(std::false_type{}). The launchers nest it to pick a
// kernel's instantiation -- and list, in ONE place per kernel, the combinations that exist at all.
template <class F>
inline void with_flag(bool flag, F&& f) { if (flag) f(std::true_type{}); else f(std::false_type{}); }

// Optional shard-membership check riding on build and probe (hj_set_shard_check): a tuple is "foreign" when its
// destination digit ((key - bias) >> shift) & mask differs from id. mask = 0 (and id = 0) switches it off at no
// cost in branches: every tuple's digit is then 0.
struct ShardCheck { uint32_t mask, shift, bias, id; };
__host__ __device__ inline bool is_foreign(uint32_t key, const ShardCheck& sc) { return (((key - sc.bias) >> sc.shift) & sc.mask) != sc.id; }

constexpr int kBlock = 256;          // 4 wavefronts of 64
constexpr int kWave = 64;

// exclusive scan over the NT threads of a workgroup: v -> the sum of the threads below; total: the sum of all. wsum: NT / 64
// words of LDS. Two barriers; every thread of the workgroup calls it.
template <int NT = kBlock>
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* wsum /*[NT/64]*/, uint32_t& total)
{
    // inclusive scan inside the wavefront
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t n = __shfl_up(inc, off, 64);
        if (lane >= off) inc += n;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t wbase = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) {
        const uint32_t s = wsum[k];
        if (k < w) wbase += s;
        tot += s;
    }
    total = tot;
    __syncthreads();
    return wbase + inc - v;
}

// words launch_sample_locality works on: 8 (five totals, [7] = the ticket) + 8 per workgroup of the sampler (its own counts)
constexpr int kSampleBlocks = 256;
constexpr int kSampleWords = 8 + 8 * kSampleBlocks;

// Device-resident counters, zeroed at the start of a build. One cache line
// apart is not needed: each is touched once per wavefront at kernel end.
struct Counters {
    unsigned long long conflicts;
    unsigned long long conflictSum;
    unsigned long long inputSum;
    unsigned long long matches;
    unsigned long long tableSumHalf;
    unsigned long long tableSumFull;
    unsigned long long badKeys;      // tuples with payload bits set or value 0
    unsigned long long prjMatches;
    unsigned long long prjChecksum;
    unsigned long long prjOverflowParts; // partitions joined in several LDS blocks
    unsigned long long deferred;         // variant 2: tuples finished by the global-atomic phase
    // Variant 2 touches only the table blocks some tuple can reach; everything else is neither cleared
    // nor read. usedLoInv / usedHi1 collect (max of ~block) and (max of block+1) over claimed blocks
    // and deferred targets; k_finalize_range turns them into the valid SLOT range
    // [validLo, validHiEx): a home slot outside it cannot match anything (k_probe skips it), slots in
    // [validLo, validHiEx + 512) hold defined values.
    // THE contract, for every build that sets the range and every reader of the table: the test is on the HOME slot --
    // home in [validLo, validHiEx) is probed, and its walk stays inside the defined slots. Everything outside
    // [validLo, validHiEx + 512) keeps what an earlier build on the context left, in that build's format, and is never
    // looked at. validHiEx is at most 1024 slots above the last slot a tuple can land on (window: the last block touched
    // + 1 is probed; rings: one ring from the granule the window stands on), and validHiEx + 512 >= tableSize makes the
    // whole table valid (set_valid_range). The bucketised probes (k_htm_probe, HtmTable) state the same per bucket: a
    // bucket is read when its four slots are defined, slot + 3 < validHiEx + 512; k_htm_sums and hj_export_buckets count
    // the buckets [validLo / 4, (validHiEx + 512) / 4). Both conventions agree on every bucket a build can fill: buckets
    // with a home in [validHiEx, validHiEx + 512) are defined and empty.
    unsigned long long usedLoInv, usedHi1;
    unsigned long long validLo, validHiEx;
    unsigned long long foreign;      // tuples of the build / probe inputs that fail the shard check (ShardCheck)
    // Variant 3 (hj_build_wave.hip): the stretch of the table its wavefronts own and write whole, [ownLo, ownHiEx)
    unsigned long long ownLo, ownHiEx;
    // Build kernel the device-side locality pre-round picked (hj_params.buildVariant 0): written by the sampler's last workgroup (k_sample_locality),
    // read through the Gate of every build kernel enqueued behind it, reported as hj_result.buildVariant
    unsigned long long variant;
    // what the pre-round would have picked had every variant been enqueued (k_sample_locality). hj_build_dev only enqueues
    // the kernels of the variant the PREVIOUS build of the context preferred (+ the classic rings behind the compact
    // ones, + global atomics: always correct); the pick is taken among those, and this word tells the host what to
    // enqueue next time (the kernel stores it into pinned host memory as well, read without waiting at the next build)
    unsigned long long preferred;
    // --algo htm (hj_htm.hip): overflow buckets linked, sum of the tuples they hold
    unsigned long long htmOverflowBuckets, htmOverflowSum;
    // raised by the LDS chain phase (k_htm_chain_lds) or by the routing of the deferred phase's conflicts when an input
    // does not fit them: the host then redoes the build without routing and chains with the generic kernels. A mask of
    // causes (kChainBail*: the table next to the caps, below in this file)
    unsigned long long htmChainBail;
    // PRJ, histogram-free partitioning (hj_prj.hip): set to 1 by the scatter kernel that finds a fragment too small;
    // the rest of that path then returns at once and the exact (histogram) path, gated on this word, runs instead
    unsigned long long prjFallback;
    // PRJ with a resident R (hj_prj_build_dev): R's prjFallback, copied here once R's passes are done. prjFallback itself
    // is reset before every probe's S passes; the join reads both words to pick each relation's layout
    unsigned long long prjFallbackR;
    // Open-addressing table formats (k_build_wave<COMPACT>, hj_build_wave.hip). tableFormat says what the table buffer
    // holds after a build: kFormatSlots8 = one 8-byte slot (index << 32 | key) per table slot, all ones = empty (every
    // build but the compact one); kFormatKeys4 = one 4-byte KEY per table slot, 0xFFFFFFFF = empty (the index words only
    // order the inserts; the compact build settles every order inside its LDS rings and never writes them out);
    // kFormatCodes1 = one code BYTE per table slot, 0xFF = empty (SlotCode below: the planar ring build of large tables). k_probe,
    // k_table_sums and hj_export_table read the word. compactFail: raised by the compact build when it meets something
    // only the classic builds can handle; k_wave_decide then resets the counters and hands over to the classic build.
    unsigned long long tableFormat, compactFail;
    // Planar retire of the classic ring build (k_build_wave<PLANAR>, hj_build_wave.hip): the table ends as kFormatKeys4 with
    // the index words in a plane of their own behind the keys (planar_index_plane). planarFail: why that build handed
    // over -- bit 0: a slice's dirty log did not fit (an input that defers nearly everything), bit 1: key 0xFFFFFFFF, the
    // 4-byte empty pattern; bit 2 (the slot-code road, kWaveCodes, only): a key whose high part no code byte holds.
    // k_wave_fixup then resets the counters and sets packedRedo = 1, the word the packed classic
    // build enqueued behind it is gated on. Counters::variant stays 3 on both roads.
    unsigned long long planarFail, packedRedo;
    // the locality pre-round's sample of hj_build_dev (k_sample_locality: launch_sample_locality's eight words, [7] = its
    // ticket) -- inside this struct so that the one memset at the start of a build clears them too
    unsigned int fit[kSampleWords];
    // The sums every wavefront contributes to at the END of a kernel (above: conflicts, conflictSum, inputSum, matches,
    // badKeys, prjMatches, prjChecksum, deferred, foreign, and the two maxima usedLoInv / usedHi1) are collected in 64
    // shards, each on a 128-byte line of its own, picked by wavefront number. Thousands of wavefronts finish together, and
    // their atomics on ONE address are served one after the other: measured 95 us at the end of k_probe (8192 wavefronts)
    // and 67 us at the end of k_build_wave whatever the size -- most of those kernels at 2^22 tuples, 17 % / 4 % at 2^27,
    // and 70 us of the deferred phase at 2^30. The fields above hold the totals only after fold_counter_shards() (host,
    // after the copy back); on the device nothing reads the sums, and the finalize kernels fold the two maxima themselves.
    struct alignas(128) Shard {
        unsigned long long conflicts, conflictSum, inputSum, matches, badKeys, prjMatches, prjChecksum, deferred, foreign;
        unsigned long long usedLoInv, usedHi1;
    };
    static constexpr int kShards = 64;
    Shard shard[kShards];
};

// minimum over the wavefront, result wave-uniform: four DPP steps inside each row of 16, then the four rows
__device__ __forceinline__ uint32_t wave_umin(uint32_t v)
{
    auto step = [](uint32_t x, const int ctrl) {
        uint32_t o;
        switch (ctrl) {     // the control word must be an immediate
            case 0: o = (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0xB1, 0xF, 0xF, true); break;   // quad_perm [1,0,3,2]
            case 1: o = (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x4E, 0xF, 0xF, true); break;   // quad_perm [2,3,0,1]
            case 2: o = (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x141, 0xF, 0xF, true); break;  // row_half_mirror
            default: o = (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x140, 0xF, 0xF, true); break; // row_mirror
        }
        return o < x ? o : x;
    };
    v = step(v, 0); v = step(v, 1); v = step(v, 2); v = step(v, 3);
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    const uint32_t ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}

// the shard of the calling wavefront
__device__ inline Counters::Shard* counter_shard(Counters* ctr)
{
    return &ctr->shard[(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) & (Counters::kShards - 1)];
}
// The two maxima (usedLoInv / usedHi1: the 512-slot blocks an LDS build claimed or deferred into) as the finalize kernels
// need them. One wavefront, a shard per lane: what was written directly + the 64 shards; the result in every lane.
struct UsedBlocks { unsigned long long loInv, hi1; };
__device__ __forceinline__ UsedBlocks fold_used_blocks(const Counters* __restrict__ ctr)
{
    static_assert(Counters::kShards == 64, "one shard per lane of the single wavefront the finalize kernels run as");
    unsigned long long loInv = ctr->shard[threadIdx.x & 63].usedLoInv, hi1 = ctr->shard[threadIdx.x & 63].usedHi1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long a = __shfl_xor(loInv, off, 64), b = __shfl_xor(hi1, off, 64);
        loInv = a > loInv ? a : loInv; hi1 = b > hi1 ? b : hi1;
    }
    return UsedBlocks{ctr->usedLoInv > loInv ? ctr->usedLoInv : loInv, ctr->usedHi1 > hi1 ? ctr->usedHi1 : hi1};
}
// The valid slot range [lo, hiEx) of a build (Counters::validLo / validHiEx). The 512 slots past it are read too, and
// probe walks wrap at the table's end: a range that reaches it makes the whole table valid.
__device__ __forceinline__ void set_valid_range(Counters* __restrict__ ctr, unsigned long long lo, unsigned long long hiEx, uint64_t tableSize)
{
    if (hiEx + 512 >= tableSize) { lo = 0; hiEx = tableSize; }
    ctr->validLo = lo; ctr->validHiEx = hiEx;
}
// host, on a copy of the counters: totals = what was added directly + the shards
inline void fold_counter_shards(Counters* h)
{
    for (int i = 0; i < Counters::kShards; ++i) {
        Counters::Shard& s = h->shard[i];
        h->conflicts += s.conflicts; h->conflictSum += s.conflictSum; h->inputSum += s.inputSum; h->matches += s.matches;
        h->badKeys += s.badKeys; h->prjMatches += s.prjMatches; h->prjChecksum += s.prjChecksum; h->deferred += s.deferred;
        h->foreign += s.foreign;
        h->usedLoInv = s.usedLoInv > h->usedLoInv ? s.usedLoInv : h->usedLoInv;
        h->usedHi1 = s.usedHi1 > h->usedHi1 ? s.usedHi1 : h->usedHi1;
        s = Counters::Shard{};
    }
}

// Device-side choice between the build variants (hj_build_dev must stay asynchronous: no host read-back). The host
// enqueues the kernels of EVERY candidate variant; each looks at the word the pre-round wrote and returns at once
// unless it is the chosen one. word = nullptr: no gate (the variant was fixed on the host).
// alt: a second value that opens the gate (the pre-pass shared by the compact and the classic ring build)
struct Gate { const unsigned long long* word; unsigned long long want; unsigned long long alt = ~0ull; };
__device__ inline bool gate_closed(const Gate& g)
{
    if (g.word == nullptr) return false;
    const unsigned long long v = *g.word;
    return v != g.want && v != g.alt;
}
constexpr Gate kNoGate{nullptr, 0ull};

constexpr uint32_t kNoRow = 0xFFFFFFFFu;        // HJ_NO_ROW: the R row of a LEFT row without a match, a NULL entry of a gather map
typedef unsigned int u4 __attribute__((ext_vector_type(4)));

// HIP events recorded right before and right after ONE kernel launch (the dominant build kernel of a variant): its device
// time for the roofline, without the pre-pass and the gated-off launches of the other variants around it
struct KernelEvents { hipEvent_t before = nullptr, after = nullptr; };     // null: the launch is not bracketed

// ---- exclusive scan of a uint32 array in place (defined in hj_scan.hip) ----
// a workgroup of kBlock threads scans kScanTile words; sums: scan_workspace_words(n) = ceil(n / kScanTile) + 1 words of workspace
constexpr int kScanPerThread = 16;
constexpr int kScanTile = kBlock * kScanPerThread;  // 4096

size_t scan_workspace_words(uint64_t n);
hipError_t launch_exclusive_scan_u32(uint32_t* data, uint64_t n, uint32_t* sums, hipStream_t s, Gate gate = kNoGate);

}  // namespace hj
