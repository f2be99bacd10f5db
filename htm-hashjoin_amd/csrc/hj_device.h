// hj_device.h -- shared declarations between the HIP kernels (hj_kernels.hip,
// hj_prj.hip) and the C-ABI implementation (hj_api.hip). gfx950 only.
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
constexpr unsigned long long kFormatSlots8 = 0, kFormatKeys4 = 1, kFormatCodes1 = 2;
// Slot codes (kFormatCodes1): with the identity hash a stored key sits d < probeLength slots above its
// home slot = key & (tableSize - 1), so the slot number, d and the key's bits above the table size say everything: one
// byte per slot, code = (hi << dbits) | d with dbits = ceil(log2(probeLength)), hi = key >> log2(tableSize). Codes use 7
// bits, the empty pattern is 0xFF. THE place where a code is made and read: build, fix-up, probe, sums and export call it.
constexpr uint32_t kCodeEmpty = 0xFFu, kCodeBits = 7;
struct SlotCode {
    uint32_t dbits;      // bits of the displacement
    uint32_t tbits;      // log2(tableSize), 32 for a table of 2^32 slots: no high bits, and nothing shifts by 32
    uint32_t hiCap;      // high parts a code can hold: 2^(7 - dbits), 0 when dbits > 7 (no code at all)
    __host__ __device__ uint32_t dmask() const { return (1u << dbits) - 1u; }
    __host__ __device__ uint32_t hi(uint32_t key) const { return tbits >= 32 ? 0u : key >> tbits; }
    // every 32-bit key has a code: the road has no failure cause of its own
    __host__ __device__ bool fits_all() const { return dbits <= kCodeBits && (32 - tbits) + dbits <= kCodeBits; }
    __host__ __device__ bool overflows(uint32_t key) const { return hi(key) >= hiCap; }
    // the first key that has no code (0: every key has one)
    __host__ __device__ uint32_t key_limit() const { return (fits_all() || tbits >= 32) ? 0u : (uint32_t)((uint64_t)hiCap << tbits); }
    __host__ __device__ uint32_t encode(uint32_t key, uint32_t slot) const { return (hi(key) << dbits) | ((slot - key) & dmask()); }
    __host__ __device__ uint32_t decode(uint32_t code, uint32_t slot, uint32_t mask32) const
    {
        const uint32_t home = (slot - (code & dmask())) & mask32;
        return tbits >= 32 ? home : home | ((code >> dbits) << tbits);
    }
};
__host__ __device__ inline SlotCode slot_code(uint64_t tableSize, uint32_t probeLen)
{
    SlotCode c;
    c.dbits = probeLen <= 1 ? 0u : 32u - (uint32_t)__builtin_clz(probeLen - 1u);      // ceil(log2(probeLength))
    c.tbits = (uint32_t)__builtin_popcountll(tableSize - 1);                           // tableSize is a power of two, at most 2^32
    c.hiCap = c.dbits <= kCodeBits ? 1u << (kCodeBits - c.dbits) : 0u;
    return c;
}
// Ring words (DESIGN.md 4.2a-bis "Build"): what a slot of a wavefront's LDS ring holds on the slot-code road. Inside a ring
// only the ORDER of the tuples matters, and a wavefront's tuples are numbered by their offset from the first position it
// reads; the key is what the slot number and the code say. So word = (rel << 7) | code -- 4 bytes, and the key never sits
// in LDS. rel is unique per tuple of a ring and monotone in the tuple index: order and equality of two words are those of
// their rel, and the empty pattern (all ones) is above every word the layout rule lets in. THE place where a ring word is
// made, stepped and read: the build kernel and hj_ring_word_layout_info call it.
struct RingWord {
    static constexpr uint32_t kEmpty = 0xFFFFFFFFu;
    static constexpr uint32_t kRelCap = (1u << (32 - kCodeBits)) - 1u;   // rel < kRelCap: no word equals the empty pattern
    SlotCode sc;
    uint32_t hiShift, hiMask;     // the key's high part lands on its place in the code in one shift and one mask
    // the layout rule: a wavefront reads fewer than `positions` positions (a slice's length bounds them)
    __host__ __device__ static bool holds(uint64_t positions) { return positions <= kRelCap; }
    // the word a tuple tries its home slot with (d = 0). A key without a code (forced road, cause 4) keeps its rel whole:
    // the table is thrown away, the ring stays in order
    __host__ __device__ uint32_t at_home(uint32_t rel, uint32_t key) const { return (rel << kCodeBits) | ((key >> hiShift) & hiMask); }
    __host__ __device__ static uint32_t rel(uint32_t word) { return word >> kCodeBits; }
    __host__ __device__ static uint32_t code(uint32_t word) { return word & ((1u << kCodeBits) - 1u); }
    // tries the tuple has left, the slot it stands at included: at least 1 for every word in a ring or a queue
    __host__ __device__ uint32_t tries_left(uint32_t word, uint32_t probeLen) const { return probeLen - (word & sc.dmask()); }
    // k slots on, k < tries_left: the displacement stays below probeLength and never carries into the high part. Whether
    // the budget is spent is decided from tries_left BEFORE the step, and a dropped tuple's key is read before it too.
    __host__ __device__ static uint32_t step(uint32_t word, uint32_t k = 1u) { return word + k; }
    // the key of the tuple that stands at slot pos with this word (SlotCode::decode: the wrap at the table's end included)
    __host__ __device__ uint32_t key(uint32_t word, uint32_t pos, uint32_t mask32) const { return sc.decode(code(word), pos, mask32); }
};
__host__ __device__ inline RingWord ring_word(const SlotCode& sc)
{
    const bool high = sc.tbits < 32 && sc.dbits <= kCodeBits;
    return RingWord{sc, high ? sc.tbits - sc.dbits : 0u, high ? ((sc.hiCap - 1u) << sc.dbits) : 0u};
}
// Planar retire: where the index plane starts in the table buffer of (tableSize + kTableSlack) 8-byte words -- behind the
// key plane and ITS slack (the probe reads up to probeLength - 1 keys past the table's end and must find them empty), at
// the next multiple of 128 bytes so that the granules' 512-byte runs stay on whole lines in both planes. One uint32 input
// index per slot, 0xFFFFFFFF = empty; walks on it wrap, so it needs no slack of its own and ends exactly at the buffer's end.
constexpr uint64_t kPlanarIndexGap = 2 * kTableSlack;      // uint32 words between the key plane's end and the index plane
static_assert(kPlanarIndexGap * sizeof(uint32_t) % 128 == 0, "whole lines");
__host__ __device__ inline uint32_t* planar_index_plane(uint64_t* table, uint64_t tableSize)
{
    return reinterpret_cast<uint32_t*>(table) + tableSize + kPlanarIndexGap;
}

// A tuple that left its LDS window (variants 2 and 3): the slot it had reached and (index << 32 | key)
struct DeferredEntry { uint64_t pos; uint64_t packed; };
// HIP events recorded right before and right after ONE kernel launch (the dominant build kernel of a variant): its device
// time for the roofline, without the pre-pass and the gated-off launches of the other variants around it
struct KernelEvents { hipEvent_t before = nullptr, after = nullptr; };     // null: the launch is not bracketed

// ---- launch wrappers (defined in hj_kernels.hip) ---------------------------
// Inputs come in two element formats: 8-byte DataGen tuples (key32 = false; value = key, payload bits must be 0)
// or bare 32-bit keys (key32 = true; what the multi-GPU exchange delivers). Index of element i = idxBase + i.
// One build as every build launcher sees it: filled once per build (hj_api.hip), handed to each of its launches
struct BuildJob {
    const void* R; bool key32; uint64_t n; uint64_t idxBase;                           // the input
    uint64_t* table; uint64_t tableSize; uint32_t hshift, probeLen; ShardCheck sc;     // the table and how it is addressed
    int nCU; Counters* ctr; hipStream_t s;                                             // where it runs
};
// fullRange != nullptr: also marks the whole table valid (variant 1 clears and may touch all of it): one launch less
void launch_fill_empty(uint64_t* table, uint64_t nSlots, Gate gate, hipStream_t s, Counters* fullRange = nullptr, uint64_t tableSize = 0);
void launch_build_atomic_min(const BuildJob& job, Gate gate);
// the probe and the checksums read Counters::tableFormat on the device: either table format, one launch
void launch_probe(const void* S, bool key32, uint64_t n, const uint64_t* table, uint64_t tableSize, uint32_t hshift,
                  uint32_t probeLen, ShardCheck sc, Counters* ctr, hipStream_t s);
void launch_table_sums(const uint64_t* table, uint64_t tableSize, uint64_t halfSlots, uint32_t probeLen, Counters* ctr, hipStream_t s);
void launch_zipf_lookup(const int* raw, uint64_t n, const double* lut, const uint32_t* alphabet, uint32_t alphabetSize,
                        uint64_t* out, hipStream_t s);
// Marks the whole table valid (variant 1 clears and may touch all of it).
void launch_set_full_range(uint64_t tableSize, Counters* ctr, Gate gate, hipStream_t s);
// multi-GPU destination split (defined in hj_prj.hip: one order-preserving radix pass, tuples in, keys out);
// destination = (key >> digitShift) & (nShards - 1)
size_t shard_work_bytes(uint64_t n, uint32_t nShards);
hipError_t launch_shard_hist(const uint64_t* in, uint64_t n, uint32_t nShards, uint32_t digitShift, void* work,
                             unsigned long long* counts, hipStream_t s);
hipError_t launch_shard_scatter_ordered(const uint64_t* in, uint64_t n, uint32_t nShards, uint32_t digitShift, void* work,
                                        uint32_t* outKeys, hipStream_t s);

// ---- ownership build (defined in hj_build_own.hip) ---------------------------
size_t own_queue_bytes(uint64_t rSize);
size_t own_owner_bytes(uint64_t tableSize);
bool   own_supported(uint64_t tableSize);
// fitCount[0] = sampled tuples outside variant 2's window, [1] = tuples sampled, [2] = outside variant 3's ring,
// [3] = sampled tuples that share their home slot with another tuple of their tile (duplicate keys),
// [4] = sampled rows of 64 tuples with disorder beyond 64 positions (8 words in all)
// pick.ctr != nullptr: the workgroup of the sample that finishes last decides on the device -- ctr->preferred = the variant
// the sample asks for (variant_for_sample: the thresholds the host applies), ctr->variant = the best one among the
// variants whose kernels are enqueued behind the sample (allowedMask: bit v set = variant v is; bit 1, global atomics,
// always is), *hostPreferred (pinned host memory, may be null) = preferred, stored by the kernel itself.
struct SamplePick {
    Counters* ctr = nullptr;
    unsigned long long* hostPreferred = nullptr;
    uint32_t allowedMask = 0x1E;
    bool canOwn = false, canWave = false, canCompact = false;
};
// zeroed: fitCount's eight words are zero already (no memset of its own)
hipError_t launch_sample_locality(const void* R, bool key32, uint64_t n, uint64_t tableSize, uint32_t hshift, uint32_t nSample,
                                  unsigned int* fitCount, hipStream_t s, bool htm = false,    // htm: the bucketised table's hash
                                  SamplePick pick = SamplePick{}, bool zeroed = false);
// the best enqueued variant for a preferred one: itself if enqueued, else the next looser build that is, else (nothing
// looser is enqueued: a context whose relation lost its locality since the last build) the tightest LDS build that is --
// rings and window are correct on any input (what falls outside goes through their deferred phases: global atomics,
// slow for that one step); the compact rings only with the classic ones behind them
__host__ __device__ inline uint32_t variant_among_allowed(uint32_t preferred, uint32_t allowedMask)
{
    for (uint32_t v = preferred; v >= 1; --v)
        if ((allowedMask >> v) & 1u) {
            if (v == 3 && preferred == 2) continue;      // loose locality: global atomics before the rings, if they are there
            return v;
        }
    for (uint32_t v = preferred + 1; v <= 3; ++v)
        if ((allowedMask >> v) & 1u) return v;
    return ((allowedMask >> 3) & 1u) ? 3u : 1u;
}
// variant worth taking for a sample (outside variant 2's window, tuples seen, outside variant 3's ring)
// dup = sampled tuples that share their home slot with another tuple of their tile: rings with few duplicate keys take the
// compact table (4: 2.6 against 3.4 ms build at 2^30 on unique keys, and a 4-byte probe), rings with many keep the classic
// one (3): on `uniform` (37 % of the tuples repeat a key) the build is bound by the vector work of its retry rounds, the
// compact build adds forced rounds to it (4.0 against 3.6 ms) and the whole step comes out even.
__host__ __device__ inline uint32_t variant_for_sample(uint64_t outOwn, uint64_t seen, uint64_t outWave, bool canOwn, bool canWave,
                                                      bool canCompact = false, uint64_t dup = 0, uint64_t farRows = 0)
{
    // farRows: sampled rows of 64 tuples that reach above the row two further on (disorder beyond 64 positions: more than
    // the compact build's seam zones cover -- it would start, give up and hand over to the classic rings)
    if (canWave && outWave * 128 <= seen) return (canCompact && dup * 8 <= seen && farRows == 0) ? 4 : 3;
    // the workgroup window while it can take at least a quarter of the tuples itself: what it defers is finished by global
    // atomics at about their own pace (2^27, local_shuffle, build + probe: W = 2^12 defers 36 % -> 2.8 ms against 5.8 ms
    // for the global-atomic build; 2^13: 71 % -> 4.7 / 5.8; 2^14: 88 % -> 5.6 / 5.9; 2^16: 97 % -> 6.6 / 5.9 -- since the
    // deferred queue is sliced per workgroup; with one global queue counter the window lost from 8 % on)
    if (canOwn && outOwn * 4 <= seen * 3) return 2;
    return 1;
}
hipError_t own_set_attributes();          // per device, at hj_create
// phase A (LDS window) -> clear of unowned blocks -> phase B (deferred tuples).
// Writes every table slot exactly once: no separate launch_fill_empty needed.
// deferCounts: kOwnMaxChunks words (the deferred queue is sliced by phase-A workgroup; entries per slice)
// htmConflicts != nullptr: the bucketised table of --algo htm through the workgroup window (tuples only, probeLen 3): the
// tuples that find their bucket full are listed per chunk, plus one last slice for the deferred phase's (own_conflict_layout)
struct OwnBufs { void* owner; void* queue; uint32_t* deferCounts; uint64_t* htmConflicts = nullptr; uint32_t* htmCounts = nullptr; };
hipError_t launch_build_own(const BuildJob& job, const OwnBufs& buf, Gate gate, int parts, KernelEvents kev = {});   // parts: 1 = phase A (kev brackets its kernel), 2 = the rest, 3 = both
constexpr uint32_t kOwnMaxChunks = 8192;
// The window build's chunk geometry for n tuples on nCU compute units and its kernels' constants (own_layout: what
// hj_own_layout_info reports; the launcher takes the same geometry and the same phase-B parts)
struct OwnLayout { uint64_t chunkLen, nChunks, tileTuples, blockSlots, winBlocks, backBlocks, seamDivisor, minTableSlots, deferredParts, maxProbeLen; };
OwnLayout own_layout(uint64_t n, int nCU);

// ---- wavefront-private build (defined in hj_build_wave.hip) ------------------
// geometry the locality sampler (k_sample_locality) needs to predict what k_build_wave would defer
constexpr uint32_t kWvGranShift = 7;      // retire granule: 128 slots = 1 KiB
constexpr uint32_t kWvRingGran = 8;       // ring = 8 granules = 1024 slots = 8 KiB per wavefront
constexpr uint32_t kWvTileTuples = 512;   // tuples per wavefront tile
constexpr uint32_t kWvWavesPerCu = 16;    // resident wavefronts per CU (what the rings' LDS allows)
constexpr uint32_t kWvMaxRounds = 8;      // chunks <= resident wavefronts x rounds (wave_layout)
size_t wave_lds_bytes();
bool   wave_supported(uint64_t tableSize);
// How n tuples are cut into chunks on nCU compute units (wave_layout: the ONLY place that works it out; hj_wave_layout_info
// reports it) and the constants the seam zones of the compact build are made of, taken from the kernel's own
struct WaveLayout {
    uint64_t chunkLen, nChunks, sliceLen;
    uint32_t tileTuples, granSlots, ringGran, look, overlap, shadow, tail, predCap, compactMaxProbe;
};
WaveLayout wave_layout(uint64_t n, int nCU);
// The bounds buffer (WaveBufs::bounds): six arrays of uint32 words, one entry per chunk, sized for the most chunks a device
// of nCU compute units is ever cut into. THE description of that buffer: whoever sizes, carves or reads it goes through here.
struct WaveScratch {
    uint32_t* raw;       // pre-pass: the granule each chunk's seam sample starts in (kNone: no valid tuple)
    uint32_t* bounds;    // [nChunks + 1] chunk c owns granules [bounds[c], bounds[c + 1])
    uint32_t* starts;    // [nChunks + 1] chunk c's tuples are R[starts[c] .. starts[c + 1])
    uint32_t* dcounts;   // entries at the front of each slice of the deferred queue (compact build: crossers out)
    uint32_t* ccounts;   // bucketised table: entries in each slice of the conflict list
    uint32_t* pcounts;   // compact build: crossers each chunk let in (its list: the tail of its queue slice)
    // planar retire: entries of each slice's dirty log. The SAME words as ccounts: a build is planar or bucketised, never
    // both (launch_build_wave refuses it; k_build_wave and k_wave_deferred have no such instantiation)
    uint32_t* lcounts;
    size_t words;
    WaveScratch(int nCU, void* buf)
    {
        const size_t maxChunks = (size_t)kWvWavesPerCu * kWvMaxRounds * (size_t)nCU;
        words = 0;
        auto take = [&](size_t k) { uint32_t* const p = buf ? static_cast<uint32_t*>(buf) + words : nullptr; words += k; return p; };
        raw = take(maxChunks); bounds = take(maxChunks + 1); starts = take(maxChunks + 1);
        dcounts = take(maxChunks); ccounts = take(maxChunks); pcounts = take(maxChunks);
        lcounts = ccounts;
    }
    size_t bytes() const { return words * sizeof(uint32_t); }
};
inline size_t wave_bounds_bytes(int nCU) { return WaveScratch(nCU, nullptr).bytes(); }
size_t wave_queue_bytes(uint64_t n, int nCU);   // deferred queue: one slice per chunk (its tenants: hj_build_wave.hip, "queue slice")
// bounds pre-pass -> k_build_wave -> valid range + edge fill -> phase B. queue: wave_queue_bytes(n, nCU), used as one
// slice per chunk (a wavefront's deferred tuples go to ITS slice: no atomics in the kernel).
// parts: kWavePre = the seam / bounds pre-pass, kWaveMain = the build kernel (kev brackets it), kWaveTail = valid range,
// edge fill and the deferred phase. mode kWaveCompact: the compact build (4-byte table, no deferred phase) -- its main
// part is k_build_wave<COMPACT> + the seam check + k_wave_decide, which on failure resets the counters and sets
// Counters::variant = 3 so that the classic build enqueued behind it (gated on that word) redoes the table;
// its tail is the edge fill alone. The pre-pass is the same for all modes (gate it with alt).
// mode kWavePlanar: the classic build with the planar retire (k_build_wave<PLANAR>: keys and indices leave for two planes,
// the table ends as kFormatKeys4). Its tail is valid range, edge fill of both planes, the deferred walks on the index
// plane and k_wave_fixup, which on Counters::planarFail sets Counters::packedRedo = 1: the word to gate the packed classic
// build behind it on. Tuples and bare keys; never the bucketised table.
constexpr int kWavePre = 1, kWaveMain = 2, kWaveTail = 4, kWaveAll = 7;
constexpr int kWaveClassic = 0, kWaveCompact = 1, kWavePlanar = 2, kWaveCodes = 3;
// mode kWaveCodes: kWavePlanar with the key plane replaced by one code byte per slot (SlotCode above; tuples only). The
// table ends as kFormatCodes1; a key without a code raises Counters::planarFail bit 2 and the packed build redoes it.
// htmRoute: the deferred phase files its conflicts under the chunk that owns their bucket (the LDS chain phase needs that)
struct WaveBufs { void* bounds; void* queue; uint64_t* htmConflicts = nullptr; bool htmRoute = false; };
hipError_t launch_build_wave(const BuildJob& job, const WaveBufs& buf, Gate gate, int parts, int mode = kWaveClassic, KernelEvents kev = {});
bool wave_compact_supported(uint64_t tableSize, uint32_t probeLen);
// mode kWaveCodes takes this build: its ring of 4-byte words (RingWord) fits the table and holds the layout's chunks
bool wave_codes_supported(uint64_t n, int nCU, uint64_t tableSize);
void launch_set_variant(Counters* ctr, uint32_t v, hipStream_t s);
// htmConflicts != nullptr: the bucketised table of --algo htm (home_slot_htm, probeLen must be 3, tuples only); every
// tuple that runs out of budget is appended as (index << 32 | key) to its chunk's slice of htmConflicts (slices and
// their counts as wave_conflict_layout describes: WaveScratch::ccounts)
struct WaveSlices { uint32_t nChunks, sliceLen; const uint32_t* counts; };
WaveSlices own_conflict_layout(uint64_t n, int nCU, void* countsBuf);
size_t own_conflict_bytes(uint64_t n, int nCU);
size_t own_conflict_count_bytes(uint64_t n, int nCU);
WaveSlices wave_conflict_layout(uint64_t n, int nCU, void* boundsBuf);
size_t wave_conflict_bytes(uint64_t n, int nCU);

// ---- bucketised table of --algo htm (defined in hj_htm.hip) -----------------
uint32_t htm_num_buckets(uint64_t rSize);         // nextpow2(rSize / 3 + 1), HTMHashBuild.hpp:61-62
hipError_t launch_htm_build_global(const uint64_t* R, uint64_t n, uint32_t sliceLen, uint32_t nSlices, uint64_t* table,
                                   uint64_t tableSlots, uint64_t idxBase, uint64_t* conflicts, uint32_t* ccounts, Counters* ctr,
                                   hipStream_t s);
// per-bucket conflict counts -> ovfCount, overflow buckets needed per bucket -> groups (to be scanned in place)
hipError_t launch_htm_count(const uint64_t* conflicts, const uint32_t* ccounts, uint32_t nSlices, uint32_t sliceLen,
                            uint32_t numBuckets, unsigned int* ovfCount, uint32_t* groups, hipStream_t s);
hipError_t launch_htm_chains(const uint64_t* conflicts, const uint32_t* ccounts, uint32_t nSlices, uint32_t sliceLen,
                             uint64_t* table, uint32_t numBuckets, const unsigned int* ovfCount, const uint32_t* ovfBase,
                             uint64_t* overflow, uint64_t overflowCapBuckets, Counters* ctr, hipStream_t s);
// the chain phase in LDS, after the ring build with routed conflicts (hj_htm.hip): count -> partGroups[nSlices * parts] (overflow
// buckets per part; scan it, one word more for the total) and info (htm_chain_info_words words); fill builds the chains
constexpr int kChainThreads = 512;
constexpr uint32_t kChainCountCap = 12288;           // buckets a slice's conflicts may span (k_htm_chain_count's LDS counters)
constexpr uint32_t kChainCap = 3072;                 // buckets per part = the fill's LDS counters; tuple slots of its overflow image (36 KiB: 4 workgroups per CU)
constexpr uint32_t kChainMaxParts = 16;
constexpr uint32_t kChainPartTuples = 4224;          // htm_chain_parts: a part per this many positions of a slice
// Counters::htmChainBail is a mask of WHY the LDS chain phase gave up (atomicOr; hj_htm_chain_info reports it):
//   bit  constant              raised by                      when
//   0    kChainBailSliceFull   k_htm_chain_count, the router  a slice took more conflicts than sliceLen (m > sliceLen; no place left)
//   1    kChainBailStray       k_htm_chain_count              a conflict lies outside its slice's bucket range [B0, B1)
//   2    kChainBailSpan        k_htm_chain_count              span > kChainCountCap
//   3    kChainBailSub         k_htm_chain_count              sub > kChainCap
//   4    kChainBailImage       k_htm_chain_count              a part needs more than kChainCap / 3 overflow buckets
// A slice over its length raises bit 0 alone (nothing else of it is looked at); bits 1 to 3 of a slice are raised together;
// bit 4 only by a slice that passed them. A workgroup that starts after the mask has become non-zero returns at once, so
// the mask read back is a NON-EMPTY SUBSET of the causes the input holds, never a cause it does not hold.
constexpr unsigned long long kChainBailSliceFull = 1, kChainBailStray = 2, kChainBailSpan = 4, kChainBailSub = 8, kChainBailImage = 16;
uint32_t htm_chain_parts(uint32_t sliceLen);
// the host's rule: the LDS phase is tried when its scratch (groups per part + total, info words) fits the per-bucket arrays.
// Only tables of two buckets or fewer fail it, and the rings need 256 (wave_supported): behind buildVariant 3 it always
// holds -- it guards the scratch arrays, it decides nothing
bool htm_chain_tries(uint32_t nSlices, uint32_t sliceLen, uint32_t numBuckets);
size_t htm_chain_info_words(uint32_t nSlices, uint32_t sliceLen);
hipError_t launch_htm_chain_count(const uint64_t* conflicts, const uint32_t* ccounts, const uint32_t* bounds, uint32_t nSlices,
                                  uint32_t sliceLen, uint32_t numBuckets, uint32_t* partGroups, uint32_t* info, Counters* ctr, hipStream_t s);
hipError_t launch_htm_chain_fill(const uint64_t* conflicts, uint32_t nSlices, uint32_t sliceLen, uint32_t numBuckets, const uint32_t* partBase,
                                 const uint32_t* info, uint64_t* table, uint64_t* overflow, Counters* ctr, hipStream_t s);
void launch_htm_probe(const uint64_t* S, uint64_t n, const uint64_t* table, uint32_t numBuckets, const uint64_t* overflow,
                      Counters* ctr, hipStream_t s);
void launch_htm_sums(const uint64_t* table, uint32_t numBuckets, const uint64_t* overflow, Counters* ctr, hipStream_t s);
// exclusive scan of a uint32 array in place (defined in hj_prj.hip); sums: ceil(n / 4096) + 1 words of workspace
size_t scan_workspace_words(uint64_t n);
hipError_t launch_exclusive_scan_u32(uint32_t* data, uint64_t n, uint32_t* sums, hipStream_t s, Gate gate = kNoGate);

// ---- materialising probe (defined in hj_pairs.hip) --------------------------
// where hj_probe_pairs_dev writes: the two gather-map planes, their length, and the 64-bit cursor the workgroups claim
// their runs from (zeroed before the launch; its final value = pairs found, written or not)
// Join kinds (hj_join_kind): `kind` picks the kernels' instantiation. cursor[1] (zeroed with the cursor) collects the S
// elements without a match under HJ_JOIN_LEFT and is touched by no other kind; HJ_JOIN_SEMI / ANTI never touch plane r.
struct PairsOut { uint32_t* s; uint32_t* r; uint64_t capacity; unsigned long long* cursor; };
typedef unsigned int u4 __attribute__((ext_vector_type(4)));
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
constexpr uint32_t kNoRow = 0xFFFFFFFFu;        // HJ_NO_ROW: the R row of a LEFT row without a match, a NULL entry of a gather map
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

// The launch of either kernel: k(mapS, mapR, nPairs, sRowBase, sRows, rRows, cols, nCols, out, S's marks).
// sMarks / rMarks: the two planes in RMarks' layout, either may be null.
template <class Kernel, class Cols>
inline hipError_t launch_pair_filter(Kernel kernel, const uint32_t* mapS, const uint32_t* mapR, uint64_t nPairs, uint32_t sRowBase, uint32_t sRows,
                                     uint32_t rRows, const Cols& cols, uint32_t nCols, const PairsOut& out, uint32_t* sMarks, uint32_t* rMarks,
                                     hipStream_t s)
{
    if (nPairs == 0) return hipSuccess;
    const RMarks mkS{sMarks, sRowBase, sMarks ? sRows : 0u}, mkR{rMarks, 0u, rMarks ? rRows : 0u};
    const PairsOutMarked o = pairs_out_of<true>(out, &mkR);
    const dim3 grid((uint32_t)((nPairs + kFilterBlockPairs - 1) / kFilterBlockPairs));        // nPairs <= 2^32 - 1: <= 2^22 workgroups
    hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, mapS, mapR, nPairs, sRowBase, sRows, rRows, cols, nCols, o, mkS);
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

// ---- gather through a row map (defined in hj_gather.hip) ---------------------
// One column of hj_gather_dev as the kernel takes it (hj_gather_col, include/htm_hashjoin.h, field for field), and the
// columns of a call, passed by value in the kernel arguments.
constexpr uint32_t kGatherMaxCols = 8;        // HJ_GATHER_MAX_COLS
struct GatherCol { const void* src; void* dst; uint32_t width, reserved; uint64_t fill[2]; };
struct GatherCols { GatherCol col[kGatherMaxCols]; };
// dst_c[k] = src_c[map[k] - rowBase] for k in [0, nRows) and c in [0, nCols); an entry that is HJ_NO_ROW, or that lies at or
// behind srcRows once the base is off, reads nothing and gives the column's fill. valid (may be null): one bit per row,
// whole words up to ceil(nRows / 32). counts[0] += the HJ_NO_ROW entries, counts[1] += the out-of-range ones. The caller
// has checked widths, alignment and nRows, srcRows <= 2^32 - 1.
hipError_t launch_gather(const uint32_t* map, uint64_t nRows, uint32_t rowBase, uint64_t srcRows, const GatherCols& cols, uint32_t nCols,
                         uint32_t* valid, unsigned long long* counts, hipStream_t s);
// The same on columns in the Arrow layout (hj_gather_col2, include/htm_hashjoin.h, field for field; defined in
// hj_gather_cols.hip): a source validity plane and 32-bit offsets per column, both optional. Columns that are fixed and
// have neither plane go through launch_gather as they are. work: the context's workspace for the variable-length columns
// of a call, which run one behind the other -- gather2_work_words(nRows) 32-bit words: the scan's own words, then one
// 64-bit partial sum per workgroup. totals: kGatherMaxCols 64-bit words, written here (0 for a fixed column): the bytes
// the rows of column c take. The caller has checked what the header says hj_gather2_dev refuses.
struct GatherCol2 { const void* src; void* dst; const uint32_t* srcOff; uint32_t* dstOff; const uint32_t* srcValid; uint32_t* dstValid;
                    uint64_t capacity; uint32_t width, flags; uint64_t fill[2]; };
struct GatherCols2 { GatherCol2 col[kGatherMaxCols]; };
size_t gather2_work_words(uint64_t nRows);
hipError_t launch_gather2(const uint32_t* map, uint64_t nRows, uint32_t rowBase, uint64_t srcRows, const GatherCols2& cols, uint32_t nCols,
                          uint32_t* valid, unsigned long long* counts, unsigned long long* totals, uint32_t* work, hipStream_t s);

// ---- joins on real key columns (defined in hj_keys.hip) ----------------------
// The key columns of a call as the kernels take them, by value in the kernel arguments: the hash reads one side
// (KeyCols2), the verify step both (KeyCols2SR). They are hj_key_col2's (include/htm_hashjoin.h): per column and side the
// values (fixed width) or the bytes buffer (width 0), the rows + 1 offsets of a variable-length column (else null) and the
// validity plane (null: no NULLs); flags: HJ_KEY_NULLS_EQUAL. An hj_key_col is the same column with null offsets, null
// planes and flags 0: hj_key_hash_dev, hj_key_hash_host and hj_pairs_verify_dev fill the descriptor that way.
// launch_key_hash2: out[i] = the join word of row i (the header's hash over the row's key columns, & mask) as an 8-byte
// tuple. mask is the effective one (never 0). nRows is also what bounds the validity words the hash reads: ceil(nRows / 32).
// launch_pairs_verify2: candidate pairs (mapS[k] - sRowBase, mapR[k]) -> the pairs whose key columns are equal as the header
// defines it, to `out` as the pairs kernels write theirs (out.cursor: two 64-bit words, zeroed before the launch: kept
// pairs, then the candidates dropped as HJ_NO_ROW or outside sRows / rRows, which are never dereferenced). Every kept pair
// sets bit s of sMarks and bit r of rMarks (RMarks' layout; either may be null).
// The caller has checked what the header says the entry points refuse, and nRows, nPairs <= 2^32 - 1.
constexpr uint32_t kKeyMaxCols = 4;           // HJ_KEY_MAX_COLS
struct KeyCols2 { const void* p[kKeyMaxCols]; const uint32_t* off[kKeyMaxCols]; const uint32_t* valid[kKeyMaxCols];
                  uint32_t width[kKeyMaxCols], flags[kKeyMaxCols]; };
struct KeyCols2SR { const void* s[kKeyMaxCols]; const void* r[kKeyMaxCols]; const uint32_t* sOff[kKeyMaxCols]; const uint32_t* rOff[kKeyMaxCols];
                    const uint32_t* sValid[kKeyMaxCols]; const uint32_t* rValid[kKeyMaxCols]; uint32_t width[kKeyMaxCols], flags[kKeyMaxCols]; };
constexpr uint32_t kKeyNullsEqual = 1u;       // HJ_KEY_NULLS_EQUAL
hipError_t launch_key_hash2(const KeyCols2& cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint64_t* out, hipStream_t s);
void key_hash2_host(const KeyCols2& cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint64_t* out);   // the same body in a host loop
hipError_t launch_pairs_verify2(const uint32_t* mapS, const uint32_t* mapR, uint64_t nPairs, uint32_t sRowBase, uint32_t sRows,
                                uint32_t rRows, const KeyCols2SR& cols, uint32_t nCols, PairsOut out, uint32_t* sMarks, uint32_t* rMarks,
                                hipStream_t s);

// ---- rows of one table grouped by their key columns (defined in hj_groups.hip, a part of hj_keys.hip) ----
// launch_key_groups: rep[i] = the lowest row with row i's key (kNoRow: NULL-keyed), firstRows = the rows with rep[i] == i,
// ascending, cut at `capacity` (null with capacity 0), group[i] = the position of rep[i] among them (null: not wanted).
// work: key_groups_work_bytes(nRows) bytes -- the table of key_groups_slots(nRows) 8-byte slots, filled with EMPTY here on
// s, the first-row plane, its popcounts and their scan, the sweep's counts; key_groups_total: where the number of groups
// lies in it after the call (one 32-bit word). ctr: four 64-bit words, zeroed here -- probe steps beyond the home slot, word
// collisions, NULL-keyed rows, the failure word. mask is the effective one (never 0). The caller has checked what the
// header says the entry point refuses, and nRows <= 2^32 - 2.
uint64_t key_groups_slots(uint64_t nRows);
size_t key_groups_work_bytes(uint64_t nRows);
const uint32_t* key_groups_total(const void* work, uint64_t nRows);
hipError_t launch_key_groups(const KeyCols2& cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint32_t* rep, uint32_t* group,
                             uint32_t* firstRows, uint64_t capacity, void* work, unsigned long long* ctr, hipStream_t s);
// the same hash and compare bodies around a sequential table; out: hj_key_groups_host's
void key_groups_host(const KeyCols2& cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint32_t* rep, uint32_t* group, uint32_t* firstRows,
                     uint64_t capacity, uint64_t out[8]);

// ---- join conditions beyond equality (defined in hj_where.hip) ----------------
// The terms of a call as the kernel takes them, by value in the kernel arguments (hj_where_term, include/htm_hashjoin.h):
// term t holds for the pair (s, r) when s[t][s] op[t] r[t][r], both elements of width[t] bytes read as type[t], and neither
// is NULL (sValid / rValid: the validity plane of that side, null: no NULLs).
constexpr uint32_t kWhereMaxTerms = 4;        // HJ_WHERE_MAX_TERMS
constexpr uint32_t kCmpEq = 0, kCmpNe = 1, kCmpLt = 2, kCmpLe = 3, kCmpGt = 4, kCmpGe = 5;     // hj_cmp_op
constexpr uint32_t kValUint = 0, kValInt = 1, kValFloat = 2;                                  // hj_val_type
struct WhereTerms { const void* s[kWhereMaxTerms]; const void* r[kWhereMaxTerms]; const uint32_t* sValid[kWhereMaxTerms];
                    const uint32_t* rValid[kWhereMaxTerms]; uint32_t width[kWhereMaxTerms], type[kWhereMaxTerms], op[kWhereMaxTerms]; };
// Pairs (mapS[k] - sRowBase, mapR[k]) -> the pairs whose terms all hold, to `out` as launch_pairs_verify2 writes its kept pairs
// (out.cursor: two 64-bit words, zeroed before the launch: kept pairs, then the pairs dropped as HJ_NO_ROW or outside sRows /
// rRows, which are never dereferenced); the marks as there. The caller has checked the terms and nPairs <= 2^32 - 1.
hipError_t launch_pairs_where(const uint32_t* mapS, const uint32_t* mapR, uint64_t nPairs, uint32_t sRowBase, uint32_t sRows,
                              uint32_t rRows, const WhereTerms& terms, uint32_t nTerms, PairsOut out, uint32_t* sMarks, uint32_t* rMarks,
                              hipStream_t s);
// the same pairs in a host loop over host pointers, the kept ones in input order; info: kept, written, 0, dropped (may be null)
void pairs_where_host(const uint32_t* mapS, const uint32_t* mapR, uint64_t nPairs, uint32_t sRowBase, uint32_t sRows, uint32_t rRows,
                      const WhereTerms& terms, uint32_t nTerms, uint32_t* outS, uint32_t* outR, uint64_t capacity, uint32_t* sMarks,
                      uint32_t* rMarks, uint64_t* info);

// What the condition step (hj_where.hip) and the as-of step (hj_asof.hip) share: how two elements compare, how one orders,
// and a term's loads for the lane's pairs of the pair-filter frame.
// the raw word of a FLOAT element as a double: binary32 widens exactly
__host__ __device__ __forceinline__ double where_real(uint64_t raw, uint32_t width)
{
    return width == 4u ? (double)__builtin_bit_cast(float, (uint32_t)raw) : __builtin_bit_cast(double, raw);
}

// Whether  a OP b  holds, a and b the zero-extended raw words of two valid elements of `width` bytes read as `type`.
// Unordered (a NaN on either side): lt and eq are false, so EQ, LT and LE fail by themselves and NE holds.
__host__ __device__ __forceinline__ bool where_holds(uint32_t type, uint32_t width, uint32_t op, uint64_t a, uint64_t b)
{
    bool lt, eq, un = false;
    if (type == kValFloat) {
        const double x = where_real(a, width), y = where_real(b, width);
        lt = x < y; eq = x == y; un = x != x || y != y;
    } else {
        // INT: sign-extended from its width, then the sign bit flipped -- the order of the signed values as unsigned ones
        const uint32_t sh = type == kValInt ? 64u - 8u * width : 0u;
        const uint64_t flip = type == kValInt ? 1ull << 63 : 0ull;
        const uint64_t x = (uint64_t)((int64_t)(a << sh) >> sh) ^ flip, y = (uint64_t)((int64_t)(b << sh) >> sh) ^ flip;
        lt = x < y; eq = x == y;
    }
    switch (op) {
        case kCmpEq: return eq;
        case kCmpNe: return !eq;
        case kCmpLt: return lt;
        case kCmpLe: return lt || eq;
        case kCmpGt: return !(lt || eq || un);
        default: return !(lt || un);                                  // kCmpGe
    }
}

// The order key of the as-of step: the zero-extended raw word of a valid element that is no NaN -> an unsigned 64-bit word
// that orders as the values do and is equal exactly where where_holds calls two values equal. Integers: where_holds's
// sign-extend and flip. Floats: widened to double, -0.0 taken for +0.0, then the bits folded -- a negative's all
// complemented, a positive's sign bit set -- so that negatives order below positives. The forward ops (LT, LE: the SMALLEST
// R value is wanted) complement the key: every kernel takes a maximum.
__host__ __device__ __forceinline__ uint64_t asof_key(uint32_t type, uint32_t width, uint32_t op, uint64_t raw)
{
    uint64_t key;
    if (type == kValFloat) {
        double x = where_real(raw, width);
        if (x == 0.0) x = 0.0;                                        // -0.0 == 0.0: one key for both
        const uint64_t bits = __builtin_bit_cast(uint64_t, x);
        key = (bits >> 63) ? ~bits : bits | (1ull << 63);
    } else {
        const uint32_t sh = type == kValInt ? 64u - 8u * width : 0u;
        key = (uint64_t)((int64_t)(raw << sh) >> sh) ^ (type == kValInt ? 1ull << 63 : 0ull);
    }
    return (op == kCmpLt || op == kCmpLe) ? ~key : key;
}

// One term's loads for the lane's pairs: both elements of every pair, and with kValid the validity word of either side
// (null plane: all valid), all of them before the first compare. The loads are unconditional -- see the pair-filter
// frame for why.
template <class E, bool kValid>
__device__ __forceinline__ void where_load(const void* sCol, const void* rCol, const uint32_t* sValid, const uint32_t* rValid,
                                           const uint32_t (&si)[kFilterLanePairs], const uint32_t (&ri)[kFilterLanePairs],
                                           uint64_t (&a)[kFilterLanePairs], uint64_t (&b)[kFilterLanePairs],
                                           uint32_t (&vs)[kFilterLanePairs], uint32_t (&vr)[kFilterLanePairs])
{
    if constexpr (kValid) {
#pragma unroll
        for (uint32_t j = 0; j < kFilterLanePairs; ++j) { vs[j] = sValid ? sValid[si[j] >> 5] : ~0u; vr[j] = rValid ? rValid[ri[j] >> 5] : ~0u; }
    }
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) { a[j] = static_cast<const E*>(sCol)[si[j]]; b[j] = static_cast<const E*>(rCol)[ri[j]]; }
    __builtin_amdgcn_sched_barrier(0);                                // no compare moves up between the loads: it would wait there
}

// element i of a column of `width` bytes, zero-extended (the host loops)
inline uint64_t where_elem_host(const void* col, uint32_t width, uint32_t i)
{
    uint64_t v = 0;
    memcpy(&v, static_cast<const uint8_t*>(col) + (size_t)i * width, width);      // little-endian: the low bytes
    return v;
}

// ---- as-of joins: one best match per S row (defined in hj_asof.hip) -----------
// The term of a call as the kernels take it (hj_asof_term, include/htm_hashjoin.h): the pair (s, r) is eligible when
// s[s] op r[r] holds as a term of the condition step does, op one of LT, LE, GT, GE.
struct AsofTerm { const void *s, *r; const uint32_t *sValid, *rValid; uint32_t width, type, op; };
// Pairs (mapS[k] - sRowBase, mapR[k]) -> per S row the eligible pair with the largest asof_key of its R element, ties to
// the lowest R row, to `out` as launch_pairs_where writes its kept pairs (out.cursor: two 64-bit words, zeroed before the
// launch: kept pairs, pairs dropped); the marks as there, set by the kept pairs alone. bestVal (sRows 64-bit words) and
// bestRow (sRows words) are initialised here, on s: after the call bestRow[i] is the R row kept for S row i or kNoRow,
// bestVal[i] its key (0 without one). The caller has checked the term and nPairs, sRows, rRows <= 2^32 - 1.
hipError_t launch_pairs_asof(const uint32_t* mapS, const uint32_t* mapR, uint64_t nPairs, uint32_t sRowBase, uint32_t sRows,
                             uint32_t rRows, const AsofTerm& term, unsigned long long* bestVal, uint32_t* bestRow, PairsOut out,
                             uint32_t* sMarks, uint32_t* rMarks, hipStream_t s);
// the same in host loops over host pointers (asof_key and where_holds are the kernels' own), the kept pairs in input
// order; info: kept, written, 0, dropped (may be null)
void pairs_asof_host(const uint32_t* mapS, const uint32_t* mapR, uint64_t nPairs, uint32_t sRowBase, uint32_t sRows, uint32_t rRows,
                     const AsofTerm& term, uint64_t* bestVal, uint32_t* bestRow, uint32_t* outS, uint32_t* outR, uint64_t capacity,
                     uint32_t* sMarks, uint32_t* rMarks, uint64_t* info);

// ---- rows in the order of their columns (defined in hj_sort.hip) --------------
// The order key of the sort: the zero-extended raw word of a valid element of `width` bytes read as `type` -> an unsigned
// word of 8 * width bits that orders as the header states it, equal exactly where two elements tie. UINT: the word. INT:
// the sign bit flipped within the width. FLOAT: folded as asof_key folds, in the element's own width -- a negative's bits all
// complemented, a positive's sign bit set, -0.0 taken for +0.0 -- and every NaN, whatever its sign or payload, all ones:
// above +inf. HJ_SORT_DESC complements the word within the width, NaN included. A NULL's key is 0: the caller's business.
constexpr uint32_t kSortMaxCols = 4;          // HJ_SORT_MAX_COLS
constexpr uint32_t kSortDesc = 1u, kSortNullsFirst = 2u;      // HJ_SORT_DESC, HJ_SORT_NULLS_FIRST
__host__ __device__ __forceinline__ uint64_t sort_key(uint32_t type, uint32_t width, uint32_t flags, uint64_t raw)
{
    const uint32_t bits = 8u * width;
    const uint64_t top = 1ull << (bits - 1u), mask = top | (top - 1ull);
    uint64_t key = raw & mask;
    if (type == kValInt) key ^= top;
    else if (type == kValFloat) {
        const uint64_t mag = key & (top - 1ull), inf = width == 4u ? 0x7F800000ull : 0x7FF0000000000000ull;
        if (mag > inf) key = mask;                                    // a NaN
        else if (mag == 0ull) key = top;                              // -0.0 == 0.0: one key for both
        else key = (key & top) ? ~key & mask : key | top;
    }
    return (flags & kSortDesc) ? ~key & mask : key;
}
// The columns of a call as the kernels take them (hj_sort_col, include/htm_hashjoin.h); cols[0] is the most significant.
struct SortCols { const void* p[kSortMaxCols]; const uint32_t* valid[kSortMaxCols]; uint32_t width[kSortMaxCols], type[kSortMaxCols], flags[kSortMaxCols]; };
// How a pass cuts nRows records of keyBytes-byte keys: a workgroup ranks tileRows records at a time and owns chunkRows (a
// multiple of it) in a pass; the workspace is two key planes and two row planes of nRows, a histogram of 256 words per
// chunk -- at most 4096 chunks at any nRows: 4 MiB -- and its scan sums. bytes is monotone in nRows.
struct SortLayout { uint32_t tileRows, chunkRows, chunks; size_t keyPlane, rowPlane, histBytes, bytes; };
SortLayout sort_layout(uint64_t nRows, uint32_t keyBytes);
uint32_t sort_key_bytes(const SortCols& cols, uint32_t nCols);       // 8 with an 8-byte column, else 4
uint32_t sort_passes(const SortCols& cols, uint32_t nCols);          // one per element byte, one more per validity plane
// perm[0 .. nRows) = the rows in the order of the columns, stable. work: sort_layout(nRows, sort_key_bytes(..)).bytes. The
// caller has checked what the header says the entry point refuses. nRows 0 enqueues nothing.
hipError_t launch_sort_rows(const SortCols& cols, uint32_t nCols, uint64_t nRows, uint32_t* perm, void* work, hipStream_t s);
void sort_rows_host(const SortCols& cols, uint32_t nCols, uint64_t nRows, uint32_t* perm);     // sort_key around std::stable_sort

// ---- PRJ (defined in hj_prj.hip) -------------------------------------------
// Fragment geometry of the histogram-free partitioning of ONE relation (hj_prj.hip, "histogram-free partitioning"):
// pass 1 cuts the relation into C1 chunks and writes bin b of chunk c to the fragment (b * C1 + c) of cap1 key slots;
// pass 2 cuts every pass-1 partition (C1 fragments) into C2 chunks and writes to fragments of cap2 slots; a final
// partition is C2 fragments. C = 0: the relation takes the exact path only.
struct PrjFrag {
    uint32_t C1, cap1, chunkLen1;
    uint32_t C2, cap2, log2C2;
};
struct PrjPlan {
    uint32_t radixBits;   // total
    uint32_t bits1, bits2;
    bool     optimistic;               // try the histogram-free path first (both relations qualify)
    PrjFrag  fragR, fragS;
    uint64_t cnt1Entries, cnt2EntriesR, cnt2EntriesS;   // fragment counters in the workspace
    uint64_t maxChunks1, maxChunks2;   // chunk descriptors per pass (upper bounds over both relations)
    uint64_t histEntries, scanBlocks;  // histogram / block-sum entries: the larger need of R's and S's layouts in
                                       // either pass (the chunk length, hence the chunk count, is NOT monotone in
                                       // the relation size: the smaller relation can need the larger histogram)
    size_t   workspaceBytes;           // everything below, excluding tuple buffers
};
// Sizes the workspace for (nR, nS): each relation is laid out with its own chunk length (run_pass), so every
// region is the maximum over the two relations' layouts.
// mode (hj_params.prjMode): 0 = histogram-free path for large relations, 1 = exact path only, 2 = histogram-free path
// at any size it can be laid out for (tests)
PrjPlan prj_plan(uint64_t nR, uint64_t nS, uint32_t radixBits, uint32_t mode = 0);
// histogram entries the passes over ONE relation of n tuples write (what run_pass memsets and scans)
uint64_t prj_hist_entries_needed(uint64_t n, uint32_t radixBits);
struct PrjBuffers {
    uint64_t* tmpA;      // max(nR,nS) tuples
    uint64_t* partR;     // nR tuples (final partitioned R)
    uint64_t* partS;     // nS tuples
    void*     work;      // plan.workspaceBytes
};
// Enqueues partition(R), partition(S) and the per-partition LDS join.
// evPartDone (may be null) is recorded between partitioning and join.
hipError_t launch_prj(const PrjPlan& plan, const PrjBuffers& buf,
                      const uint64_t* R, uint64_t nR, const uint64_t* S, uint64_t nS, int nCU,
                      Counters* ctr, hipEvent_t evPartDone, hipEvent_t evScatter0, hipEvent_t evScatter1, hipStream_t s);
// evScatter0/1 (may be null): recorded around the pass-1 scatter of R, PRJ's dominant kernel
hipError_t prj_set_attributes();          // per device, at hj_create

// ---- PRJ with a resident R (hj_prj_build_dev / hj_prj_probe_dev, defined in hj_prj.hip) ----
// Everything of R's partitioning that must outlive the scratch workspace (whose layout every slice plan re-carves) and
// the per-probe work-item list, in one buffer of prj_resident_bytes(radixBits, maxSlice) sized at hj_reserve.
struct PrjResident {
    uint32_t* offR;                 // [P + 1] R's partition offsets (exact passes)
    uint32_t* cnt2R;                // [P * 16] R's pass-2 fragment counts (histogram-free passes)
    uint32_t* itemCnt;              // [2P + 1] items per partition: split partitions first, then the rest; scanned in place
    uint32_t* scanSums;             // scan workspace of itemCnt
    uint2* items;                   // [P + maxSlice / kPrjItemS + 1] (partition, S chunk)
    unsigned long long* stats;      // [4] next item ticket, items, split partitions, largest S partition;
                                    // [4]: the pair count of a counting probe against a {key, row} R (hj_prj_probe_dev)
};
constexpr uint32_t kPrjItemS = 1u << 16;  // S tuples per join work item at most (hj_prj.hip, k_prj_probe_items)
size_t prj_resident_bytes(uint32_t radixBits, uint64_t maxSlice);
PrjResident prj_resident_carve(void* base, uint32_t radixBits, uint64_t maxSlice);
// R's passes into buf.partR / res (plan = prj_plan(nR, 0, ...)), then R's checksum (k_prj_join without S);
// Counters::prjFallbackR = R's fallback. evPartDone: between the passes and the checksum.
hipError_t launch_prj_build(const PrjPlan& plan, const PrjBuffers& buf, const PrjResident& res, const uint64_t* R, uint64_t nR,
                            int nCU, Counters* ctr, hipEvent_t evPartDone, hipEvent_t evScatter0, hipEvent_t evScatter1, hipStream_t s);
// S's passes into buf.partS (planS = prj_plan(nS, nS, ...)), the work-item list, the skew-split join against the resident R
// (planR = the build's plan). evPartDone: after S's passes; evJoin0: right before the join kernel.
hipError_t launch_prj_probe(const PrjPlan& planR, uint64_t nR, const PrjPlan& planS, const PrjBuffers& buf, const PrjResident& res,
                            const uint64_t* S, uint64_t nS, int nCU, Counters* ctr, hipEvent_t evPartDone, hipEvent_t evJoin0,
                            hipStream_t s);

// ---- row-id form of the resident radix join (HJ_FLAG_KEEP_ROW_IDS; defined in hj_prj_pairs.hip) ----
// buf.partR / partS / tmpA hold 8-byte {key, row} elements; exact passes only (plan = prj_plan(.., mode 1)).
// R's passes (row = position in R) into buf.partR / res.offR, then R's checksum.
hipError_t launch_prj_build_rows(const PrjPlan& plan, const PrjBuffers& buf, const PrjResident& res, const uint64_t* R, uint64_t nR,
                                 int nCU, Counters* ctr, hipEvent_t evPartDone, hipEvent_t evScatter0, hipEvent_t evScatter1, hipStream_t s);
// S's passes (row = sIdxBase + position in S), the work-item list, the join that emits (S row, R row) pairs to `out`
// (out.cursor is zeroed on the stream first; out.capacity 0: the pairs are counted only). Adds to Counters::prjMatches.
// kind: hj_join_kind. HJ_JOIN_LEFT and HJ_JOIN_ANTI give partitions with S tuples and no R tuple a work item of their own.
// marks != nullptr (kinds INNER and LEFT only): the join's MARK instantiation (RMarks above; base 0, the row is the position in R)
hipError_t launch_prj_probe_rows(uint32_t kind, const PrjPlan& planR, const PrjPlan& planS, const PrjBuffers& buf, const PrjResident& res,
                                 const uint64_t* S, uint64_t nS, uint64_t sIdxBase, PairsOut out, int nCU, Counters* ctr,
                                 hipEvent_t evPartDone, hipEvent_t evJoin0, hipStream_t s, const RMarks* marks = nullptr);

// ---- aggregating joins: COUNT / SUM / MIN / MAX per group row (hj_prj_agg.hip, hj_agg.hip) ----
// The columns of a call as the kernels take them, by value in the kernel arguments: the ops (hj_agg_spec; sgn: HJ_AGG_SIGNED),
// the sources (hj_agg_src) and the accumulator planes. Every accumulator is 64 bits wide.
constexpr uint32_t kAggMaxCols = 4;           // HJ_AGG_MAX_COLS
constexpr uint32_t kAggCount = 0, kAggSum = 1, kAggMin = 2, kAggMax = 3;      // hj_agg_op
struct AggOps { uint32_t op[kAggMaxCols], width[kAggMaxCols], sgn[kAggMaxCols]; };
struct AggSrc { const void* p[kAggMaxCols]; const uint32_t* valid[kAggMaxCols]; };
struct AggPlanes { unsigned long long* count; unsigned long long* acc[kAggMaxCols]; };
struct AggRowsOut { unsigned long long* col[kAggMaxCols]; unsigned long long* count; };
// the identity of a column's op: what an accumulator holds before its first value
__device__ __forceinline__ unsigned long long agg_identity(uint32_t op, uint32_t sgn)
{
    if (op == kAggMin) return sgn ? 0x7FFFFFFFFFFFFFFFull : 0xFFFFFFFFFFFFFFFFull;
    if (op == kAggMax) return sgn ? 0x8000000000000000ull : 0ull;
    return 0ull;
}
// acc op= v, without a returned value; SCOPE: the workgroup for an LDS entry, the agent for a global one
template <int SCOPE>
__device__ __forceinline__ void agg_apply(unsigned long long* acc, uint32_t op, uint32_t sgn, unsigned long long v)
{
    if (op <= kAggSum) __hip_atomic_fetch_add(acc, v, __ATOMIC_RELAXED, SCOPE);
    else if (op == kAggMin) {
        if (sgn) __hip_atomic_fetch_min(reinterpret_cast<long long*>(acc), (long long)v, __ATOMIC_RELAXED, SCOPE);
        else __hip_atomic_fetch_min(acc, v, __ATOMIC_RELAXED, SCOPE);
    } else {
        if (sgn) __hip_atomic_fetch_max(reinterpret_cast<long long*>(acc), (long long)v, __ATOMIC_RELAXED, SCOPE);
        else __hip_atomic_fetch_max(acc, v, __ATOMIC_RELAXED, SCOPE);
    }
}
// a op b, for the reductions in registers that run in front of an atomic
__device__ __forceinline__ unsigned long long agg_combine(uint32_t op, uint32_t sgn, unsigned long long a, unsigned long long b)
{
    if (op <= kAggSum) return a + b;
    if (op == kAggMin) return sgn ? ((long long)a < (long long)b ? a : b) : (a < b ? a : b);
    return sgn ? ((long long)a > (long long)b ? a : b) : (a > b ? a : b);
}
// the 64-bit value of element i of a column: COUNT brings 1, a 4-byte element is sign- or zero-extended
__device__ __forceinline__ unsigned long long agg_value(const void* __restrict__ src, uint32_t op, uint32_t width, uint32_t sgn, uint32_t i)
{
    if (op == kAggCount) return 1ull;
    if (width == 8) return static_cast<const unsigned long long*>(src)[i];
    const uint32_t w = static_cast<const uint32_t*>(src)[i];
    return sgn ? (unsigned long long)(long long)(int32_t)w : (unsigned long long)w;
}

// The resident radix join's planes hold n = rSize entries each, indexed by resident position (the index into partR).
// what: 0 slots, 1 R tuples per LDS build, 2 S elements per round of a workgroup, 3 kPrjItemS (hj_prj_agg_layout_info)
uint32_t agg_layout(uint32_t nCols, uint32_t what);
hipError_t launch_agg_fill(const AggPlanes& pl, const AggOps& ops, uint32_t nCols, uint64_t n, int nCU, hipStream_t s);
// out.col[c][partR[pos].y] = pl.acc[c][pos], out.count likewise (may be null); plain stores, the planes are only read
hipError_t launch_agg_rows(const uint64_t* partR, const AggPlanes& pl, const AggRowsOut& out, uint32_t nCols, uint64_t n, int nCU, hipStream_t s);
// launch_prj_probe_rows with the accumulators in place of the pairs: S's row-id passes (rows from 0: src is indexed by the
// position in S), the work-item list, k_prj_join_agg. Adds to Counters::prjMatches and to *last, which is zeroed here first.
hipError_t launch_prj_probe_agg(const PrjPlan& planR, const PrjPlan& planS, const PrjBuffers& buf, const PrjResident& res,
                                const uint64_t* S, uint64_t nS, const AggSrc& src, const AggOps& ops, uint32_t nCols, const AggPlanes& pl,
                                unsigned long long* last, int nCU, Counters* ctr, hipEvent_t evPartDone, hipEvent_t evJoin0, hipStream_t s);
// The reduction over a pair list (hj_agg.hip): for pair k with g = mapG[k] - gBase, v = mapV[k] - vBase: acc[c][g] op= src[c][v],
// count[g] += 1 (count may be null, and mapV when no column reads a value). An entry that is HJ_NO_ROW or out of range on
// either side is never dereferenced: counts[1] += 1, else counts[0] += 1 (two 64-bit words, zeroed before the launch).
struct PairAggCols { AggSrc src; AggOps ops; unsigned long long* acc[kAggMaxCols]; };
hipError_t launch_pairs_agg(const uint32_t* mapG, const uint32_t* mapV, uint64_t nPairs, uint32_t gBase, uint32_t gRows, uint32_t vBase,
                            uint32_t vRows, const PairAggCols& cols, uint32_t nCols, unsigned long long* count, unsigned long long* counts,
                            hipStream_t s);

}  // namespace hj
