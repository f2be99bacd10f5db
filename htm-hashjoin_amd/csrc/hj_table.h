// hj_table.h -- the hash tables and their builds: the table formats (SlotCode, RingWord, the planar index plane), one
// build as its launchers see it (BuildJob), the locality sampler, the window / ring / bucketised builds and their
// layouts, and the counting probes. What reads or writes a table without producing pairs belongs here.
#pragma once

#include "hj_common.h"

namespace hj {

// ---- table formats: what the table buffer holds after a build (Counters::tableFormat) ----
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

}  // namespace hj
