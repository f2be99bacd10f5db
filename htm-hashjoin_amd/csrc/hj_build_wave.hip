// hj_build_wave.hip -- build variant 3: wavefront-private LDS windows over statically owned slot ranges.
//
// What it replaces: HOT LOOP 1 of the reference (NoCCHashBuild.hpp:37-62 / AtomicHashBuild.hpp:37-67, and the
// TSX group insert of HTMHashBuild.hpp:157-238) for inputs whose locality is TIGHT -- the reference's own
// default, `--shuffleRange 16`, and anything up to a few hundred positions of disorder. Variant 2
// (hj_build_own.hip) keeps a 64 KiB window per 512-thread workgroup, claims table blocks with global atomics and
// synchronises its eight wavefronts five times per tile; rocprof showed it neither HBM nor issue bound but
// waiting (51 % of the wave-cycles parked at barriers and on dependent LDS round trips, profiles/r01_*). Here
// nothing is shared between wavefronts, so nothing has to be waited for:
//
//   * R is cut into contiguous chunks, one per wavefront: as many as there are resident wavefronts (16 per CU), and
//     for large relations up to eight times as many (wave_chunk_len: later workgroups take over from the ones that
//     finish, which balances the wavefronts' uneven progress). The chunk's slot range
//     [bounds[c], bounds[c+1]) is fixed BEFORE the build by a pre-pass that looks at the first 64 tuples of
//     every chunk (k_wave_bounds): start = lowest home slot among them, made monotone by a prefix maximum.
//     A wavefront owns its range outright -- no claims, no owner table, no atomics on HBM.
//   * The wavefront walks its chunk in tiles of 64 x PER tuples with a ring of 2^WINLOG slots (8 KiB) of ITS
//     range in LDS. Inserts run the index-priority protocol of hj_kernels.hip with LDS atomics: the PER
//     home-slot attempts of a tile are issued back to back (independent round trips), whatever fails goes
//     through a compacted per-wavefront retry queue in dense rounds (as in variant 2).
//   * When the tile's lowest home slot moves on, the ring's tail leaves for HBM in 1 KiB granules (one
//     16-byte store per lane), empties included: every slot of the range is written exactly once, in order,
//     by its owner. At the end of the chunk the rest of the range is written the same way.
//   * A tuple that cannot be handled inside the range and the ring -- a straggler across a chunk seam, a key
//     far from its neighbours, a probe walk that leaves the range -- is "aborted" into the global deferred
//     queue with the slot it reached, and k_build_deferred (hj_build_own.hip) finishes it with global atomics
//     after this kernel: the protocol is confluent, so WHICH tuples take that road never changes the table.
//     On inputs without locality nearly every tuple takes it (correct, slow); hj_api.hip only picks this
//     variant when a sample of R says the ring will do.
//
// All integer work on 8-byte tuples (or bare 32-bit keys); HBM traffic = R read once + every reachable slot
// written once = the algorithmic 16 bytes per tuple of SURVEY.md 8d. No MFMA.

#include "hj_table.h"

#include <type_traits>

namespace hj {

constexpr int kWvThreads = 256;                     // 4 wavefronts per workgroup; they never synchronise
constexpr int kWvWaves = kWvThreads / 64;
constexpr uint32_t kGranShift = kWvGranShift;       // retire granule: 128 slots = 1 KiB = 64 lanes x 16 bytes
constexpr uint32_t kGranSlots = 1u << kGranShift;
constexpr uint32_t kNone = 0xFFFFFFFFu;

// ring and tile geometry come from hj_table.h, which describes them to the locality sampler
constexpr int kWvTile = (int)kWvTileTuples;
constexpr int kWvPer = kWvTile / 64;                // tuples per lane per tile
constexpr int kWvPf = 1;                            // tiles of R in flight per wavefront (register prefetch depth)
constexpr uint32_t kWvGran = kWvRingGran;           // ring granules
constexpr uint32_t kWvWin = kWvGran << kGranShift;  // ring slots per wavefront
constexpr uint32_t kWvQCap = 128;                   // retry queue entries per wavefront
constexpr uint32_t kWvRoundAt = 64;                 // a retry round runs once this many entries wait (<= 64)
// wavefronts per SIMD the registers must allow (16 per CU: what the rings' LDS allows; the compact build fits in 115
// VGPRs once the chunk state is scalar)
constexpr int kWvWpe = 4;
// ... and on the slot-code road, whose ring of words leaves LDS for up to eight workgroups per CU (kWvWordLdsBytes below): 7, i.e.
// at most 72 VGPRs. The kernel is a chain of dependent LDS round trips per wavefront and every further resident wavefront hides
// some of the waiting (profiles/ring_words.md section 4, profiles/ring_occupancy.md), so the occupancy is asked for here and not
// left to what the register allocator happens to need; the kernel fits without scratch because its attempts and push rows go in
// batches of kWvWordRows rows and the next tile's loads are issued behind classify() (k_build_wave). Eight (64 VGPRs) needs
// scratch. Chunk geometry and priority rotation still count kWvWavesPerCu wavefronts per CU: the dispatcher simply keeps the
// further workgroups resident.
constexpr int kWvWordWpe = 7;
constexpr int kWvWordRows = 4;                      // rows of a tile per batch of attempts + push rows on that road
// kWvWavesPerCu resident wavefronts per CU, chunks = resident wavefronts x up to kWvMaxRounds rounds (hj_table.h; wave_layout below)
constexpr uint32_t kWvMinChunk = 32768;             // tuples: a second round of workgroups only while chunks stay this long
constexpr uint32_t kWvShortestChunk = 4 * kWvTileTuples;   // tuples: no chunk is cut shorter
// issue priorities rotate in time among a CU's workgroup slots; period = 2^shift ticks of the 100 MHz clock (10.24 us)
constexpr uint32_t kWvPrioShift = 10;
static_assert(kWvQCap >= 128 && (kWvQCap & (kWvQCap - 1)) == 0, "FIFO ring: a power of two that takes one full step on top of < 64 waiting entries");
constexpr size_t kWvLdsBytes = (size_t)kWvWaves * (kWvWin * sizeof(uint64_t) + 3 * kWvQCap * sizeof(uint32_t));
// slot-code road: the ring holds 4-byte ring words (RingWord, hj_table.h) and a queue entry is (pos, word)
// ring granules on that road: 1024 slots in 4 KiB. 16 granules were measured against 8 at 2^30 `uniform` (profiles/ring_words.md
// section 2): the deferred tail shrinks from 203 to 41 us, the build kernel grows by 320, the step is slower
constexpr uint32_t kWvWordGran = 8;
constexpr size_t kWvWordLdsBytes = (size_t)kWvWaves * ((kWvWordGran << kGranShift) * sizeof(uint32_t) + 2 * kWvQCap * sizeof(uint32_t));
static_assert((kWvWordGran & (kWvWordGran - 1)) == 0 && kWvWordLdsBytes <= kWvLdsBytes, "a ring of words costs no more LDS than the 8-byte ring");
static_assert((size_t)kWvWordWpe * kWvWordLdsBytes <= 160u * 1024u, "the workgroups the registers allow fit a CU's 160 KiB of LDS");

// The lane mask of a condition. HIP's __ballot(int) compares an INTEGER with zero: a condition that already is a lane mask
// (every compare produces one) is first turned into 0 / 1 per lane and compared again -- two vector instructions per
// ballot, ~50 per tile in a kernel whose retry rounds are bound by vector issue. This form takes the mask as it is.
__device__ __forceinline__ unsigned long long wv_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }


// ---- pre-pass: where every chunk starts and which slot range it owns -----------------------------------------------
// Chunk c nominally starts at position p = c * chunkLen. The seam is moved to where the data crosses a granule
// boundary: with m = the lowest home slot among the 64 tuples from p, the chunk starts at the first position q in
// [p, p + kWvLook) whose home slot lies in a later granule than m's, and its slot range starts at that granule --
// so (on near-sorted input) no tuple before q belongs above the boundary, and the few tuples after q that still
// belong below it are taken by the previous wavefront, which reads kWvOverlap positions past its own end. Without
// this every seam cost ~70 deferred tuples on `uniform` (half a granule's worth), each a cascade of global atomics.
// starts[c] = q (or p if no crossing shows up: many tuples per granule), raw[c] = the granule (kNone: no valid tuple).
constexpr uint32_t kWvLook = 256;
constexpr uint32_t kWvOverlap = 64;
// COMPACT build: positions before its seam a wavefront also reads (shadow zone), so that shadow zone + head zone are
// exactly its first tile; and the crossers one seam may let in before the build gives up on the compact table
constexpr uint32_t kWvShadow = kWvTile - kWvOverlap;
constexpr uint32_t kWvTail = kWvOverlap;         // the last positions of a chunk whose next-range tuples the NEXT wavefront inserts
constexpr uint32_t kWvPredCap = 64;

// ---- queue slice: chunk c's sliceLen entries of the deferred queue and their three tenants -----------------------------
// E = DeferredEntry for the kernels that write, const DeferredEntry for the ones that only read.
//   * deferred entries, from the front: dcounts[c] of them (a tuple leaves at most once: <= clen + kWvOverlap <= sliceLen);
//     the compact build lists there, `packed` only, the crossers that leave its range at the upper seam
template <class E>
__host__ __device__ inline E* slice_deferred(E* queue, uint32_t c, uint32_t sliceLen) { return queue + (uint64_t)c * sliceLen; }
//   * compact build: the crossers the chunk let in at its lower seam, pcounts[c] of at most kWvPredCap 8-byte words
//     (index << 32 | key) at the slice's very end
template <class E>
__host__ __device__ inline auto slice_crossers(E* queue, uint32_t c, uint32_t sliceLen)
{
    using Word = std::conditional_t<std::is_const_v<E>, const uint64_t, uint64_t>;
    return reinterpret_cast<Word*>(slice_deferred(queue, c + 1, sliceLen)) - kWvPredCap;
}
// k_wave_validate accepts a seam with at most kWvPredCap crossers on either side: even in the shortest slice the ones
// going out (16-byte entries from the front) and the ones let in (8-byte words at the end) never meet
static_assert(kWvPredCap * (sizeof(DeferredEntry) + sizeof(uint64_t)) <= (kWvShortestChunk + kWvLook + kWvOverlap) * sizeof(DeferredEntry),
              "the crosser list fits behind the most crossers a compact slice can hold");
//   * planar retire: the dirty log of the slice's deferred walks, lcounts[c] slot numbers behind the dcount deferred
//     entries -- 4 per entry the chunk did not defer
template <class W> struct DirtyLog { W* slot; uint32_t cap; };
template <class E>
__host__ __device__ inline auto slice_dirty_log(E* queue, uint32_t c, uint32_t sliceLen, uint32_t dcount)
{
    using Word = std::conditional_t<std::is_const_v<E>, const uint32_t, uint32_t>;
    return DirtyLog<Word>{reinterpret_cast<Word*>(slice_deferred(queue, c, sliceLen) + dcount),
                          dcount < sliceLen ? (sliceLen - dcount) * (uint32_t)(sizeof(DeferredEntry) / sizeof(uint32_t)) : 0u};
}
template <bool KEY32, bool HTM>
__global__ void __launch_bounds__(kBlock)
k_wave_seams(const void* __restrict__ Rv, uint64_t n, uint32_t chunkLen, uint32_t nChunks, uint64_t mask,
             uint32_t hshift, uint32_t* __restrict__ starts, uint32_t* __restrict__ raw, Gate gate)
{
    if (gate_closed(gate)) return;
    using Elem = typename std::conditional<KEY32, uint32_t, uint64_t>::type;
    const Elem* __restrict__ R = static_cast<const Elem*>(Rv);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (c > nChunks) return;
    if (c == nChunks) { if (lane == 0) starts[c] = (uint32_t)n; return; }
    const uint64_t p = (uint64_t)c * chunkLen;
    // The look proceeds in steps of 128 tuples (two loads per lane) and stops at the first crossing: on the reference's
    // inputs one or two steps do (a granule is 128 slots), and the pre-pass reads 1-2 KiB per seam instead of 4 KiB
    // (32768 seams at 2^30: the full look was 134 MB of reads, 35 us).
    auto load_home = [&](uint64_t i) -> uint32_t {
        if (i >= n) return kNone;
        const uint64_t t = R[i];
        return ((t >> 32) == 0 && t != 0) ? home32<HTM>((uint32_t)t, hshift, (uint32_t)mask) : kNone;
    };
    uint32_t h0 = load_home(p + lane), h1 = load_home(p + 64 + lane);
    const uint32_t m = wave_umin(h0);
    uint32_t start = (uint32_t)p, g = m == kNone ? kNone : m >> kGranShift;
    if (c > 0 && p + kWvLook > n) {
        // A last chunk shorter than the look (a radix shard's key count is no multiple of the chunk length): too few tuples
        // to place a seam among -- without a crossing the seam would sit at p, in the middle of a granule's worth of tuples
        // that then belong to the other side in bulk. The previous chunk takes these tuples too (its slice has room for
        // kWvLook more), and this chunk starts at the relation's end, owning the table from the granule after the highest
        // home slot among them: no tuples, only its part of the table (and, in the compact build, its shadow granule).
        uint32_t mx = 0;                                              // highest home slot among this lane's valid tuples
        if (h0 != kNone) mx = h0;
        if (h1 != kNone && h1 > mx) mx = h1;
        for (uint32_t k = 2; k < kWvLook / 64; ++k) { const uint32_t h = load_home(p + 64 * k + lane); if (h != kNone && h > mx) mx = h; }
        const uint32_t hi = ~wave_umin(~mx);
        start = (uint32_t)n;
        g = m == kNone ? kNone : (hi >> kGranShift) + 1u;
    } else if (c > 0 && m != kNone) {
        const uint32_t edge = ((m >> kGranShift) + 1) << kGranShift;          // first slot of the next granule (0 on wrap: no crossing)
        for (uint32_t k = 0; k < kWvLook / 64 && edge != 0; k += 2) {
            if (k) { h0 = load_home(p + 64 * k + lane); h1 = load_home(p + 64 * (k + 1) + lane); }
            const unsigned long long hit0 = wv_ballot(h0 != kNone && h0 >= edge), hit1 = wv_ballot(h1 != kNone && h1 >= edge);
            if (hit0 | hit1) {
                start = hit0 ? (uint32_t)(p + 64 * k + (uint32_t)__ffsll((long long)hit0) - 1)
                             : (uint32_t)(p + 64 * (k + 1) + (uint32_t)__ffsll((long long)hit1) - 1);
                g = edge >> kGranShift;
                break;
            }
        }
    }
    if (lane == 0) { starts[c] = start; raw[c] = g; }
}

// bounds[c] = max over chunks <= c of raw (chunks without a valid sample inherit; chunks before the first valid sample
// take the first one's: nothing below it is owned), bounds[nChunks] = the table's end. Every workgroup takes kBlock
// consecutive chunks and finds the maximum over all chunks before its own by itself (coalesced reads of an array of at most
// 128 KiB that sits in L2) -- no second kernel, no look-back chain; the single-workgroup version of round 2 took 60 us
// for 32768 chunks.
__global__ void __launch_bounds__(kBlock)
k_wave_bounds_scan(const uint32_t* __restrict__ raw, uint32_t nChunks, uint32_t numGran, uint32_t* __restrict__ bounds, Gate gate)
{
    if (gate_closed(gate)) return;
    __shared__ uint32_t wmax[kBlock / 64], wscan[kBlock / 64];
    const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
    const uint32_t base = blockIdx.x * kBlock, c = base + t;
    // maximum over the valid samples of every chunk before this workgroup's (kNone = no sample = contributes nothing)
    uint32_t before = 0;
    bool any = false;
    {   // 16-byte loads, four in flight per thread: the loop is a chain of L2 round trips otherwise (34 us for 32768 chunks)
        const uint4* raw4 = reinterpret_cast<const uint4*>(raw);          // raw is the start of a hipMalloc'ed buffer; base % 256 == 0
        const uint32_t nv = base >> 2;
        auto take = [&](uint32_t v) { before = (v != kNone && v > before) ? v : before; any |= v != kNone; };
        uint32_t k = t;
        for (; k + 3 * kBlock < nv; k += 4 * kBlock) {
            const uint4 a = raw4[k], b = raw4[k + kBlock], c4 = raw4[k + 2 * kBlock], d = raw4[k + 3 * kBlock];
            take(a.x); take(a.y); take(a.z); take(a.w); take(b.x); take(b.y); take(b.z); take(b.w);
            take(c4.x); take(c4.y); take(c4.z); take(c4.w); take(d.x); take(d.y); take(d.z); take(d.w);
        }
        for (; k < nv; k += kBlock) { const uint4 a = raw4[k]; take(a.x); take(a.y); take(a.z); take(a.w); }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const uint32_t o = __shfl_xor(before, off, 64); before = o > before ? o : before; }
    const unsigned long long anyW = wv_ballot(any);
    if (lane == 0) { wmax[w] = before; wscan[w] = anyW ? 1u : 0u; }
    __syncthreads();
    uint32_t run = 0; bool have = false;
    for (int k = 0; k < kBlock / 64; ++k) { run = wmax[k] > run ? wmax[k] : run; have |= wscan[k] != 0; }
    __syncthreads();
    // inclusive prefix maximum inside the workgroup
    const uint32_t v = c < nChunks ? raw[c] : kNone;
    uint32_t inc = v == kNone ? 0u : v;
    const unsigned long long validMask = wv_ballot(v != kNone);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t o = __shfl_up(inc, off, 64); if ((int)lane >= off) inc = o > inc ? o : inc; }
    if (lane == 63) wmax[w] = inc;
    if (lane == 0) wscan[w] = validMask ? 1u : 0u;
    __syncthreads();
    bool haveHere = have || (validMask & ((2ull << lane) - 1ull)) != 0;
    for (uint32_t k = 0; k < w; ++k) { run = wmax[k] > run ? wmax[k] : run; haveHere |= wscan[k] != 0; }
    run = inc > run ? inc : run;
    if (c < nChunks) {
        if (!haveHere) {
            // no valid sample up to this chunk: the first valid one after it opens the first range (a relation that
            // starts with invalid tuples: rare, and the walk is short)
            run = 0;
            for (uint32_t k = c + 1; k < nChunks; ++k) { const uint32_t x = raw[k]; if (x != kNone) { run = x; break; } }
        }
        bounds[c] = run < numGran ? run : numGran;
    }
    if (blockIdx.x == 0 && t == 0) bounds[nChunks] = numGran;
}

// ---- the build ------------------------------------------------------------------------------------------------
// COMPACT (the fast path of the open-addressing table, hj_table.h "table formats"): the ring still holds (index << 32 | key),
// but what leaves for HBM is the KEY WORD alone -- 4 bytes per slot instead of 8, and the probe reads 4 bytes per slot too.
// The index words exist only to order the inserts, and inside a wavefront's ring they have done that by the time a granule
// retires; nothing after this kernel may therefore need them: there is no deferred phase. Every way a tuple used to get
// deferred is either handled here or raises Counters::compactFail, after which the classic 8-byte build (gated on the word
// k_wave_decide rewrites) redoes the whole table:
//   * walks that cross the seam into the next wavefront's range ("crossers", ~1.6 per seam on `uniform`): wavefront c
//     ALSO inserts, into a shadow granule below its range that it never writes out, the tuples whose home slot lies in
//     the last 128 slots of wavefront c-1's range (it reads kWvShadow positions before its seam for them), and so sees
//     for itself which of them walk across. Influence only flows towards higher slots, so c-1's own range never depends
//     on c's. Whether the shadow saw the truth is CHECKED, not assumed: c-1 lists the tuples that really left its range
//     at the seam, c lists the ones it let in, k_wave_validate compares the two lists seam by seam (equal lists = one
//     consistent run of the protocol over both ranges = the unique fixed point).
//   * retry entries the ring is about to leave behind get their rounds before it moves (forced rounds);
//   * anything else (a key far from its neighbours, a walk that wraps around the table end, key 0xFFFFFFFF = the compact
//     empty pattern) raises the flag.
// PLANAR (the classic build of a context that keeps no row ids): everything above stays what it is -- ring, inserts, retry
// queue, seams, deferral --, only the retire differs: a granule leaves as two 512-byte runs, key words to the key plane (the
// start of the table buffer: exactly the compact format) and index words to the index plane behind it
// (planar_index_plane), so that the probe reads 4 bytes per slot. The deferred phase then walks on the index plane alone
// (k_wave_deferred<PLANAR>, k_wave_fixup). Key 0xFFFFFFFF cannot live in a 4-byte table: Counters::planarFail, and the
// packed build redoes it.
// CODES (PLANAR on 8-byte tuples only, mode kWaveCodes): the key run of a retiring granule is 128 code bytes instead of 512
// bytes of keys (SlotCode, hj_table.h) -- one 2-byte store per lane, one 128-byte line per instruction; the index run, the
// deferred walks and the log stay what they are. Any key has a code when the table is large enough (the host's rule);
// otherwise (forced road) a tile holding a key at or above keyLimit raises Counters::planarFail bit 2. Key 0xFFFFFFFF is a
// key like any other here: the empty pattern is a code no key produces.
// On this road the RING holds 4-byte ring words, (offset in the chunk << 7 | code), not (index << 32 | key): the code is made
// once, at insertion, a step to the next slot is word + 1, every atomic, look, compare and select is a 32-bit one, a queue
// entry is (pos, word), and a ring of kWvWordGran granules costs half the LDS of as many 8-byte ones. Whether a tuple's budget
// is spent is decided when its try FAILS, from the word before the step (RingWord::tries_left), so every word in the ring
// or the queue has a try left. The key comes back out of (pos, word) where it is needed: the sum of the dropped keys
// and a deferred entry, which is today's (pos, index << 32 | key). Everything around the ring is the one copy below.
struct WordRing { RingWord rw; uint32_t keyLimit; };
inline WordRing word_ring(const SlotCode& sc) { return WordRing{ring_word(sc), sc.key_limit()}; }
template <bool KEY32, bool CHECK, bool HTM, bool COMPACT, bool PLANAR, bool CODES = false>
__global__ void __launch_bounds__(kWvThreads, CODES ? kWvWordWpe : kWvWpe)
k_build_wave(const void* __restrict__ Rv, uint64_t n, uint32_t sliceLen, uint32_t nChunks, const uint32_t* __restrict__ starts,
             const uint32_t* __restrict__ bounds, uint64_t* __restrict__ table, uint64_t mask, uint32_t hshift,
             uint32_t probeLen, uint64_t idxBase, ShardCheck sc, DeferredEntry* __restrict__ queue,
             uint32_t* __restrict__ dcounts, Counters* __restrict__ ctr, Gate gate, uint64_t* __restrict__ htmConflicts,
             uint32_t* __restrict__ ccounts, uint32_t residentWG, uint32_t* __restrict__ pcounts, WordRing cr)
{
    static_assert(!(COMPACT && HTM), "the bucketised table keeps its own layout");
    static_assert(!(PLANAR && (COMPACT || HTM)), "the planar retire belongs to the classic open-addressing build");
    static_assert(!CODES || (PLANAR && !KEY32), "slot codes: the planar retire of a tuple build (identity hash)");
    if (gate_closed(gate)) return;
    extern __shared__ __align__(16) uint64_t lds[];
    // the wavefront's number inside the workgroup is the same in all its lanes, but the compiler only knows that when told:
    // everything derived from the chunk number (its seams, its slot range, the ring's position, every test against them) then
    // lives in scalar registers and is computed by the scalar unit -- the vector unit is what this kernel runs out of
    const uint32_t lane = threadIdx.x & 63, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t c = blockIdx.x * kWvWaves + wave;
    if (c >= nChunks) return;                                            // whole wavefronts leave; nobody waits for them
    if constexpr (COMPACT) {
        // some wavefront has met an input the compact table cannot take: the classic build will redo everything,
        // whatever is written from here on is never looked at (k_wave_decide reads the flag before anything else)
        if (*reinterpret_cast<volatile unsigned long long*>(&ctr->compactFail)) return;
    }
    // ring geometry of this instantiation: RGRAN granules of RWIN slots, 8-byte slots or (CODES) 4-byte ring words
    constexpr uint32_t RGRAN = CODES ? kWvWordGran : kWvGran, RWIN = RGRAN << kGranShift;
    constexpr uint32_t QWORDS = CODES ? 2u : 3u;                         // words of a queue entry
    uint64_t* const win = lds + wave * kWvWin;                           // ring: slot s lives at win[s & (kWvWin - 1)]
    uint32_t* const win32 = reinterpret_cast<uint32_t*>(lds) + wave * RWIN;   // CODES: slot s lives at win32[s & (RWIN - 1)]
    uint32_t* const myQPos = (CODES ? reinterpret_cast<uint32_t*>(lds) + kWvWaves * RWIN : reinterpret_cast<uint32_t*>(lds + kWvWaves * kWvWin))
                             + wave * QWORDS * kWvQCap;
    uint32_t* const myQLo = myQPos + kWvQCap;                            // CODES: the ring word
    uint32_t* const myQHi = myQLo + kWvQCap;                             // CODES: no such word
    const RingWord& rw = cr.rw;
    (void)win; (void)win32; (void)myQHi; (void)rw;

    // workgroups per quarter of the first, resident round (residentWG = what this device holds at once, from the launch)
    const uint32_t prioDiv = ((gridDim.x <= residentWG ? gridDim.x : residentWG) + 3u) / 4u;
    const bool lastChunk = c + 1 == nChunks;
    const uint64_t cb0 = starts[c];
    const uint32_t clen = starts[c + 1] - starts[c];                     // the chunk proper: its tuples are counted here
    // COMPACT: the kWvShadow positions before the seam are read too (shadow zone, see above); every offset below is
    // relative to the first position READ, cb = cb0 - S, and the chunk proper is [S, S + clen)
    const uint32_t S = (COMPACT && c) ? (cb0 < kWvShadow ? (uint32_t)cb0 : kWvShadow) : 0u;
    const uint64_t cb = cb0 - S;
    const uint32_t cend = S + clen;
    // COMPACT: tuples of the NEXT range that sit before the seam ("early arrivals": keys a little ahead of their neighbours)
    // are left to the next wavefront, which reads those positions anyway (its shadow zone). Where they can sit is known
    // from the NOMINAL seam alone, which both sides know: the pre-pass moved the real seam forward from it by less than
    // kWvLook positions, to the first position of the next range -- so early arrivals lie before the nominal seam, a shuffle
    // window's length at most; the zone starts kWvTail positions before it. [tailFrom, cend): my tail zone;
    // [claimFrom, S): the previous chunk's tail zone as I see it.
    const uint32_t chunkLenNom = sliceLen - kWvLook - kWvOverlap;
    const uint32_t tailFrom = (COMPACT && !lastChunk) ? (uint32_t)((uint64_t)(c + 1) * chunkLenNom - cb) - kWvTail : 0xFFFFFFFFu;
    const uint32_t claimFrom = (COMPACT && c) ? (uint32_t)((uint64_t)c * chunkLenNom - cb) - kWvTail : 0u;
    static_assert(kWvShadow >= kWvLook + kWvTail, "the shadow zone reaches back past the previous chunk's tail zone");
    (void)tailFrom; (void)claimFrom;
    // ... and kWvOverlap positions of the next chunk are read too: its stragglers below the seam are inserted here
    const uint32_t plen = (uint32_t)((cb + cend + kWvOverlap < n ? cb + cend + kWvOverlap : n) - cb);
    const uint32_t mask32 = (uint32_t)mask;
    const uint32_t numGran = (uint32_t)((mask + 1) >> kGranShift);
    if constexpr (!KEY32) hshift = 0u;            // 8-byte tuples always hash with shift 0 (launch_build_wave checks): one shift less per home slot
    using Elem = typename std::conditional<KEY32, uint32_t, uint64_t>::type;
    const Elem* __restrict__ Rc = static_cast<const Elem*>(Rv) + cb;
    const uint32_t idx0 = (uint32_t)(idxBase + cb);
    // this wavefront's slot range, in granules: [loG, limG). The last chunk's range is open up to the table's end;
    // how far it got is published below (ownHiEx).
    const uint32_t loG = bounds[c];
    const uint32_t limG = lastChunk ? numGran : bounds[c + 1];
    const uint32_t loSlot = c ? loG << kGranShift : 0u;                 // head zone: tuples below it are the previous wavefront's
    const uint32_t limSlot = limG << kGranShift;                        // overlap zone: only tuples below it are mine (0 = 2^32: table end)
    // COMPACT: the shadow granule [shadowLo, loSlot) of the previous wavefront's range is simulated here, never written
    bool shadowOn = COMPACT && S != 0 && loG != 0;  // wave-uniform: the shadow granule is still in the ring (the first tile and its rounds)
    uint32_t pCount = 0;                         // COMPACT: crossers let in at the seam so far (wave-uniform)
    // COMPACT: something only the classic build can handle raises Counters::compactFail at once (a rare path: no register is
    // kept for it); the per-tuple tests of classify() collect in one lane mask that is looked at once per tile
    auto raise = [&](bool cond, unsigned long long why) {
        if (wv_ballot(cond) && lane == 0) atomicOr(&ctr->compactFail, why);
    };
    bool ffSeen = false;                         // a key equal to the compact empty pattern
    (void)pCount; (void)ffSeen;

    if constexpr (CODES) {
        for (uint32_t i = lane; i < RWIN / 4; i += 64)
            reinterpret_cast<uint4*>(win32)[i] = make_uint4(RingWord::kEmpty, RingWord::kEmpty, RingWord::kEmpty, RingWord::kEmpty);
    } else {
        for (uint32_t i = lane; i < kWvWin / 2; i += 64) reinterpret_cast<ulonglong2*>(win)[i] = make_ulonglong2(kEmpty, kEmpty);
    }

    uint32_t winLoG = shadowOn ? loG - 1 : loG;  // ring = granules [winLoG, winLoG + RGRAN), wave-uniform
    uint32_t qCount = 0, qHead = 0;              // retry queue (FIFO ring): entries and position of the oldest, wave-uniform
    uint32_t rounds = 0;                         // retry rounds so far (wave-uniform)
    unsigned long long dropSum = 0, inSum = 0;
    uint32_t drops = 0, bad = 0, foreign = 0;
    // CODES: the three counts are wave-uniform -- the lane count of a ballot, kept by the scalar unit -- and not one vector
    // register each (kWvWordWpe); lane 0 hands them in at the end
    uint32_t dCount = 0;                         // tuples deferred so far (wave-uniform)
    DeferredEntry* const myDeferred = slice_deferred(queue, c, sliceLen);
    uint32_t cCount = 0;                         // HTM: conflicts recorded so far (wave-uniform)
    uint64_t* const myConflicts = HTM ? htmConflicts + (uint64_t)c * sliceLen : nullptr;
    (void)cCount; (void)myConflicts;
    uint32_t usedLo = kNone, usedHi1 = 0;        // 512-slot blocks this lane deferred into (Counters::usedLoInv / usedHi1)

    // this lane's two slots of granule g's place in the ring
    auto ring_granule = [&](uint32_t g) -> ulonglong2* {
        return reinterpret_cast<ulonglong2*>(win + ((g & (kWvGran - 1)) << kGranShift)) + lane;
    };
    // the ring's tail up to granule `target` leaves for HBM (empties included) and its LDS copy is reset
    auto advance = [&](uint32_t target) {
        typedef unsigned int u2 __attribute__((ext_vector_type(2)));
        while (winLoG < target) {
            if constexpr (CODES) {
                // 128 code bytes and the 512-byte index run, out of this lane's two ring words: the code is the word's low
                // bits as they stand, the index is the chunk's first plus the word's rel
                uint2* const src = reinterpret_cast<uint2*>(win32 + ((winLoG & (RGRAN - 1)) << kGranShift)) + lane;
                const uint2 t = *src;
                const bool e0 = t.x == RingWord::kEmpty, e1 = t.y == RingWord::kEmpty;
                const uint32_t c0 = e0 ? kCodeEmpty : RingWord::code(t.x), c1 = e1 ? kCodeEmpty : RingWord::code(t.y);
                u2 ii;
                ii.x = e0 ? kNone : idx0 + RingWord::rel(t.x); ii.y = e1 ? kNone : idx0 + RingWord::rel(t.y);
                // the granule's two runs start at wave-uniform addresses, and the optimiser is held to that: left alone it keeps
                // a 64-bit address per lane and run alive around the tile loop, four registers the road's occupancy has no
                // room for now that the ring moves from two places (kWvWordWpe)
                unsigned short* codes = reinterpret_cast<unsigned short*>(reinterpret_cast<uint8_t*>(table) + ((uint64_t)winLoG << kGranShift));
                u2* idxRun = reinterpret_cast<u2*>(planar_index_plane(table, mask + 1) + ((uint64_t)winLoG << kGranShift));
                uint32_t ln = lane;                                       // ... nor the lane's two offsets
                asm volatile("" : "+s"(codes), "+s"(idxRun), "+v"(ln));
                __builtin_nontemporal_store((unsigned short)(c0 | (c1 << 8)), codes + ln);
                __builtin_nontemporal_store(ii, idxRun + ln);
                *src = make_uint2(RingWord::kEmpty, RingWord::kEmpty);
                ++winLoG;
                continue;
            }
            ulonglong2* src = ring_granule(winLoG);
            const ulonglong2 t = *src;
            if constexpr (COMPACT) {
                // the key words alone leave: 512 bytes per granule (the empty pattern's low word is the compact empty
                // pattern); the shadow granule belongs to the previous wavefront and is not written
                if (winLoG >= loG) {
                    u2 vv; vv.x = (uint32_t)t.x; vv.y = (uint32_t)t.y;
                    __builtin_nontemporal_store(vv, reinterpret_cast<u2*>(reinterpret_cast<uint32_t*>(table) + ((uint64_t)winLoG << kGranShift)) + lane);
                }
            } else if constexpr (PLANAR) {
                // two 512-byte runs: the key words, the index words (the empty pattern's two words are the planes' empty patterns)
                u2 kk, ii;
                kk.x = (uint32_t)t.x; kk.y = (uint32_t)t.y; ii.x = (uint32_t)(t.x >> 32); ii.y = (uint32_t)(t.y >> 32);
                uint32_t* const keys = reinterpret_cast<uint32_t*>(table) + ((uint64_t)winLoG << kGranShift);
                __builtin_nontemporal_store(kk, reinterpret_cast<u2*>(keys) + lane);
                __builtin_nontemporal_store(ii, reinterpret_cast<u2*>(keys + (mask + 1 + kPlanarIndexGap)) + lane);
            } else {
                // written once and not read again by this kernel: nontemporal stores (-1.5 % kernel time at 2^30, and
                // the probe that follows runs 1 % faster; nontemporal LOADS of R were slower)
                typedef unsigned long long v2 __attribute__((ext_vector_type(2)));
                v2 vv; vv.x = t.x; vv.y = t.y;
                __builtin_nontemporal_store(vv, reinterpret_cast<v2*>(table + ((uint64_t)winLoG << kGranShift)) + lane);
            }
            *src = make_ulonglong2(kEmpty, kEmpty);
            ++winLoG;
        }
    };
    // may this wavefront touch slot pos right now: inside the ring and inside the owned range
    auto in_ring = [&](uint32_t pos) -> bool {
        const uint32_t g = pos >> kGranShift;
        return (g - winLoG < RGRAN) & (g < limG);
    };
    // a tuple leaves for this wavefront's OWN slice of the deferred queue, [cb, cb + clen): a tuple leaves at most once, so
    // the slice cannot overflow, and no atomic is needed to place it (a returning global atomic per round with a
    // straggler stalled the wavefront for microseconds). dm = the lanes that defer, not empty.
    auto defer = [&](unsigned long long dm, bool toDefer, uint32_t pos, uint64_t packed) {
        if (toDefer) {
            DeferredEntry* q = myDeferred + dCount + lane_rank(dm);
            q->pos = pos; q->packed = packed;
            const uint32_t db = pos >> 9;
            usedLo = db < usedLo ? db : usedLo; usedHi1 = db + 1 > usedHi1 ? db + 1 : usedHi1;
        }
        dCount += (uint32_t)__popcll(dm);
    };
    // CODES: the round on the entry (pos, word) a lane holds; the same terminal events. The entry has a try left at pos.
    auto round_words = [&](uint32_t& pos, uint32_t& word, const bool has) -> bool {
        const bool ownOk = in_ring(pos);
        const bool toDefer = has & !ownOk, work = has & ownOk;
        // look before leaping (below): four consecutive ring words, compared whole -- their order is that of their rel
        const bool inGran = (pos & (kGranSlots - 1)) <= kGranSlots - 4;
        const uint32_t rd = (work & inGran) ? pos : (winLoG << kGranShift);
        const uint32_t* w = win32 + (rd & (RWIN - 1));
        const bool c0 = w[0] < word, c1 = c0 & (w[1] < word), c2 = c1 & (w[2] < word), c3 = c2 & (w[3] < word);
        uint32_t skip = (uint32_t)c0 + (uint32_t)c1 + (uint32_t)c2 + (uint32_t)c3;
        skip = (work & inGran) ? skip : 0u;
        const bool drop1 = work & (skip >= rw.tries_left(word, probeLen));   // every slot it had left holds an earlier tuple
        const uint32_t fwd = drop1 ? 0u : skip;                               // a dropped tuple's (pos, word) stay as they are
        pos = (pos + fwd) & mask32; word = RingWord::step(word, fwd);
        const bool recheck = work & !drop1 & (skip == 4);                     // may have left the granule: next round
        const bool doAtomic = work & !drop1 & !recheck;
        uint32_t old = RingWord::kEmpty;
        if (doAtomic) old = atomicMin(&win32[pos & (RWIN - 1)], word);
        const bool fail = doAtomic & (old != RingWord::kEmpty) & (old != word);
        word = (fail & (old > word)) ? old : word;                            // displaced a later tuple: carry it on
        const bool spent = fail & (rw.tries_left(word, probeLen) <= 1u);      // that was the carried tuple's last slot
        const bool dropped = drop1 | spent;
        if (wv_ballot(dropped)) {
            drops += (uint32_t)__popcll(wv_ballot(dropped)); dropSum += dropped ? (unsigned long long)rw.key(word, pos, mask32) : 0ull;
        }
        const unsigned long long dm = wv_ballot(toDefer);
        if (dm) defer(dm, toDefer, pos, pack64(idx0 + RingWord::rel(word), rw.key(word, pos, mask32)));
        const bool on = fail & !spent;
        pos = on ? ((pos + 1) & mask32) : pos; word = on ? RingWord::step(word) : word;
        return recheck | on;
    };

    // One round on the entry (pos, mlo, mhi) a lane holds (hj_build_own.hip's round, with range + ring standing in
    // for block ownership): terminal events are placed / dropped (budget exhausted, NoCCHashBuild.hpp:57-58) /
    // deferred; returns "not finished" with the entry's next state in place.
    auto round_body = [&](uint32_t& pos, uint32_t& mlo, uint32_t& mhi, const bool has) -> bool {
        if constexpr (CODES) return round_words(pos, mlo, has);
        const uint32_t key = mlo;
        const uint32_t homeOfKey = home32<HTM>(key, hshift, mask32);
        uint32_t budget = probeLen - ((pos - homeOfKey) & mask32);
        if constexpr (COMPACT) {
            // a tuple of the shadow granule arriving at my first slot: a crosser I let in (each passes pos == loSlot
            // exactly once: walks advance slot by slot, and the look never skips across a granule boundary)
            if (shadowOn) {
                const bool cross = has & (pos == loSlot) & (homeOfKey < loSlot) & (budget != 0);
                const unsigned long long xm = wv_ballot(cross);
                if (xm) {
                    const uint32_t at = pCount + lane_rank(xm);
                    uint64_t* const myPred = slice_crossers(queue, c, sliceLen);
                    if (cross & (at < kWvPredCap)) myPred[at] = pack64(mhi, mlo);
                    raise(cross & (at >= kWvPredCap), 2ull);
                    pCount += (uint32_t)__popcll(xm);
                }
            }
        }
        const bool ownOk = in_ring(pos);
        const bool drop0 = has & (budget == 0);
        const bool toDefer = has & !drop0 & !ownOk;
        const bool work = has & !drop0 & ownOk;
        const uint64_t mine = pack64(mhi, mlo);
        // look before leaping: the next 4 slots, when they sit in the same granule (contiguous in the ring and owned
        // together); slot values only decrease, so a slot seen below `mine` stays below it
        const bool inGran = (pos & (kGranSlots - 1)) <= kGranSlots - 4;
        const uint32_t rd = (work & inGran) ? pos : (winLoG << kGranShift);
        // slot values are (index << 32 | key) with one index per tuple, the empty pattern has the highest index word: order
        // and equality of two values are those of their INDEX words. The look reads those alone (half the LDS bytes,
        // two ds_read2_b32) and every compare is a 32-bit one.
        const uint32_t* w = reinterpret_cast<const uint32_t*>(&win[rd & (kWvWin - 1)]) + 1;
        const uint32_t myIdx = mhi;
        const bool c0 = w[0] < myIdx, c1 = c0 & (w[2] < myIdx), c2 = c1 & (w[4] < myIdx), c3 = c2 & (w[6] < myIdx);
        uint32_t skip = (uint32_t)c0 + (uint32_t)c1 + (uint32_t)c2 + (uint32_t)c3;
        skip = (work & inGran) ? (skip < budget ? skip : budget) : 0u;
        pos = (pos + skip) & mask32; budget -= skip;
        const bool drop1 = work & (budget == 0);
        const bool recheck = work & !drop1 & (skip == 4);                  // may have left the granule: next round
        const bool doAtomic = work & !drop1 & !recheck;
        unsigned long long old = kEmpty;
        if (doAtomic)
            old = atomicMin(reinterpret_cast<unsigned long long*>(&win[pos & (kWvWin - 1)]), (unsigned long long)mine);
        const uint32_t oldIdx = (uint32_t)(old >> 32);
        const bool fail = doAtomic & (oldIdx != 0xFFFFFFFFu) & (oldIdx != myIdx);
        const bool disp = fail & (oldIdx > myIdx);                         // displaced a later tuple: carry it on
        mlo = disp ? (uint32_t)old : mlo; mhi = disp ? (uint32_t)(old >> 32) : mhi;
        bool dropped = drop0 | drop1;
        if constexpr (COMPACT) {
            // a shadow tuple that runs out of budget BELOW my range is the previous wavefront's conflict, not mine; one that
            // tried a slot of my range first (its last try is home + probeLen - 1) came in as a crosser and is mine
            if (shadowOn) dropped = dropped & ((homeOfKey >= loSlot) | (homeOfKey + (probeLen - 1u) >= loSlot));
        }
        drops += dropped ? 1u : 0u; dropSum += dropped ? (unsigned long long)key : 0ull;
        if constexpr (HTM) {       // the bucket is full: the tuple is one of the reference's conflicts (HTMHashBuild.hpp:181-183)
            const unsigned long long cm = wv_ballot(dropped);
            if (cm) {
                if (dropped) myConflicts[cCount + lane_rank(cm)] = mine;
                cCount += (uint32_t)__popcll(cm);
            }
        }
        const unsigned long long dm = wv_ballot(toDefer);
        if (dm) {
            if constexpr (COMPACT) {
                // no deferred phase: a walk that leaves my range at the seam is listed for the check against what the
                // next wavefront let in (it has inserted the tuple itself); everything else only the classic build can do
                const bool crosser = toDefer & (pos == limSlot) & (homeOfKey < limSlot) & !lastChunk;
                const unsigned long long cmk = wv_ballot(crosser);
                raise(toDefer & !crosser, 1ull);
                if (cmk) {
                    if (crosser) myDeferred[dCount + lane_rank(cmk)].packed = mine;
                    dCount += (uint32_t)__popcll(cmk);
                }
            } else {
                defer(dm, toDefer, pos, mine);
            }
        }
        pos = fail ? ((pos + 1) & mask32) : pos;
        return recheck | fail;
    };
    // The retry queue is a FIFO ring (oldest entries first): a round takes the up to 64 oldest entries, whatever is
    // not finished goes back to the front. The queue is NOT drained at the end of a tile: fewer than
    // 64 entries wait for the next tile's failures, so that every round is dense (draining a tile to completion cost
    // ~10 sparse rounds per tile, more instructions than all the dense work together -- PMC, profiles/r02_*).
    auto retry_round = [&]() {
        const uint32_t take = qCount < 64u ? qCount : 64u;
        const bool has = lane < take;
        // lanes >= take read stale-but-in-bounds entries and ignore them
        const uint32_t at0 = (qHead + lane) & (kWvQCap - 1);
        uint32_t pos = myQPos[at0], mlo = myQLo[at0], mhi = CODES ? 0u : myQHi[at0];
        qHead = (qHead + take) & (kWvQCap - 1);
        qCount -= take;
        const bool again = round_body(pos, mlo, mhi, has);
        const unsigned long long am = wv_ballot(again);
        // what did not finish goes back to the queue's FRONT: an entry then gets its (at most probeLength) rounds one after
        // the other and is done while its slots are still far from the ring's tail, instead of waiting behind a tile's
        // worth of newer entries (COMPACT has no deferred phase: an entry the ring is about to leave behind costs a
        // forced round, below)
        const uint32_t back = (uint32_t)__popcll(am);
        qHead = (qHead - back) & (kWvQCap - 1);
        if (again) {
            const uint32_t at = (qHead + lane_rank(am)) & (kWvQCap - 1);
            myQPos[at] = pos; myQLo[at] = mlo; if constexpr (!CODES) myQHi[at] = mhi;
        }
        qCount += back;
        ++rounds;
    };
    // to completion: dense rounds while more than a wavefront's worth is queued, then the last <= 64 entries stay in
    // registers until they are done
    auto drain = [&]() {
        while (qCount > 64u) retry_round();
        bool act = lane < qCount;
        const uint32_t at0 = (qHead + lane) & (kWvQCap - 1);
        uint32_t pos = myQPos[at0], mlo = myQLo[at0], mhi = CODES ? 0u : myQHi[at0];
        qCount = 0;
        while (wv_ballot(act)) act = round_body(pos, mlo, mhi, act);
    };

    // tile t covers chunk offsets [t * kWvTile, ...); lane's tuple j sits at offset t * kWvTile + 64 j + lane
    // register prefetch, kWvPf tiles deep: the loads are issued unconditionally (lanes past the chunk's end are
    // masked, not branched around), so the compiler can count them and wait for one tile's loads only
    Elem nxt[kWvPf][kWvPer];
    auto issue = [&](Elem (&buf)[kWvPer], uint32_t at) {
#pragma unroll
        for (int j = 0; j < kWvPer; ++j) {
            const uint32_t o = at + lane + 64 * j;
            buf[j] = o < plen ? Rc[o] : (Elem)0;
        }
    };
#pragma unroll
    for (int p = 0; p < kWvPf; ++p) issue(nxt[p], (uint32_t)p * kWvTile);

    // COMPACT: lowest / highest home slot of the tile about to start, taken from its keys at the end of the tile before it
    // (forced rounds, below); only for full tiles
    uint32_t tminF = kNone, tmaxF = 0;
    (void)tminF; (void)tmaxF;
    static_assert(!COMPACT || kWvPf == 1, "the forced rounds look one tile ahead");
    for (uint32_t tb0 = 0; tb0 < plen; tb0 += kWvPf * kWvTile) {
#pragma unroll
      for (int p = 0; p < kWvPf; ++p) {
        const uint32_t tb = tb0 + (uint32_t)p * kWvTile;
        if (tb >= plen) break;                                        // wave-uniform
        uint32_t klo[kWvPer], khi[kWvPer];
#pragma unroll
        for (int j = 0; j < kWvPer; ++j) {
            klo[j] = (uint32_t)nxt[p][j];
            khi[j] = KEY32 ? 0u : (uint32_t)((uint64_t)nxt[p][j] >> 32);
        }
        {   // The CU arbitrates oldest wavefront first, and the four workgroups of a CU are dispatched one after the other:
            // measured at 2^27 (a development build recorded every wavefront's start and end), the wavefronts of a CU's first
            // workgroup took 349 us for their chunk, those of the second 380, the third 421, the fourth 470 -- the kernel
            // lasted 497 us and ran half empty for its last fifth. So every wavefront sets its issue priority per tile
            // from the wall clock: the four workgroup slots of a CU take turns at the top (10 us each). With it: 389 / 398 /
            // 398 / 400 us, kernel 446 us. (From 2^28 tuples on the later rounds of workgroups do the balancing; no gain or
            // loss there. An input without retry rounds is memory bound and hardly reacts: the arbitration that is
            // unfair to its younger wavefronts is the memory system's.)
            const uint32_t slot = (blockIdx.x / prioDiv) & 3u;
            const uint32_t pr = ((uint32_t)(wall_clock64() >> kWvPrioShift) + slot) & 3u;
            if (pr == 0) __builtin_amdgcn_s_setprio(0);
            else if (pr == 1) __builtin_amdgcn_s_setprio(1);
            else if (pr == 2) __builtin_amdgcn_s_setprio(2);
            else __builtin_amdgcn_s_setprio(3);
        }
        // wave-uniform: no shadow / head zone, no overlap zone (COMPACT: and no tail zone)
        if constexpr (COMPACT) {
            // somebody has raised the flag: nothing written from here on is ever looked at (every 8th tile: one scalar load)
            if ((tb & (8u * kWvTile - 1u)) == 7u * kWvTile && *reinterpret_cast<volatile unsigned long long*>(&ctr->compactFail)) return;
        }
        const bool full = (tb + kWvTile <= (cend < tailFrom ? cend : tailFrom)) & (tb >= S + kWvOverlap);
        // the next tile's loads: behind classify() on the slot-code road (below), where they can take the registers of this tile's high words
        if constexpr (!CODES) issue(nxt[p], tb + kWvPf * kWvTile);
        const uint32_t roundsAtTileStart = rounds;
        (void)roundsAtTileStart;
        uint32_t myMin = kNone, myMaxInv = kNone;                     // max kept as min of the complement
        uint32_t home[kWvPer];
        // per row: "a tuple this wavefront inserts" / "... and whose home slot it may touch now". Kept as one boolean per
        // row -- a lane mask in a scalar register pair, free to produce and to branch on -- not as bits of a per-lane word
        // (two VALU instructions per tuple to pack, two to unpack, in a kernel whose retry rounds are VALU bound)
        // (`own` is a batch's: the attempts and push rows below go in batches of ROWS rows)
        constexpr int ROWS = CODES ? kWvWordRows : kWvPer;
        static_assert(kWvPer % ROWS == 0, "whole batches");
        bool live[kWvPer], own[ROWS];
        // row j's home slot where the attempts and the push rows need it. CODES: made again from the key (identity hash: one
        // v_and) against a copy of the mask the optimiser cannot see through, so that no row's home slot stays in a register
        // from classify() to its push row -- eight VGPRs the road's occupancy has no room for
        auto home_of = [&](int j) -> uint32_t {
            if constexpr (CODES) {
                uint32_t m = mask32;
                asm volatile("" : "+s"(m));
                return klo[j] & m;
            } else {
                return home[j];
            }
        };
        // FULL tiles (every position is this chunk's own, no seam zone) skip the zone tests: they are all but the
        // first and the last one or two tiles of a chunk
        uint32_t badTile = 0;                                         // wave-uniform: invalid tuples of a full tile
        // COMPACT, first and last tiles of a chunk: which of the tile's tuples are inserted here (bit j) and counted here
        // (bit 8 + j). The zone tests are many, and unrolled over the tile's eight tuples per lane their lane masks took ~40
        // scalar registers more than the kernel has (spilled to vector lanes all over the hot path); so this cold path
        // takes the tuples one at a time in a rolled loop, re-reading the keys (cache hits).
        uint32_t zb = 0;
        (void)zb;
        if constexpr (COMPACT) {
            if (!full) {
#pragma unroll 1
                for (int j = 0; j < kWvPer; ++j) {
                    const uint32_t o = tb + lane + 64 * j;
                    const Elem t = o < plen ? Rc[o] : (Elem)0;
                    const uint32_t key = (uint32_t)t;
                    const bool okKey = (KEY32 || (uint32_t)((uint64_t)t >> 32) == 0) & (key != 0);
                    const uint32_t h = home32<HTM>(key, hshift, mask32);
                    const bool in = (o >= S) & (o < cend);
                    // inserted here: my tuples, except head-zone stragglers of the previous range; plus the next chunk's
                    // stragglers of MY range in the overlap zone ...
                    bool mine = o < cend ? !((o < S + kWvOverlap) & (h < loSlot)) : ((o < plen) & !lastChunk & (h < limSlot));
                    // ... shadow zone and head zone: tuples of the previous range's last granule are simulated here as well
                    // (it lists the ones that really leave it; k_wave_validate compares)
                    const bool shadowTuple = (o < S + kWvOverlap) & (h - loSlot + kGranSlots < kGranSlots) & (loSlot != 0);
                    // ... and a tuple of MY range that sits before the seam ("early arrival": a key a little ahead of its
                    // neighbours) is mine to insert; the previous wavefront leaves it (its tail zone, below)
                    if (o < S) mine = shadowTuple | ((o >= claimFrom) & (h >= loSlot)); else mine = mine | shadowTuple;
                    // my tail zone: tuples of the next range are the next wavefront's
                    if ((o >= tailFrom) & (o < cend) & (h >= limSlot)) mine = false;
                    // a tuple of the chunk proper, past the head zone, that belongs below my range: nobody else will insert
                    // it (the previous wavefront reads kWvOverlap positions past its end, no more)
                    const bool below = okKey & (o >= S + kWvOverlap) & (o < cend) & (h < loSlot);
                    raise(below, 8ull);
                    mine = mine & !below;
                    zb |= ((mine ? 1u : 0u) << j) | ((in ? 1u : 0u) << (8 + j));
                }
            }
        }
        auto classify = [&](auto fullTag) {
            constexpr bool FULL = decltype(fullTag)::value;
#pragma unroll
            for (int j = 0; j < kWvPer; ++j) {
                const uint32_t o = tb + lane + 64 * j;
                bool in, mineHere;
                if constexpr (COMPACT && !FULL) {
                    in = ((zb >> (8 + j)) & 1u) != 0; mineHere = ((zb >> j) & 1u) != 0;
                } else {
                    in = FULL || ((o >= S) & (o < cend));                         // counted here
                }
                bool okKey = (khi[j] == 0) & (klo[j] != 0);
                home[j] = home32<HTM>(klo[j], hshift, mask32);
                if constexpr (!(COMPACT && !FULL)) {
                    // inserted here: my tuples, except head-zone stragglers of the previous range; plus the next chunk's
                    // stragglers of MY range in the overlap zone
                    mineHere = FULL || (o < cend ? !((o < S + kWvOverlap) & (home[j] < loSlot))
                                                 : ((o < plen) & !lastChunk & (home[j] < limSlot)));
                }
                if constexpr (COMPACT) {
                    // the compact empty pattern cannot be a key: the classic build takes such an input. Its home slot is the
                    // table's last one, so a full tile (whose highest home slot is already known, tmaxF) only looks when
                    // that slot occurs at all -- one vector instruction per tuple saved in every other tile
                    if (!FULL || tmaxF == mask32) ffSeen |= in & (klo[j] == 0xFFFFFFFFu);
                }
                const bool ok = mineHere & okKey;
                inSum += in ? (unsigned long long)pack64(khi[j], klo[j]) : 0ull;
                if constexpr (FULL) badTile += 64u - (uint32_t)__popcll(wv_ballot(okKey));     // scalar: no per-lane count
                else if constexpr (CODES) bad += (uint32_t)__popcll(wv_ballot(in & !okKey));
                else bad += (in & !okKey) ? 1u : 0u;
                if constexpr (CHECK && CODES) foreign += (uint32_t)__popcll(wv_ballot(in & is_foreign(klo[j], sc)));
                else if constexpr (CHECK) foreign += (in & is_foreign(klo[j], sc)) ? 1u : 0u;
                live[j] = ok;
                if constexpr (FULL && COMPACT) {
                    // the bounds of a full tile were taken at its top (forced rounds)
                } else if constexpr (FULL) {
                    // full tiles take the bounds over every tuple, valid or not: an invalid key (the build fails with
                    // HJ_ERR_KEY_RANGE anyway) can only make the ring move less, and every access stays guarded
                    myMin = home[j] < myMin ? home[j] : myMin;
                    myMaxInv = ~home[j] < myMaxInv ? ~home[j] : myMaxInv;
                } else {
                    myMin = (ok & (home[j] < myMin)) ? home[j] : myMin;
                    myMaxInv = (ok & (~home[j] < myMaxInv)) ? ~home[j] : myMaxInv;
                }
            }
        };
        if (full) classify(std::true_type{}); else classify(std::false_type{});
        // CODES: the next tile's loads are issued here and not at the tile's top: khi[] is dead from here on, so the eight 64-bit
        // loads in flight cost eight registers less where the tile needs the most (kWvWordWpe)
        if constexpr (CODES) issue(nxt[p], tb + kWvPf * kWvTile);
        if constexpr (CODES) bad += badTile; else bad += lane == 0 ? badTile : 0u;
        uint32_t tmin, tmax = 0;                                      // tmin == kNone: the tile holds no valid tuple
        if (COMPACT && full) { tmin = tminF; tmax = tmaxF; }          // taken from the keys at the end of the tile before
        else { tmin = wave_umin(myMin); if (tmin != kNone) tmax = ~wave_umin(myMaxInv); }
        bool allIn = false;                                           // wave-uniform: every home slot of the tile lies in ring and range
        // CODES: the ring moves before each batch, only as far as that batch's highest home slot needs (below): rows 0-3 need
        // no room for rows 4-7, and the granules that stay are the history that queued entries and displacement chains of the
        // last tile or two still live in -- one move per tile, all the way, left 1.38 M tuples of 2^30 `uniform` behind the
        // ring, this leaves 0.25 M (tools/sim/ring_moves.c, profiles/ring_moves.md; rounds in front of a move for the entries
        // below its target take that to 0.05 M and cost the kernel more than the tail gives back: measured, not kept). Rounds
        // never move the ring, so where it stands for the second batch is known here: its target and its allIn wait in two
        // scalars.
        [[maybe_unused]] uint32_t target1 = 0;
        [[maybe_unused]] bool allIn1 = false;
        // how far the ring must move for the highest home slot `hi` (+ a probe walk) to fit: no further, so it keeps as much
        // history as it can, never past the tile's lowest home slot (an outlier key is deferred, not the tile), never out of
        // the range
        [[maybe_unused]] auto ring_target = [&](uint32_t hi, uint32_t gmin) -> uint32_t {
            const uint32_t top = (uint32_t)(((uint64_t)hi + probeLen + 8u) >> kGranShift) + 1u;
            uint32_t target = top > RGRAN ? top - RGRAN : 0u;
            target = target < gmin ? target : gmin;
            return target < limG ? target : limG;
        };
        if (tmin != kNone) {
            // The ring moves only as far as it must for the tile's highest home slot (+ a probe walk) to fit, so it
            // keeps as much history as it can: retry entries carried over from the previous tile are still inside.
            // It never moves past the tile's lowest home slot (an outlier key is deferred, not the tile).
            const uint32_t top = (uint32_t)(((uint64_t)tmax + probeLen + 8u) >> kGranShift) + 1u;
            uint32_t target = top > RGRAN ? top - RGRAN : 0u;
            const uint32_t gmin = tmin >> kGranShift;
            target = target < gmin ? target : gmin;
            target = target < limG ? target : limG;
            if constexpr (!CODES) advance(target);
            if constexpr (CODES) {
                // forced road only (keyLimit = 0: every key has a code): a key whose high part no code holds
                if (cr.keyLimit) {
                    bool over = false;
#pragma unroll
                    for (int j = 0; j < kWvPer; ++j) over |= live[j] & (klo[j] >= cr.keyLimit);
                    if (wv_ballot(over) && lane == 0) atomicOr(&ctr->planarFail, 4ull);
                }
            } else if constexpr (PLANAR) {
                // key 0xFFFFFFFF, the 4-byte empty pattern: its home slot is the table's last one, so only a tile that reaches
                // that slot looks for it (one scalar compare per tile otherwise)
                if (tmax == mask32) {
                    bool ff = false;
#pragma unroll
                    for (int j = 0; j < kWvPer; ++j) ff |= live[j] & (klo[j] == 0xFFFFFFFFu);
                    if (wv_ballot(ff) && lane == 0) atomicOr(&ctr->planarFail, 2ull);
                }
            }
            const uint32_t gmax = tmax >> kGranShift;
            if constexpr (!CODES) allIn = full & (gmin - winLoG < RGRAN) & (gmax - winLoG < RGRAN) & (gmax < limG);
        }
        if (tmin != kNone) {
            if constexpr (CODES) {
                const uint32_t gmin = tmin >> kGranShift, gmax = tmax >> kGranShift;
                // the highest home slot of the first batch's rows, taken here from the keys: inside classify() it would cost
                // a register through rows 4-7, where the tile has none to spare (a full tile's bounds go over every tuple)
                uint32_t myMaxA = 0;
#pragma unroll
                for (int j = 0; j < ROWS; ++j) {
                    const uint32_t h = home_of(j);
                    myMaxA = ((full | live[j]) & (h > myMaxA)) ? h : myMaxA;
                }
                const uint32_t tmaxA = ~wave_umin(~myMaxA), gmaxA = tmaxA >> kGranShift;
                advance(ring_target(tmaxA, gmin));
                allIn = full & (gmin - winLoG < RGRAN) & (gmaxA - winLoG < RGRAN) & (gmaxA < limG);
                target1 = ring_target(tmax, gmin);
                const uint32_t lo1 = winLoG > target1 ? winLoG : target1;
                allIn1 = full & (gmin - lo1 < RGRAN) & (gmax - lo1 < RGRAN) & (gmax < limG);
            }
        }

        // ---- the home-slot attempts and the push rows, one batch of ROWS rows after the other ----
        // ROWS = kWvPer (the 8-byte rings): the tile's eight attempts are issued together, then its eight rows are pushed.
        // ROWS = kWvWordRows (the slot-code road): the same for rows 0-3, then for rows 4-7, so that four returned words and
        // four `own` masks are live at a time instead of eight -- the registers the road's occupancy hangs on (kWvWordWpe).
        // The table is the same. The protocol is confluent (index-priority protocol): the slots' final values do
        // not depend on the order of the atomicMins, and the attempts of rows 4-7 are the same operations, applied after
        // rows 0-3 were pushed and perhaps had a round. Rows 0-3 hold the tile's first 256 positions, so nothing of rows 4-7
        // can be displaced by them later; a round between the batches treats what it finds in a slot as any round does.
        // The queue's invariant is per row (`while (qCount >= kWvRoundAt)` before every push leaves room for one full
        // step of 64). The 8-byte rings moved once, above; the slot-code road moves its ring before each batch, and each batch
        // has its own allIn: in_ring holds through a batch because rounds never move the ring.
        int b = 0;                                                    // the batch's first row
#pragma unroll
        do {
        if constexpr (CODES) {
            if (b) { advance(target1); allIn = allIn1; }
        }
        std::conditional_t<CODES, uint32_t, unsigned long long> oldv[ROWS];
        // the PER home-slot attempts of a batch, issued together (independent LDS round trips)
        // (when the tile's lowest and highest home slot are inside ring and range -- nearly every full tile -- the
        // per-tuple test is skipped: the retry rounds leave the VALU little to spare, hj DESIGN 4.2)
        auto attempts = [&](auto allTag) {
            constexpr bool ALL = decltype(allTag)::value;
#pragma unroll
            for (int r = 0; r < ROWS; ++r) {
                const int j = b + r;
                const uint32_t hm = home_of(j);
                own[r] = live[j] & (ALL || in_ring(hm));
                if constexpr (CODES) {
                    oldv[r] = RingWord::kEmpty;
                    if (own[r]) oldv[r] = atomicMin(&win32[hm & (RWIN - 1)], rw.at_home(tb + lane + 64 * j, klo[j]));
                } else {
                oldv[r] = kEmpty;
                if (own[r])
                    oldv[r] = atomicMin(reinterpret_cast<unsigned long long*>(&win[hm & (kWvWin - 1)]),
                                        (unsigned long long)pack64(idx0 + tb + lane + 64 * j, klo[j]));
                }
            }
        };
        if (allIn) attempts(std::true_type{}); else attempts(std::false_type{});
        // ---- whatever did not finish goes to the retry queue, compacted ----
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int j = b + r;
            while (qCount >= kWvRoundAt) retry_round();                // dense rounds; leaves room for one full step
            const bool lv = live[j], ow = own[r];
            const uint32_t hm = home_of(j);
            uint32_t pos, mlo, mhi;
            bool again;
            if constexpr (CODES) {
                mlo = rw.at_home(tb + lane + 64 * j, klo[j]); mhi = 0u;
                const bool fail = ow & (oldv[r] != RingWord::kEmpty);  // the slot was taken
                mlo = (fail & (oldv[r] > mlo)) ? oldv[r] : mlo;        // ... by a later tuple: it moves on instead
                // the home slot was the carried tuple's last try (the displaced one's, or probeLength 1): dropped here
                const bool spent = fail & (rw.tries_left(mlo, probeLen) <= 1u);
                if (wv_ballot(spent)) {
                    drops += (uint32_t)__popcll(wv_ballot(spent)); dropSum += spent ? (unsigned long long)rw.key(mlo, hm, mask32) : 0ull;
                }
                const bool on = fail & !spent;
                pos = on ? ((hm + 1) & mask32) : hm; mlo = on ? RingWord::step(mlo) : mlo;
                again = on | (lv & !ow);
            } else {
            mlo = klo[j]; mhi = idx0 + tb + lane + 64 * j;
            const uint32_t oldIdx = (uint32_t)(oldv[r] >> 32);
            const bool fail = ow & (oldIdx != 0xFFFFFFFFu);            // the slot was taken
            const bool disp = fail & (oldIdx > mhi);                   // ... by a later tuple: it moves on instead
            mlo = disp ? (uint32_t)oldv[r] : mlo; mhi = disp ? (uint32_t)(oldv[r] >> 32) : mhi;
            pos = fail ? ((hm + 1) & mask32) : hm;
            again = fail | (lv & !ow);                                 // outside ring or range: the retry round defers it
            }
            const unsigned long long am = wv_ballot(again);
            if (am) {
                if (again) {
                    const uint32_t at = (qHead + qCount + lane_rank(am)) & (kWvQCap - 1);
                    myQPos[at] = pos; myQLo[at] = mlo; if constexpr (!CODES) myQHi[at] = mhi;
                }
                qCount += (uint32_t)__popcll(am);
            }
        }
        b += ROWS;
        } while (ROWS < kWvPer && b < kWvPer);                        // one batch: no loop at all, whatever the optimiser does
        if constexpr (COMPACT) {
            // Forced rounds. A queued entry whose slot the ring is about to leave behind would have to be deferred, and
            // there is no deferred phase: it gets its rounds now, at the end of the tile, where nothing of the tile is
            // in registers any more and the one retry loop of this place serves (fewer than 64 entries wait then: one
            // lane each). How far the ring will move is known from the NEXT tile's keys, which the prefetch has already
            // brought: a full tile's bounds go over every tuple, valid or not (rule of the ring above), and stay in two
            // scalar registers for its classification; before a chunk's first and last tiles everything queued simply
            // finishes. The first tile (shadow zone + head zone) ends the shadow phase the same way: once the queue is
            // empty the shadow granule is dropped (it is never written), so that from here on a tuple that belongs below
            // my range cannot land in it unnoticed -- it falls out of the ring and raises the flag.
            const uint32_t tbN = tb + kWvTile;
            uint32_t tslot = 0xFFFFFFFFu;
            const bool endShadow = shadowOn;
            if ((tbN + kWvTile <= (cend < tailFrom ? cend : tailFrom)) & (tbN >= S + kWvOverlap)) {
                uint32_t mn = kNone, mxInv = kNone;
#pragma unroll
                for (int j = 0; j < kWvPer; ++j) {
                    const uint32_t h = home32<HTM>((uint32_t)nxt[p][j], hshift, mask32);
                    mn = h < mn ? h : mn; mxInv = ~h < mxInv ? ~h : mxInv;
                }
                tminF = wave_umin(mn); tmaxF = ~wave_umin(mxInv);
                const uint32_t top = (uint32_t)(((uint64_t)tmaxF + probeLen + 8u) >> kGranShift) + 1u;
                uint32_t target = top > kWvGran ? top - kWvGran : 0u;
                const uint32_t gmin = tminF >> kGranShift;
                target = target < gmin ? target : gmin;
                target = target < limG ? target : limG;
                if (!endShadow) tslot = target > winLoG ? target << kGranShift : 0u;
            }
            for (;;) {
                bool need = qCount >= kWvRoundAt;
                if (!need && qCount && tslot) {
                    const uint32_t qp = myQPos[(qHead + lane) & (kWvQCap - 1)];
                    need = wv_ballot((lane < qCount) & (qp < tslot)) != 0;
                }
                if (!need) break;
                retry_round();
            }
            if (endShadow) {
                shadowOn = false;
                while (winLoG < loG) {
                    *ring_granule(winLoG) = make_ulonglong2(kEmpty, kEmpty);
                    ++winLoG;
                }
            }
        } else {
        while (qCount >= kWvRoundAt) retry_round();
        // an entry may wait for company for one tile, not longer (the ring moves on): no round during this tile -> one now
        if (qCount && rounds == roundsAtTileStart) retry_round();
        }
      }
    }
    if (qCount) drain();

    // ---- the rest of the range: what is left in the ring, then empties up to the next chunk's range ----
    uint32_t endG = limG;
    if (lastChunk) endG = winLoG + RGRAN < numGran ? winLoG + RGRAN : numGran;
    advance(endG);
    if (lane == 0) {
        if (c == 0) ctr->ownLo = (unsigned long long)loG << kGranShift;
        if (lastChunk) ctr->ownHiEx = (unsigned long long)winLoG << kGranShift;
        dcounts[c] = dCount;
        if constexpr (HTM) ccounts[c] = cCount;
        if constexpr (COMPACT) pcounts[c] = pCount;
    }
    if constexpr (COMPACT) {
        raise(ffSeen, 4ull);
        dCount = 0;                              // crossers are not deferred tuples: the next wavefront has inserted them
    }

    __builtin_amdgcn_s_setprio(0);               // the rotation's priority is not carried into the counter atomics
    // counters: one atomic per wavefront
    if constexpr (CODES) { if (lane != 0) drops = bad = foreign = 0u; }
    unsigned long long c0 = drops, c3 = bad | ((unsigned long long)foreign << 32);
    const unsigned long long c4 = dCount;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        c0 += __shfl_down(c0, off, 64);
        dropSum += __shfl_down(dropSum, off, 64);
        inSum += __shfl_down(inSum, off, 64);
        c3 += __shfl_down(c3, off, 64);
    }
    uint32_t loInv = ~usedLo, hi1 = usedHi1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t a = __shfl_down(loInv, off, 64), b = __shfl_down(hi1, off, 64);
        loInv = a > loInv ? a : loInv; hi1 = b > hi1 ? b : hi1;
    }
    if (lane == 0) {
        Counters::Shard* const sh = counter_shard(ctr);
        if (c0) atomicAdd(&sh->conflicts, c0);
        if (dropSum) atomicAdd(&sh->conflictSum, dropSum);
        if (inSum) atomicAdd(&sh->inputSum, inSum);
        if (c3 & 0xFFFFFFFFull) atomicAdd(&sh->badKeys, c3 & 0xFFFFFFFFull);
        if (c3 >> 32) atomicAdd(&sh->foreign, c3 >> 32);
        if (c4) atomicAdd(&sh->deferred, c4);
        if (hi1) { atomicMax(&sh->usedLoInv, (unsigned long long)loInv); atomicMax(&sh->usedHi1, (unsigned long long)hi1); }
    }
}

// Phase B for the sliced deferred queue: chunk c's entries are queue[c * chunkLen .. + dcounts[c]). Same walk as
// k_build_deferred (hj_build_own.hip): the probe walk of every deferred tuple finished with global atomics. The walks
// are chains of dependent memory-side atomics, and what bounds the phase is their THROUGHPUT, not its shape: 947 k entries
// at 2^30 `uniform` take 101-107 us whether a workgroup takes a slice (round 2), a wavefront does (now), or the entries are
// numbered through and dealt out to all lanes (round 3, binary search in a prefix of the counts: 104 us) -- 1.8 returning
// 64-bit atomics per entry at the 17 G/s the global-atomic build reaches too.
// PLANAR (the table of k_build_wave<PLANAR>): the same walk on the INDEX plane alone, with a 32-bit atomicMin. Order and
// equality of slot values are those of their index words (round_body's look relies on the same), so the index plane
// decides every step; the key of a displaced tuple is no longer in the slot and is read from R by its index, R[old -
// idxBase] (R is resident for the whole build). The walks never write the key plane: two walkers that win the same slot one
// after the other would race with plain stores. Every successful atomicMin instead appends its slot number to the walker's
// dirty log -- the unused rest of the slice it walks, 4 slot numbers per free entry; one wavefront per slice, so a ballot
// rank and a wave-uniform count place it -- and k_wave_fixup, behind the kernel boundary, writes the key of every logged
// slot from what the index plane holds then. A log that does not fit raises Counters::planarFail (an input that defers
// nearly everything: the rings forced onto a relation without locality).
struct PlanarWalk { const void* R; bool key32; uint64_t idxBase; uint32_t* lcounts; };
// the key of the tuple with index word idx (the index plane holds nothing but indices the build handed out, and empty)
__device__ __forceinline__ uint32_t planar_key_of(const PlanarWalk& pw, uint32_t idx)
{
    const uint32_t at = idx - (uint32_t)pw.idxBase;
    return pw.key32 ? static_cast<const uint32_t*>(pw.R)[at] : (uint32_t)static_cast<const uint64_t*>(pw.R)[at];
}
template <bool HTM, bool PLANAR>
__global__ void __launch_bounds__(kBlock)
k_wave_deferred(DeferredEntry* __restrict__ queue, const uint32_t* __restrict__ dcounts, uint32_t nChunks,
                uint32_t chunkLen, uint64_t* __restrict__ table, uint64_t mask, uint32_t hshift, uint32_t probeLen,
                Counters* __restrict__ ctr, Gate gate, uint64_t* __restrict__ htmConflicts, uint32_t* __restrict__ ccounts,
                const uint32_t* __restrict__ routeBounds, PlanarWalk pw)
{
    static_assert(!(HTM && PLANAR), "the bucketised table keeps its packed slots");
    if (gate_closed(gate)) return;
    // Key 0xFFFFFFFF seen by k_build_wave: the packed build redoes everything. Other wavefronts of THIS kernel raise bit 0 while
    // this plain load runs, so some may return here and others walk on: harmless only because k_wave_fixup, behind the kernel
    // boundary, throws the whole planar table away when any bit is set.
    if constexpr (PLANAR) { if (ctr->planarFail) return; }
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t mask32 = (uint32_t)mask;
    [[maybe_unused]] uint32_t* const idxPlane = PLANAR ? planar_index_plane(table, mask + 1) : nullptr;
    unsigned long long drops = 0, dropSum = 0;
    // a wavefront per slice (~220 entries per slice on `uniform` with one round of chunks, ~29 in each of 32768 slices at 2^30)
    for (uint32_t c = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); c < nChunks; c += gridDim.x * (kBlock / 64)) {
        const uint32_t cnt = dcounts[c];
        DeferredEntry* const q = slice_deferred(queue, c, chunkLen);
        [[maybe_unused]] const auto log = slice_dirty_log(queue, c, chunkLen, cnt);      // PLANAR
        [[maybe_unused]] uint32_t logCount = 0;                                           // wave-uniform
        for (uint32_t i0 = 0; i0 < cnt; i0 += 64) {
            const uint32_t i = i0 + lane;
            const bool has = i < cnt;
            const uint64_t first = has ? q[i].packed : 0ull;
            uint32_t key = (uint32_t)first, idx = (uint32_t)(first >> 32);
            uint32_t pos = has ? (uint32_t)q[i].pos : 0u;
            uint32_t budget = probeLen - ((pos - home32<HTM>(key, hshift, mask32)) & mask32);
            bool dropped = false;
            // one step of every walk per turn, the wavefront together (the log's count stays wave-uniform)
            for (bool act = has; wv_ballot(act);) {
                const bool out = act & (budget == 0);
                if (out) { drops += 1; dropSum += key; dropped = true; }
                act &= !out;
                uint32_t oldIdx = idx, oldKey = 0;
                if (act) {
                    if constexpr (PLANAR) {
                        oldIdx = atomicMin(idxPlane + pos, idx);
                    } else {
                        const unsigned long long old = atomicMin(reinterpret_cast<unsigned long long*>(table + pos),
                                                                 (unsigned long long)pack64(idx, key));
                        oldIdx = (uint32_t)(old >> 32); oldKey = (uint32_t)old;
                    }
                }
                if constexpr (PLANAR) {
                    const unsigned long long wm = wv_ballot(oldIdx > idx);         // the slot's index word changed
                    if (wm) {
                        const uint32_t at = logCount + lane_rank(wm);
                        if ((oldIdx > idx) & (at < log.cap)) log.slot[at] = pos;
                        logCount += (uint32_t)__popcll(wm);
                    }
                }
                // empty (the highest index word) or my own: placed
                act &= (oldIdx != kNone) & (oldIdx != idx);
                if (act) {
                    if (oldIdx > idx) {                                            // I stay, the displaced tuple walks on
                        if constexpr (PLANAR) oldKey = planar_key_of(pw, oldIdx);
                        key = oldKey; idx = oldIdx;
                        // (a tuple sits less than probeLen slots from its home; anything else ends the walk)
                        const uint32_t dist = (pos - home32<HTM>(key, hshift, mask32)) & mask32;
                        budget = dist < probeLen ? probeLen - (dist + 1) : 0u;
                    } else {
                        budget -= 1;
                    }
                    pos = (pos + 1) & mask32;
                }
            }
            if constexpr (HTM) {
                const uint64_t mine = pack64(idx, key);
                // the slice's conflict list is appended to by four wavefronts now: one atomic per wavefront reserves the places
                // (ccounts[c] holds what k_build_wave recorded; the list's order is free, the chain phase sorts by index)
                if (routeBounds) {
                    // routed (hj_htm.hip, the chain phase in LDS): the conflict is filed under the chunk that OWNS its bucket's
                    // granule -- the last chunk whose first granule is not above it --, so that a slice of the list holds all
                    // conflicts of its chunk's range. A slice that cannot take it: the host redoes the build unrouted.
                    if (dropped) {
                        const uint32_t gran = (uint32_t)(home32<true>((uint32_t)mine, hshift, (uint32_t)mask) >> kGranShift);
                        uint32_t a = 0, b = nChunks;                                   // bounds[a] <= gran (or a = 0), answer in [a, b)
                        while (b - a > 1) { const uint32_t mid = (a + b) >> 1; if (routeBounds[mid] <= gran) a = mid; else b = mid; }
                        const uint32_t at = atomicAdd(&ccounts[a], 1u);
                        if (at < chunkLen) htmConflicts[(uint64_t)a * chunkLen + at] = mine;
                        else atomicOr(&ctr->htmChainBail, kChainBailSliceFull);
                    }
                    continue;
                }
                const unsigned long long cm = wv_ballot(dropped);
                if (cm) {
                    uint32_t base = 0;
                    if (lane == (uint32_t)__ffsll((long long)cm) - 1u) base = atomicAdd(&ccounts[c], (uint32_t)__popcll(cm));
                    base = (uint32_t)__shfl((int)base, __ffsll((long long)cm) - 1, 64);
                    if (dropped) htmConflicts[(uint64_t)c * chunkLen + base + lane_rank(cm)] = mine;
                }
            }
        }
        if constexpr (PLANAR) {
            if (lane == 0) {
                pw.lcounts[c] = logCount < log.cap ? logCount : log.cap;
                if (logCount > log.cap) atomicOr(&ctr->planarFail, 1ull);
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        drops += __shfl_down(drops, off, 64);
        dropSum += __shfl_down(dropSum, off, 64);
    }
    if (lane == 0) {
        if (drops) atomicAdd(&counter_shard(ctr)->conflicts, drops);
        if (dropSum) atomicAdd(&counter_shard(ctr)->conflictSum, dropSum);
    }
}

// as if the build so far had never run: every sum and maximum a build kernel adds to (one wavefront, a shard per lane)
__device__ __forceinline__ void reset_build_counters(Counters* __restrict__ ctr, uint32_t lane)
{
    static_assert(Counters::kShards == 64, "one shard per lane");
    ctr->shard[lane] = Counters::Shard{};
    if (lane == 0) {
        ctr->conflicts = 0; ctr->conflictSum = 0; ctr->inputSum = 0; ctr->badKeys = 0; ctr->deferred = 0; ctr->foreign = 0;
        ctr->usedLoInv = 0; ctr->usedHi1 = 0; ctr->ownLo = 0; ctr->ownHiEx = 0;
    }
}

// PLANAR, behind the walks' kernel boundary (the only ordering used): a wavefront per slice writes, for every slot of the
// slice's dirty log, the key that belongs to what the index plane holds now -- key[s] = index[s] == empty ? empty : low word
// of R[index[s] - idxBase]. A slot logged twice (by one walker after the other) gets the same value twice. The first
// wavefront also closes the planar build: no flag raised -> the table is in the 4-byte format; otherwise counters back to
// zero and Counters::packedRedo = 1, on which the packed classic build behind this kernel is gated (it writes every slot
// again; nothing of this build is looked at).
__global__ void __launch_bounds__(kBlock)
k_wave_fixup(const DeferredEntry* __restrict__ queue, const uint32_t* __restrict__ dcounts, uint32_t nChunks, uint32_t sliceLen,
             uint64_t* __restrict__ table, uint64_t tableSize, Counters* __restrict__ ctr, Gate gate, PlanarWalk pw,
             bool codes, SlotCode sc)
{
    if (gate_closed(gate)) return;
    const uint32_t lane = threadIdx.x & 63;
    const bool fail = ctr->planarFail != 0;                // final: raised by the kernels before this one only
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        if (fail) {
            reset_build_counters(ctr, lane);
            if (lane == 0) { ctr->tableFormat = kFormatSlots8; ctr->packedRedo = 1; }
        } else if (lane == 0) {
            ctr->tableFormat = codes ? kFormatCodes1 : kFormatKeys4;
        }
    }
    if (fail) return;
    uint32_t* const keys = reinterpret_cast<uint32_t*>(table);
    uint8_t* const codePlane = reinterpret_cast<uint8_t*>(table);
    const uint32_t* const idxPlane = planar_index_plane(table, tableSize);
    for (uint32_t c = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); c < nChunks; c += gridDim.x * (kBlock / 64)) {
        const uint32_t* const log = slice_dirty_log(queue, c, sliceLen, dcounts[c]).slot;
        const uint32_t cnt = pw.lcounts[c];
        for (uint32_t i = lane; i < cnt; i += 64) {
            const uint32_t s = log[i];                     // a walker's pos: masked, always inside the table
            const uint32_t idx = idxPlane[s];
            // codes: a byte store per logged slot -- two logged slots of one 4-byte word each get their own byte, nobody
            // reads a word to write it back
            if (codes) codePlane[s] = (uint8_t)(idx == kNone ? kCodeEmpty : sc.encode(planar_key_of(pw, idx), s));
            else keys[s] = idx == kNone ? kNone : planar_key_of(pw, idx);
        }
    }
}

// After k_build_wave: the valid slot range (hj_common.h, Counters) = the owned stretch [ownLo, ownHiEx) joined
// with the blocks deferred tuples start from (+1: a probe walk spills at most probeLen - 1 slots). If it reaches
// the table's end the whole table is made valid (set_valid_range). One wavefront. (Round 3 tried this fold inside
// k_wave_fill_edges, every workgroup for itself, to save the launch: 4 us at 2^22 -- and 55 us at 2^30, with 128 or
// with 1024 workgroups, against 4.4 + 4.9 us for the two launches: taken back.)
__global__ void k_wave_finalize_range(Counters* __restrict__ ctr, uint64_t tableSize, Gate gate)
{
    if (blockIdx.x != 0 || threadIdx.x >= 64 || gate_closed(gate)) return;
    const UsedBlocks used = fold_used_blocks(ctr);
    if (threadIdx.x != 0) return;
    unsigned long long lo = ctr->ownLo, hiEx = ctr->ownHiEx;
    if (used.hi1) {
        const unsigned long long dlo = (unsigned long long)(uint32_t)~(uint32_t)used.loInv << 9, dhi = (used.hi1 + 1) << 9;
        lo = dlo < lo ? dlo : lo; hiEx = dhi > hiEx ? dhi : hiEx;
    }
    set_valid_range(ctr, lo, hiEx, tableSize);
}

// Slots of the valid range (+512 slots of defined contents past it, + the slack past the table) that no wavefront
// owned: [validLo, ownLo) and [ownHiEx, validHiEx + 512). W = the table's word: uint64_t packed slots, or uint32_t, the key
// plane of the 4-byte formats; the empty pattern is all ones in both, written 16 bytes per store.
// plane2 != nullptr (the planar retire's index plane): the same stretches there read empty too -- that is everywhere a
// deferred walk can step outside the owned range (the valid range covers the blocks the walks start from + one)
// (uint8_t: the code plane of kFormatCodes1, 16 slots per store; its index plane is the same plane of 4-byte words)
template <class W>
__global__ void __launch_bounds__(kBlock)
k_wave_fill_edges(W* __restrict__ table, uint32_t* __restrict__ plane2, const Counters* __restrict__ ctr, uint64_t tableSize, Gate gate)
{
    if (gate_closed(gate)) return;
    const uint4 e = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    const uint64_t stride = (uint64_t)gridDim.x * kBlock, t0 = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    uint64_t hi = ctr->validHiEx + 512;
    hi = hi < tableSize ? hi : tableSize;
    const uint64_t validLo = ctr->validLo, ownLo = ctr->ownLo, ownHiEx = ctr->ownHiEx;
    auto fill = [&](void* plane, uint32_t perStore) {                    // all bounds are multiples of 128 (granules) or 512
        const uint64_t a0 = validLo / perStore, a1 = ownLo / perStore, b0 = ownHiEx / perStore, b1 = hi / perStore;
        uint4* const p4 = static_cast<uint4*>(plane);
        for (uint64_t v = a0 + t0; v < a1; v += stride) p4[v] = e;
        for (uint64_t v = b0 + t0; v < b1; v += stride) p4[v] = e;
    };
    fill(table, sizeof(uint4) / sizeof(W));
    if constexpr (sizeof(W) <= sizeof(uint32_t)) { if (plane2) fill(plane2, sizeof(uint4) / sizeof(uint32_t)); }   // only the planar formats have a second plane
    if (blockIdx.x == 0 && threadIdx.x < kTableSlack) table[tableSize + threadIdx.x] = (W)~(W)0;
}


// ---- compact table: the check and the decision (see k_build_wave<COMPACT>) ----------------------------------------
// Seam c (between chunks c-1 and c): the tuples that left chunk c-1's range at its upper end must be exactly the ones
// chunk c let in from its shadow granule. One thread per seam; the lists hold a handful of entries.
__global__ void __launch_bounds__(kBlock)
k_wave_validate(const DeferredEntry* __restrict__ queue, const uint32_t* __restrict__ dcounts, const uint32_t* __restrict__ pcounts,
                uint32_t nChunks, uint32_t sliceLen, Counters* __restrict__ ctr, Gate gate)
{
    if (gate_closed(gate)) return;
    if (*reinterpret_cast<volatile unsigned long long*>(&ctr->compactFail)) return;    // counts of skipped chunks are not defined
    const uint32_t c = blockIdx.x * kBlock + threadIdx.x + 1;
    if (c >= nChunks) return;
    const uint32_t nOut = dcounts[c - 1], nIn = pcounts[c];
    bool ok = nOut == nIn && nIn <= kWvPredCap;
    if (ok && nIn) {
        const DeferredEntry* out = slice_deferred(queue, c - 1, sliceLen);
        const uint64_t* in = slice_crossers(queue, c, sliceLen);
        for (uint32_t i = 0; i < nOut && ok; ++i) {
            const uint64_t v = out[i].packed;
            bool found = false;
            for (uint32_t k = 0; k < nIn; ++k) found |= in[k] == v;
            ok = found;                            // index words are unique: equal counts + every element found = equal sets
        }
    }
    if (!ok) atomicOr(&ctr->compactFail, 16ull);
}

// One wavefront. All seams check out and nobody raised the flag: the table is in the compact format, its valid range is
// what the wavefronts owned. Otherwise: as if the compact build had never run -- counters back to zero, and the variant
// word set to the classic build that is enqueued behind this kernel, gated on it.
__global__ void k_wave_decide(Counters* __restrict__ ctr, uint64_t tableSize, uint32_t fallbackVariant, Gate gate)
{
    if (blockIdx.x != 0 || threadIdx.x >= 64 || gate_closed(gate)) return;
    const bool fail = ctr->compactFail != 0;
    if (fail) {
        reset_build_counters(ctr, threadIdx.x);
        if (threadIdx.x == 0) {
            ctr->tableFormat = kFormatSlots8;
            ctr->variant = fallbackVariant;
        }
        return;
    }
    if (threadIdx.x != 0) return;
    set_valid_range(ctr, ctr->ownLo, ctr->ownHiEx, tableSize);
    ctr->tableFormat = kFormatKeys4;
}

__global__ void k_set_variant(Counters* __restrict__ ctr, uint32_t v)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) ctr->variant = v;
}
void launch_set_variant(Counters* ctr, uint32_t v, hipStream_t s) { hipLaunchKernelGGL(k_set_variant, dim3(1), dim3(64), 0, s, ctr, v); }

// ---- host side ----------------------------------------------------------------------------------------------------
size_t wave_lds_bytes() { return kWvLdsBytes; }
bool wave_supported(uint64_t tableSize) { return tableSize >= (uint64_t)kWvWin; }
bool wave_codes_supported(uint64_t n, int nCU, uint64_t tableSize)
{
    // the table is no smaller than a ring, and every position a wavefront reads has a ring word (RingWord::holds: a slice
    // is longer than anything a wavefront reads). Otherwise the caller retires 4-byte keys out of the 8-byte ring.
    return tableSize >= ((uint64_t)kWvWordGran << kGranShift) && RingWord::holds(wave_layout(n, nCU).sliceLen);
}
constexpr uint32_t kWvCompactMaxProbe = 32;         // the largest probeLength the compact build takes
bool wave_compact_supported(uint64_t tableSize, uint32_t probeLen)
{
    // the shadow granule must cover every slot a walk across the seam can start from
    return wave_supported(tableSize) && probeLen >= 1 && probeLen <= kWvCompactMaxProbe;
}
static uint64_t wave_chunk_len(uint64_t n, int nCU)
{
    // One chunk per resident wavefront is a single round of workgroups -- and the kernel then lasts as long as its
    // SLOWEST wavefront: the streams of 4096 wavefronts do not advance at the same rate (memory channels, neighbours on the
    // CU), and with a static split nobody takes over from a wavefront that is done. Measured: the kernel's time is
    // 97 us + 1.81 ms per 2^29 tuples from 2^27 to 2^30 -- a size-independent ~100 us of waiting for stragglers. So large
    // relations are cut into several rounds' worth of chunks and the hardware's workgroup dispatcher does the balancing
    // (a workgroup that finishes makes room for the next four chunks): 2^30 tuples in 4 x 4096 chunks 3.68 -> 3.49 ms,
    // in 8 x 4096 chunks 3.46 ms.
    // Chunks stay >= kWvMinChunk tuples, though: every chunk pays for its ring (fill, final flush) and for two seam
    // tiles, and at 2^27 two rounds of 16384-tuple chunks were 2 % SLOWER than one round, four rounds 6 % (32768 against
    // 65536 as the minimum: the same at 2^28, -2 % at 2^29, -1..3 % at 2^30; 16 rounds instead of 8: slower).
    const uint32_t resident = kWvWavesPerCu * (uint32_t)nCU;
    uint64_t rounds = n / ((uint64_t)resident * kWvMinChunk);
    rounds = rounds < 1 ? 1 : rounds > kWvMaxRounds ? kWvMaxRounds : rounds;
    const uint64_t chunks = (uint64_t)resident * rounds;
    uint64_t chunkLen = (n + chunks - 1) / chunks;
    chunkLen = (chunkLen + kWvTile - 1) / kWvTile * kWvTile;
    return chunkLen < kWvShortestChunk ? kWvShortestChunk : chunkLen;
}
// the geometry of a build: every other function takes it from here. A slice has room for the chunk and for what the seams
// on either side may add to it (the pre-pass moves a seam forward by less than kWvLook; kWvOverlap positions of the next chunk)
WaveLayout wave_layout(uint64_t n, int nCU)
{
    static_assert(kWvShortestChunk > kWvLook + kWvOverlap, "a seam may move by less than the shortest chunk");
    static_assert(kWvShadow + kWvOverlap == (uint32_t)kWvTile, "shadow zone + head zone = the first tile of a compact chunk");
    const uint64_t chunkLen = wave_chunk_len(n, nCU);
    return WaveLayout{chunkLen, (n + chunkLen - 1) / chunkLen, chunkLen + kWvLook + kWvOverlap, kWvTileTuples, kGranSlots, kWvGran,
                      kWvLook, kWvOverlap, kWvShadow, kWvTail, kWvPredCap, kWvCompactMaxProbe};
}
static size_t wave_queue_entries(const WaveLayout& w) { return (size_t)(w.nChunks * w.sliceLen + 64); }
size_t wave_queue_bytes(uint64_t n, int nCU) { return wave_queue_entries(wave_layout(n, nCU)) * sizeof(DeferredEntry); }
// the conflict list of the bucketised table: a slice per chunk like the deferred queue's, of 8-byte entries
size_t wave_conflict_bytes(uint64_t n, int nCU) { return wave_queue_entries(wave_layout(n, nCU)) * sizeof(uint64_t); }
WaveSlices wave_conflict_layout(uint64_t n, int nCU, void* boundsBuf)
{
    const WaveLayout w = wave_layout(n, nCU);
    return WaveSlices{(uint32_t)w.nChunks, (uint32_t)w.sliceLen, WaveScratch(nCU, boundsBuf).ccounts};
}

hipError_t launch_build_wave(const BuildJob& j, const WaveBufs& buf, Gate gate, int parts, int mode, KernelEvents kev)
{
    const bool htm = buf.htmConflicts != nullptr;
    const bool codes = mode == kWaveCodes;
    const bool compact = mode == kWaveCompact, planar = mode == kWavePlanar || codes;
    const SlotCode code = slot_code(j.tableSize, j.probeLen);
    if (codes && (j.key32 || j.hshift || code.dbits > kCodeBits)) return hipErrorInvalidValue;   // tuples under the identity hash
    if (codes && !wave_codes_supported(j.n, j.nCU, j.tableSize)) return hipErrorInvalidValue;    // the ring of words and its rule
    // (planar + bucketised is refused here: the dirty-log counts live in the conflict counts' words, WaveScratch::lcounts)
    if (htm && (j.key32 || j.probeLen != 3 || j.sc.mask || compact || planar)) return hipErrorInvalidValue;
    if (!j.key32 && j.hshift) return hipErrorInvalidValue;         // the kernel's tuple instances assume it
    const WaveLayout w = wave_layout(j.n, j.nCU);
    const uint32_t chunkLen = (uint32_t)w.chunkLen, sliceLen = (uint32_t)w.sliceLen, nChunks = (uint32_t)w.nChunks;
    const WaveScratch ws(j.nCU, buf.bounds);
    DeferredEntry* const queue = static_cast<DeferredEntry*>(buf.queue);
    const uint64_t mask = j.tableSize - 1;
    const uint32_t numGran = (uint32_t)(j.tableSize >> kGranShift);
    // workgroups a device of nCU compute units holds at once (the rotation of issue priorities goes by it)
    const uint32_t residentWG = kWvWavesPerCu * (uint32_t)(j.nCU > 0 ? j.nCU : 256) / (uint32_t)kWvWaves;
    const std::true_type yes{};
    const std::false_type no{};
    hipError_t e;
    const dim3 gRaw((nChunks + 1 + kBlock / 64 - 1) / (kBlock / 64)), gMain((nChunks + kWvWaves - 1) / kWvWaves);
    if (parts & kWavePre) {
        auto seams = [&](auto k32, auto htmTag) {
            hipLaunchKernelGGL((k_wave_seams<decltype(k32)::value, decltype(htmTag)::value>), gRaw, dim3(kBlock), 0, j.s, j.R, j.n, chunkLen,
                               nChunks, mask, j.hshift, ws.starts, ws.raw, gate);
        };
        // every instantiation there is: the bucketised table's hash on tuples; else the key format
        if (htm) seams(no, yes);
        else with_flag(j.key32, [&](auto k32) { seams(k32, no); });
        hipLaunchKernelGGL(k_wave_bounds_scan, dim3((nChunks + kBlock - 1) / kBlock), dim3(kBlock), 0, j.s, ws.raw, nChunks, numGran, ws.bounds, gate);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (parts & kWaveMain) {
        if (kev.before && (e = hipEventRecord(kev.before, j.s)) != hipSuccess) return e;
        auto build = [&](auto k32, auto chk, auto htmTag, auto cmp, auto pln, auto cds) {
            hipLaunchKernelGGL((k_build_wave<decltype(k32)::value, decltype(chk)::value, decltype(htmTag)::value, decltype(cmp)::value, decltype(pln)::value,
                                             decltype(cds)::value>),
                               gMain, dim3(kWvThreads), decltype(cds)::value ? kWvWordLdsBytes : kWvLdsBytes, j.s, j.R, j.n, sliceLen, nChunks, ws.starts, ws.bounds, j.table, mask,
                               j.hshift, j.probeLen, j.idxBase, j.sc, queue, ws.dcounts, j.ctr, gate, buf.htmConflicts, ws.ccounts,
                               residentWG, ws.pcounts, codes ? word_ring(code) : WordRing{});
        };
        // every instantiation there is: the bucketised table on tuples without a shard check; else key format x "counts
        // foreign tuples" for each of the three modes; the slot codes on tuples alone, with and without the count
        if (htm) build(no, no, yes, no, no, no);
        else if (codes) with_flag(j.sc.mask != 0, [&](auto chk) { build(no, chk, no, no, yes, yes); });
        else with_flag(j.key32, [&](auto k32) {
            with_flag(j.sc.mask != 0, [&](auto chk) {
                if (compact) build(k32, chk, no, yes, no, no);
                else if (planar) build(k32, chk, no, no, yes, no);
                else build(k32, chk, no, no, no, no);
            });
        });
        if (kev.after && (e = hipEventRecord(kev.after, j.s)) != hipSuccess) return e;
        if (compact) {
            // the seams check out or the classic build takes over (Counters::variant := 3)
            hipLaunchKernelGGL(k_wave_validate, dim3((nChunks + kBlock - 1) / kBlock), dim3(kBlock), 0, j.s,
                               static_cast<const DeferredEntry*>(queue), ws.dcounts, ws.pcounts, nChunks, sliceLen, j.ctr, gate);
            hipLaunchKernelGGL(k_wave_decide, dim3(1), dim3(64), 0, j.s, j.ctr, j.tableSize, 3u, gate);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (!(parts & kWaveTail)) return hipSuccess;
    uint32_t* const keys = reinterpret_cast<uint32_t*>(j.table);
    if (compact) {
        hipLaunchKernelGGL(k_wave_fill_edges<uint32_t>, dim3(512), dim3(kBlock), 0, j.s, keys, static_cast<uint32_t*>(nullptr), j.ctr, j.tableSize, gate);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_wave_finalize_range, dim3(1), dim3(64), 0, j.s, j.ctr, j.tableSize, gate);
    const dim3 gDef((nChunks + kBlock / 64 - 1) / (kBlock / 64));   // one wavefront per slice
    auto deferred = [&](auto htmTag, auto pln, uint32_t* ccounts, const uint32_t* route, PlanarWalk pw) {
        hipLaunchKernelGGL((k_wave_deferred<decltype(htmTag)::value, decltype(pln)::value>), gDef, dim3(kBlock), 0, j.s, queue, ws.dcounts,
                           nChunks, sliceLen, j.table, mask, j.hshift, j.probeLen, j.ctr, gate, buf.htmConflicts, ccounts, route, pw);
    };
    if (planar) {
        const PlanarWalk pw{j.R, j.key32, j.idxBase, ws.lcounts};
        // 1024 workgroups: the compact road's 512 for one plane of 4-byte words, doubled for two (4.9 us at 2^30, as the packed fill)
        if (codes)
            hipLaunchKernelGGL(k_wave_fill_edges<uint8_t>, dim3(1024), dim3(kBlock), 0, j.s, reinterpret_cast<uint8_t*>(j.table),
                               planar_index_plane(j.table, j.tableSize), j.ctr, j.tableSize, gate);
        else
        hipLaunchKernelGGL(k_wave_fill_edges<uint32_t>, dim3(1024), dim3(kBlock), 0, j.s, keys, planar_index_plane(j.table, j.tableSize),
                           j.ctr, j.tableSize, gate);
        deferred(no, yes, nullptr, nullptr, pw);
        hipLaunchKernelGGL(k_wave_fixup, gDef, dim3(kBlock), 0, j.s, queue, ws.dcounts, nChunks, sliceLen, j.table, j.tableSize, j.ctr, gate, pw,
                           codes, code);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_wave_fill_edges<uint64_t>, dim3(2048), dim3(kBlock), 0, j.s, j.table, static_cast<uint32_t*>(nullptr), j.ctr, j.tableSize, gate);
    if (htm) deferred(yes, no, ws.ccounts, buf.htmRoute ? ws.bounds : nullptr, PlanarWalk{});
    else deferred(no, no, nullptr, nullptr, PlanarWalk{});
    return hipGetLastError();
}

}  // namespace hj
