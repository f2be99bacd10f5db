// hj_keys.hip -- joins on real key columns for gfx950 (MI355X): hj_key_hash_dev and hj_pairs_verify_dev.
//
// The joins of this library match on one 32-bit word. A key of 64 bits, of several columns or of 16 bytes is joined as
// hash -> candidate join -> verify: k_key_hash turns the key columns of a row into a 32-bit join word (the header's
// MurmurHash3_x86_32, include/htm_hashjoin.h), the resident radix join produces the pairs that agree on that word, and
// k_pairs_verify compares the real key bytes of every candidate, keeps the equal ones and marks their S and R rows.
//
// k_key_hash. Shape: one workgroup of kBlock lanes per kHashBlockRows = 1024 consecutive rows; a wavefront owns 256 of
// them and a lane kHashLaneRows = 4, one per step of 64, so a wave-instruction reads 64 * width contiguous bytes of a
// column and stores 512 contiguous bytes of tuples. The hash runs over the columns in order, so the lane carries four
// running hashes through them column by column: the four loads of a column are issued straight, then its words are
// mixed. The width of a column is picked by a switch on a kernel argument (uniform: a scalar branch) rather than by a
// template parameter per column -- 5^4 width lists are too many to instantiate. The price, seen in the ISA: the wait
// counters cannot tell the arms of a switch apart, so a column's loads wait for those of the column before; inside an
// arm the four loads are in flight together, and the other wavefronts of the CU cover the rest (no LDS, 8 per SIMD).
// A row behind the end reads the last row instead of branching around its loads. Loads are nontemporal: every column is
// read once. key_hash_rows is ONE __host__ __device__ body: hj_key_hash_host runs it in a host loop, a row at a time.
// What it does NOT do: no atomics, no LDS, no validity plane (NULL keys are not a notion here yet).
//
// k_pairs_verify. Shape: one workgroup of kBlock lanes per kVerifyBlockPairs = 1024 consecutive candidates, so the LDS
// stage (PairStage, hj_device.h) is flushed exactly once; a wavefront owns 256 consecutive candidates and takes them as
// kVerifyLanePairs = 4 steps of 64, the map reads coalesced and nontemporal. A candidate with an HJ_NO_ROW entry, or with
// a row outside its relation, is dropped before anything is dereferenced. The keys are compared column by column: the S
// and the R element of the column for all four candidates of the lane -- eight element-granular random loads -- are in
// flight before the first compare; a candidate that an earlier column has rejected is read again and a dropped one reads
// a spare row, instead of branching around their loads (a branch would make every load wait for the one before it).
// (All columns at once would be 4 x 2 x 4 sixteen-byte cells per lane; by column it is 32 registers.)
// The kept count is agreed on by stage_reserve (wavefront scan + LDS totals, one barrier), the kept pairs are staged,
// the run is claimed with one atomicAdd on the 64-bit cursor and leaves through flush_plane (stage_flush). The marks
// of both sides are set from the stage: neighbouring lanes hold neighbouring pairs, and a pair the capacity cuts marks
// like any other (mark_r_row: a relaxed load first, the OR only while the bit reads clear).
// What it does NOT do: the candidates are taken in the order the radix join left them, which is by partition; the S side
// is near-sequential only if that order happens to be, and the R side is a random element read per column.

#include "hj_device.h"

namespace hj {

namespace {

// ---- the hash -------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// one 32-bit word into the running hash (MurmurHash3_x86_32's block step)
__host__ __device__ __forceinline__ uint32_t mm3_mix(uint32_t h, uint32_t k)
{
    k *= 0xcc9e2d51u; k = rotl32(k, 15); k *= 0x1b873593u;
    h ^= k; h = rotl32(h, 13);
    return h * 5u + 0xe6546b64u;
}

__host__ __device__ __forceinline__ uint32_t mm3_final(uint32_t h, uint32_t len)
{
    h ^= len;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

// one element of W bytes as the kernels load it
template <int W> struct KeyElemOf { typedef uint32_t type; };
template <> struct KeyElemOf<1> { typedef uint8_t type; };
template <> struct KeyElemOf<2> { typedef uint16_t type; };
template <> struct KeyElemOf<8> { typedef uint64_t type; };
template <> struct KeyElemOf<16> { typedef u4 type; };
template <int W> using KeyElem = typename KeyElemOf<W>::type;

// the words of one element into the running hash: width 1 and 2 zero-extended to one word, the others their
// little-endian words in order
__host__ __device__ __forceinline__ uint32_t mm3_mix_elem(uint32_t h, uint8_t v) { return mm3_mix(h, v); }
__host__ __device__ __forceinline__ uint32_t mm3_mix_elem(uint32_t h, uint16_t v) { return mm3_mix(h, v); }
__host__ __device__ __forceinline__ uint32_t mm3_mix_elem(uint32_t h, uint32_t v) { return mm3_mix(h, v); }
__host__ __device__ __forceinline__ uint32_t mm3_mix_elem(uint32_t h, uint64_t v) { return mm3_mix(mm3_mix(h, (uint32_t)v), (uint32_t)(v >> 32)); }
__host__ __device__ __forceinline__ uint32_t mm3_mix_elem(uint32_t h, const u4& v) { return mm3_mix(mm3_mix(mm3_mix(mm3_mix(h, v.x), v.y), v.z), v.w); }

// One key column of K rows into their running hashes: the K loads first, straight, then the words.
template <int W, int K>
__host__ __device__ __forceinline__ void key_mix_col(const void* col, const uint64_t (&row)[K], uint32_t (&h)[K])
{
    KeyElem<W> v[K];
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = __builtin_nontemporal_load(static_cast<const KeyElem<W>*>(col) + row[j]);
#ifdef __HIP_DEVICE_COMPILE__
    __builtin_amdgcn_sched_barrier(0);                                // no mix moves up between the loads: it would wait there
#endif
#pragma unroll
    for (int j = 0; j < K; ++j) h[j] = mm3_mix_elem(h[j], v[j]);
}

// The join words of K rows: column by column, the width picked by a switch that is uniform on the device.
template <int K>
__host__ __device__ __forceinline__ void key_hash_rows(const KeyCols& cols, uint32_t nCols, const uint64_t (&row)[K], uint32_t mask,
                                                       uint32_t (&word)[K])
{
    uint32_t h[K], words = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) h[j] = 0;
#pragma unroll
    for (uint32_t c = 0; c < kKeyMaxCols; ++c) {
        if (c >= nCols) continue;
        switch (cols.width[c]) {
            case 1: key_mix_col<1, K>(cols.p[c], row, h); break;
            case 2: key_mix_col<2, K>(cols.p[c], row, h); break;
            case 4: key_mix_col<4, K>(cols.p[c], row, h); break;
            case 8: key_mix_col<8, K>(cols.p[c], row, h); break;
            default: key_mix_col<16, K>(cols.p[c], row, h); break;
        }
        words += cols.width[c] <= 4 ? 1u : cols.width[c] / 4u;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) word[j] = mm3_final(h[j], 4u * words) & mask;
}

constexpr uint32_t kHashLaneRows = 4;                                 // rows per lane, kWave apart: a wavefront owns 256 consecutive rows
constexpr uint32_t kHashBlockRows = kHashLaneRows * kBlock;           // 1024

// ---- the verify step ------------------------------------------------------------------------------------------------
constexpr uint32_t kVerifyStepPairs = kWave;
constexpr uint32_t kVerifyLanePairs = 4;                              // candidates in flight per lane, kVerifyStepPairs apart
constexpr uint32_t kVerifyWavePairs = kVerifyStepPairs * kVerifyLanePairs;
constexpr uint32_t kVerifyWaves = kBlock / kWave;
constexpr uint32_t kVerifyBlockPairs = kVerifyWavePairs * kVerifyWaves;      // 1024
static_assert(kVerifyBlockPairs <= kStagePairs, "a workgroup's candidates fit one stage: it is flushed exactly once");

template <class E> __device__ __forceinline__ bool same_bytes(const E& a, const E& b) { return a == b; }
template <> __device__ __forceinline__ bool same_bytes<u4>(const u4& a, const u4& b)
{
    return (((a.x ^ b.x) | (a.y ^ b.y)) | ((a.z ^ b.z) | (a.w ^ b.w))) == 0u;
}

// One key column of the lane's candidates: both elements of every candidate, all eight loads before the first compare.
// The loads are unconditional -- a load under a per-lane condition is a branch around it, and the wait counters in front
// of the next one would then wait for it. So a candidate that an earlier column has rejected is read again, and a
// dropped one (its caller's doing) reads a row that exists.
template <int W>
__device__ __forceinline__ void verify_col(const void* sCol, const void* rCol, const uint32_t (&si)[kVerifyLanePairs],
                                           const uint32_t (&ri)[kVerifyLanePairs], bool (&live)[kVerifyLanePairs])
{
    using E = KeyElem<W>;
    E a[kVerifyLanePairs], b[kVerifyLanePairs];
#pragma unroll
    for (uint32_t j = 0; j < kVerifyLanePairs; ++j) { a[j] = static_cast<const E*>(sCol)[si[j]]; b[j] = static_cast<const E*>(rCol)[ri[j]]; }
    __builtin_amdgcn_sched_barrier(0);                                // no compare moves up between the loads: it would wait there
#pragma unroll
    for (uint32_t j = 0; j < kVerifyLanePairs; ++j) live[j] = live[j] && same_bytes<E>(a[j], b[j]);
}

}  // namespace

__global__ void __launch_bounds__(kBlock)
k_key_hash(KeyCols cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint64_t* __restrict__ out)
{
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * kHashBlockRows + w * (kHashLaneRows * kWave) + lane;     // the lane's first row
    uint64_t row[kHashLaneRows];
    uint32_t word[kHashLaneRows];
#pragma unroll
    for (uint32_t j = 0; j < kHashLaneRows; ++j) {
        const uint64_t i = i0 + j * kWave;
        row[j] = i < nRows ? i : nRows - 1;                           // a row behind the end reads the last one and stores nothing
    }
    key_hash_rows<(int)kHashLaneRows>(cols, nCols, row, mask, word);
#pragma unroll
    for (uint32_t j = 0; j < kHashLaneRows; ++j)
        if (i0 + j * kWave < nRows) out[i0 + j * kWave] = (uint64_t)word[j];
}

// out: the planes, their capacity and the cursor (cursor[0]: kept pairs; cursor[1]: dropped candidates); out.marks: R's
// plane. sMarks: S's plane, its base the sRowBase of the maps. A plane that is not wanted has rows = 0 and marks nothing.
__global__ void __launch_bounds__(kBlock)
k_pairs_verify(const uint32_t* __restrict__ mapS, const uint32_t* __restrict__ mapR, uint64_t nPairs, uint32_t sRowBase, uint32_t sRows,
               uint32_t rRows, KeyColsSR cols, uint32_t nCols, PairsOutMarked out, RMarks sMarks)
{
    __shared__ uint32_t ldsS[kVerifyBlockPairs], ldsR[kVerifyBlockPairs], ldsTot[2 * kVerifyWaves], ldsDrop[kVerifyWaves];
    __shared__ unsigned long long ldsBase;
    PairStage<kBlock> st{ldsS, ldsR, ldsTot, &ldsBase, 0u, 0u, 0ull, 0ull, 0u};
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const uint64_t k0 = (uint64_t)blockIdx.x * kVerifyBlockPairs + w * kVerifyWavePairs + lane;   // the lane's first candidate

    // the map entries of the lane's four candidates, all in flight before the first is looked at
    uint32_t es[kVerifyLanePairs], er[kVerifyLanePairs];
#pragma unroll
    for (uint32_t j = 0; j < kVerifyLanePairs; ++j) {
        const uint64_t k = k0 + j * kVerifyStepPairs;
        es[j] = er[j] = kNoRow;
        if (k < nPairs) { es[j] = __builtin_nontemporal_load(mapS + k); er[j] = __builtin_nontemporal_load(mapR + k); }
    }

    uint32_t si[kVerifyLanePairs], ri[kVerifyLanePairs];
    bool live[kVerifyLanePairs];
    uint32_t nDrop = 0;                                               // of this wavefront (ballots: the same in every lane)
#pragma unroll
    for (uint32_t j = 0; j < kVerifyLanePairs; ++j) {
        const bool in = k0 + j * kVerifyStepPairs < nPairs;
        si[j] = es[j] - sRowBase; ri[j] = er[j];
        live[j] = in && es[j] != kNoRow && er[j] != kNoRow && si[j] < sRows && ri[j] < rRows;     // the raw entries: whatever the base
        nDrop += (uint32_t)__popcll(__ballot(in && !live[j]));
    }
    if (lane == 0) ldsDrop[w] = nDrop;                                // read behind stage_reserve's barrier

    // sRows or rRows 0: every candidate is dropped, and there is no row to read
    if (sRows && rRows) {
        // a dropped candidate reads, and ignores, one of the first rows: neighbouring lanes neighbouring rows, not all one address
        const uint32_t spareS = threadIdx.x < sRows ? threadIdx.x : sRows - 1u, spareR = threadIdx.x < rRows ? threadIdx.x : rRows - 1u;
#pragma unroll
        for (uint32_t j = 0; j < kVerifyLanePairs; ++j) { si[j] = live[j] ? si[j] : spareS; ri[j] = live[j] ? ri[j] : spareR; }
#pragma unroll
        for (uint32_t c = 0; c < kKeyMaxCols; ++c) {
            if (c >= nCols) continue;                                 // kernel arguments: uniform
            switch (cols.width[c]) {
                case 1: verify_col<1>(cols.s[c], cols.r[c], si, ri, live); break;
                case 2: verify_col<2>(cols.s[c], cols.r[c], si, ri, live); break;
                case 4: verify_col<4>(cols.s[c], cols.r[c], si, ri, live); break;
                case 8: verify_col<8>(cols.s[c], cols.r[c], si, ri, live); break;
                default: verify_col<16>(cols.s[c], cols.r[c], si, ri, live); break;
            }
        }
    }

    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < kVerifyLanePairs; ++j) m += (uint32_t)live[j];
    bool any;
    uint32_t pos = stage_reserve<kInner>(st, out, m, false, any);     // never flushes: the stage was empty and takes every candidate
#pragma unroll
    for (uint32_t j = 0; j < kVerifyLanePairs; ++j)
        if (live[j]) { st.s[pos] = es[j]; st.r[pos] = er[j]; ++pos; }
    if (threadIdx.x == 0) {
        uint32_t d = 0;
#pragma unroll
        for (uint32_t i = 0; i < kVerifyWaves; ++i) d += ldsDrop[i];
        if (d) atomicAdd(out.cursor + 1, (unsigned long long)d);
    }
    const uint32_t kept = st.fill;                                    // the same in every thread
    if (kept == 0) return;                                            // workgroup-uniform
    stage_flush<kInner>(st, out);                                     // the claim, both planes, R's marks
    mark_plane<kBlock>(st.s, kept, sMarks);                           // the stage is still as it was flushed
}

hipError_t launch_key_hash(const KeyCols& cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint64_t* out, hipStream_t s)
{
    if (nRows == 0) return hipSuccess;
    const dim3 grid((uint32_t)((nRows + kHashBlockRows - 1) / kHashBlockRows));               // nRows <= 2^32 - 1: <= 2^22 workgroups
    hipLaunchKernelGGL(k_key_hash, grid, dim3(kBlock), 0, s, cols, nCols, nRows, mask, out);
    return hipGetLastError();
}

void key_hash_host(const KeyCols& cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint64_t* out)
{
    for (uint64_t i = 0; i < nRows; ++i) {
        const uint64_t row[1] = {i};
        uint32_t word[1];
        key_hash_rows<1>(cols, nCols, row, mask, word);
        out[i] = (uint64_t)word[0];
    }
}

hipError_t launch_pairs_verify(const uint32_t* mapS, const uint32_t* mapR, uint64_t nPairs, uint32_t sRowBase, uint32_t sRows,
                               uint32_t rRows, const KeyColsSR& cols, uint32_t nCols, PairsOut out, uint32_t* sMarks, uint32_t* rMarks,
                               hipStream_t s)
{
    if (nPairs == 0) return hipSuccess;
    const RMarks mkS{sMarks, sRowBase, sMarks ? sRows : 0u}, mkR{rMarks, 0u, rMarks ? rRows : 0u};
    const PairsOutMarked o = pairs_out_of<true>(out, &mkR);
    const dim3 grid((uint32_t)((nPairs + kVerifyBlockPairs - 1) / kVerifyBlockPairs));        // nPairs <= 2^32 - 1: <= 2^22 workgroups
    hipLaunchKernelGGL(k_pairs_verify, grid, dim3(kBlock), 0, s, mapS, mapR, nPairs, sRowBase, sRows, rRows, cols, nCols, o, mkS);
    return hipGetLastError();
}

}  // namespace hj
