// hj_gather.hip -- payload columns through the join's row maps for gfx950 (MI355X): hj_gather_dev, and behind it hj_gather2_dev.
//
// Every materialising call of the library ends in uint32 gather maps (hj_probe_join_dev, hj_prj_probe_join_dev,
// hj_r_rows_dev). k_gather takes one such map and up to kGatherMaxCols columns and writes, for output row k with
// e = map[k]:
//   e == HJ_NO_ROW (the raw entry, before the base is taken off)   a NULL row: every column gets its fill, validity bit 0
//   i = e - rowBase (unsigned) >= srcRows                          out of range: never dereferenced, handled like a NULL
//                                                                  row, counted apart
//   otherwise                                                      dst_c[k] = src_c[i] for every column c, validity bit 1
//
// Shape. One workgroup of kBlock lanes per kGatherBlockRows = 1024 consecutive rows, so the seams lie at known row numbers.
// A wavefront owns 256 consecutive rows and takes them as kGatherLaneRows = 4 steps of kGatherStepRows = 64: a
// wave-instruction reads 256 contiguous bytes of the map and stores 64 * width contiguous bytes of a column. The loads of
// ALL columns for a lane's four rows are issued before the first store (v[][], registers): the source reads are
// element-granular and random by nature, and loads in flight are the only lever there is. A row without a source row
// issues no load: its cell keeps the fill it started with. A 16-byte element moves as one 16-byte load and one store.
// Instantiations: the element width (1, 2, 4, 8, 16) x the columns there are registers for (1, 2, 4, 8), so that one
// 4-byte column does not pay for eight 16-byte ones and no load is picked by a switch at run time (the compiler's wait
// counters cannot tell the arms of one apart and would make each load wait for the one before). A call whose columns
// differ in width is one launch per width present, widest first, over the same map; the first launch writes the validity
// plane and counts, the others get neither.
// Output stores are nontemporal: the output is not read again here, and the source lines are what should stay in L2.
// Validity plane (Arrow layout: bit k & 31 of word k >> 5, 1 = valid): __ballot over a step gives two whole words, which
// lane 0 stores as 8 bytes (as two words when the plane is only 4-byte aligned); bits at or behind nRows are 0, words at
// or behind ceil(nRows / 32) are not written; no atomics. NULL and out-of-range rows are counted per wavefront with
// popcounts of the ballots, and a workgroup adds them to the two device counters once.
//
// k_gather's map prologue, plane store and count epilogue are a WRITTEN-OUT COPY of take_rows / store_plane_step / add_counts,
// which its three siblings further down call (a change to one is made in both). Put on the helpers, the twenty k_gather
// instances compile to other code (mostly three VGPRs fewer; k_gather<16, 8> 137 VGPRs for 136 and two spilled SGPRs; no
// scratch, no wavefront lost), and measured parent, change, parent, change at 2^27 rows the medians of three of the
// thirty-six configurations lay above the parent's slowest single launch -- s_sorted, one 16-byte column, in both runs:
// 832 and 821 us against 819 us (profiles/gather.md, "k_gather on the shared helpers"). So the text stays.
//
// What it does NOT do: the map is neither sorted nor bucketed before the gather. A random map (the R side of a join on a
// shuffled R) therefore fetches one cache line per element -- the amplification the counting probe shows under a
// scattered S -- and nothing here hides it.

#include "hj_columns.h"

#include <utility>

namespace hj {

namespace {

constexpr uint32_t kGatherStepRows = kWave;                           // rows of one wavefront step: two validity words
constexpr uint32_t kGatherLaneRows = 4;                               // rows in flight per lane, kGatherStepRows apart
constexpr uint32_t kGatherWaveRows = kGatherStepRows * kGatherLaneRows;
constexpr uint32_t kGatherWaves = kBlock / kWave;
constexpr uint32_t kGatherBlockRows = kGatherWaveRows * kGatherWaves; // 1024

// One element of W bytes in registers: 32-bit words, two (W up to 8) or four (W = 16), as ONE vector. It starts as the
// column's fill, before the column's loads are issued, and a load replaces the words W fills: the store then takes the
// vector as it is. Nothing but its store may follow a load -- no zero extension, no select against the fill -- because
// such an instruction would wait for it.
template <int W> struct CellOf { typedef uint2 type; };
template <> struct CellOf<16> { typedef u4 type; };
template <int W> using Cell = typename CellOf<W>::type;
__device__ __forceinline__ void fill_cell(uint2& c, const GatherCol& col) { c.x = (uint32_t)col.fill[0]; c.y = (uint32_t)(col.fill[0] >> 32); }
__device__ __forceinline__ void fill_cell(u4& c, const GatherCol& col)
{
    c.x = (uint32_t)col.fill[0]; c.y = (uint32_t)(col.fill[0] >> 32); c.z = (uint32_t)col.fill[1]; c.w = (uint32_t)(col.fill[1] >> 32);
}

// The rows of a lane are written out as packs (J...) and the columns as a recursion (C), not as loops: every index into
// v[][] is a constant from the start, and v[][] is registers whatever the optimiser does first.
using GatherRows = std::make_integer_sequence<uint32_t, kGatherLaneRows>;

// one element out of a column, into the words of the cell that W fills
template <int W>
__device__ __forceinline__ void load_row(Cell<W>& c, const void* src, uint32_t i)
{
    if constexpr (W == 1) c.x = static_cast<const uint8_t*>(src)[i];
    else if constexpr (W == 2) c.x = static_cast<const uint16_t*>(src)[i];
    else if constexpr (W == 4) c.x = static_cast<const uint32_t*>(src)[i];
    else if constexpr (W == 8) { const uint2 t = static_cast<const uint2*>(src)[i]; c.x = t.x; c.y = t.y; }
    else c = static_cast<const u4*>(src)[i];
}

// ... and into a column's output: row k if it is below nRows
template <int W>
__device__ __forceinline__ void store_row(const Cell<W>& c, void* dst, uint64_t k, uint64_t nRows)
{
    if (k >= nRows) return;
    if constexpr (W == 1) __builtin_nontemporal_store((uint8_t)c.x, static_cast<uint8_t*>(dst) + k);
    else if constexpr (W == 2) __builtin_nontemporal_store((uint16_t)c.x, static_cast<uint16_t*>(dst) + k);
    else if constexpr (W == 4) __builtin_nontemporal_store(c.x, static_cast<uint32_t*>(dst) + k);
    else if constexpr (W == 8) __builtin_nontemporal_store((uint64_t)c.x | ((uint64_t)c.y << 32), static_cast<uint64_t*>(dst) + k);
    else __builtin_nontemporal_store(c, static_cast<u4*>(dst) + k);
}

// The rows of a lane out of one column: the fill, then the loads for the rows that have a source row -- the entry of any
// other row (NULL, out of range, behind nRows) is never dereferenced.
template <int W, uint32_t... J>
__device__ __forceinline__ void load_rows(Cell<W> (&v)[kGatherLaneRows], const GatherCol& col, const uint32_t (&idx)[kGatherLaneRows],
                                          const bool (&ok)[kGatherLaneRows], std::integer_sequence<uint32_t, J...>)
{
    (fill_cell(v[J], col), ...);
    ((ok[J] ? load_row<W>(v[J], col.src, idx[J]) : (void)0), ...);
}

template <int W, int NC, int C = 0>
__device__ __forceinline__ void load_cols(Cell<W> (&v)[NC][kGatherLaneRows], const GatherCols& cols, uint32_t nCols,
                                          const uint32_t (&idx)[kGatherLaneRows], const bool (&ok)[kGatherLaneRows])
{
    if constexpr (C < NC) {
        if ((uint32_t)C < nCols) load_rows<W>(v[C], cols.col[C], idx, ok, GatherRows{});
        load_cols<W, NC, C + 1>(v, cols, nCols, idx, ok);
    }
}

// the rows k0 + J * kGatherStepRows of every column
template <int W, uint32_t... J>
__device__ __forceinline__ void store_rows(const Cell<W> (&v)[kGatherLaneRows], void* dst, uint64_t k0, uint64_t nRows,
                                           std::integer_sequence<uint32_t, J...>)
{
    (store_row<W>(v[J], dst, k0 + J * kGatherStepRows, nRows), ...);
}

template <int W, int NC, int C = 0>
__device__ __forceinline__ void store_cols(const Cell<W> (&v)[NC][kGatherLaneRows], const GatherCols& cols, uint32_t nCols, uint64_t k0,
                                           uint64_t nRows)
{
    if constexpr (C < NC) {
        if ((uint32_t)C < nCols) store_rows<W>(v[C], cols.col[C].dst, k0, nRows, GatherRows{});
        store_cols<W, NC, C + 1>(v, cols, nCols, k0, nRows);
    }
}

}  // namespace

// W: the width of every column of the launch; NC: columns the instantiation has registers for (nCols <= NC). valid and
// counts may be null (the launches of a call behind its first): counts[0] += NULL rows, counts[1] += out-of-range entries.
template <int W, int NC>
__global__ void __launch_bounds__(kBlock)
k_gather(const uint32_t* __restrict__ map, uint64_t nRows, uint32_t rowBase, uint64_t srcRows, GatherCols cols, uint32_t nCols,
         uint32_t* __restrict__ valid, unsigned long long* __restrict__ counts)
{
    __shared__ uint32_t wNull[kGatherWaves], wOor[kGatherWaves];
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const uint64_t row0 = (uint64_t)blockIdx.x * kGatherBlockRows + w * kGatherWaveRows;     // of this wavefront
    const uint64_t k0 = row0 + lane;                                  // the lane's first row; the others kGatherStepRows apart
    const bool valid8 = (reinterpret_cast<uintptr_t>(valid) & 7u) == 0;

    // the four map entries of the lane, all in flight before the first is looked at
    uint32_t e[kGatherLaneRows];
#pragma unroll
    for (uint32_t j = 0; j < kGatherLaneRows; ++j) {
        e[j] = kNoRow;
        if (k0 + j * kGatherStepRows < nRows) e[j] = __builtin_nontemporal_load(map + k0 + j * kGatherStepRows);
    }

    uint32_t idx[kGatherLaneRows];
    bool ok[kGatherLaneRows];
    uint32_t nNull = 0, nOor = 0;                                     // of this wavefront (ballots: the same in every lane)
#pragma unroll
    for (uint32_t j = 0; j < kGatherLaneRows; ++j) {
        const uint64_t first = row0 + j * kGatherStepRows;            // of the step
        const bool in = first + lane < nRows;
        const bool null = e[j] == kNoRow;                             // the raw entry: whatever the base
        idx[j] = e[j] - rowBase;
        const bool oor = !null && (uint64_t)idx[j] >= srcRows;
        ok[j] = !null && !oor;
        const unsigned long long bits = __ballot(ok[j]);
        nNull += (uint32_t)__popcll(__ballot(in && null));
        nOor += (uint32_t)__popcll(__ballot(oor));
        if (valid && lane == 0 && first < nRows) {
            uint32_t* const word = valid + (first >> 5);
            const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
            if (first + 32 >= nRows) word[0] = lo;                    // the plane ends with this word
            else if (valid8) *reinterpret_cast<uint2*>(word) = make_uint2(lo, hi);
            else { word[0] = lo; word[1] = hi; }
        }
    }

    // every load of the lane's rows, all columns, before the first store
    Cell<W> v[NC][kGatherLaneRows];
    load_cols<W, NC>(v, cols, nCols, idx, ok);
    store_cols<W, NC>(v, cols, nCols, k0, nRows);

    if (!counts) return;                                              // kernel argument: uniform
    if (lane == 0) { wNull[w] = nNull; wOor[w] = nOor; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0;
#pragma unroll
        for (uint32_t i = 0; i < kGatherWaves; ++i) { a += wNull[i]; b += wOor[i]; }
        if (a) atomicAdd(counts, (unsigned long long)a);
        if (b) atomicAdd(counts + 1, (unsigned long long)b);
    }
}

namespace {

template <int W>
void launch_gather_width(dim3 grid, hipStream_t s, const uint32_t* map, uint64_t nRows, uint32_t rowBase, uint64_t srcRows,
                         const GatherCols& cols, uint32_t nCols, uint32_t* valid, unsigned long long* counts)
{
    if (nCols <= 1) hipLaunchKernelGGL((k_gather<W, 1>), grid, dim3(kBlock), 0, s, map, nRows, rowBase, srcRows, cols, nCols, valid, counts);
    else if (nCols <= 2) hipLaunchKernelGGL((k_gather<W, 2>), grid, dim3(kBlock), 0, s, map, nRows, rowBase, srcRows, cols, nCols, valid, counts);
    else if (nCols <= 4) hipLaunchKernelGGL((k_gather<W, 4>), grid, dim3(kBlock), 0, s, map, nRows, rowBase, srcRows, cols, nCols, valid, counts);
    else hipLaunchKernelGGL((k_gather<W, 8>), grid, dim3(kBlock), 0, s, map, nRows, rowBase, srcRows, cols, nCols, valid, counts);
}

}  // namespace

hipError_t launch_gather(const uint32_t* map, uint64_t nRows, uint32_t rowBase, uint64_t srcRows, const GatherCols& cols, uint32_t nCols,
                         uint32_t* valid, unsigned long long* counts, hipStream_t s)
{
    if (nRows == 0) return hipSuccess;
    const dim3 grid((uint32_t)((nRows + kGatherBlockRows - 1) / kGatherBlockRows));          // nRows <= 2^32 - 1: <= 2^22 workgroups
    // one launch per width among the columns, widest first; the first one also writes the validity plane and counts
    bool first = true;
    for (const uint32_t width : {16u, 8u, 4u, 2u, 1u}) {
        GatherCols part{};
        uint32_t n = 0;
        for (uint32_t c = 0; c < nCols; ++c)
            if (cols.col[c].width == width) part.col[n++] = cols.col[c];
        if (n == 0 && !(width == 1 && first)) continue;               // no column at all: the plane and the counts alone
        uint32_t* const v = first ? valid : nullptr;
        unsigned long long* const k = first ? counts : nullptr;
        switch (width) {
            case 16: launch_gather_width<16>(grid, s, map, nRows, rowBase, srcRows, part, n, v, k); break;
            case 8: launch_gather_width<8>(grid, s, map, nRows, rowBase, srcRows, part, n, v, k); break;
            case 4: launch_gather_width<4>(grid, s, map, nRows, rowBase, srcRows, part, n, v, k); break;
            case 2: launch_gather_width<2>(grid, s, map, nRows, rowBase, srcRows, part, n, v, k); break;
            default: launch_gather_width<1>(grid, s, map, nRows, rowBase, srcRows, part, n, v, k); break;
        }
        first = false;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// hj_gather2_dev: columns in the Arrow layout -- a source validity plane and 32-bit offsets per column, both optional.
//
// A column that is fixed and has neither plane is k_gather's, unchanged (launch_gather2 hands those to launch_gather).
// The others are siblings of k_gather with its row-to-lane layout and seams -- steps of 64 rows, 256 rows per wavefront,
// 1024 per workgroup -- one column per launch, so that the plain instances stay as narrow as they are:
//   k_gather_nullable<W>  a fixed column with srcValid and / or dstValid: per row the validity word of the element, loaded
//                         before the element and only for a row that has a source row; the element load is predicated on
//                         the bit, so a NULL element fetches no line; dstValid from __ballot over a step, like dValid
//   k_gather_lengths      variable length, step 1: the length of row k (offsets[i + 1] - offsets[i] of a valid element,
//                         else 0) to dstOffsets[k], a zero word behind the last row, dstValid, and the 64-bit sum of the
//                         workgroup's lengths to partials[workgroup] -- a plain store, no atomic
//   k_gather_total        one workgroup adds the partials up: the column's total, exact in 64 bits
//   (exclusive scan)      launch_exclusive_scan_u32 over the nRows + 1 words in place (the idiom of launch_r_sweep)
//   k_gather_copy         step 3, below
// The first launch of a call also writes the call-level plane and the two counts, as the first launch of launch_gather
// does.
//
// k_gather_copy is driven by the OUTPUT, not by the rows. A workgroup owns the contiguous output range of its 1024 rows,
// [dstOffsets[row0], dstOffsets[row0 + 1024]), cut at dstCapacity, and holds the 1025 offsets and the 1024 source starts
// in LDS (8 KiB: many workgroups per CU). It walks the range in passes of kCopyPassBytes = 256 lanes x 16 bytes: a lane
// owns one 16-byte block of the destination (aligned in the address space, whatever dst is), finds the row its first byte
// belongs to by a binary search in the LDS offsets, and assembles the block from the rows that cross it -- for each, the
// five aligned source words around its bytes, brought to the block's alignment by one funnel shift per word
// (v_alignbyte: the shift is the same for the whole segment, whichever of the 16 source / destination alignment pairs it
// is) and masked to the segment's bytes. The block leaves as ONE 16-byte nontemporal store, consecutive lanes storing
// consecutive blocks; only the first and the last block of the workgroup's range, which it shares with its neighbours or
// with the cut, go out bytewise. So the stores are coalesced by construction, an element longer than a block is copied by
// as many lanes as it has blocks, one longer than a pass by the whole workgroup in several, and no lane ever loops over
// an element: there is no threshold between a lane's copy and a cooperative one, and no LDS tile to overflow.
// What it costs: ~10 dependent LDS reads per block for the search, 4-byte source loads (five per segment, consecutive
// lanes reading consecutive words when the map ascends), and a lane walks the EMPTY rows that lie inside its block one
// by one (two LDS reads each; the leading ones are skipped by the search).
// A column whose total is above 2^32 - 1 has offsets that wrapped: the kernel reads the total first and returns.

namespace {

constexpr uint32_t kCopyBlockBytes = 16;                              // one lane's store
constexpr uint32_t kCopyPassBytes = kBlock * kCopyBlockBytes;         // one pass of a workgroup: 4096 bytes

// The four map entries of a lane as k_gather takes them: idx / ok per row, the call-level plane (may be null) written from
// the ballots, the wavefront's NULL and out-of-range rows counted.
__device__ __forceinline__ void store_plane_step(uint32_t* __restrict__ plane, uint64_t first, uint64_t nRows, unsigned long long bits, uint32_t lane)
{
    if (lane != 0 || first >= nRows) return;
    uint32_t* const word = plane + (first >> 5);
    const uint32_t lo = (uint32_t)bits, hi = (uint32_t)(bits >> 32);
    if (first + 32 >= nRows) word[0] = lo;                            // the plane ends with this word
    else if ((reinterpret_cast<uintptr_t>(word) & 7u) == 0) *reinterpret_cast<uint2*>(word) = make_uint2(lo, hi);
    else { word[0] = lo; word[1] = hi; }
}

__device__ __forceinline__ void take_rows(const uint32_t* __restrict__ map, uint64_t nRows, uint32_t rowBase, uint64_t srcRows, uint64_t row0,
                                          uint32_t lane, uint32_t* __restrict__ valid, uint32_t (&idx)[kGatherLaneRows],
                                          bool (&ok)[kGatherLaneRows], uint32_t& nNull, uint32_t& nOor)
{
    uint32_t e[kGatherLaneRows];
#pragma unroll
    for (uint32_t j = 0; j < kGatherLaneRows; ++j) {
        e[j] = kNoRow;
        if (row0 + lane + j * kGatherStepRows < nRows) e[j] = __builtin_nontemporal_load(map + row0 + lane + j * kGatherStepRows);
    }
    nNull = nOor = 0;
#pragma unroll
    for (uint32_t j = 0; j < kGatherLaneRows; ++j) {
        const uint64_t first = row0 + j * kGatherStepRows;
        const bool in = first + lane < nRows;
        const bool null = e[j] == kNoRow;                             // the raw entry: whatever the base
        idx[j] = e[j] - rowBase;
        const bool oor = !null && (uint64_t)idx[j] >= srcRows;
        ok[j] = !null && !oor;
        const unsigned long long bits = __ballot(ok[j]);
        nNull += (uint32_t)__popcll(__ballot(in && null));
        nOor += (uint32_t)__popcll(__ballot(oor));
        if (valid) store_plane_step(valid, first, nRows, bits, lane);
    }
}

// el[j]: row j has a source row and its element is valid. The validity words of the four rows are in flight together; a
// row without a source row loads none.
__device__ __forceinline__ void element_bits(const uint32_t* __restrict__ srcValid, const uint32_t (&idx)[kGatherLaneRows],
                                             const bool (&ok)[kGatherLaneRows], bool (&el)[kGatherLaneRows])
{
    uint32_t word[kGatherLaneRows];
#pragma unroll
    for (uint32_t j = 0; j < kGatherLaneRows; ++j) {
        word[j] = 0xFFFFFFFFu;
        if (srcValid && ok[j]) word[j] = srcValid[idx[j] >> 5];
    }
#pragma unroll
    for (uint32_t j = 0; j < kGatherLaneRows; ++j) el[j] = ok[j] && word_bit(word[j], idx[j]);
}

// the wavefronts' NULL and out-of-range rows -> the two device counters, once per workgroup (k_gather's epilogue)
__device__ __forceinline__ void add_counts(unsigned long long* __restrict__ counts, uint32_t* wNull, uint32_t* wOor, uint32_t nNull, uint32_t nOor)
{
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    if (lane == 0) { wNull[w] = nNull; wOor[w] = nOor; }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t a = 0, b = 0;
#pragma unroll
        for (uint32_t i = 0; i < kGatherWaves; ++i) { a += wNull[i]; b += wOor[i]; }
        if (a) atomicAdd(counts, (unsigned long long)a);
        if (b) atomicAdd(counts + 1, (unsigned long long)b);
    }
}

// bytes [lo, hi) of a 32-bit word, 0 <= lo, hi <= 4 (hi <= lo: none)
__device__ __forceinline__ uint32_t byte_mask(uint32_t lo, uint32_t hi)
{
    return hi > lo ? (uint32_t)(((1ull << (8u * hi)) - 1ull) & ~((1ull << (8u * lo)) - 1ull)) : 0u;
}

}  // namespace

template <int W>
__global__ void __launch_bounds__(kBlock)
k_gather_nullable(const uint32_t* __restrict__ map, uint64_t nRows, uint32_t rowBase, uint64_t srcRows, GatherCol2 col,
                  uint32_t* __restrict__ valid, unsigned long long* __restrict__ counts)
{
    __shared__ uint32_t wNull[kGatherWaves], wOor[kGatherWaves];
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const uint64_t row0 = (uint64_t)blockIdx.x * kGatherBlockRows + w * kGatherWaveRows;
    uint32_t idx[kGatherLaneRows], nNull, nOor;
    bool ok[kGatherLaneRows], el[kGatherLaneRows];
    take_rows(map, nRows, rowBase, srcRows, row0, lane, valid, idx, ok, nNull, nOor);
    element_bits(col.srcValid, idx, ok, el);
    if (col.dstValid) {                                               // kernel argument: uniform
#pragma unroll
        for (uint32_t j = 0; j < kGatherLaneRows; ++j) {
            const unsigned long long bits = __ballot(el[j]);
            store_plane_step(col.dstValid, row0 + j * kGatherStepRows, nRows, bits, lane);
        }
    }
    const GatherCol plain{col.src, col.dst, col.width, 0u, {col.fill[0], col.fill[1]}};
    Cell<W> v[kGatherLaneRows];
    load_rows<W>(v, plain, idx, el, GatherRows{});                    // the fill, then the loads of the valid elements alone
    store_rows<W>(v, col.dst, row0 + lane, nRows, GatherRows{});
    if (counts) add_counts(counts, wNull, wOor, nNull, nOor);
}

// Step 1 of a variable-length column. The grid covers nRows + 1 rows: the row behind the last gets the zero word the scan
// turns into the total.
__global__ void __launch_bounds__(kBlock)
k_gather_lengths(const uint32_t* __restrict__ map, uint64_t nRows, uint32_t rowBase, uint64_t srcRows, GatherCol2 col,
                 uint32_t* __restrict__ valid, unsigned long long* __restrict__ counts, unsigned long long* __restrict__ partials)
{
    __shared__ uint32_t wNull[kGatherWaves], wOor[kGatherWaves];
    __shared__ unsigned long long wSum[kGatherWaves];
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const uint64_t row0 = (uint64_t)blockIdx.x * kGatherBlockRows + w * kGatherWaveRows;
    uint32_t idx[kGatherLaneRows], nNull, nOor;
    bool ok[kGatherLaneRows], el[kGatherLaneRows];
    take_rows(map, nRows, rowBase, srcRows, row0, lane, valid, idx, ok, nNull, nOor);
    element_bits(col.srcValid, idx, ok, el);
    // the two offsets of every valid element, all in flight; any other row reads none
    uint32_t from[kGatherLaneRows], to[kGatherLaneRows];
#pragma unroll
    for (uint32_t j = 0; j < kGatherLaneRows; ++j) {
        from[j] = to[j] = 0;
        if (el[j]) { from[j] = col.srcOff[idx[j]]; to[j] = col.srcOff[(uint64_t)idx[j] + 1]; }
    }
    unsigned long long sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kGatherLaneRows; ++j) {
        const uint64_t k = row0 + lane + j * kGatherStepRows;
        const uint32_t len = to[j] - from[j];
        sum += len;
        if (k <= nRows) col.dstOff[k] = len;                          // k == nRows: the zero word (no map entry: len 0)
        if (col.dstValid) {
            const unsigned long long bits = __ballot(el[j]);
            store_plane_step(col.dstValid, row0 + j * kGatherStepRows, nRows, bits, lane);
        }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) sum += __shfl_down(sum, off, kWave);
    if (lane == 0) wSum[w] = sum;
    if (counts) add_counts(counts, wNull, wOor, nNull, nOor);         // (has the barrier)
    else __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (uint32_t i = 0; i < kGatherWaves; ++i) t += wSum[i];
        partials[blockIdx.x] = t;
    }
}

// one workgroup: total = the sum of partials[0 .. n)
__global__ void __launch_bounds__(kBlock)
k_gather_total(const unsigned long long* __restrict__ partials, uint32_t n, unsigned long long* __restrict__ total)
{
    __shared__ unsigned long long wSum[kGatherWaves];
    unsigned long long sum = 0;
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) sum += partials[i];
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) sum += __shfl_down(sum, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) wSum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
#pragma unroll
        for (uint32_t i = 0; i < kGatherWaves; ++i) t += wSum[i];
        *total = t;
    }
}

// Step 3 (see the head of this part). dstOff: the scanned offsets; total: the column's 64-bit total.
__global__ void __launch_bounds__(kBlock)
k_gather_copy(const uint32_t* __restrict__ map, uint64_t nRows, uint32_t rowBase, GatherCol2 col, const unsigned long long* __restrict__ total)
{
    __shared__ uint32_t dOff[kGatherBlockRows + 1];                   // output offsets of the workgroup's rows and the end of the last
    __shared__ uint32_t sOff[kGatherBlockRows];                       // where the element of a row that has bytes starts in src
    if (*total > 0xFFFFFFFFull) return;                               // the offsets wrapped: nothing of this column is written
    const uint64_t row0 = (uint64_t)blockIdx.x * kGatherBlockRows;
    const uint32_t rows = nRows - row0 < kGatherBlockRows ? (uint32_t)(nRows - row0) : kGatherBlockRows;
    for (uint32_t t = threadIdx.x; t <= rows; t += kBlock) dOff[t] = col.dstOff[row0 + t];
    __syncthreads();
    const uint64_t begin = dOff[0];
    const uint64_t end = (uint64_t)dOff[rows] < col.capacity ? (uint64_t)dOff[rows] : col.capacity;
    if (begin >= end) return;                                         // workgroup-uniform: no byte of these rows is in the output
    // A row has bytes exactly when the lengths kernel found a valid element for it: its entry is in range, and only such a
    // row reads its entry and its offset again. Rows at or behind the cut read nothing.
#pragma unroll
    for (uint32_t j = 0; j < kGatherBlockRows / kBlock; ++j) {
        const uint32_t t = threadIdx.x + j * kBlock;
        if (t < rows && dOff[t + 1] > dOff[t] && dOff[t] < end) sOff[t] = col.srcOff[map[row0 + t] - rowBase];
    }
    __syncthreads();

    const uint64_t dstA = reinterpret_cast<uintptr_t>(col.dst), srcA = reinterpret_cast<uintptr_t>(col.src);
    const uint64_t absBegin = dstA + begin, absEnd = dstA + end;
    for (uint64_t block = (absBegin & ~(uint64_t)(kCopyBlockBytes - 1)) + (uint64_t)threadIdx.x * kCopyBlockBytes; block < absEnd;
         block += kCopyPassBytes) {
        const uint64_t lo = block > absBegin ? block : absBegin, hi = block + kCopyBlockBytes < absEnd ? block + kCopyBlockBytes : absEnd;
        const uint32_t pLo = (uint32_t)(lo - dstA), pHi = (uint32_t)(hi - dstA);   // output positions: below 2^32 (lo < hi always)
        // the last row whose offset is at or below pLo: the row that holds byte pLo (dOff[a] <= pLo < dOff[b] throughout)
        uint32_t a = 0, b = rows;
        while (b - a > 1) {
            const uint32_t mid = (a + b) >> 1;
            if (dOff[mid] > pLo) b = mid; else a = mid;
        }
        uint32_t acc[4] = {0, 0, 0, 0};
        uint32_t pos = pLo;
        for (uint32_t r = a; pos < pHi; ++r) {                        // pHi <= dOff[rows]: r stays below rows
            const uint32_t o = dOff[r], oe = dOff[r + 1];
            if (oe <= pos) continue;                                  // an empty row inside the block
            const uint32_t segEnd = oe < pHi ? oe : pHi;
            const uint32_t cb = (uint32_t)(dstA + pos - block), ce = (uint32_t)(dstA + segEnd - block);   // the block's bytes [cb, ce)
            // the source address of block byte 0 if the segment went that far (it need not: only words that hold a byte
            // of [cb, ce) are loaded), its alignment, and the five aligned words around the block
            const uint64_t base = srcA + sOff[r] + (pos - o) - cb;
            const uint32_t sh = (uint32_t)base & 3u;
            const uint64_t w0 = base & ~3ull;
            const uint64_t first = (base + cb) & ~3ull, last = (base + ce - 1) & ~3ull;
            uint32_t word[5];
#pragma unroll
            for (uint32_t q = 0; q < 5; ++q) {
                const uint64_t at = w0 + 4ull * q;
                word[q] = 0;
                if (at >= first && at <= last) word[q] = *reinterpret_cast<const uint32_t*>(at);
            }
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t lo4 = cb > 4 * q ? cb - 4 * q : 0u, hi4 = ce > 4 * q ? ce - 4 * q : 0u;
                acc[q] |= __builtin_amdgcn_alignbyte(word[q + 1], word[q], sh) & byte_mask(lo4 < 4 ? lo4 : 4u, hi4 < 4 ? hi4 : 4u);
            }
            pos = segEnd;
        }
        if (hi - lo == kCopyBlockBytes) {
            u4 out; out.x = acc[0]; out.y = acc[1]; out.z = acc[2]; out.w = acc[3];
            __builtin_nontemporal_store(out, reinterpret_cast<u4*>(block));
        } else {                                                      // the range's first or last block: its own bytes alone
            for (uint32_t t = (uint32_t)(lo - block); t < (uint32_t)(hi - block); ++t) {
                const uint32_t wsel = t < 4 ? acc[0] : t < 8 ? acc[1] : t < 12 ? acc[2] : acc[3];
                reinterpret_cast<uint8_t*>(block)[t] = (uint8_t)(wsel >> (8u * (t & 3u)));
            }
        }
    }
}

namespace {

inline bool gather2_plain(const GatherCol2& c) { return c.width && !c.srcValid && !c.dstValid; }

template <int W>
void launch_nullable(dim3 grid, hipStream_t s, const uint32_t* map, uint64_t nRows, uint32_t rowBase, uint64_t srcRows, const GatherCol2& col,
                     uint32_t* valid, unsigned long long* counts)
{
    hipLaunchKernelGGL((k_gather_nullable<W>), grid, dim3(kBlock), 0, s, map, nRows, rowBase, srcRows, col, valid, counts);
}

}  // namespace

// the scan's words for nRows + 1 offsets, then (8-byte aligned) one partial per workgroup of k_gather_lengths
static size_t gather2_scan_words(uint64_t nRows) { return (scan_workspace_words(nRows + 1) + 1) & ~(size_t)1; }
static uint32_t gather2_length_blocks(uint64_t nRows) { return (uint32_t)((nRows + 1 + kGatherBlockRows - 1) / kGatherBlockRows); }
size_t gather2_work_words(uint64_t nRows) { return gather2_scan_words(nRows) + 2 * (size_t)gather2_length_blocks(nRows); }

hipError_t launch_gather2(const uint32_t* map, uint64_t nRows, uint32_t rowBase, uint64_t srcRows, const GatherCols2& cols, uint32_t nCols,
                          uint32_t* valid, unsigned long long* counts, unsigned long long* totals, uint32_t* work, hipStream_t s)
{
    if (nRows == 0) return hipSuccess;
    hipError_t e;
    if ((e = hipMemsetAsync(totals, 0, kGatherMaxCols * sizeof(unsigned long long), s)) != hipSuccess) return e;
    // the plain columns, as hj_gather_dev launches them; with them, or with no column at all, the plane and the counts
    GatherCols plain{};
    uint32_t nPlain = 0;
    for (uint32_t c = 0; c < nCols; ++c)
        if (gather2_plain(cols.col[c]))
            plain.col[nPlain++] = GatherCol{cols.col[c].src, cols.col[c].dst, cols.col[c].width, 0u, {cols.col[c].fill[0], cols.col[c].fill[1]}};
    bool first = true;
    if (nPlain || nPlain == nCols) {
        if ((e = launch_gather(map, nRows, rowBase, srcRows, plain, nPlain, valid, counts, s)) != hipSuccess) return e;
        first = false;
    }
    const dim3 grid((uint32_t)((nRows + kGatherBlockRows - 1) / kGatherBlockRows));
    const uint32_t lengthBlocks = gather2_length_blocks(nRows);
    unsigned long long* const partials = reinterpret_cast<unsigned long long*>(work + gather2_scan_words(nRows));
    for (uint32_t c = 0; c < nCols; ++c) {
        const GatherCol2& col = cols.col[c];
        if (gather2_plain(col)) continue;
        uint32_t* const v = first ? valid : nullptr;
        unsigned long long* const k = first ? counts : nullptr;
        first = false;
        switch (col.width) {
            case 16: launch_nullable<16>(grid, s, map, nRows, rowBase, srcRows, col, v, k); continue;
            case 8: launch_nullable<8>(grid, s, map, nRows, rowBase, srcRows, col, v, k); continue;
            case 4: launch_nullable<4>(grid, s, map, nRows, rowBase, srcRows, col, v, k); continue;
            case 2: launch_nullable<2>(grid, s, map, nRows, rowBase, srcRows, col, v, k); continue;
            case 1: launch_nullable<1>(grid, s, map, nRows, rowBase, srcRows, col, v, k); continue;
            default: break;
        }
        hipLaunchKernelGGL(k_gather_lengths, dim3(lengthBlocks), dim3(kBlock), 0, s, map, nRows, rowBase, srcRows, col, v, k, partials);
        hipLaunchKernelGGL(k_gather_total, dim3(1), dim3(kBlock), 0, s, partials, lengthBlocks, totals + c);
        if ((e = launch_exclusive_scan_u32(col.dstOff, nRows + 1, work, s)) != hipSuccess) return e;
        if (col.capacity) hipLaunchKernelGGL(k_gather_copy, grid, dim3(kBlock), 0, s, map, nRows, rowBase, col, totals + c);
    }
    return hipGetLastError();
}

}  // namespace hj
