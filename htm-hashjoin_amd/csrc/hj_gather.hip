// hj_gather.hip -- payload columns through the join's row maps for gfx950 (MI355X): hj_gather_dev.
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
// What it does NOT do: the map is neither sorted nor bucketed before the gather. A random map (the R side of a join on a
// shuffled R) therefore fetches one cache line per element -- the amplification the counting probe shows under a
// scattered S -- and nothing here hides it.

#include "hj_device.h"

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

}  // namespace hj
