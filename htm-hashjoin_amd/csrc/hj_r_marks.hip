// hj_r_marks.hip -- the sweep of the R-side match marks for gfx950 (MI355X): hj_r_rows_dev.
//
// The pairs kernels of a context reserved with HJ_FLAG_TRACK_R_MATCHES leave one bit per R row of the last build (RMarks,
// hj_pairs.h). The sweep turns the set bits, or the clear ones, into rows: an ORDERED compaction, so that the R-only tail
// of a right or full outer join comes out ascending and a truncated call yields the first `capacity` rows.
//
//   k_r_sweep_count   one workgroup per kSweepWords words of the plane: the rows it will write -> counts[block]
//   (exclusive scan)  launch_exclusive_scan_u32 over the counts and one zero word behind them, which ends as the total
//   k_r_sweep_write   the same words again: a wavefront prefix of the popcounts (block_prefix) gives every lane the place
//                     of its first row in the workgroup's run; the rows are staged in LDS in ascending order and leave as
//                     16-byte stores through flush_plane, which cuts the run at the capacity
//
// The plane is rows / 8 bytes and is read twice; a row written is 4 bytes: at half of the rows produced the plane is a
// sixteenth of the traffic. The complement is taken on the fly, and the last word is masked to the build's rows in both
// kernels by the same function, so that a clear bit behind the last row is no row.

#include "hj_pairs.h"

namespace hj {

namespace {

constexpr uint32_t kSweepWords = kBlock;                  // words of the plane per workgroup, one per lane
constexpr uint32_t kSweepRows = 32u * kSweepWords;        // rows of one workgroup: its stage, 32 KiB of LDS
constexpr uint32_t kSweepWaves = kBlock / kWave;

// the bits of word `w` of the plane that are rows to write: the word, or its complement, without the bits at or behind
// `rows`; 0 for a word behind the plane
__device__ __forceinline__ uint32_t sweep_bits(const RMarks& mk, uint32_t w, bool set)
{
    const uint64_t first = (uint64_t)w << 5;
    if (first >= mk.rows) return 0u;
    const uint32_t left = mk.rows - (uint32_t)first;          // rows from this word's bit 0 on (>= 1)
    const uint32_t live = left >= 32u ? 0xFFFFFFFFu : (1u << left) - 1u;
    const uint32_t v = mk.words[w];
    return (set ? v : ~v) & live;
}

// exclusive prefix of v over the workgroup, its total in `total`; wsum: kSweepWaves words of LDS
__device__ __forceinline__ uint32_t block_prefix(uint32_t v, uint32_t* wsum, uint32_t& total)
{
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const uint32_t below = __shfl_up(inc, off, kWave);
        if (lane >= (uint32_t)off) inc += below;
    }
    if (lane == kWave - 1) wsum[w] = inc;
    __syncthreads();
    uint32_t wbase = 0, tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSweepWaves; ++k) {
        const uint32_t c = wsum[k];
        if (k < w) wbase += c;
        tot += c;
    }
    total = tot;
    return wbase + inc - v;
}

}  // namespace

__global__ void __launch_bounds__(kBlock)
k_r_sweep_count(RMarks mk, bool set, uint32_t* __restrict__ counts)
{
    __shared__ uint32_t wsum[kSweepWaves];
    const uint32_t c = (uint32_t)__popc(sweep_bits(mk, blockIdx.x * kSweepWords + threadIdx.x, set));
    uint32_t total;
    block_prefix(c, wsum, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// bases: the scanned counts. The workgroups' runs follow each other in block order and every run is ascending inside.
__global__ void __launch_bounds__(kBlock)
k_r_sweep_write(RMarks mk, bool set, const uint32_t* __restrict__ bases, uint32_t* __restrict__ out, uint64_t capacity)
{
    __shared__ uint32_t stage[kSweepRows];
    __shared__ uint32_t wsum[kSweepWaves];
    const uint64_t base = bases[blockIdx.x];
    if (base >= capacity) return;                             // workgroup-uniform: nothing of this run exists in the output
    const uint32_t w = blockIdx.x * kSweepWords + threadIdx.x;
    uint32_t bits = sweep_bits(mk, w, set);
    uint32_t total;
    uint32_t pos = block_prefix((uint32_t)__popc(bits), wsum, total);
    const uint32_t row0 = mk.base + (w << 5);                 // (no overflow: base + rows <= 2^32 - 1, and bits == 0 behind the plane)
    for (; bits; bits &= bits - 1u) stage[pos++] = row0 + (uint32_t)__builtin_ctz(bits);
    __syncthreads();
    flush_plane<kBlock>(stage, total, out, base, capacity);
}

uint32_t r_sweep_blocks(uint64_t rows) { return (uint32_t)((rows + kSweepRows - 1) / kSweepRows); }

size_t r_sweep_count_words(uint64_t rows)
{
    const uint64_t n = (uint64_t)r_sweep_blocks(rows) + 1;
    return (size_t)n + scan_workspace_words(n);
}

hipError_t launch_r_sweep(const RMarks& marks, bool set, uint32_t* out, uint64_t capacity, uint32_t* counts, hipStream_t s)
{
    const uint32_t blocks = r_sweep_blocks(marks.rows);
    if (blocks == 0) return hipSuccess;
    hipError_t e;
    if ((e = hipMemsetAsync(counts + blocks, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_r_sweep_count, dim3(blocks), dim3(kBlock), 0, s, marks, set, counts);
    if ((e = launch_exclusive_scan_u32(counts, (uint64_t)blocks + 1, counts + blocks + 1, s)) != hipSuccess) return e;
    if (capacity) hipLaunchKernelGGL(k_r_sweep_write, dim3(blocks), dim3(kBlock), 0, s, marks, set, counts, out, capacity);
    return hipGetLastError();
}

}  // namespace hj
