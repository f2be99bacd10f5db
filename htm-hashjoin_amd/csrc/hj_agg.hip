// hj_agg.hip -- the reduction over a pair list for gfx950 (MI355X): hj_pairs_agg_dev. COUNT / SUM / MIN / MAX of the values
// one map names, grouped by the rows the other map names -- for the joins whose pairs must exist first (join_on and
// join_on_columns verify their candidates; the table probes have no resident partitions).
//
//   k_pairs_agg        one pair per lane, a wavefront's 64 pairs neighbours in the list. The lanes of a RUN of equal group
//                      rows combine their values with a segmented scan over the wavefront (shuffles, no LDS), and the last
//                      lane of the run issues one 64-bit global atomic per column: the radix join emits the pairs of a hot
//                      R row in runs, so a run of 64 costs one memory-side request where 64 lanes would have queued on one
//                      address. Runs do not reach across wavefronts.
//
// The cost is one memory-side atomic request per run and column, scattered: a list without runs (a foreign-key join grouped
// by its unique side) pays one request per pair and column. Exact: integer ops only, so no result depends on the order.
#include "hj_columns.h"

namespace hj {

namespace {

__global__ void __launch_bounds__(kBlock)
k_pairs_agg(const uint32_t* __restrict__ mapG, const uint32_t* __restrict__ mapV, uint64_t nPairs, uint32_t gBase, uint32_t gRows,
            uint32_t vBase, uint32_t vRows, PairAggCols cols, uint32_t nCols, unsigned long long* __restrict__ count,
            unsigned long long* __restrict__ counts)
{
    const uint32_t lane = threadIdx.x & (kWave - 1);
    unsigned long long applied = 0, skipped = 0;
    // every lane of a wavefront runs the same number of rounds: the scans below take the whole wavefront
    for (uint64_t k0 = (uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~(uint32_t)(kWave - 1)); k0 < nPairs; k0 += (uint64_t)gridDim.x * kBlock) {
        const uint64_t k = k0 + lane;
        const bool in = k < nPairs;
        const uint32_t eg = in ? mapG[k] : kNoRow, ev = (in && mapV) ? mapV[k] : 0u;
        const uint32_t g = eg - gBase, v = ev - vBase;
        const bool live = in && eg != kNoRow && g < gRows && (!mapV || (ev != kNoRow && v < vRows));    // the raw entries: whatever the base
        applied += live;
        skipped += in && !live;
        // runs: neighbouring lanes with the same group row; a lane that applies nothing is a run of its own kind
        const uint32_t key = live ? g : kNoRow;
        const uint32_t before = __shfl_up(key, 1, kWave);
        const bool head = lane == 0 || before != key;
        const unsigned long long heads = __ballot(head);
        const uint32_t start = 63u - (uint32_t)__clzll(heads & (~0ull >> (63u - lane)));        // the head of this lane's run
        const bool tail = lane == kWave - 1 || ((heads >> (lane + 1)) & 1ull);
        if (count && live && tail) __hip_atomic_fetch_add(&count[g], (unsigned long long)(lane - start + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (uint32_t c = 0; c < nCols; ++c) {
            const uint32_t op = cols.ops.op[c], sgn = cols.ops.sgn[c];
            const unsigned long long id = agg_identity(op, sgn);
            const uint32_t* const valid = cols.src.valid[c];
            const bool ok = live && (!valid || valid_bit(valid, v));
            unsigned long long x = ok ? agg_value(cols.src.p[c], op, cols.ops.width[c], sgn, v) : id;
#pragma unroll
            for (uint32_t off = 1; off < (uint32_t)kWave; off <<= 1) {
                const unsigned long long below = __shfl_up(x, off, kWave);
                if (lane >= start + off) x = agg_combine(op, sgn, x, below);
            }
            if (live && tail && x != id) agg_apply<__HIP_MEMORY_SCOPE_AGENT>(&cols.acc[c][g], op, sgn, x);
        }
    }
    applied = wave_sum(applied);
    skipped = wave_sum(skipped);
    if (lane == 0) {
        if (applied) atomicAdd(&counts[0], applied);
        if (skipped) atomicAdd(&counts[1], skipped);
    }
}

}  // namespace

hipError_t launch_pairs_agg(const uint32_t* mapG, const uint32_t* mapV, uint64_t nPairs, uint32_t gBase, uint32_t gRows, uint32_t vBase,
                            uint32_t vRows, const PairAggCols& cols, uint32_t nCols, unsigned long long* count, unsigned long long* counts,
                            hipStream_t s)
{
    if (nPairs == 0) return hipSuccess;
    const uint64_t blocks = (nPairs + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_pairs_agg, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(kBlock), 0, s, mapG, mapV, nPairs, gBase, gRows,
                       vBase, vRows, cols, nCols, count, counts);
    return hipGetLastError();
}

}  // namespace hj
