// hj_shard.hip -- the destination split of the multi-GPU path for gfx950 (MI355X): hj_shard_histogram_dev /
// hj_shard_scatter_dev. One radix pass on the low log2(nShards) key bits, tuples in, bare keys out, and STABLE: inside a
// destination the keys keep their input order exactly. The join's semantics are "insert in input order"; the receiving
// rank takes a key's position in its receive buffer as that order, so the scatter may not permute anything (the radix
// join's scatter, k_radix_scatter of hj_prj.hip, ranks with LDS atomics and is only stable tile by tile -- the radix join
// does not care). It also keeps a near-sorted input near-sorted, so the receiver's locality pre-round still picks the
// LDS-window build. The histogram is the radix join's exact pass (pass_offsets, hj_prj.hip, through hj_prj_impl.h); the
// scatter kernels are this file's own.
//
// Ranking without atomics (k_shard_scatter_stable): lane l of wavefront w holds, for k = 0..7, the tile's element
// k*1024 + 64 w + l, so (k, w, l) is input order. For one k a wavefront finds, per lane, the lanes with the same
// destination (log2(fan) ballots) -- its rank among them is a popcount of the lower lanes, their number goes to
// cnt[bin][k][w]. An exclusive scan of cnt in exactly that order gives every (bin, k, w) group its place in the tile's
// staged order.

#include "hj_prj_impl.h"

namespace hj {

constexpr int kStabThreads = 1024;
constexpr int kStabPer = 8;                                    // tuples per thread per tile
constexpr int kStabTile = kStabThreads * kStabPer;             // 8192
constexpr int kStabGroups = kStabPer * (kStabThreads / 64);    // (k, wavefront) groups per tile = 128
constexpr int kStabMaxFan = 64;

__global__ void __launch_bounds__(kStabThreads, 8)
k_shard_scatter_stable(const uint64_t* __restrict__ in, uint32_t* __restrict__ out, PassParams p,
                       const uint32_t* __restrict__ scanned)
{
    extern __shared__ uint32_t stab[];              // cnt[fan][kStabGroups], then stage[kStabTile + kStabTile/32 + 1]
    uint32_t* const cnt = stab;
    const uint32_t nCnt = p.fan * kStabGroups;
    uint32_t* const stage = stab + nCnt;
    __shared__ unsigned int delta[kStabMaxFan];     // write cursor of the bin - its offset in the staged tile
    __shared__ unsigned int cursor[kStabMaxFan];
    __shared__ uint32_t wsum[kStabThreads / 64];
    constexpr uint32_t kDump = kStabTile + (kStabTile >> 5);

    const uint32_t c = blockIdx.x;
    if (c >= p.chunkBase[p.nSeg]) return;
    const ChunkRange r = chunk_range(p, c);
    const uint32_t fmask = p.fan - 1;
    const uint32_t len = r.end - r.begin;
    const uint32_t wave = threadIdx.x >> 6;
    int bits = 0;
    while ((1u << bits) < p.fan) ++bits;
    if (threadIdx.x < p.fan) cursor[threadIdx.x] = scanned[hist_index(p, r, threadIdx.x)];
    const uint32_t perThread = nCnt / kStabThreads;               // fan * 128 / 1024 = fan / 8 (fan >= 8) ...
    const uint32_t items = perThread ? perThread : 1;             // ... or 1 with some threads idle (fan < 8)
    __syncthreads();

    for (uint32_t tb = 0; tb < len; tb += kStabTile) {
        for (uint32_t i = threadIdx.x; i < nCnt; i += kStabThreads) cnt[i] = 0;
        uint32_t key[kStabPer], rk4[kStabPer / 4];    // ranks are < 64: four to a register
        uint32_t okMask = 0;
#pragma unroll
        for (int k = 0; k < kStabPer / 4; ++k) rk4[k] = 0;
#pragma unroll
        for (int k = 0; k < kStabPer; ++k) {
            const uint32_t rel = tb + (uint32_t)k * kStabThreads + threadIdx.x;
            const bool ok = rel < len;
            const uint64_t t = ok ? in[(uint64_t)r.begin + rel] : 0ull;
            key[k] = (t >> 32) ? 0u : (uint32_t)t;                 // payload bits set: see PassParams::zeroBad
            okMask |= ok ? (1u << k) : 0u;
        }
        __syncthreads();                                          // cnt is zero
#pragma unroll
        for (int k = 0; k < kStabPer; ++k) {
            const bool ok = (okMask >> k) & 1u;
            const uint32_t bin = ((key[k] - p.bias) >> p.shift) & fmask;
            unsigned long long peers = __ballot(ok);
            for (int b = 0; b < bits; ++b) {
                const bool bit = (bin >> b) & 1u;
                const unsigned long long m = __ballot(bit);
                peers &= bit ? m : ~m;
            }
            const uint32_t rk = lane_rank(peers);
            rk4[k / 4] |= rk << (8 * (k % 4));
            if (ok && rk == 0) cnt[(bin * kStabPer + k) * (kStabThreads / 64) + wave] = (uint32_t)__popcll(peers);
        }
        __syncthreads();
        {   // exclusive scan of cnt[0..nCnt) in place, `items` consecutive entries per thread
            const uint32_t base = threadIdx.x * items;
            uint32_t local = 0;
            for (uint32_t i = 0; i < items; ++i) local += (base + i < nCnt) ? cnt[base + i] : 0u;
            uint32_t total;
            uint32_t ex = block_exclusive_scan<kStabThreads>(local, wsum, total);
            for (uint32_t i = 0; i < items; ++i) {
                if (base + i < nCnt) { const uint32_t v = cnt[base + i]; cnt[base + i] = ex; ex += v; }
            }
        }
        __syncthreads();
        if (threadIdx.x < p.fan) {
            const uint32_t off = cnt[threadIdx.x * kStabGroups];                      // first group of the bin
            const uint32_t end = threadIdx.x + 1 < p.fan ? cnt[(threadIdx.x + 1) * kStabGroups]
                                                         : (len - tb < (uint32_t)kStabTile ? len - tb : (uint32_t)kStabTile);
            const uint32_t cu = cursor[threadIdx.x];
            delta[threadIdx.x] = cu - off;
            cursor[threadIdx.x] = cu + (end - off);
        }
#pragma unroll
        for (int k = 0; k < kStabPer; ++k) {
            const uint32_t bin = ((key[k] - p.bias) >> p.shift) & fmask;
            const uint32_t at = cnt[(bin * kStabPer + k) * (kStabThreads / 64) + wave] + ((rk4[k / 4] >> (8 * (k % 4))) & 0xFFu);
            stage[((okMask >> k) & 1u) ? at + (at >> 5) : kDump] = key[k];
        }
        __syncthreads();
        const uint32_t valid = len - tb < (uint32_t)kStabTile ? len - tb : (uint32_t)kStabTile;
#pragma unroll 4
        for (int k = 0; k < kStabPer; ++k) {
            const uint32_t q = (uint32_t)k * kStabThreads + threadIdx.x;
            if (q < valid) {
                const uint32_t t = stage[q + (q >> 5)];
                out[delta[((t - p.bias) >> p.shift) & fmask] + q] = t;
            }
        }
        __syncthreads();                                          // stage, cnt and delta are reused by the next tile
    }
}


// The same split for fan-outs <= 16 (every multi-GPU node there is), one WAVEFRONT per chunk and no workgroup barrier:
// the kernel above synchronises its 16 wavefronts seven times per tile (3.0 TB/s of its 12 bytes per tuple). Here a
// wavefront walks its chunk in tiles of 512 tuples (lane l holds tile elements 64 k + l, k = 0..7: (k, l) is input
// order), ranks them bin by bin with ballots -- fan x 8 ballots per tile, the running count is the tile offset of the
// next bin -- stages the tile in its own 2 KiB of LDS grouped by destination and writes the runs out through cursors it
// keeps in registers (start = the chunk's scanned histogram entries). Same output, element for element.
constexpr int kSwThreads = 256;
constexpr int kSwPer = 8;
constexpr int kSwTile = 64 * kSwPer;             // 512 tuples per wavefront tile
constexpr int kSwMaxFan = 16;

__global__ void __launch_bounds__(kSwThreads)
k_shard_scatter_wave(const uint64_t* __restrict__ in, uint32_t* __restrict__ out, PassParams p,
                     const uint32_t* __restrict__ scanned)
{
    __shared__ uint32_t stage[kSwThreads / 64][kSwTile];
    __shared__ uint32_t delta[kSwThreads / 64][kSwMaxFan];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t c = blockIdx.x * (kSwThreads / 64) + wave;
    if (c >= p.chunkBase[p.nSeg]) return;                          // whole wavefronts leave; nobody waits for them
    const ChunkRange r = chunk_range(p, c);
    const uint32_t fan = p.fan, fmask = fan - 1;
    const uint32_t len = r.end - r.begin;
    uint32_t cur[kSwMaxFan];                                       // write cursor per destination (wave-uniform)
#pragma unroll
    for (int b = 0; b < kSwMaxFan; ++b)
        cur[b] = (uint32_t)b < fan ? (uint32_t)__builtin_amdgcn_readfirstlane((int)scanned[hist_index(p, r, (uint32_t)b)]) : 0u;
    const uint64_t* __restrict__ src = in + r.begin;
    uint64_t nxt[kSwPer];
#pragma unroll
    for (int k = 0; k < kSwPer; ++k) { const uint32_t rel = 64u * k + lane; nxt[k] = rel < len ? src[rel] : 0ull; }
    for (uint32_t tb = 0; tb < len; tb += kSwTile) {
        uint32_t key[kSwPer], bin[kSwPer], pos[kSwPer];
        uint32_t okMask = 0;
#pragma unroll
        for (int k = 0; k < kSwPer; ++k) {
            const uint64_t t = nxt[k];
            key[k] = (t >> 32) ? 0u : (uint32_t)t;                 // payload bits set: travels as key 0 (PassParams::zeroBad)
            const bool ok = tb + 64u * k + lane < len;
            bin[k] = ok ? ((key[k] - p.bias) >> p.shift) & fmask : 0xFFFFFFFFu;   // past the chunk's end: no destination's
            okMask |= ok ? (1u << k) : 0u;
            pos[k] = 0;
        }
#pragma unroll
        for (int k = 0; k < kSwPer; ++k) { const uint32_t rel = tb + kSwTile + 64u * k + lane; nxt[k] = rel < len ? src[rel] : 0ull; }
        uint32_t off = 0;                                          // staged position where the next destination's run starts
#pragma unroll
        for (int b = 0; b < kSwMaxFan; ++b) {
            if ((uint32_t)b < fan) {                               // wave-uniform
                uint32_t cnt = 0;
#pragma unroll
                for (int k = 0; k < kSwPer; ++k) {
                    const bool mine = bin[k] == (uint32_t)b;
                    const unsigned long long m = __ballot(mine);
                    pos[k] = mine ? off + cnt + lane_rank(m) : pos[k];
                    cnt += (uint32_t)__popcll(m);
                }
                if (lane == 0) delta[wave][b] = cur[b] - off;      // output index of staged position q = delta[bin] + q
                cur[b] += cnt;
                off += cnt;
            }
        }
#pragma unroll
        for (int k = 0; k < kSwPer; ++k)
            if ((okMask >> k) & 1u) stage[wave][pos[k]] = key[k];
        // (LDS operations of one wavefront complete in issue order: the reads below see the stores above)
        const uint32_t valid = len - tb < (uint32_t)kSwTile ? len - tb : (uint32_t)kSwTile;
#pragma unroll
        for (int k = 0; k < kSwPer; ++k) {
            const uint32_t q = 64u * k + lane;
            if (q < valid) {
                const uint32_t t = stage[wave][q];
                out[delta[wave][((t - p.bias) >> p.shift) & fmask] + q] = t;
            }
        }
    }
}

namespace {
struct ShardWork { uint32_t *seg0, *segOut, *chunkBase, *hist, *sums; };
ShardWork shard_carve(void* base, uint64_t n, uint32_t fan)
{
    const PassLayout l = pass_layout(n, 1, fan);
    char* p = static_cast<char*>(base);
    ShardWork w;
    w.seg0 = reinterpret_cast<uint32_t*>(p); p += 256;
    w.segOut = reinterpret_cast<uint32_t*>(p); p += align_up(sizeof(uint32_t) * (fan + 1), 256);
    w.chunkBase = reinterpret_cast<uint32_t*>(p); p += 256;
    w.hist = reinterpret_cast<uint32_t*>(p); p += align_up(sizeof(uint32_t) * l.histEntries, 256);
    w.sums = reinterpret_cast<uint32_t*>(p);
    return w;
}
__global__ void k_shard_counts(const uint32_t* __restrict__ segOut, uint32_t fan, unsigned long long* __restrict__ counts)
{
    if (threadIdx.x < fan) counts[threadIdx.x] = segOut[threadIdx.x + 1] - segOut[threadIdx.x];
}
}  // namespace

size_t shard_work_bytes(uint64_t n, uint32_t nShards)
{
    const PassLayout l = pass_layout(n, 1, nShards);
    return 256 + align_up(sizeof(uint32_t) * (nShards + 1), 256) + 256 +
           align_up(sizeof(uint32_t) * l.histEntries, 256) + align_up(sizeof(uint32_t) * (l.scanBlocks + 1), 256);
}

hipError_t launch_shard_hist(const uint64_t* in, uint64_t n, uint32_t nShards, uint32_t digitShift, void* work,
                             unsigned long long* counts, hipStream_t s)
{
    const ShardWork w = shard_carve(work, n, nShards);
    const PassLayout l = pass_layout(n, 1, nShards);
    launch_init_seg(w.seg0, (uint32_t)n, s);
    launch_chunk_base(w.seg0, 1u, l.chunkLen, w.chunkBase, s);
    const PassParams p{w.seg0, 1u, l.chunkLen, w.chunkBase, digitShift & 0xFFu, nShards, (digitShift >> 8) & 1u, 1u};
    const hipError_t e = pass_offsets(in, false, PassRows{false, nullptr, 0u}, p, l, n, w.hist, w.sums, w.segOut, kNoGate, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_shard_counts, dim3(1), dim3(64), 0, s, w.segOut, nShards, counts);
    return hipGetLastError();
}

// tuples in, bare keys out, stable: the exchange moves 4 bytes per tuple and no index
hipError_t launch_shard_scatter_ordered(const uint64_t* in, uint64_t n, uint32_t nShards, uint32_t digitShift, void* work,
                                        uint32_t* outKeys, hipStream_t s)
{
    const ShardWork w = shard_carve(work, n, nShards);
    const PassLayout l = pass_layout(n, 1, nShards);
    PassParams p{w.seg0, 1u, l.chunkLen, w.chunkBase, digitShift & 0xFFu, nShards, (digitShift >> 8) & 1u, 1u};
    const size_t lds = sizeof(uint32_t) * ((size_t)nShards * kStabGroups + kStabTile + (kStabTile >> 5) + 1);   // <= 65.1 KiB
    if (nShards <= (uint32_t)kSwMaxFan)
        hipLaunchKernelGGL(k_shard_scatter_wave, dim3((unsigned)((l.maxChunks + kSwThreads / 64 - 1) / (kSwThreads / 64))),
                           dim3(kSwThreads), 0, s, in, outKeys, p, w.hist);
    else
        hipLaunchKernelGGL(k_shard_scatter_stable, dim3((unsigned)l.maxChunks), dim3(kStabThreads), lds, s,
                           in, outKeys, p, w.hist);
    return hipGetLastError();
}

hipError_t shard_set_attributes()
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_shard_scatter_stable),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               sizeof(uint32_t) * (kStabMaxFan * kStabGroups + kStabTile + (kStabTile >> 5) + 1));
}

}  // namespace hj
