// hj_sort.hip -- the rows of ONE table in the order of up to four typed, nullable columns for gfx950 (MI355X):
// hj_sort_rows_dev / hj_sort_rows_host (ORDER BY a DESC, b NULLS FIRST, c, d). An LSD radix sort, 8 bits per pass, over
// (key, row) records kept as two planes -- the keys (4 bytes for elements of 1, 2 and 4 bytes, 8 for 8-byte ones) and the
// rows -- so that a kernel that needs one plane alone reads that plane alone.
//
// Columns are processed LAST TO FIRST; every pass is stable, so the order a later column left decides the ties of an
// earlier one, and the row number -- the order the first keys kernel starts from -- decides what is left. Per column:
//   (keys)      k_sort_keys: key[i] = sort_key(col[row[i]]) (hj_columns.h; 0 under a NULL). On the first column processed
//               the rows are the identity: a coalesced read, no row load, and the kernel writes the row plane itself.
//               After that it is a gather through the rows the previous column left.
//   per byte of the element, lowest first:
//   (histogram) k_sort_hist: the digit's counts per chunk, laid out (bin, chunk). A chunk is what ONE workgroup owns in
//               the pass (sort_layout). The counts are taken per pass: which records a chunk holds is what the pass
//               before decided, so one histogram per column cannot give them.
//   (scan)      launch_exclusive_scan_u32 over the 256 x chunks counts: a chunk's scanned entry is its first output
//               position in the bin.
//   (scatter)   k_sort_scatter: see there. The last byte pass of a column carries only the rows on (kRowsOut).
//   A column with a validity plane gets one more pass behind them, on the valid bit read through the row (kValidBit): two
//   bins, which is first follows HJ_SORT_NULLS_FIRST. The keys under the NULLs are 0, so the NULLs tie and keep their order.
// The last pass of the call writes its rows to the caller's dPerm; nothing else is written outside the workspace.
//
// No lane waits for another workgroup: there is no decoupled look-back and no flag anybody spins on -- the three launches
// of a pass order the passes, and every loop is bounded by the chunk. Passes are never skipped: the decision would have to
// be the device's (no host round trip), and then no launch would know which of the two planes holds the records.
#include "hj_columns.h"

#include <algorithm>
#include <vector>

namespace hj {
namespace {

constexpr int kSortThreads = 256;                              // four wavefronts
constexpr int kSortPer = 8;                                    // records per thread per tile
constexpr int kSortWaves = kSortThreads / 64;
constexpr uint32_t kSortTile = kSortThreads * kSortPer;        // 2048: what one workgroup ranks at a time
constexpr uint32_t kSortBins = 256;
constexpr uint32_t kSortGroups = kSortPer * kSortWaves;        // (element slot, wavefront) groups per bin = 32
constexpr uint32_t kSortCnt = kSortBins * kSortGroups;         // 8192 group counts ...
constexpr uint32_t kSortCntPad = kSortCnt + (kSortCnt >> 5);   // ... one word of padding per 32: see the scan
constexpr uint32_t kSortStage = kSortTile + (kSortTile >> 5) + 1;   // the staged tile, padded likewise, and the dump word
constexpr uint32_t kSortMinTiles = 2;                          // tiles per chunk at least: the tile loop runs at any size
constexpr uint32_t kSortMaxChunks = 4096;                      // the histogram of a pass: at most 256 x 4096 words = 4 MiB

enum SortMode { kKeysOut = 0, kRowsOut = 1, kValidBit = 2 };

__device__ __forceinline__ uint32_t pad32(uint32_t i) { return i + (i >> 5); }

// element i of a column of `width` bytes, zero-extended
__device__ __forceinline__ uint64_t sort_elem(const void* __restrict__ col, uint32_t width, uint32_t i)
{
    switch (width) {
        case 1: return static_cast<const uint8_t*>(col)[i];
        case 2: return static_cast<const uint16_t*>(col)[i];
        case 4: return static_cast<const uint32_t*>(col)[i];
        default: return static_cast<const unsigned long long*>(col)[i];
    }
}

// rowsIn null: the identity, and rowsOut gets it
template <class K>
__global__ void __launch_bounds__(kSortThreads)
k_sort_keys(const void* __restrict__ col, const uint32_t* __restrict__ valid, uint32_t width, uint32_t type, uint32_t flags,
            const uint32_t* __restrict__ rowsIn, uint32_t* __restrict__ rowsOut, K* __restrict__ keys, uint64_t n)
{
    const uint64_t base = (uint64_t)blockIdx.x * (kSortThreads * 4) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint64_t i = base + (uint64_t)k * kSortThreads;
        if (i >= n) break;
        const uint32_t row = rowsIn ? rowsIn[i] : (uint32_t)i;
        const uint64_t raw = sort_elem(col, width, row);                       // read under a NULL too: the bytes exist
        const bool ok = !valid || valid_bit(valid, row);
        keys[i] = ok ? (K)sort_key(type, width, flags, raw) : (K)0;
        if (!rowsIn) rowsOut[i] = row;
    }
}

// the digit of a record: a byte of its key, or (kValidBit) the valid bit of its row, flipped so that bin 0 is what comes first
template <class K, int MODE>
__device__ __forceinline__ uint32_t sort_bin(K key, uint32_t row, const uint32_t* __restrict__ valid, uint32_t arg)
{
    if constexpr (MODE == kValidBit) return (uint32_t)valid_bit(valid, row) ^ arg;
    else return (uint32_t)(key >> arg) & (kSortBins - 1);
}

// hist[bin * chunks + chunk] = the records of the chunk whose digit is `bin`. arg: the shift, or kValidBit's flip
template <class K, int MODE>
__global__ void __launch_bounds__(kSortThreads)
k_sort_hist(const K* __restrict__ keys, const uint32_t* __restrict__ rows, const uint32_t* __restrict__ valid, uint32_t arg, uint64_t n,
            uint32_t chunkRows, uint32_t chunks, uint32_t* __restrict__ hist)
{
    __shared__ uint32_t h[kSortBins];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t begin = (uint64_t)blockIdx.x * chunkRows;
    const uint32_t len = n - begin < chunkRows ? (uint32_t)(n - begin) : chunkRows;
    for (uint32_t tb = 0; tb < len; tb += kSortThreads) {
        const uint32_t rel = tb + threadIdx.x;
        const bool ok = rel < len;
        uint32_t bin = 0;
        if (ok) {
            if constexpr (MODE == kValidBit) bin = sort_bin<K, MODE>(0, rows[begin + rel], valid, arg);
            else bin = sort_bin<K, MODE>(keys[begin + rel], 0u, nullptr, arg);
        }
        // a wavefront whose records all have one digit (a high byte of small values, a plane without NULLs) adds once
        const unsigned long long live = __ballot(ok);
        const uint32_t first = __builtin_amdgcn_readfirstlane(bin);
        if (__ballot(ok && bin == first) == live) {
            if ((threadIdx.x & 63) == 0 && ok) atomicAdd(&h[first], (uint32_t)__popcll(live));
        } else if (ok) {
            atomicAdd(&h[bin], 1u);
        }
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * chunks + blockIdx.x] = h[threadIdx.x];
}

// The stable scatter of one pass: one workgroup per chunk, tile by tile, and no atomic anywhere -- the ranking of
// k_shard_scatter_stable (hj_shard.hip) at fan 256. Lane l of wavefront w holds, for k = 0..7, the tile's record
// k * 256 + 64 w + l, so (k, w, l) is input order. For one k a wavefront finds, per lane, the lanes with the same digit
// (8 ballots); a record's rank among them is a popcount of the lower lanes, their number goes to cnt[bin][k][w]. One
// exclusive scan of cnt in exactly that order gives every (bin, k, w) group its place in the staged tile: the records are
// staged in LDS grouped by bin, in input order inside a bin, and go out through per-bin cursors that start at the
// chunk's scanned histogram entries -- stores coalesced within a bin.
// LDS (8-byte keys): cnt 33 KiB + keys 16.5 KiB + rows 8.3 KiB + cursors 2 KiB = 59.8 KiB, two workgroups to a CU's
// 160 KiB. cnt holds 4 x tile words whatever the shape (256 bins x tile / 64 groups); the shard kernel's trick of packing
// the ranks below 64 into bytes is kept for the registers (rk4), the counts stay words: they are scanned as they lie.
// The scan gives a thread 32 consecutive counts; one word of padding per 32 puts the threads of a half wavefront on 32
// different banks. The staged planes are padded the same way.
template <class K, int MODE>
__global__ void __launch_bounds__(kSortThreads)
k_sort_scatter(const K* __restrict__ keysIn, const uint32_t* __restrict__ rowsIn, K* __restrict__ keysOut, uint32_t* __restrict__ rowsOut,
               const uint32_t* __restrict__ valid, uint32_t arg, uint64_t n, uint32_t chunkRows, uint32_t chunks,
               const uint32_t* __restrict__ scanned)
{
    __shared__ uint32_t cnt[kSortCntPad];
    __shared__ K stageK[MODE == kValidBit ? 1 : kSortStage];
    __shared__ uint32_t stageR[kSortStage];
    __shared__ uint32_t delta[kSortBins];           // write cursor of the bin - its offset in the staged tile
    __shared__ uint32_t cursor[kSortBins];
    __shared__ uint32_t wsum[kSortWaves];
    constexpr uint32_t kDump = kSortStage - 1;

    const uint64_t begin = (uint64_t)blockIdx.x * chunkRows;
    const uint32_t len = n - begin < chunkRows ? (uint32_t)(n - begin) : chunkRows;
    const uint32_t wave = threadIdx.x >> 6;
    cursor[threadIdx.x] = scanned[(uint64_t)threadIdx.x * chunks + blockIdx.x];
    __syncthreads();

    for (uint32_t tb = 0; tb < len; tb += kSortTile) {
        const uint32_t live = len - tb < kSortTile ? len - tb : kSortTile;
        for (uint32_t i = threadIdx.x; i < kSortCntPad; i += kSortThreads) cnt[i] = 0;
        K key[kSortPer];
        uint32_t row[kSortPer], bin[kSortPer], rk4[kSortPer / 4];          // ranks are < 64: four to a register
#pragma unroll
        for (int k = 0; k < kSortPer / 4; ++k) rk4[k] = 0;
#pragma unroll
        for (int k = 0; k < kSortPer; ++k) {
            const uint32_t q = (uint32_t)k * kSortThreads + threadIdx.x;
            const bool ok = q < live;
            key[k] = 0;
            if constexpr (MODE != kValidBit) key[k] = ok ? keysIn[begin + tb + q] : (K)0;
            row[k] = ok ? rowsIn[begin + tb + q] : 0u;
        }
#pragma unroll
        for (int k = 0; k < kSortPer; ++k) {
            const bool ok = (uint32_t)k * kSortThreads + threadIdx.x < live;
            bin[k] = ok ? sort_bin<K, MODE>(key[k], row[k], valid, arg) : 0u;
        }
        __syncthreads();                                          // cnt is zero
#pragma unroll
        for (int k = 0; k < kSortPer; ++k) {
            const bool ok = (uint32_t)k * kSortThreads + threadIdx.x < live;
            unsigned long long peers = __ballot(ok);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (bin[k] >> b) & 1u;
                const unsigned long long m = __ballot(bit);
                peers &= bit ? m : ~m;
            }
            const uint32_t rk = lane_rank(peers);
            rk4[k / 4] |= rk << (8 * (k % 4));
            if (ok && rk == 0) cnt[pad32((bin[k] * kSortPer + k) * kSortWaves + wave)] = (uint32_t)__popcll(peers);
        }
        __syncthreads();
        {   // exclusive scan of the kSortCnt counts in place, 32 consecutive ones per thread
            constexpr uint32_t kItems = kSortCnt / kSortThreads;
            const uint32_t base = threadIdx.x * kItems;
            uint32_t local = 0;
#pragma unroll 8
            for (uint32_t i = 0; i < kItems; ++i) local += cnt[pad32(base + i)];
            uint32_t total;
            uint32_t ex = block_exclusive_scan<kSortThreads>(local, wsum, total);
#pragma unroll 8
            for (uint32_t i = 0; i < kItems; ++i) { const uint32_t v = cnt[pad32(base + i)]; cnt[pad32(base + i)] = ex; ex += v; }
        }
        __syncthreads();
        {
            const uint32_t off = cnt[pad32(threadIdx.x * kSortGroups)];                   // first group of the bin
            const uint32_t end = threadIdx.x + 1 < kSortBins ? cnt[pad32((threadIdx.x + 1) * kSortGroups)] : live;
            const uint32_t cu = cursor[threadIdx.x];
            delta[threadIdx.x] = cu - off;
            cursor[threadIdx.x] = cu + (end - off);
        }
#pragma unroll
        for (int k = 0; k < kSortPer; ++k) {
            const bool ok = (uint32_t)k * kSortThreads + threadIdx.x < live;
            const uint32_t at = cnt[pad32((bin[k] * kSortPer + k) * kSortWaves + wave)] + ((rk4[k / 4] >> (8 * (k % 4))) & 0xFFu);
            const uint32_t to = ok ? pad32(at) : kDump;
            if constexpr (MODE != kValidBit) stageK[to] = key[k];
            stageR[to] = row[k];
        }
        __syncthreads();
        const uint32_t split = cnt[pad32(kSortGroups)];           // kValidBit: where bin 1 starts in the staged tile
#pragma unroll
        for (int k = 0; k < kSortPer; ++k) {
            const uint32_t q = (uint32_t)k * kSortThreads + threadIdx.x;
            if (q < live) {
                const uint32_t r = stageR[pad32(q)];
                uint32_t b;
                K t = 0;
                if constexpr (MODE == kValidBit) b = q >= split ? 1u : 0u;
                else { t = stageK[pad32(q)]; b = sort_bin<K, MODE>(t, 0u, nullptr, arg); }
                const uint32_t pos = delta[b] + q;
                if constexpr (MODE == kKeysOut) keysOut[pos] = t;
                rowsOut[pos] = r;
            }
        }
        __syncthreads();                                          // the stage, cnt and delta are reused by the next tile
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// layout, workspace, launches
// ---------------------------------------------------------------------------
SortLayout sort_layout(uint64_t n, uint32_t keyBytes)
{
    SortLayout l{};
    const uint64_t tiles = (n + kSortTile - 1) / kSortTile;
    const uint64_t perChunk = std::max<uint64_t>(kSortMinTiles, (tiles + kSortMaxChunks - 1) / kSortMaxChunks);
    l.tileRows = kSortTile;
    l.chunkRows = (uint32_t)(perChunk * kSortTile);                // 2^32 rows: 512 tiles, 2^20 rows
    l.chunks = (uint32_t)((n + l.chunkRows - 1) / l.chunkRows);    // <= kSortMaxChunks
    // the histogram is sized for what the chunk rule can ask for at any smaller n too: the workspace grows with n
    const uint64_t histChunks = std::min<uint64_t>(kSortMaxChunks, std::max<uint64_t>(1, (tiles + kSortMinTiles - 1) / kSortMinTiles));
    auto up = [](uint64_t b) { return (b + 255) & ~255ull; };
    l.keyPlane = up(n * keyBytes);
    l.rowPlane = up(n * sizeof(uint32_t));
    l.histBytes = up(histChunks * kSortBins * sizeof(uint32_t));
    l.bytes = 2 * l.keyPlane + 2 * l.rowPlane + l.histBytes + up(scan_workspace_words(histChunks * kSortBins) * sizeof(uint32_t));
    return l;
}

uint32_t sort_key_bytes(const SortCols& cols, uint32_t nCols)
{
    uint32_t kb = 4;
    for (uint32_t c = 0; c < nCols; ++c) if (cols.width[c] == 8) kb = 8;
    return kb;
}

uint32_t sort_passes(const SortCols& cols, uint32_t nCols)
{
    uint32_t p = 0;
    for (uint32_t c = 0; c < nCols; ++c) p += cols.width[c] + (cols.valid[c] ? 1u : 0u);
    return p;
}

namespace {
// one pass: histogram, scan, scatter
template <class K, int MODE>
hipError_t sort_pass(const K* keysIn, const uint32_t* rowsIn, K* keysOut, uint32_t* rowsOut, const uint32_t* valid, uint32_t arg, uint64_t n,
                     const SortLayout& l, uint32_t* hist, uint32_t* sums, hipStream_t s)
{
    constexpr int kHistMode = MODE == kValidBit ? kValidBit : kKeysOut;         // the digit is read the same way whatever goes out
    hipLaunchKernelGGL((k_sort_hist<K, kHistMode>), dim3(l.chunks), dim3(kSortThreads), 0, s, keysIn, rowsIn, valid, arg, n, l.chunkRows, l.chunks, hist);
    const hipError_t e = launch_exclusive_scan_u32(hist, (uint64_t)kSortBins * l.chunks, sums, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_sort_scatter<K, MODE>), dim3(l.chunks), dim3(kSortThreads), 0, s, keysIn, rowsIn, keysOut, rowsOut, valid, arg, n,
                       l.chunkRows, l.chunks, hist);
    return hipGetLastError();
}

template <class K>
hipError_t sort_column(const SortCols& cols, uint32_t c, bool first, uint32_t passesLeft, uint64_t n, const SortLayout& l, K* keys[2],
                       uint32_t* rows[2], uint32_t* perm, int* ri, uint32_t* hist, uint32_t* sums, hipStream_t s)
{
    hipError_t e;
    const unsigned blocks = (unsigned)((n + kSortThreads * 4 - 1) / (kSortThreads * 4));
    hipLaunchKernelGGL(k_sort_keys<K>, dim3(blocks), dim3(kSortThreads), 0, s, cols.p[c], cols.valid[c], cols.width[c], cols.type[c],
                       cols.flags[c], first ? nullptr : rows[*ri], rows[*ri], keys[0], n);
    int ki = 0;
    const uint32_t own = cols.width[c] + (cols.valid[c] ? 1u : 0u);
    for (uint32_t d = 0; d < own; ++d) {
        // the last pass of the call writes the caller's plane
        uint32_t* const out = passesLeft - d == 1 ? perm : rows[*ri ^ 1];
        if (d + 1 < cols.width[c]) e = sort_pass<K, kKeysOut>(keys[ki], rows[*ri], keys[ki ^ 1], out, nullptr, 8 * d, n, l, hist, sums, s);
        else if (d < cols.width[c]) e = sort_pass<K, kRowsOut>(keys[ki], rows[*ri], nullptr, out, nullptr, 8 * d, n, l, hist, sums, s);
        else e = sort_pass<K, kValidBit>(nullptr, rows[*ri], nullptr, out, cols.valid[c], (cols.flags[c] & kSortNullsFirst) ? 0u : 1u, n, l,
                                         hist, sums, s);
        if (e != hipSuccess) return e;
        ki ^= 1; *ri ^= 1;
    }
    return hipSuccess;
}
}  // namespace

hipError_t launch_sort_rows(const SortCols& cols, uint32_t nCols, uint64_t nRows, uint32_t* perm, void* work, hipStream_t s)
{
    if (nRows == 0) return hipSuccess;
    const uint32_t kb = sort_key_bytes(cols, nCols);
    const SortLayout l = sort_layout(nRows, kb);
    char* p = static_cast<char*>(work);
    void* keyPlane[2] = {p, p + l.keyPlane};
    p += 2 * l.keyPlane;
    uint32_t* rows[2] = {reinterpret_cast<uint32_t*>(p), reinterpret_cast<uint32_t*>(p + l.rowPlane)};
    p += 2 * l.rowPlane;
    uint32_t* const hist = reinterpret_cast<uint32_t*>(p);
    uint32_t* const sums = reinterpret_cast<uint32_t*>(p + l.histBytes);
    uint32_t left = sort_passes(cols, nCols);
    int ri = 0;
    for (uint32_t c = nCols; c-- > 0;) {
        hipError_t e;
        const bool first = c + 1 == nCols;
        if (cols.width[c] == 8) {
            unsigned long long* keys[2] = {static_cast<unsigned long long*>(keyPlane[0]), static_cast<unsigned long long*>(keyPlane[1])};
            e = sort_column<unsigned long long>(cols, c, first, left, nRows, l, keys, rows, perm, &ri, hist, sums, s);
        } else {
            uint32_t* keys[2] = {static_cast<uint32_t*>(keyPlane[0]), static_cast<uint32_t*>(keyPlane[1])};
            e = sort_column<uint32_t>(cols, c, first, left, nRows, l, keys, rows, perm, &ri, hist, sums, s);
        }
        if (e != hipSuccess) return e;
        left -= cols.width[c] + (cols.valid[c] ? 1u : 0u);
    }
    return hipSuccess;
}

// the same order on host pointers: sort_key is the kernels' own, the passes are one std::stable_sort per column, last to first
void sort_rows_host(const SortCols& cols, uint32_t nCols, uint64_t nRows, uint32_t* perm)
{
    for (uint64_t i = 0; i < nRows; ++i) perm[i] = (uint32_t)i;
    std::vector<uint64_t> key(nRows);
    std::vector<uint8_t> bin(nRows);
    for (uint32_t c = nCols; c-- > 0;) {
        const uint32_t flip = (cols.flags[c] & kSortNullsFirst) ? 0u : 1u;
        for (uint64_t i = 0; i < nRows; ++i) {
            const bool ok = !cols.valid[c] || valid_bit(cols.valid[c], (uint32_t)i);
            key[i] = ok ? sort_key(cols.type[c], cols.width[c], cols.flags[c], col_elem(cols.p[c], cols.width[c], (uint32_t)i)) : 0ull;
            bin[i] = cols.valid[c] ? (uint8_t)((ok ? 1u : 0u) ^ flip) : 0;
        }
        std::stable_sort(perm, perm + nRows, [&](uint32_t a, uint32_t b) { return bin[a] != bin[b] ? bin[a] < bin[b] : key[a] < key[b]; });
    }
}

}  // namespace hj
