// hj_groups.hip -- the rows of ONE table grouped by their key columns for gfx950 (MI355X): hj_key_groups_dev /
// hj_key_groups_host. The hash is the join's key_hash2_rows, the element compare its same_bytes and its var_* word walk:
// hj_keys_impl.h, which this file shares with hj_keys.hip.
//
// What comes out: rep[i] = the lowest row whose key equals row i's (column equality as in the verify step), the first rows
// (rep[i] == i) ascending, and group[i] = the position of rep[i] among them -- a dense id in order of first occurrence.
// A NULL-keyed row is in no group: HJ_NO_ROW in both planes, counted apart, its key bytes never compared.
//
// The table: a power of two of at least 2 * nRows slots of 8 bytes, (join word << 32) | row, all ones = EMPTY, filled with
// EMPTY on the stream at the start of every call. (Above 2^31 rows it stays at 2^32 slots -- a slot number is one word of
// rep -- and slot 0xFFFFFFFF, which would read as HJ_NO_ROW there, is left out of every probe sequence.) The home slot is
// the join word spread by a multiplication, so that a weak keyMask (a few distinct words) gives a few separate clusters,
// not one.
//
//   k_groups_insert   The hash kernel's shape and row layout (1024 rows per workgroup, four per lane, 64 apart), so the
//                     column loads stay coalesced; the lane computes its rows' join words, loads their four home slots
//                     together, then walks row by row, linear probing:
//                       EMPTY           CAS the row's own word in. A lost CAS returns what the slot now holds, and the
//                                       lane looks at that -- the same slot again, no second load.
//                       another word    next slot.
//                       the same word   the real key of row i against the key of the row in the slot (key_rows_equal:
//                                       random element reads, once per row that is not its key's first). Different: a
//                                       word collision, next slot. Equal: this is the key's slot; atomicMin only while
//                                       the row read from the slot is above i -- under a hot key almost every row sees
//                                       a lower one and issues no atomic, as mark_r_row does for the R marks.
//                     rep[i] = the SLOT the row ended on. Probe steps, word collisions and NULL-keyed rows are summed per
//                     workgroup and added with one atomic each.
//   k_groups_resolve  a launch of its own, so the table is final: rep[i] = row(table[rep[i]]) in place, bit i of the
//                     first-row plane where rep[i] == i (a ballot per 64 rows, two word stores, no atomics), and the
//                     popcount of every plane word for the ranks.
//   (first rows)      launch_r_sweep over the plane: the ordered compaction of hj_r_marks.hip, cut at the capacity.
//   (ranks)           launch_exclusive_scan_u32 over the words' popcounts; rank(r) = pre[r >> 5] + popc(bits below r).
//   k_groups_ids      group[i] = rank(rep[i]).
//
// Why the result does not depend on scheduling. A slot goes EMPTY -> occupied once (the CAS) and an occupied slot changes
// only by atomicMin between words that share their upper half: it never changes its key. All rows of a key walk one probe
// sequence (same word, same home) and stop at the first slot holding their key; a slot they pass holds another key for
// good. Two rows of a key cannot stop on different slots: the later slot's occupant passed the earlier one, so the earlier
// held another key then and holds it still. So a key has ONE slot, whatever the order, and its content ends as the minimum
// over its rows. Which slot that is depends on the order; nothing returned does.
//
// Reading the table while other XCDs update it: slots are read with RELAXED AGENT-SCOPE ATOMIC LOADS (decided: no plain
// load of a slot in the insert kernel), which L2 serves coherently. What a load returns may still be old by the time it
// is used, and that is harmless: slot contents are monotone. EMPTY read where the slot is taken: the CAS fails and returns
// the occupant. A row r read where a lower one now sits: r is still a row of that slot's key, so the compare gives the
// same answer, and the atomicMin is issued or not by r against i -- not issuing it needs r < i, which a lower occupant
// only confirms. The key columns are inputs and are read plainly.
//
// No lane waits for another: no lock, no spin on a value. The probe loop is bounded by the slot count; a row that exceeds
// it sets the failure word (hj_key_groups_info out[7]) and stops with HJ_NO_ROW.
// What it does NOT do: the table lives for one call (no keys arriving in slices); the rows of a lane are walked one after
// the other, so a lane's probes overlap only with those of the other wavefronts.

#include "hj_keys_impl.h"

namespace hj {

namespace {

constexpr unsigned long long kGroupsEmpty = ~0ull;
constexpr uint32_t kGroupsSpread = 0x9E3779B1u;                       // 2^32 / golden ratio: consecutive words land far apart
constexpr uint32_t kGroupsWaves = kBlock / kWave;
// ctr: [0] probe steps beyond the home slot, [1] word collisions, [2] NULL-keyed rows, [3] the failure word
constexpr uint32_t kGroupsCtrWords = 4;

// slot 0xFFFFFFFF exists only in a table of 2^32 slots and is never used: in rep it would read as HJ_NO_ROW
__host__ __device__ __forceinline__ uint32_t groups_usable(uint32_t slot) { return slot == kNoRow ? 0u : slot; }
__host__ __device__ __forceinline__ uint32_t groups_home(uint32_t word, uint32_t shift) { return groups_usable((word * kGroupsSpread) >> shift); }
__host__ __device__ __forceinline__ uint32_t groups_next(uint32_t slot, uint32_t slotMask) { return groups_usable((slot + 1u) & slotMask); }

// Which of K rows are NULL-keyed -- some column WITHOUT the flag is NULL in them: the header's definition, which
// key_hash2_rows applies inside the hash and keeps to itself. The validity words are read as the hash reads them
// (key_valid_bits: the wavefront's eight words in one load), a second time and from cache.
template <int K>
__host__ __device__ __forceinline__ void key_null_rows(const KeyCols2& cols, uint32_t nCols, const uint64_t (&at)[K], uint64_t nRows, bool (&nullKey)[K])
{
#pragma unroll
    for (int j = 0; j < K; ++j) nullKey[j] = false;
#pragma unroll
    for (uint32_t c = 0; c < kKeyMaxCols; ++c) {
        if (c >= nCols || !cols.valid[c] || (cols.flags[c] & kKeyNullsEqual)) continue;     // kernel arguments: uniform
        bool ok[K];
        key_valid_bits<K>(cols.valid[c], at, nRows, ok);
#pragma unroll
        for (int j = 0; j < K; ++j) nullKey[j] = nullKey[j] || !ok[j];
    }
}

// ---- the key of row a against the key of row b of the same columns ------------------------------------------------------
template <int W>
__host__ __device__ __forceinline__ bool key_elems_equal(const void* col, uint64_t a, uint64_t b)
{
    const KeyElem<W>* const p = static_cast<const KeyElem<W>*>(col);
    return same_bytes<KeyElem<W>>(p[a], p[b]);
}

// variable length: the same length, then the words of both elements side by side (the device walks aligned words)
__host__ __device__ __forceinline__ bool key_varlen_equal(const void* bytes, const uint32_t* off, uint64_t a, uint64_t b)
{
    const uint32_t a0 = off[a], len = off[a + 1] - a0, b0 = off[b];
    if (len != off[b + 1] - b0) return false;
    const uint32_t nW = var_words_of(len);
#ifdef __HIP_DEVICE_COMPILE__
    VarWords va = var_begin<false>(bytes, a0, len), vb = var_begin<false>(bytes, b0, len);
    for (uint32_t w = 0; w < nW; ++w) {
        const uint32_t na = var_fetch<false>(va, w, true), nb = var_fetch<false>(vb, w, true);
        if (var_word(va, na, len, w) != var_word(vb, nb, len, w)) return false;
    }
#else
    const uint8_t* const p = static_cast<const uint8_t*>(bytes);
    for (uint32_t w = 0; w < nW; ++w)
        if (var_word_host(p + a0, len, w) != var_word_host(p + b0, len, w)) return false;
#endif
    return true;
}

// Column equality as the verify step defines it, for two rows of one side. Neither row is NULL-keyed (the callers looked),
// so two NULLs meet only in a column with the flag; the flag is asked all the same.
template <bool kVar>
__host__ __device__ __forceinline__ bool key_rows_equal(const KeyCols2& cols, uint32_t nCols, uint64_t a, uint64_t b)
{
    for (uint32_t c = 0; c < kKeyMaxCols; ++c) {
        if (c >= nCols) break;
        if (cols.valid[c]) {
            const bool okA = (cols.valid[c][a >> 5] >> (a & 31u)) & 1u, okB = (cols.valid[c][b >> 5] >> (b & 31u)) & 1u;
            if (!okA || !okB) {
                if (!okA && !okB && (cols.flags[c] & kKeyNullsEqual)) continue;
                return false;
            }
        }
        bool same;
        if (kVar && cols.off[c]) same = key_varlen_equal(cols.p[c], cols.off[c], a, b);
        else switch (cols.width[c]) {
            case 1: same = key_elems_equal<1>(cols.p[c], a, b); break;
            case 2: same = key_elems_equal<2>(cols.p[c], a, b); break;
            case 4: same = key_elems_equal<4>(cols.p[c], a, b); break;
            case 8: same = key_elems_equal<8>(cols.p[c], a, b); break;
            default: same = key_elems_equal<16>(cols.p[c], a, b); break;
        }
        if (!same) return false;
    }
    return true;
}

struct GroupsTable {
    unsigned long long* slots;
    uint32_t slotMask, shift;                                         // slots - 1; 32 - log2(slots)
    uint64_t bound;                                                   // the slot count: the most steps a row may take
};
inline GroupsTable groups_table(unsigned long long* slots, uint64_t count)
{
    uint32_t bits = 0;
    while ((1ull << bits) < count) ++bits;
    return GroupsTable{slots, (uint32_t)(count - 1), 32u - bits, count};
}

__device__ __forceinline__ unsigned long long groups_load(const unsigned long long* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// v summed over the workgroup into thread 0 (the others get their wavefront's part); red: kGroupsWaves words of LDS
__device__ __forceinline__ unsigned long long groups_block_sum(unsigned long long v, unsigned long long* red)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        v = 0;
#pragma unroll
        for (uint32_t k = 0; k < kGroupsWaves; ++k) v += red[k];
    }
    return v;
}

}  // namespace

// Two instances, as k_key_hash2 has: kVar = false when no column has offsets, so that fixed columns carry neither word loop.
template <bool kVar>
__global__ void __launch_bounds__(kBlock)
k_groups_insert(KeyCols2 cols, uint32_t nCols, uint64_t nRows, uint32_t mask, GroupsTable t, uint32_t* __restrict__ rep,
                unsigned long long* __restrict__ ctr)
{
    __shared__ unsigned long long red[3][kGroupsWaves];
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * kHashBlockRows + w * (kHashLaneRows * kWave) + lane;     // the lane's first row
    uint64_t row[kHashLaneRows], at[kHashLaneRows];
    uint32_t word[kHashLaneRows];
    bool nullKey[kHashLaneRows];
#pragma unroll
    for (uint32_t j = 0; j < kHashLaneRows; ++j) {
        at[j] = i0 + j * kWave;
        row[j] = at[j] < nRows ? at[j] : nRows - 1;                   // a row behind the end reads the last one and inserts nothing
    }
    key_hash2_rows<(int)kHashLaneRows, kVar>(cols, nCols, row, at, nRows, mask, word);
    key_null_rows<(int)kHashLaneRows>(cols, nCols, at, nRows, nullKey);

    // the four home slots, in flight together (a row that inserts nothing reads a slot that exists all the same)
    uint32_t slot[kHashLaneRows];
    unsigned long long cur[kHashLaneRows];
#pragma unroll
    for (uint32_t j = 0; j < kHashLaneRows; ++j) { slot[j] = groups_home(word[j], t.shift); cur[j] = groups_load(t.slots + slot[j]); }

    unsigned long long steps = 0, collisions = 0, nulls = 0;
    bool failed = false;
#pragma unroll
    for (uint32_t j = 0; j < kHashLaneRows; ++j) {
        if (at[j] >= nRows) continue;
        uint32_t res = kNoRow;
        if (nullKey[j]) ++nulls;
        else {
            const uint32_t i = (uint32_t)at[j];
            const unsigned long long mine = ((unsigned long long)word[j] << 32) | i;
            uint32_t s = slot[j];
            unsigned long long c = cur[j];
            uint64_t n = 0;                                           // steps beyond the home slot
            for (;;) {
                if (c == kGroupsEmpty) {
                    const unsigned long long old = atomicCAS(t.slots + s, kGroupsEmpty, mine);
                    if (old == kGroupsEmpty) { res = s; break; }
                    c = old;                                          // lost: the slot is taken for good -- look at its occupant
                }
                if ((uint32_t)(c >> 32) == word[j]) {
                    const uint32_t r = (uint32_t)c;
                    if (key_rows_equal<kVar>(cols, nCols, i, r)) {
                        if (r > i) atomicMin(t.slots + s, mine);      // a lower row read: no atomic, now or later
                        res = s;
                        break;
                    }
                    ++collisions;
                }
                if (++n >= t.bound) { failed = true; break; }         // cannot happen in a table with more slots than rows
                s = groups_next(s, t.slotMask);
                c = groups_load(t.slots + s);
            }
            steps += n;
        }
        rep[at[j]] = res;
    }
    if (failed) atomicMax(ctr + 3, 1ull);

    steps = groups_block_sum(steps, red[0]);
    collisions = groups_block_sum(collisions, red[1]);
    nulls = groups_block_sum(nulls, red[2]);
    if (threadIdx.x == 0) {
        if (steps) atomicAdd(ctr + 0, steps);
        if (collisions) atomicAdd(ctr + 1, collisions);
        if (nulls) atomicAdd(ctr + 2, nulls);
    }
}

// rep: slots in, rows out. plane: ceil(nRows / 32) words, every one of them written here; pops: their popcounts (null: no ids wanted).
__global__ void __launch_bounds__(kBlock)
k_groups_resolve(const unsigned long long* __restrict__ slots, uint32_t* __restrict__ rep, uint64_t nRows, uint32_t* __restrict__ plane,
                 uint32_t* __restrict__ pops)
{
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * kHashBlockRows + w * (kHashLaneRows * kWave) + lane;
    const uint64_t nWords = (nRows + 31u) >> 5;
    uint32_t s[kHashLaneRows];
    unsigned long long v[kHashLaneRows];
#pragma unroll
    for (uint32_t j = 0; j < kHashLaneRows; ++j) { const uint64_t i = i0 + j * kWave; s[j] = i < nRows ? __builtin_nontemporal_load(rep + i) : kNoRow; }
#pragma unroll
    for (uint32_t j = 0; j < kHashLaneRows; ++j) v[j] = slots[s[j] == kNoRow ? 0u : s[j]];       // a row without a slot reads one that exists
#pragma unroll
    for (uint32_t j = 0; j < kHashLaneRows; ++j) {
        const uint64_t i = i0 + j * kWave;
        const uint32_t r = s[j] == kNoRow ? kNoRow : (uint32_t)v[j];
        if (i < nRows) rep[i] = r;
        const unsigned long long firsts = __ballot(i < nRows && r == (uint32_t)i);
        const uint64_t wi = ((i - lane) >> 5) + lane;                 // lanes 0 and 1: the two words of the wavefront's 64 rows
        if (lane < 2u && wi < nWords) {
            const uint32_t bits = (uint32_t)(firsts >> (32u * lane));
            plane[wi] = bits;
            if (pops) pops[wi] = (uint32_t)__popc(bits);
        }
    }
}

// pre: the exclusive scan of the plane words' popcounts
__global__ void __launch_bounds__(kBlock)
k_groups_ids(const uint32_t* __restrict__ rep, uint64_t nRows, const uint32_t* __restrict__ plane, const uint32_t* __restrict__ pre,
             uint32_t* __restrict__ group)
{
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * kHashBlockRows + w * (kHashLaneRows * kWave) + lane;
    uint32_t r[kHashLaneRows], bits[kHashLaneRows], below[kHashLaneRows];
#pragma unroll
    for (uint32_t j = 0; j < kHashLaneRows; ++j) { const uint64_t i = i0 + j * kWave; r[j] = i < nRows ? __builtin_nontemporal_load(rep + i) : kNoRow; }
#pragma unroll
    for (uint32_t j = 0; j < kHashLaneRows; ++j) {
        const uint32_t wi = r[j] == kNoRow ? 0u : r[j] >> 5;          // word 0 exists
        bits[j] = plane[wi]; below[j] = pre[wi];
    }
#pragma unroll
    for (uint32_t j = 0; j < kHashLaneRows; ++j) {
        const uint64_t i = i0 + j * kWave;
        if (i < nRows) group[i] = r[j] == kNoRow ? kNoRow : below[j] + (uint32_t)__popc(bits[j] & ((1u << (r[j] & 31u)) - 1u));
    }
}

// ---- the workspace of a call: the table, the first-row plane, its popcounts with their scan, the sweep's counts ---------
uint64_t key_groups_slots(uint64_t nRows)
{
    uint64_t slots = 2;
    while (slots < 2 * nRows && slots < (1ull << 32)) slots <<= 1;
    return slots;
}

namespace {
struct GroupsWork { unsigned long long* table; uint32_t *plane, *pre, *sweep; size_t bytes; };
GroupsWork groups_carve(void* base, uint64_t nRows)
{
    const uint64_t nWords = (nRows + 31) >> 5;
    char* p = static_cast<char*>(base);
    GroupsWork wk;
    size_t at = 0;
    const auto take = [&](size_t bytes) { char* q = p + at; at += (bytes + 255) & ~(size_t)255; return q; };
    wk.table = reinterpret_cast<unsigned long long*>(take(key_groups_slots(nRows) * sizeof(unsigned long long)));
    wk.plane = reinterpret_cast<uint32_t*>(take(nWords * sizeof(uint32_t)));
    wk.pre = reinterpret_cast<uint32_t*>(take((nWords + 1 + scan_workspace_words(nWords + 1)) * sizeof(uint32_t)));
    wk.sweep = reinterpret_cast<uint32_t*>(take(r_sweep_count_words(nRows) * sizeof(uint32_t)));
    wk.bytes = at;
    return wk;
}
}  // namespace

size_t key_groups_work_bytes(uint64_t nRows) { return groups_carve(nullptr, nRows).bytes; }
const uint32_t* key_groups_total(const void* work, uint64_t nRows) { return groups_carve(const_cast<void*>(work), nRows).sweep + r_sweep_blocks(nRows); }

hipError_t launch_key_groups(const KeyCols2& cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint32_t* rep, uint32_t* group,
                             uint32_t* firstRows, uint64_t capacity, void* work, unsigned long long* ctr, hipStream_t s)
{
    if (nRows == 0) return hipSuccess;
    const GroupsWork wk = groups_carve(work, nRows);
    const uint64_t slots = key_groups_slots(nRows), nWords = (nRows + 31) >> 5;
    const GroupsTable t = groups_table(wk.table, slots);
    hipError_t e;
    if ((e = hipMemsetAsync(wk.table, 0xFF, slots * sizeof(unsigned long long), s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(ctr, 0, kGroupsCtrWords * sizeof(unsigned long long), s)) != hipSuccess) return e;
    const dim3 grid((uint32_t)((nRows + kHashBlockRows - 1) / kHashBlockRows));               // nRows <= 2^32 - 2: <= 2^22 workgroups
    bool var = false;
    for (uint32_t c = 0; c < nCols; ++c) var = var || cols.off[c];
    if (var) hipLaunchKernelGGL(k_groups_insert<true>, grid, dim3(kBlock), 0, s, cols, nCols, nRows, mask, t, rep, ctr);
    else hipLaunchKernelGGL(k_groups_insert<false>, grid, dim3(kBlock), 0, s, cols, nCols, nRows, mask, t, rep, ctr);
    hipLaunchKernelGGL(k_groups_resolve, grid, dim3(kBlock), 0, s, wk.table, rep, nRows, wk.plane, group ? wk.pre : nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // the first rows: the plane's set bits in ascending order, cut at the capacity; their number ends behind the block counts
    if ((e = launch_r_sweep(RMarks{wk.plane, 0u, (uint32_t)nRows}, true, firstRows, capacity, wk.sweep, s)) != hipSuccess) return e;
    if (!group) return hipSuccess;
    if ((e = hipMemsetAsync(wk.pre + nWords, 0, sizeof(uint32_t), s)) != hipSuccess) return e;
    if ((e = launch_exclusive_scan_u32(wk.pre, nWords + 1, wk.pre + nWords + 1, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_groups_ids, grid, dim3(kBlock), 0, s, rep, nRows, wk.plane, wk.pre, group);
    return hipGetLastError();
}

// The host twin: the same hash and compare bodies around a sequential table. Rows go in ascending, so the row that takes a
// slot is its key's lowest and the first rows come out in order by themselves.
void key_groups_host(const KeyCols2& cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint32_t* rep, uint32_t* group, uint32_t* firstRows,
                     uint64_t capacity, uint64_t out[8])
{
    for (int k = 0; k < 8; ++k) out[k] = 0;
    if (nRows == 0) return;
    const uint64_t slots = key_groups_slots(nRows);
    unsigned long long* const table = new unsigned long long[slots];
    const GroupsTable t = groups_table(table, slots);
    uint32_t* const ids = group ? group : new uint32_t[nRows];        // the id of a first row, read back by the rows behind it
    for (uint64_t k = 0; k < slots; ++k) table[k] = kGroupsEmpty;
    uint64_t groups = 0, nulls = 0;
    for (uint64_t i = 0; i < nRows; ++i) {
        const uint64_t row[1] = {i};
        uint32_t word[1];
        bool nullKey[1];
        key_hash2_rows<1, true>(cols, nCols, row, row, nRows, mask, word);
        key_null_rows<1>(cols, nCols, row, nRows, nullKey);
        if (nullKey[0]) { rep[i] = ids[i] = kNoRow; ++nulls; continue; }
        uint32_t s = groups_home(word[0], t.shift);
        for (;; s = groups_next(s, t.slotMask)) {
            if (table[s] == kGroupsEmpty) {
                table[s] = ((unsigned long long)word[0] << 32) | (uint32_t)i;
                if (groups < capacity) firstRows[groups] = (uint32_t)i;
                rep[i] = (uint32_t)i; ids[i] = (uint32_t)groups++;
                break;
            }
            const uint32_t r = (uint32_t)table[s];
            if ((uint32_t)(table[s] >> 32) == word[0] && key_rows_equal<true>(cols, nCols, i, r)) { rep[i] = r; ids[i] = ids[r]; break; }
        }
    }
    delete[] table;
    if (!group) delete[] ids;
    out[0] = groups; out[1] = groups < capacity ? groups : capacity; out[3] = nulls;
}

}  // namespace hj
