// hj_keys_impl.h -- internal to the key-column family (hj_keys.hip, hj_groups.hip): the hash of a row's key columns
// (MurmurHash3_x86_32 over their words, key_hash2_rows: ONE __host__ __device__ body) and how two elements compare --
// KeyElem, same_bytes and the word walk of a variable-length element. One copy of each for the join and the groups.
#pragma once

#include "hj_columns.h"

namespace hj {

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

constexpr uint32_t kHashLaneRows = 4;                                 // rows per lane, kWave apart: a wavefront owns 256 consecutive rows
constexpr uint32_t kHashBlockRows = kHashLaneRows * kBlock;           // 1024

// ---- the verify step ------------------------------------------------------------------------------------------------
template <class E> __host__ __device__ __forceinline__ bool same_bytes(const E& a, const E& b) { return a == b; }
template <> __host__ __device__ __forceinline__ bool same_bytes<u4>(const u4& a, const u4& b)
{
    return (((a.x ^ b.x) | (a.y ^ b.y)) | ((a.z ^ b.z) | (a.w ^ b.w))) == 0u;
}

// ---- key columns in the Arrow layout: validity planes and variable-length elements (k_key_hash2, k_pairs_verify2) -----
constexpr uint32_t kNullSeed = 0x4E554C4Cu;                           // "NULL": a NULL-keyed row hashes its position, not its columns
constexpr uint32_t kNullWord = 0xFFFFFFFFu;                           // what a NULL contributes in a HJ_KEY_NULLS_EQUAL column

// Word w of a variable-length element, as the hash mixes it and the verify step compares it: its bytes [4w, 4w + 4),
// little-endian, zero behind its end. On the host they are read one by one.
__host__ __device__ __forceinline__ uint32_t var_tail_mask(uint32_t len, uint32_t w)
{
    const uint32_t rem = len - 4u * w;                                // > 0: w < ceil(len / 4)
    return rem < 4u ? (1u << (8u * rem)) - 1u : 0xFFFFFFFFu;
}
__host__ __forceinline__ uint32_t var_word_host(const uint8_t* e, uint32_t len, uint32_t w)
{
    uint32_t k = 0;
    for (uint32_t b = 0; b < 4u && 4u * w + b < len; ++b) k |= (uint32_t)e[4u * w + b] << (8u * b);
    return k;
}
__host__ __device__ __forceinline__ uint32_t var_words_of(uint32_t len) { return len / 4u + ((len & 3u) ? 1u : 0u); }

// On the device the words of ONE element are walked in order through the ALIGNED 32-bit words that hold it: the word that
// holds its first byte up to the one that holds its last, nothing outside them (the header's promise), whatever the
// alignment of the buffer and of the element in it. Word w of the element is a byte-align of the aligned words w and
// w + 1, so every aligned word is loaded once and carried: var_fetch is the load of one step, var_word the arithmetic.
struct VarWords {
    const uint32_t* a;                                                // the aligned word that holds the first byte
    uint32_t sh, last, cur;                                           // the first byte's place in it; the aligned word of the last byte; aligned word w
};
template <bool NT> __device__ __forceinline__ uint32_t var_load(const uint32_t* p) { return NT ? __builtin_nontemporal_load(p) : *p; }
template <bool NT>
__device__ __forceinline__ VarWords var_begin(const void* bytes, uint32_t o0, uint32_t len)
{
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(bytes) + o0;
    VarWords v;
    v.a = reinterpret_cast<const uint32_t*>(a0 & ~(uintptr_t)3);
    v.sh = (uint32_t)(a0 & 3u);
    v.last = len ? (uint32_t)(((uint64_t)v.sh + len - 1u) >> 2) : 0u;
    v.cur = len ? var_load<NT>(v.a) : 0u;                             // an empty element reads nothing
    return v;
}
// the aligned word behind the one carried, where the element reaches into it (on: the element has a word w at all)
template <bool NT>
__device__ __forceinline__ uint32_t var_fetch(const VarWords& v, uint32_t w, bool on) { return on && w + 1u <= v.last ? var_load<NT>(v.a + w + 1u) : 0u; }
__device__ __forceinline__ uint32_t var_word(VarWords& v, uint32_t nxt, uint32_t len, uint32_t w)
{
    const uint32_t k = __builtin_amdgcn_alignbyte(nxt, v.cur, v.sh);  // ({nxt, cur} >> 8 * sh): a misaligned start costs no byte loads
    v.cur = nxt;
    return k & var_tail_mask(len, w);
}

// The validity bits of K rows of one plane. Host: the word of the row, shifted. Device (k_key_hash2's rows: a wavefront
// owns 256 consecutive ones from a multiple of 256, the lane's K = 4 rows 64 apart): the wavefront's eight words are read
// ONCE, by its lanes 0 .. 7 in one load, and handed round -- a word per 32 rows, not a load per row. A word at or behind
// ceil(nRows / 32) is not read and counts as 0: rows behind the end, which store nothing.
template <int K>
__host__ __device__ __forceinline__ void key_valid_bits(const uint32_t* plane, const uint64_t (&at)[K], uint64_t nRows, bool (&ok)[K])
{
#ifdef __HIP_DEVICE_COMPILE__
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t w0 = (at[0] - lane) >> 5, nWords = (nRows + 31u) >> 5;
    uint32_t mine = 0;
    if (lane < 2u * K && w0 + lane < nWords) mine = __builtin_nontemporal_load(plane + w0 + lane);
#pragma unroll
    for (int j = 0; j < K; ++j) ok[j] = (__shfl(mine, 2 * j + (int)(lane >> 5)) >> (lane & 31u)) & 1u;
#else
    (void)nRows;
    for (int j = 0; j < K; ++j) ok[j] = valid_bit(plane, (uint32_t)at[j]);
#endif
}

// One variable-length column of K rows into their running hashes: the K (off[i], off[i + 1]) pairs first, straight, then
// per valid row the length and its words; a NULL row (ok false) mixes nothing here and reads no byte. The device loop
// runs to the lane's own longest element: each step loads the next aligned word of every row that still has words, all
// of them before the first mix.
template <int K>
__host__ __device__ __forceinline__ void key_mix_varlen(const void* bytes, const uint32_t* off, const uint64_t (&row)[K], const bool (&ok)[K],
                                                        uint32_t (&h)[K], uint32_t (&words)[K])
{
    uint32_t o0[K], o1[K], len[K], nW[K], maxW = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) { o0[j] = __builtin_nontemporal_load(off + row[j]); o1[j] = __builtin_nontemporal_load(off + row[j] + 1); }
#ifdef __HIP_DEVICE_COMPILE__
    __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
    for (int j = 0; j < K; ++j) {
        len[j] = ok[j] ? o1[j] - o0[j] : 0u;
        nW[j] = var_words_of(len[j]);
        if (ok[j]) { h[j] = mm3_mix(h[j], len[j]); words[j] += 1u + nW[j]; }
        maxW = nW[j] > maxW ? nW[j] : maxW;
    }
#ifdef __HIP_DEVICE_COMPILE__
    VarWords v[K];
#pragma unroll
    for (int j = 0; j < K; ++j) v[j] = var_begin<true>(bytes, o0[j], len[j]);
    for (uint32_t w = 0; w < maxW; ++w) {
        uint32_t nxt[K];
#pragma unroll
        for (int j = 0; j < K; ++j) nxt[j] = var_fetch<true>(v[j], w, w < nW[j]);
        __builtin_amdgcn_sched_barrier(0);                            // the K loads of a step are in flight together
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (w < nW[j]) h[j] = mm3_mix(h[j], var_word(v[j], nxt[j], len[j], w));
    }
#else
    (void)maxW;
    for (int j = 0; j < K; ++j)
        for (uint32_t w = 0; w < nW[j]; ++w) h[j] = mm3_mix(h[j], var_word_host(static_cast<const uint8_t*>(bytes) + o0[j], len[j], w));
#endif
}

// The join words of K rows: column by column, the width picked by a switch that is uniform on the device. row: the rows
// read (behind the end: the last one); at: their positions in the call, which pick the validity bit and are the word of a
// NULL-keyed row. A column without a plane and without offsets costs its K loads and its mixes, nothing else per row.
// kVar false: no column has offsets (the caller looked), and the word loop with its registers is not compiled in.
template <int K, bool kVar>
__host__ __device__ __forceinline__ void key_hash2_rows(const KeyCols2& cols, uint32_t nCols, const uint64_t (&row)[K], const uint64_t (&at)[K],
                                                        uint64_t nRows, uint32_t mask, uint32_t (&word)[K])
{
    uint32_t h[K], words[K];
    bool nullKey[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { h[j] = 0; words[j] = 0; nullKey[j] = false; }
#pragma unroll
    for (uint32_t c = 0; c < kKeyMaxCols; ++c) {
        if (c >= nCols) continue;
        bool ok[K];
#pragma unroll
        for (int j = 0; j < K; ++j) ok[j] = true;
        if (cols.valid[c]) key_valid_bits<K>(cols.valid[c], at, nRows, ok);
        if (kVar && cols.off[c]) {
            key_mix_varlen<K>(cols.p[c], cols.off[c], row, ok, h, words);
        } else {
            uint32_t t[K];                                            // a NULL's element is read (it exists) and its mix thrown away
#pragma unroll
            for (int j = 0; j < K; ++j) t[j] = h[j];
            switch (cols.width[c]) {
                case 1: key_mix_col<1, K>(cols.p[c], row, t); break;
                case 2: key_mix_col<2, K>(cols.p[c], row, t); break;
                case 4: key_mix_col<4, K>(cols.p[c], row, t); break;
                case 8: key_mix_col<8, K>(cols.p[c], row, t); break;
                default: key_mix_col<16, K>(cols.p[c], row, t); break;
            }
            const uint32_t n = cols.width[c] <= 4 ? 1u : cols.width[c] / 4u;
#pragma unroll
            for (int j = 0; j < K; ++j) { h[j] = ok[j] ? t[j] : h[j]; words[j] += ok[j] ? n : 0u; }
        }
        if (cols.valid[c]) {
            const bool nullsEqual = (cols.flags[c] & kKeyNullsEqual) != 0u;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if (ok[j]) continue;
                if (nullsEqual) { h[j] = mm3_mix(h[j], kNullWord); words[j] += 1u; }
                else nullKey[j] = true;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
        word[j] = (nullKey[j] ? mm3_final(mm3_mix(kNullSeed, (uint32_t)at[j]), 4u) : mm3_final(h[j], 4u * words[j])) & mask;
}

}  // namespace hj
