// hj_columns.h -- the relational layer's column code: validity and mark bits, gather, key columns, groups, join
// conditions and as-of (how two elements compare and order), sort keys, range joins, the aggregates over a pair list, and
// the window functions along a permutation.
// Column descriptors as the kernels take them, the element helpers host and device share, and the launchers.
#pragma once

#include "hj_common.h"
#include "hj_pairs.h"

namespace hj {

// ---- validity and mark bits: one bit per row, bit (i & 31) of word i >> 5 ----
// THE test of a bit: of a word that is held already, and of a plane. Every host loop and the kernels of hj_agg, hj_gather,
// hj_sort and hj_prj_agg go through them. Four device functions keep the expression written out, because through the
// helpers their kernels compile to other code (registers, block placement; tools/asm_diff.py): verify_col2 / verify_varlen
// (k_pairs_verify2), the term loops of k_pairs_where and asof_pairs, and key_rows_equal (k_groups_insert); so does the
// device branch of key_valid_bits, which reads eight words once per wavefront.
__host__ __device__ __forceinline__ bool word_bit(uint32_t word, uint32_t i) { return (word >> (i & 31u)) & 1u; }
__host__ __device__ __forceinline__ bool valid_bit(const uint32_t* plane, uint32_t i) { return word_bit(plane[i >> 5], i); }
// the host loops' mark of row i (the kernels mark with atomics: mark_r_row)
inline void set_mark_bit(uint32_t* plane, uint32_t i) { plane[i >> 5] |= 1u << (i & 31u); }

// ---- gather through a row map (defined in hj_gather.hip) ---------------------
// One column of hj_gather_dev as the kernel takes it (hj_gather_col, include/htm_hashjoin.h, field for field), and the
// columns of a call, passed by value in the kernel arguments.
constexpr uint32_t kGatherMaxCols = 8;        // HJ_GATHER_MAX_COLS
struct GatherCol { const void* src; void* dst; uint32_t width, reserved; uint64_t fill[2]; };
struct GatherCols { GatherCol col[kGatherMaxCols]; };
// dst_c[k] = src_c[map[k] - rowBase] for k in [0, nRows) and c in [0, nCols); an entry that is HJ_NO_ROW, or that lies at or
// behind srcRows once the base is off, reads nothing and gives the column's fill. valid (may be null): one bit per row,
// whole words up to ceil(nRows / 32). counts[0] += the HJ_NO_ROW entries, counts[1] += the out-of-range ones. The caller
// has checked widths, alignment and nRows, srcRows <= 2^32 - 1.
hipError_t launch_gather(const uint32_t* map, uint64_t nRows, uint32_t rowBase, uint64_t srcRows, const GatherCols& cols, uint32_t nCols,
                         uint32_t* valid, unsigned long long* counts, hipStream_t s);
// The same on columns in the Arrow layout (hj_gather_col2, include/htm_hashjoin.h, field for field; defined in
// hj_gather_cols.hip): a source validity plane and 32-bit offsets per column, both optional. Columns that are fixed and
// have neither plane go through launch_gather as they are. work: the context's workspace for the variable-length columns
// of a call, which run one behind the other -- gather2_work_words(nRows) 32-bit words: the scan's own words, then one
// 64-bit partial sum per workgroup. totals: kGatherMaxCols 64-bit words, written here (0 for a fixed column): the bytes
// the rows of column c take. The caller has checked what the header says hj_gather2_dev refuses.
struct GatherCol2 { const void* src; void* dst; const uint32_t* srcOff; uint32_t* dstOff; const uint32_t* srcValid; uint32_t* dstValid;
                    uint64_t capacity; uint32_t width, flags; uint64_t fill[2]; };
struct GatherCols2 { GatherCol2 col[kGatherMaxCols]; };
size_t gather2_work_words(uint64_t nRows);
hipError_t launch_gather2(const uint32_t* map, uint64_t nRows, uint32_t rowBase, uint64_t srcRows, const GatherCols2& cols, uint32_t nCols,
                          uint32_t* valid, unsigned long long* counts, unsigned long long* totals, uint32_t* work, hipStream_t s);

// ---- joins on real key columns (defined in hj_keys.hip) ----------------------
// The key columns of a call as the kernels take them, by value in the kernel arguments: the hash reads one side
// (KeyCols2), the verify step both (KeyCols2SR). They are hj_key_col2's (include/htm_hashjoin.h): per column and side the
// values (fixed width) or the bytes buffer (width 0), the rows + 1 offsets of a variable-length column (else null) and the
// validity plane (null: no NULLs); flags: HJ_KEY_NULLS_EQUAL. An hj_key_col is the same column with null offsets, null
// planes and flags 0: hj_key_hash_dev, hj_key_hash_host and hj_pairs_verify_dev fill the descriptor that way.
// launch_key_hash2: out[i] = the join word of row i (the header's hash over the row's key columns, & mask) as an 8-byte
// tuple. mask is the effective one (never 0). nRows is also what bounds the validity words the hash reads: ceil(nRows / 32).
// launch_pairs_verify2: candidate pairs (mapS[k] - sRowBase, mapR[k]) -> the pairs whose key columns are equal as the header
// defines it, to `to.out` as the pairs kernels write theirs (its cursor: two 64-bit words, zeroed before the launch: kept
// pairs, then the candidates dropped as HJ_NO_ROW or outside sRows / rRows, which are never dereferenced). Every kept pair
// sets bit s of to.sMarks and bit r of to.rMarks.
// The caller has checked what the header says the entry points refuse, and nRows, nPairs <= 2^32 - 1.
constexpr uint32_t kKeyMaxCols = 4;           // HJ_KEY_MAX_COLS
struct KeyCols2 { const void* p[kKeyMaxCols]; const uint32_t* off[kKeyMaxCols]; const uint32_t* valid[kKeyMaxCols];
                  uint32_t width[kKeyMaxCols], flags[kKeyMaxCols]; };
struct KeyCols2SR { const void* s[kKeyMaxCols]; const void* r[kKeyMaxCols]; const uint32_t* sOff[kKeyMaxCols]; const uint32_t* rOff[kKeyMaxCols];
                    const uint32_t* sValid[kKeyMaxCols]; const uint32_t* rValid[kKeyMaxCols]; uint32_t width[kKeyMaxCols], flags[kKeyMaxCols]; };
constexpr uint32_t kKeyNullsEqual = 1u;       // HJ_KEY_NULLS_EQUAL
hipError_t launch_key_hash2(const KeyCols2& cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint64_t* out, hipStream_t s);
void key_hash2_host(const KeyCols2& cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint64_t* out);   // the same body in a host loop
hipError_t launch_pairs_verify2(const PairList& in, const KeyCols2SR& cols, uint32_t nCols, const PairSink& to, hipStream_t s);

// ---- rows of one table grouped by their key columns (defined in hj_groups.hip) ----
// launch_key_groups: rep[i] = the lowest row with row i's key (kNoRow: NULL-keyed), firstRows = the rows with rep[i] == i,
// ascending, cut at `capacity` (null with capacity 0), group[i] = the position of rep[i] among them (null: not wanted).
// work: key_groups_work_bytes(nRows) bytes -- the table of key_groups_slots(nRows) 8-byte slots, filled with EMPTY here on
// s, the first-row plane, its popcounts and their scan, the sweep's counts; key_groups_total: where the number of groups
// lies in it after the call (one 32-bit word). ctr: four 64-bit words, zeroed here -- probe steps beyond the home slot, word
// collisions, NULL-keyed rows, the failure word. mask is the effective one (never 0). The caller has checked what the
// header says the entry point refuses, and nRows <= 2^32 - 2.
uint64_t key_groups_slots(uint64_t nRows);
size_t key_groups_work_bytes(uint64_t nRows);
const uint32_t* key_groups_total(const void* work, uint64_t nRows);
hipError_t launch_key_groups(const KeyCols2& cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint32_t* rep, uint32_t* group,
                             uint32_t* firstRows, uint64_t capacity, void* work, unsigned long long* ctr, hipStream_t s);
// the same hash and compare bodies around a sequential table; out: hj_key_groups_host's
void key_groups_host(const KeyCols2& cols, uint32_t nCols, uint64_t nRows, uint32_t mask, uint32_t* rep, uint32_t* group, uint32_t* firstRows,
                     uint64_t capacity, uint64_t out[8]);

// ---- join conditions beyond equality (defined in hj_where.hip) ----------------
// The terms of a call as the kernel takes them, by value in the kernel arguments (hj_where_term, include/htm_hashjoin.h):
// term t holds for the pair (s, r) when s[t][s] op[t] r[t][r], both elements of width[t] bytes read as type[t], and neither
// is NULL (sValid / rValid: the validity plane of that side, null: no NULLs).
constexpr uint32_t kWhereMaxTerms = 4;        // HJ_WHERE_MAX_TERMS
constexpr uint32_t kCmpEq = 0, kCmpNe = 1, kCmpLt = 2, kCmpLe = 3, kCmpGt = 4, kCmpGe = 5;     // hj_cmp_op
constexpr uint32_t kValUint = 0, kValInt = 1, kValFloat = 2;                                  // hj_val_type
struct WhereTerms { const void* s[kWhereMaxTerms]; const void* r[kWhereMaxTerms]; const uint32_t* sValid[kWhereMaxTerms];
                    const uint32_t* rValid[kWhereMaxTerms]; uint32_t width[kWhereMaxTerms], type[kWhereMaxTerms], op[kWhereMaxTerms]; };
// Pairs (mapS[k] - sRowBase, mapR[k]) -> the pairs whose terms all hold, to `to.out` as launch_pairs_verify2 writes its kept pairs
// (its cursor: two 64-bit words, zeroed before the launch: kept pairs, then the pairs dropped as HJ_NO_ROW or outside sRows /
// rRows, which are never dereferenced); the marks as there. The caller has checked the terms and nPairs <= 2^32 - 1.
hipError_t launch_pairs_where(const PairList& in, const WhereTerms& terms, uint32_t nTerms, const PairSink& to, hipStream_t s);
// the same pairs in a host loop over host pointers, the kept ones in input order; info: kept, written, 0, dropped (may be null)
void pairs_where_host(const PairList& in, const WhereTerms& terms, uint32_t nTerms, const PairSink& to, uint64_t* info);

// What the condition step (hj_where.hip) and the as-of step (hj_asof.hip) share: how two elements compare, how one orders,
// and a term's loads for the lane's pairs of the pair-filter frame.
// the raw word of a FLOAT element as a double: binary32 widens exactly
__host__ __device__ __forceinline__ double where_real(uint64_t raw, uint32_t width)
{
    return width == 4u ? (double)__builtin_bit_cast(float, (uint32_t)raw) : __builtin_bit_cast(double, raw);
}

// Whether  a OP b  holds, a and b the zero-extended raw words of two valid elements of `width` bytes read as `type`.
// Unordered (a NaN on either side): lt and eq are false, so EQ, LT and LE fail by themselves and NE holds.
__host__ __device__ __forceinline__ bool where_holds(uint32_t type, uint32_t width, uint32_t op, uint64_t a, uint64_t b)
{
    bool lt, eq, un = false;
    if (type == kValFloat) {
        const double x = where_real(a, width), y = where_real(b, width);
        lt = x < y; eq = x == y; un = x != x || y != y;
    } else {
        // INT: sign-extended from its width, then the sign bit flipped -- the order of the signed values as unsigned ones
        const uint32_t sh = type == kValInt ? 64u - 8u * width : 0u;
        const uint64_t flip = type == kValInt ? 1ull << 63 : 0ull;
        const uint64_t x = (uint64_t)((int64_t)(a << sh) >> sh) ^ flip, y = (uint64_t)((int64_t)(b << sh) >> sh) ^ flip;
        lt = x < y; eq = x == y;
    }
    switch (op) {
        case kCmpEq: return eq;
        case kCmpNe: return !eq;
        case kCmpLt: return lt;
        case kCmpLe: return lt || eq;
        case kCmpGt: return !(lt || eq || un);
        default: return !(lt || un);                                  // kCmpGe
    }
}

// The order key of the as-of step: the zero-extended raw word of a valid element that is no NaN -> an unsigned 64-bit word
// that orders as the values do and is equal exactly where where_holds calls two values equal. Integers: where_holds's
// sign-extend and flip. Floats: widened to double, -0.0 taken for +0.0, then the bits folded -- a negative's all
// complemented, a positive's sign bit set -- so that negatives order below positives. The forward ops (LT, LE: the SMALLEST
// R value is wanted) complement the key: every kernel takes a maximum.
__host__ __device__ __forceinline__ uint64_t asof_key(uint32_t type, uint32_t width, uint32_t op, uint64_t raw)
{
    uint64_t key;
    if (type == kValFloat) {
        double x = where_real(raw, width);
        if (x == 0.0) x = 0.0;                                        // -0.0 == 0.0: one key for both
        const uint64_t bits = __builtin_bit_cast(uint64_t, x);
        key = (bits >> 63) ? ~bits : bits | (1ull << 63);
    } else {
        const uint32_t sh = type == kValInt ? 64u - 8u * width : 0u;
        key = (uint64_t)((int64_t)(raw << sh) >> sh) ^ (type == kValInt ? 1ull << 63 : 0ull);
    }
    return (op == kCmpLt || op == kCmpLe) ? ~key : key;
}

// One term's loads for the lane's pairs: both elements of every pair, and with kValid the validity word of either side
// (null plane: all valid), all of them before the first compare. The loads are unconditional -- see the pair-filter
// frame for why. The switch on the width around it (1 / 2 / 4 / 8, uniform) is written out in both callers, k_pairs_where and
// asof_pairs: as one where_load_width<kValid> it left k_pairs_where's code as it was and placed the blocks of both
// k_asof_best instances differently (tools/asm_diff.py).
template <class E, bool kValid>
__device__ __forceinline__ void where_load(const void* sCol, const void* rCol, const uint32_t* sValid, const uint32_t* rValid,
                                           const uint32_t (&si)[kFilterLanePairs], const uint32_t (&ri)[kFilterLanePairs],
                                           uint64_t (&a)[kFilterLanePairs], uint64_t (&b)[kFilterLanePairs],
                                           uint32_t (&vs)[kFilterLanePairs], uint32_t (&vr)[kFilterLanePairs])
{
    if constexpr (kValid) {
#pragma unroll
        for (uint32_t j = 0; j < kFilterLanePairs; ++j) { vs[j] = sValid ? sValid[si[j] >> 5] : ~0u; vr[j] = rValid ? rValid[ri[j] >> 5] : ~0u; }
    }
#pragma unroll
    for (uint32_t j = 0; j < kFilterLanePairs; ++j) { a[j] = static_cast<const E*>(sCol)[si[j]]; b[j] = static_cast<const E*>(rCol)[ri[j]]; }
    __builtin_amdgcn_sched_barrier(0);                                // no compare moves up between the loads: it would wait there
}

// A pair the host loops drop as the pair-filter frame does: an HJ_NO_ROW entry, or a row outside its relation
inline bool dropped_pair(uint32_t es, uint32_t er, uint32_t sRowBase, uint32_t sRows, uint32_t rRows)
{
    return es == kNoRow || er == kNoRow || es - sRowBase >= sRows || er >= rRows;
}

// element i of a column of `width` bytes, zero-extended; the pointer is aligned to the width (the host loops, and win_peers)
__host__ __device__ __forceinline__ uint64_t col_elem(const void* col, uint32_t width, uint32_t i)
{
    switch (width) {
        case 1: return static_cast<const uint8_t*>(col)[i];
        case 2: return static_cast<const uint16_t*>(col)[i];
        case 4: return static_cast<const uint32_t*>(col)[i];
        default: return static_cast<const unsigned long long*>(col)[i];
    }
}

// The host loops' frame of a call on a pair list: a pair the pair-filter frame drops is counted; one that keep(si, ri) keeps
// -- the rows with S's base off -- is written while the capacity lasts, in input order, and sets its marks whether written
// or not. info: kept, written, 0, dropped (may be null).
template <class Keep>
inline void pairs_keep_host(const PairList& in, const PairSink& to, uint64_t* info, Keep&& keep)
{
    uint64_t kept = 0, dropped = 0;
    for (uint64_t k = 0; k < in.n; ++k) {
        const uint32_t es = in.mapS[k], er = in.mapR[k], si = es - in.sRowBase, ri = er;
        if (dropped_pair(es, er, in.sRowBase, in.sRows, in.rRows)) { ++dropped; continue; }
        if (!keep(si, ri)) continue;
        if (kept < to.out.capacity) { to.out.s[kept] = es; to.out.r[kept] = er; }
        if (to.sMarks) set_mark_bit(to.sMarks, si);
        if (to.rMarks) set_mark_bit(to.rMarks, ri);
        ++kept;
    }
    if (info) { info[0] = kept; info[1] = kept < to.out.capacity ? kept : to.out.capacity; info[2] = 0; info[3] = dropped; }
}

// ---- as-of joins: one best match per S row (defined in hj_asof.hip) -----------
// The term of a call as the kernels take it (hj_asof_term, include/htm_hashjoin.h): the pair (s, r) is eligible when
// s[s] op r[r] holds as a term of the condition step does, op one of LT, LE, GT, GE.
struct AsofTerm { const void *s, *r; const uint32_t *sValid, *rValid; uint32_t width, type, op; };
// Pairs (mapS[k] - sRowBase, mapR[k]) -> per S row the eligible pair with the largest asof_key of its R element, ties to
// the lowest R row, to `to.out` as launch_pairs_where writes its kept pairs (its cursor: two 64-bit words, zeroed before the
// launch: kept pairs, pairs dropped); the marks as there, set by the kept pairs alone. bestVal (sRows 64-bit words) and
// bestRow (sRows words) are initialised here, on s: after the call bestRow[i] is the R row kept for S row i or kNoRow,
// bestVal[i] its key (0 without one). The caller has checked the term and nPairs, sRows, rRows <= 2^32 - 1.
hipError_t launch_pairs_asof(const PairList& in, const AsofTerm& term, unsigned long long* bestVal, uint32_t* bestRow, const PairSink& to,
                             hipStream_t s);
// the same in host loops over host pointers (asof_key and where_holds are the kernels' own), the kept pairs in input
// order; info: kept, written, 0, dropped (may be null)
void pairs_asof_host(const PairList& in, const AsofTerm& term, uint64_t* bestVal, uint32_t* bestRow, const PairSink& to, uint64_t* info);

// ---- rows in the order of their columns (defined in hj_sort.hip) --------------
// The order key of the sort: the zero-extended raw word of a valid element of `width` bytes read as `type` -> an unsigned
// word of 8 * width bits that orders as the header states it, equal exactly where two elements tie. UINT: the word. INT:
// the sign bit flipped within the width. FLOAT: folded as asof_key folds, in the element's own width -- a negative's bits all
// complemented, a positive's sign bit set, -0.0 taken for +0.0 -- and every NaN, whatever its sign or payload, all ones:
// above +inf. HJ_SORT_DESC complements the word within the width, NaN included. A NULL's key is 0: the caller's business.
constexpr uint32_t kSortMaxCols = 4;          // HJ_SORT_MAX_COLS
constexpr uint32_t kSortDesc = 1u, kSortNullsFirst = 2u;      // HJ_SORT_DESC, HJ_SORT_NULLS_FIRST
__host__ __device__ __forceinline__ uint64_t sort_key(uint32_t type, uint32_t width, uint32_t flags, uint64_t raw)
{
    const uint32_t bits = 8u * width;
    const uint64_t top = 1ull << (bits - 1u), mask = top | (top - 1ull);
    uint64_t key = raw & mask;
    if (type == kValInt) key ^= top;
    else if (type == kValFloat) {
        const uint64_t mag = key & (top - 1ull), inf = width == 4u ? 0x7F800000ull : 0x7FF0000000000000ull;
        if (mag > inf) key = mask;                                    // a NaN
        else if (mag == 0ull) key = top;                              // -0.0 == 0.0: one key for both
        else key = (key & top) ? ~key & mask : key | top;
    }
    return (flags & kSortDesc) ? ~key & mask : key;
}
// The columns of a call as the kernels take them (hj_sort_col, include/htm_hashjoin.h); cols[0] is the most significant.
struct SortCols { const void* p[kSortMaxCols]; const uint32_t* valid[kSortMaxCols]; uint32_t width[kSortMaxCols], type[kSortMaxCols], flags[kSortMaxCols]; };
// How a pass cuts nRows records of keyBytes-byte keys: a workgroup ranks tileRows records at a time and owns chunkRows (a
// multiple of it) in a pass; the workspace is two key planes and two row planes of nRows, a histogram of 256 words per
// chunk -- at most 4096 chunks at any nRows: 4 MiB -- and its scan sums. bytes is monotone in nRows.
struct SortLayout { uint32_t tileRows, chunkRows, chunks; size_t keyPlane, rowPlane, histBytes, bytes; };
SortLayout sort_layout(uint64_t nRows, uint32_t keyBytes);
uint32_t sort_key_bytes(const SortCols& cols, uint32_t nCols);       // 8 with an 8-byte column, else 4
uint32_t sort_passes(const SortCols& cols, uint32_t nCols);          // one per element byte, one more per validity plane
// perm[0 .. nRows) = the rows in the order of the columns, stable. work: sort_layout(nRows, sort_key_bytes(..)).bytes. The
// caller has checked what the header says the entry point refuses. nRows 0 enqueues nothing.
hipError_t launch_sort_rows(const SortCols& cols, uint32_t nCols, uint64_t nRows, uint32_t* perm, void* work, hipStream_t s);
void sort_rows_host(const SortCols& cols, uint32_t nCols, uint64_t nRows, uint32_t* perm);     // sort_key around std::stable_sort

// ---- range joins without an equality key (defined in hj_range.hip) -------------
// The index of one column: perm = launch_sort_rows' ascending permutation of it, keys[q] = sort_key of the element of row
// perm[q] in a plane of 4-byte words (widths 1, 2, 4) or 8-byte ones, head = rows indexed (the leading positions whose
// element is valid and no NaN), NULL rows, NaN rows, key bytes. work: the sort's workspace for the one column.
hipError_t launch_range_index(const SortCols& col, uint64_t nRows, uint32_t* perm, void* keys, uint32_t* head, void* work, hipStream_t s);
void range_index_host(const SortCols& col, uint64_t nRows, uint32_t* perm, void* keys, uint32_t head[4]);
// The term of a range call as the kernels take it (hj_range_term, include/htm_hashjoin.h, field for field)
struct RangeTerm { const void *lo, *hi; const uint32_t *loValid, *hiValid; uint32_t width, type, flags, pick; };
// How a call cuts its work: the index of nRows rows is searched through `pivots` keys, every stride-th (a power of two),
// held in ldsBytes of LDS at most; a workgroup takes chunkRows S rows to their bounds, another tilePairs output positions.
// The workspace: the pivots, the two bound planes, three planes of one 64-bit word per chunk, the difference plane of
// nRows + 1 words and its scan sums. bytes is monotone in both arguments.
struct RangeLayout { uint32_t pivots, stride, tilePairs, chunkRows, chunks, ldsBytes; size_t pivotBytes, boundBytes, chunkBytes, diffBytes, bytes; };
RangeLayout range_layout(uint64_t nRows, uint64_t sRows);
// S row i -> the pairs (sRowBase + i, perm[q]) for the positions q of the indexed prefix whose key lies in the row's
// interval, or the one the pick keeps; to `to` as launch_pairs_where writes its kept pairs, without a cursor: the planes fill
// from 0 in S-row order of the tiles. head is read on the device; an index of the other key width counts as empty. words:
// four 64-bit words, written here -- pairs, S rows with a pair, S rows with a NULL or NaN bound, rows indexed. work:
// range_layout(rRows, sRows).bytes. The caller has checked what the header says the entry point refuses.
hipError_t launch_range_pairs(const void* keys, const uint32_t* perm, const uint32_t* head, uint32_t rRows, const RangeTerm& t, uint32_t sRows,
                              uint32_t sRowBase, const PairSink& to, void* work, unsigned long long* words, hipStream_t s);
// the same on host pointers, the pairs in S-row order and ascending positions; info: hj_range_pairs_host's (may be null)
void range_pairs_host(const void* keys, const uint32_t* perm, const uint32_t* head, uint32_t rRows, const RangeTerm& t, uint32_t sRows,
                      uint32_t sRowBase, const PairSink& to, uint64_t info[8]);

// ---- aggregating joins: COUNT / SUM / MIN / MAX per group row (hj_prj_agg.hip, hj_agg.hip) ----
// The columns of a call as the kernels take them, by value in the kernel arguments: the ops (hj_agg_spec; sgn: HJ_AGG_SIGNED),
// the sources (hj_agg_src) and the accumulator planes. Every accumulator is 64 bits wide.
constexpr uint32_t kAggMaxCols = 4;           // HJ_AGG_MAX_COLS
constexpr uint32_t kAggCount = 0, kAggSum = 1, kAggMin = 2, kAggMax = 3;      // hj_agg_op
struct AggOps { uint32_t op[kAggMaxCols], width[kAggMaxCols], sgn[kAggMaxCols]; };
struct AggSrc { const void* p[kAggMaxCols]; const uint32_t* valid[kAggMaxCols]; };
struct AggPlanes { unsigned long long* count; unsigned long long* acc[kAggMaxCols]; };
struct AggRowsOut { unsigned long long* col[kAggMaxCols]; unsigned long long* count; };
// The accumulators of the aggregates and of the window functions' running ops: op is an hj_agg_op, T 64 bits wide
// (values) or uint32_t (the window's positions and counts).
// the identity of an op: what an accumulator holds before its first value
template <class T = unsigned long long>
__host__ __device__ __forceinline__ T agg_identity(uint32_t op, uint32_t sgn)
{
    constexpr T top = (T)1 << (8 * sizeof(T) - 1);
    if (op == kAggMin) return sgn ? (T)(top - 1) : (T)~(T)0;
    if (op == kAggMax) return sgn ? top : (T)0;
    return (T)0;
}
// acc op= v, without a returned value; SCOPE: the workgroup for an LDS entry, the agent for a global one
template <int SCOPE>
__device__ __forceinline__ void agg_apply(unsigned long long* acc, uint32_t op, uint32_t sgn, unsigned long long v)
{
    if (op <= kAggSum) __hip_atomic_fetch_add(acc, v, __ATOMIC_RELAXED, SCOPE);
    else if (op == kAggMin) {
        if (sgn) __hip_atomic_fetch_min(reinterpret_cast<long long*>(acc), (long long)v, __ATOMIC_RELAXED, SCOPE);
        else __hip_atomic_fetch_min(acc, v, __ATOMIC_RELAXED, SCOPE);
    } else {
        if (sgn) __hip_atomic_fetch_max(reinterpret_cast<long long*>(acc), (long long)v, __ATOMIC_RELAXED, SCOPE);
        else __hip_atomic_fetch_max(acc, v, __ATOMIC_RELAXED, SCOPE);
    }
}
// a op b, for the reductions in registers that run in front of an atomic. NOT one body with win_op, its twin of the window's
// scans: with either text for both, the other side's kernels compile to other code (k_pairs_agg; k_win_apply, k_win_carry,
// k_win_summary; tools/asm_diff.py).
__device__ __forceinline__ unsigned long long agg_combine(uint32_t op, uint32_t sgn, unsigned long long a, unsigned long long b)
{
    if (op <= kAggSum) return a + b;
    if (op == kAggMin) return sgn ? ((long long)a < (long long)b ? a : b) : (a < b ? a : b);
    return sgn ? ((long long)a > (long long)b ? a : b) : (a > b ? a : b);
}
// the 64-bit value of element i of a column: COUNT brings 1, a 4-byte element is sign- or zero-extended
__host__ __device__ __forceinline__ unsigned long long agg_value(const void* __restrict__ src, uint32_t op, uint32_t width, uint32_t sgn, uint32_t i)
{
    if (op == kAggCount) return 1ull;
    if (width == 8) return static_cast<const unsigned long long*>(src)[i];
    const uint32_t w = static_cast<const uint32_t*>(src)[i];
    return sgn ? (unsigned long long)(long long)(int32_t)w : (unsigned long long)w;
}

// The reduction over a pair list (hj_agg.hip): for pair k with g = mapG[k] - gBase, v = mapV[k] - vBase: acc[c][g] op= src[c][v],
// count[g] += 1 (count may be null, and mapV when no column reads a value). An entry that is HJ_NO_ROW or out of range on
// either side is never dereferenced: counts[1] += 1, else counts[0] += 1 (two 64-bit words, zeroed before the launch).
struct PairAggCols { AggSrc src; AggOps ops; unsigned long long* acc[kAggMaxCols]; };
hipError_t launch_pairs_agg(const uint32_t* mapG, const uint32_t* mapV, uint64_t nPairs, uint32_t gBase, uint32_t gRows, uint32_t vBase,
                            uint32_t vRows, const PairAggCols& cols, uint32_t nCols, unsigned long long* count, unsigned long long* counts,
                            hipStream_t s);

// ---- window functions over runs along a permutation (defined in hj_window.hip) ----
// What the kernels and the host loop share: how a position's head bits come about (win_head: partition head, peer head,
// skipped entry), and what a row brings to a running accumulator (win_value, over the aggregates' agg_identity and agg_value) and how two of them combine (win_op).
constexpr uint32_t kWinMaxFuncs = 8;          // HJ_WIN_MAX_FUNCS
constexpr uint32_t kWinRowNumber = 0, kWinRank = 1, kWinDenseRank = 2, kWinPartRows = 3, kWinLag = 4, kWinLead = 5, kWinFirstRow = 6,
                   kWinLastRow = 7, kWinRunCount = 8, kWinRunMax = 11;                        // hj_win_op
// the head byte of a position: it starts a partition, it starts a peer run (set with every partition head), its entry is
// HJ_NO_ROW or at / behind nRows (then all three are set: the entry is a run of its own and belongs to no partition)
constexpr uint32_t kHeadPart = 1u, kHeadPeer = 2u, kHeadSkip = 4u;
// rows a and b tie in every order column: both NULL, or both valid with one sort_key (the flags do not change equality)
__host__ __device__ __forceinline__ bool win_peers(const SortCols& cols, uint32_t nOrder, uint32_t a, uint32_t b)
{
    bool same = true;
#pragma unroll
    for (uint32_t c = 0; c < kSortMaxCols; ++c) {
        if (c >= nOrder) break;
        const bool va = !cols.valid[c] || valid_bit(cols.valid[c], a), vb = !cols.valid[c] || valid_bit(cols.valid[c], b);
        if (va && vb)
            same = same && sort_key(cols.type[c], cols.width[c], 0u, col_elem(cols.p[c], cols.width[c], a)) ==
                               sort_key(cols.type[c], cols.width[c], 0u, col_elem(cols.p[c], cols.width[c], b));
        else same = same && va == vb;
    }
    return same;
}
// the head byte of position p. perm null: the identity (the caller has checked nPos <= nRows). part null: one value.
__host__ __device__ __forceinline__ uint32_t win_head(const uint32_t* perm, uint64_t p, uint32_t nRows, const uint32_t* part,
                                                      const SortCols& cols, uint32_t nOrder)
{
    const uint32_t row = perm ? perm[p] : (uint32_t)p;
    if (row >= nRows) return kHeadPart | kHeadPeer | kHeadSkip;         // HJ_NO_ROW too: nRows <= 2^32 - 2
    if (p == 0) return kHeadPart | kHeadPeer;
    const uint32_t prev = perm ? perm[p - 1] : (uint32_t)(p - 1);
    if (prev >= nRows || (part && part[row] != part[prev])) return kHeadPart | kHeadPeer;
    return win_peers(cols, nOrder, row, prev) ? 0u : kHeadPeer;
}
// a op b in the window's scans, T as agg_identity's (see agg_combine)
template <class T>
__host__ __device__ __forceinline__ T win_op(uint32_t op, uint32_t sgn, T a, T b)
{
    if (op <= kAggSum) return a + b;
    constexpr T top = (T)1 << (8 * sizeof(T) - 1);
    const T flip = sgn ? top : (T)0;                                    // the order of the signed values as unsigned ones
    const bool less = (T)(a ^ flip) < (T)(b ^ flip);
    return (op == kAggMin) == less ? a : b;
}
// what row `row` brings to a running op: COUNT 1, else the element sign- or zero-extended; under a NULL the identity
__host__ __device__ __forceinline__ unsigned long long win_value(const void* src, const uint32_t* valid, uint32_t op, uint32_t width,
                                                                 uint32_t sgn, uint32_t row)
{
    if (valid && !valid_bit(valid, row)) return agg_identity(op, sgn);
    return agg_value(src, op, width, sgn, row);
}
// The functions of a call as the kernels take them, by value in the kernel arguments (hj_win_func, include/htm_hashjoin.h);
// op: the hj_win_op, sgn: HJ_AGG_SIGNED.
struct WinFuncs { const void* src[kWinMaxFuncs]; const uint32_t* valid[kWinMaxFuncs]; void* out[kWinMaxFuncs];
                  uint32_t op[kWinMaxFuncs], width[kWinMaxFuncs], sgn[kWinMaxFuncs], offset[kWinMaxFuncs]; };
// How a call cuts nPos positions: a workgroup scans tilePos positions at a time and owns chunkPos (a multiple of it); at
// most 4096 chunks at any nPos. The workspace: one head byte and one 4-byte end per position, and the chunk summaries
// (their size does not depend on nPos). bytes is monotone in nPos.
struct WindowLayout { uint32_t tilePos, chunkPos, chunks; size_t headBytes, endBytes, sumBytes, bytes; };
WindowLayout window_layout(uint64_t nPos);
// out[row(p)] of every function for p in [0, nPos): see hj_window_rows_dev. work: window_layout(nPos).bytes. totals: three
// 64-bit words, written here -- partitions, peer runs, entries skipped. The caller has checked what the header says the
// entry point refuses. nPos 0 enqueues nothing.
hipError_t launch_window_rows(const uint32_t* perm, uint64_t nPos, uint32_t nRows, const uint32_t* part, const SortCols& order, uint32_t nOrder,
                              const WinFuncs& funcs, uint32_t nFuncs, void* work, unsigned long long* totals, hipStream_t s);
// the same in one sequential loop over host pointers; totals as above
void window_rows_host(const uint32_t* perm, uint64_t nPos, uint32_t nRows, const uint32_t* part, const SortCols& order, uint32_t nOrder,
                      const WinFuncs& funcs, uint32_t nFuncs, uint64_t totals[3]);
// the head bytes alone (k_win_heads): heads[p] = win_head(p) for p in [0, nPos). What the frames below start from.
void launch_window_heads(const uint32_t* perm, uint64_t nPos, uint32_t nRows, const uint32_t* part, const SortCols& order, uint32_t nOrder,
                         uint8_t* heads, hipStream_t s);

// ---- sliding window frames over the same runs (defined in hj_frames.hip) ----
// One function of a call (hj_frame_func, include/htm_hashjoin.h): op an hj_agg_op, sgn HJ_AGG_SIGNED, unbLo / unbHi the
// two HJ_FRAME_UNBOUNDED_* flags (their offset is 0 then), lo <= hi in [-(2^32 - 1), 2^32 - 1] otherwise.
constexpr uint32_t kFrameMaxFuncs = 8;        // HJ_FRAME_MAX_FUNCS
struct FrameFunc { const void* src; const uint32_t* valid; void* out; long long lo, hi; uint32_t op, width, sgn, unbLo, unbHi; };
// How a call cuts nPos positions: window_layout's tiles and chunks. The workspace: one head byte and one 4-byte end per
// position, TWO 8-byte planes per position that the functions of a call share one after another (the values, which the
// backward scan turns into H in place, and G), and the chunk summaries (their size does not depend on nPos): 21 bytes per
// position, whatever nFuncs. bytes is monotone in nPos.
struct FramesLayout { uint32_t tilePos, chunkPos, chunks; size_t headBytes, endBytes, planeBytes, sumBytes, bytes; };
FramesLayout frames_layout(uint64_t nPos);
// out[row(p)] of every function for p in [0, nPos): see hj_window_frames_dev. work: frames_layout(nPos).bytes. totals: three
// 64-bit words, written here -- partitions, 0, entries skipped. The caller has checked what the header says the entry
// point refuses. nPos 0 enqueues nothing.
hipError_t launch_window_frames(const uint32_t* perm, uint64_t nPos, uint32_t nRows, const uint32_t* part, const FrameFunc* funcs, uint32_t nFuncs,
                                void* work, unsigned long long* totals, hipStream_t s);
// The same on host pointers by ANOTHER algorithm: one sequential loop per function, a running window for COUNT / SUM and a
// monotonic deque for MIN / MAX; totals as above.
void window_frames_host(const uint32_t* perm, uint64_t nPos, uint32_t nRows, const uint32_t* part, const FrameFunc* funcs, uint32_t nFuncs,
                        uint64_t totals[3]);

}  // namespace hj
