// hj_api_rows.hip -- the C ABI's calls on rows: the R-side match marks and their sweep, the gather through a row map, the
// joins on real key columns (hash, verify, sweep of a caller's plane), the rows of one table grouped by their key columns and sorted by them, the window functions along a permutation, the
// join conditions beyond equality, the as-of step, and the *_info entry point of every call that has a record (hj_host.h:
// CallRecord). Host-side glue only.
#include "hj_host.h"

using namespace hjapi;

extern "C" {

// Waits for the stream. The last call of `rec` in the common form of the *_info entry points: out[0] = the first counter word the
// call left at dWords (`bytes` of them, at most 16: one 32-bit total or two 64-bit words; nullptr: none), out[1] = min(out[0], capacity),
// out[2] = its device time in microseconds, out[3] = the second word. All 0 for a call that was never made, or forgotten since.
static int call_info(hj_ctx* c, const CallRecord& rec, const void* dWords, size_t bytes, uint64_t out[4])
{
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!rec.called) return HJ_OK;
    unsigned long long words[2] = {0, 0};
    if (dWords) HJ_HIP(c, hipMemcpy(words, dWords, bytes, hipMemcpyDeviceToHost));
    float ms = 0;
    if (!rec.timed || hipEventElapsedTime(&ms, rec.ev[0], rec.ev[1]) != hipSuccess) ms = 0;
    out[0] = words[0];
    out[1] = words[0] < rec.capacity ? words[0] : rec.capacity;
    out[2] = (uint64_t)((double)ms * 1000.0 + 0.5);
    out[3] = words[1];
    return HJ_OK;
}

int hj_pairs_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_PAIRS];      // the cursor = rows found; LEFT's unmatched S tuples
    if (const int rc = call_info(c, r, c->buf[B_PAIRS_CURSOR].p, 16, out)) return rc;
    // unmatched S tuples of the call: SEMI wrote one row per matched tuple, ANTI one per unmatched one
    if (r.kind != HJ_JOIN_LEFT) out[3] = r.kind == HJ_JOIN_SEMI ? r.rows - out[0] : r.kind == HJ_JOIN_ANTI ? out[0] : 0;
    return HJ_OK;
}

// ---- R-side match marks ---------------------------------------------------
// what the three calls need: a context reserved with the flag whose plane describes its last build
static int marks_state(hj_ctx* c, const char* fn)
{
    if (!tracks(c)) return fail(c, HJ_ERR_STATE, fn, "context reserved without HJ_FLAG_TRACK_R_MATCHES");
    if (!c->marks.built) return fail(c, HJ_ERR_STATE, fn, "the last build was not hj_build_dev / hj_prj_build_dev (or there was none)");
    return HJ_OK;
}

int hj_r_marks_clear(hj_ctx* c)
{
    HJ_ENTER(c, true);
    if (const int rc = marks_state(c, "hj_r_marks_clear")) return rc;
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipMemsetAsync(c->buf[B_R_MARKS].p, 0, marks_bytes(c->marks.rows), c->stream));
    return HJ_OK;
}

int hj_r_rows_dev(hj_ctx* c, uint32_t which, uint32_t* dOutR, uint64_t capacity)
{
    HJ_ENTER(c, true);
    if (const int rc = marks_state(c, "hj_r_rows_dev")) return rc;
    if (which > HJ_R_MATCHED) return fail(c, HJ_ERR_INVALID, "hj_r_rows_dev: which must be HJ_R_UNMATCHED or HJ_R_MATCHED");
    if (capacity && !dOutR) return fail(c, HJ_ERR_INVALID, "hj_r_rows_dev: output pointer NULL with capacity > 0");
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipEventRecord(c->call[CALL_R_ROWS].ev[0], c->stream));
    const RMarks mk{c->buf[B_R_MARKS].as<uint32_t>(), (uint32_t)c->marks.base, (uint32_t)c->marks.rows};
    HJ_HIP(c, launch_r_sweep(mk, which == HJ_R_MATCHED, dOutR, capacity, c->buf[B_R_SWEEP].as<uint32_t>(), c->stream));
    return call_end(c, CALL_R_ROWS, capacity, c->marks.rows);
}

int hj_r_rows_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    if (const int rc = marks_state(c, "hj_r_rows_info")) return rc;
    // the word behind the block counts: their total after the scan
    const CallRecord& r = c->call[CALL_R_ROWS];
    if (const int rc = call_info(c, r, c->buf[B_R_SWEEP].as<uint32_t>() + r_sweep_blocks(c->marks.rows), sizeof(uint32_t), out)) return rc;
    out[3] = c->marks.rows;                     // also with no hj_r_rows_dev since the build
    return HJ_OK;
}

// ---- gather through a row map ----------------------------------------------
static bool gather_width_ok(uint32_t w) { return w == 1 || w == 2 || w == 4 || w == 8 || w == 16; }
static bool word_ptr_ok(const void* p) { return !(reinterpret_cast<uintptr_t>(p) & 3u); }     // NULL passes: the pointer is optional
// a column's pointer: there, and aligned to the column's width
static bool col_ptr_ok(const void* p, uint32_t width) { return p && !(reinterpret_cast<uintptr_t>(p) & (width - 1)); }

// what hj_gather_dev and hj_gather2_dev refuse before they look at a column
static int gather_args(hj_ctx* c, const char* fn, const uint32_t* dMap, uint64_t nRows, uint64_t srcRows, const void* cols, uint32_t nCols,
                       const uint32_t* dValid)
{
    if (nCols > HJ_GATHER_MAX_COLS) return fail(c, HJ_ERR_INVALID, fn, "more than HJ_GATHER_MAX_COLS columns");
    if (nCols && !cols) return fail(c, HJ_ERR_INVALID, fn, "cols NULL with nCols > 0");
    if (nRows > 0xFFFFFFFFull || srcRows > 0xFFFFFFFFull) return fail(c, HJ_ERR_INVALID, fn, "nRows or srcRows above 2^32 - 1");
    if (nRows && !dMap) return fail(c, HJ_ERR_INVALID, fn, "dMap NULL with nRows > 0");
    if (nRows && !nCols && !dValid) return fail(c, HJ_ERR_INVALID, fn, "neither a column nor a validity plane");
    return HJ_OK;
}

int hj_gather_dev(hj_ctx* c, const uint32_t* dMap, uint64_t nRows, uint32_t rowBase, uint64_t srcRows, const hj_gather_col* cols,
                  uint32_t nCols, uint32_t* dValid)
{
    HJ_ENTER(c, true);
    if (const int rc = gather_args(c, "hj_gather_dev", dMap, nRows, srcRows, cols, nCols, dValid)) return rc;
    GatherCols k{};
    for (uint32_t i = 0; i < nCols; ++i) {
        const hj_gather_col& col = cols[i];
        if (!gather_width_ok(col.width)) return fail(c, HJ_ERR_INVALID, "hj_gather_dev: a width that is not 1, 2, 4, 8 or 16");
        if (col.reserved) return fail(c, HJ_ERR_INVALID, "hj_gather_dev: hj_gather_col.reserved must be 0");
        if (!col_ptr_ok(col.dst, col.width)) return fail(c, HJ_ERR_INVALID, "hj_gather_dev: a dst that is NULL or not aligned to its width");
        if (srcRows && !col_ptr_ok(col.src, col.width))                               // srcRows 0: src is never read
            return fail(c, HJ_ERR_INVALID, "hj_gather_dev: a src that is NULL or not aligned to its width");
        k.col[i] = GatherCol{col.src, col.dst, col.width, 0, {col.fill[0], col.fill[1]}};
    }
    if (nRows == 0) return HJ_OK;
    HJ_HIP(c, hipSetDevice(c->device));
    unsigned long long* const counts = c->buf[B_GATHER_CTR].as<unsigned long long>();
    HJ_HIP(c, hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), c->stream));
    HJ_HIP(c, hipEventRecord(c->call[CALL_GATHER].ev[0], c->stream));
    HJ_HIP(c, launch_gather(dMap, nRows, rowBase, srcRows, k, nCols, dValid, counts, c->stream));
    return call_end(c, CALL_GATHER, 0, nRows);
}

int hj_gather_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_GATHER];     // NULL rows, out-of-range entries
    if (const int rc = call_info(c, r, c->buf[B_GATHER_CTR].p, 16, out)) return rc;
    out[1] = out[0]; out[0] = r.rows;
    return HJ_OK;
}

// ---- ... on columns in the Arrow layout (hj_gather_col2) ---------------------
// what hj_gather2_dev refuses of its columns (the message), or nullptr; *k: the columns as the kernels take them
static const char* gather_cols2_error(const hj_gather_col2* cols, uint32_t nCols, uint64_t nRows, uint64_t srcRows, const uint32_t* dValid,
                                      GatherCols2* k)
{
    // every output range of the call, for the one aliasing rule: a variable-length dst overlaps no other output
    struct Range { uintptr_t lo, hi; bool bytes; } out[4 * HJ_GATHER_MAX_COLS + 1];
    uint32_t nOut = 0;
    const auto add = [&](const void* p, uint64_t bytes, bool isBytes) {
        if (p && bytes) out[nOut++] = Range{reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p) + bytes, isBytes};
    };
    const uint64_t planeBytes = (nRows + 31) / 32 * sizeof(uint32_t);
    add(dValid, planeBytes, false);
    for (uint32_t i = 0; i < nCols; ++i) {
        const hj_gather_col2& col = cols[i];
        if (col.width && !gather_width_ok(col.width)) return "a width that is not 0, 1, 2, 4, 8 or 16";
        if (col.flags) return "hj_gather_col2.flags must be 0";
        if (col.width && (col.srcOffsets || col.dstOffsets)) return "offsets on a column whose width is not 0";
        if (!col.width && (!col.srcOffsets || !col.dstOffsets)) return "width 0 without srcOffsets or without dstOffsets";
        if (!word_ptr_ok(col.srcOffsets) || !word_ptr_ok(col.dstOffsets) || !word_ptr_ok(col.srcValid) || !word_ptr_ok(col.dstValid))
            return "an offsets or validity pointer that is not 4-byte aligned";
        const uint32_t align = col.width ? col.width : 1u;            // a bytes buffer may start anywhere
        if (col.width ? !col_ptr_ok(col.dst, align) : (col.dstCapacity && !col.dst)) return "a dst that is NULL or not aligned to its width";
        if (col.width && col.dstCapacity) return "dstCapacity on a fixed-width column";
        if (srcRows && !col_ptr_ok(col.src, align)) return "a src that is NULL or not aligned to its width";   // srcRows 0: src is never read
        k->col[i] = GatherCol2{col.src, col.dst, col.srcOffsets, col.dstOffsets, col.srcValid, col.dstValid, col.dstCapacity, col.width, 0u,
                               {col.fill[0], col.fill[1]}};
        add(col.dst, col.width ? nRows * col.width : col.dstCapacity, !col.width);
        add(col.dstOffsets, (nRows + 1) * sizeof(uint32_t), false);
        add(col.dstValid, planeBytes, false);
    }
    for (uint32_t a = 0; a < nOut; ++a)
        for (uint32_t b = 0; out[a].bytes && b < nOut; ++b)
            if (a != b && out[a].lo < out[b].hi && out[b].lo < out[a].hi) return "a variable-length dst that overlaps another output of the call";
    return nullptr;
}

int hj_gather2_dev(hj_ctx* c, const uint32_t* dMap, uint64_t nRows, uint32_t rowBase, uint64_t srcRows, const hj_gather_col2* cols,
                   uint32_t nCols, uint32_t* dValid)
{
    HJ_ENTER(c, true);
    if (const int rc = gather_args(c, "hj_gather2_dev", dMap, nRows, srcRows, cols, nCols, dValid)) return rc;
    GatherCols2 k{};
    if (const char* what = gather_cols2_error(cols, nCols, nRows, srcRows, dValid, &k)) return fail(c, HJ_ERR_INVALID, "hj_gather2_dev", what);
    if (nRows == 0) return HJ_OK;
    HJ_HIP(c, hipSetDevice(c->device));
    bool varlen = false;
    for (uint32_t i = 0; i < nCols; ++i) varlen = varlen || !k.col[i].width;
    if (varlen)
        if (const int rc = c->buf[B_GATHER2_WORK].reserve(c, gather2_work_words(nRows) * sizeof(uint32_t))) return rc;
    unsigned long long* const counts = c->buf[B_GATHER2_CTR].as<unsigned long long>();
    HJ_HIP(c, hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), c->stream));
    HJ_HIP(c, hipEventRecord(c->call[CALL_GATHER2].ev[0], c->stream));
    HJ_HIP(c, launch_gather2(dMap, nRows, rowBase, srcRows, k, nCols, dValid, counts, counts + 2, c->buf[B_GATHER2_WORK].as<uint32_t>(), c->stream));
    return call_end(c, CALL_GATHER2, 0, nRows);
}

int hj_gather2_info(hj_ctx* c, uint64_t out[4 + HJ_GATHER_MAX_COLS])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_GATHER2];
    for (uint32_t i = 0; i < HJ_GATHER_MAX_COLS; ++i) out[4 + i] = 0;
    if (const int rc = call_info(c, r, c->buf[B_GATHER2_CTR].p, 16, out)) return rc;
    out[1] = out[0]; out[0] = r.rows;
    if (!r.called) { out[0] = 0; return HJ_OK; }
    unsigned long long totals[HJ_GATHER_MAX_COLS];
    HJ_HIP(c, hipMemcpy(totals, c->buf[B_GATHER2_CTR].as<unsigned long long>() + 2, sizeof(totals), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < HJ_GATHER_MAX_COLS; ++i) out[4 + i] = totals[i];
    return HJ_OK;
}

// ---- joins on real key columns: hash, verify, sweep of a caller's plane -----
// Two column descriptors, hj_key_col and hj_key_col2 (the Arrow layout), each with its own entry points and its own
// checks; behind the checks there is one path: an hj_key_col is the hj_key_col2 with null offsets, null planes and flags 0.

// The hj_key_col columns of a call, checked: nCols, widths, reserved, and the pointers of the sides in use (rows > 0 on that side)
static const char* key_cols_error(const hj_key_col* cols, uint32_t nCols, bool useS, bool useR)
{
    if (nCols == 0 || nCols > HJ_KEY_MAX_COLS) return "nCols must be 1 .. HJ_KEY_MAX_COLS";
    if (!cols) return "cols NULL";
    for (uint32_t i = 0; i < nCols; ++i) {
        const hj_key_col& col = cols[i];
        if (!gather_width_ok(col.width)) return "a width that is not 1, 2, 4, 8 or 16";
        if (col.reserved) return "hj_key_col.reserved must be 0";
        if (useS && !col_ptr_ok(col.s, col.width)) return "an S column that is NULL or not aligned to its width";
        if (useR && !col_ptr_ok(col.r, col.width)) return "an R column that is NULL or not aligned to its width";
    }
    return nullptr;
}

// The hj_key_col2 columns of a call, checked likewise, and what the descriptor adds
static const char* key_cols_error(const hj_key_col2* cols, uint32_t nCols, bool useS, bool useR)
{
    if (nCols == 0 || nCols > HJ_KEY_MAX_COLS) return "nCols must be 1 .. HJ_KEY_MAX_COLS";
    if (!cols) return "cols NULL";
    for (uint32_t i = 0; i < nCols; ++i) {
        const hj_key_col2& col = cols[i];
        if (col.width && !gather_width_ok(col.width)) return "a width that is not 0, 1, 2, 4, 8 or 16";
        if (col.flags & ~HJ_KEY_NULLS_EQUAL) return "hj_key_col2.flags has bits other than HJ_KEY_NULLS_EQUAL";
        if (col.width && (col.sOffsets || col.rOffsets)) return "offsets on a column whose width is not 0";
        if (!word_ptr_ok(col.sOffsets) || !word_ptr_ok(col.rOffsets) || !word_ptr_ok(col.sValid) || !word_ptr_ok(col.rValid))
            return "an offsets or validity pointer that is not 4-byte aligned";
        const uint32_t align = col.width ? col.width : 1u;            // a bytes buffer may start anywhere
        if (useS && !col_ptr_ok(col.s, align)) return "an S column that is NULL or not aligned to its width";
        if (useR && !col_ptr_ok(col.r, align)) return "an R column that is NULL or not aligned to its width";
        if (!col.width && ((useS && !col.sOffsets) || (useR && !col.rOffsets))) return "width 0 without offsets on a side in use";
    }
    return nullptr;
}

extern "C++" {      // templates: one body per descriptor

static hj_key_col2 key_col2_of(const hj_key_col& col) { return hj_key_col2{col.s, col.r, nullptr, nullptr, nullptr, nullptr, col.width, 0u}; }
static hj_key_col2 key_col2_of(const hj_key_col2& col) { return col; }

// the `side` pointers of checked columns as the kernels take them
template <class Col>
static void key_side_cols(const Col* cols, uint32_t nCols, uint32_t side, KeyCols2* k)
{
    const bool S = side == HJ_KEY_SIDE_S;
    for (uint32_t i = 0; i < nCols; ++i) {
        const hj_key_col2 col = key_col2_of(cols[i]);
        k->p[i] = S ? col.s : col.r; k->off[i] = S ? col.sOffsets : col.rOffsets;
        k->valid[i] = S ? col.sValid : col.rValid; k->width[i] = col.width; k->flags[i] = col.flags;
    }
}

// The arguments of a key hash entry point, on the device or on the host -> the kernel's columns; the message of what is
// wrong, or nullptr
template <class Col>
static const char* key_hash_args(const Col* cols, uint32_t nCols, uint32_t side, uint64_t nRows, const uint64_t* out, KeyCols2* k)
{
    if (side > HJ_KEY_SIDE_R) return "side must be HJ_KEY_SIDE_S or HJ_KEY_SIDE_R";
    if (nRows > 0xFFFFFFFFull) return "nRows above 2^32 - 1";
    if (const char* what = key_cols_error(cols, nCols, nRows && side == HJ_KEY_SIDE_S, nRows && side == HJ_KEY_SIDE_R)) return what;
    if (nRows && !out) return "output pointer NULL with nRows > 0";
    key_side_cols(cols, nCols, side, k);
    return nullptr;
}

// hj_key_hash_dev and hj_key_hash2_dev behind their names
template <class Col>
static int key_hash_dev(hj_ctx* c, const char* fn, const Col* cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask,
                        uint64_t* dOutTuples)
{
    KeyCols2 k{};
    if (const char* what = key_hash_args(cols, nCols, side, nRows, dOutTuples, &k)) return fail(c, HJ_ERR_INVALID, fn, what);
    if (nRows == 0) return HJ_OK;
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, launch_key_hash2(k, nCols, nRows, keyMask ? keyMask : 0xFFFFFFFFu, dOutTuples, c->stream));
    return HJ_OK;
}

template <class Col>
static int key_hash_on_host(const Col* cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask, uint64_t* outTuples)
{
    KeyCols2 k{};
    if (key_hash_args(cols, nCols, side, nRows, outTuples, &k)) return HJ_ERR_INVALID;
    key_hash2_host(k, nCols, nRows, keyMask ? keyMask : 0xFFFFFFFFu, outTuples);
    return HJ_OK;
}

// hj_pairs_verify_dev and hj_pairs_verify2_dev behind their names: one call record and one cursor (hj_verify_info reports
// the last call of either)
template <class Col>
static int pairs_verify_dev(hj_ctx* c, const char* fn, const uint32_t* dMapS, const uint32_t* dMapR, uint64_t nPairs, uint32_t sRowBase,
                            uint64_t sRows, uint64_t rRows, const Col* cols, uint32_t nCols, uint32_t* dOutS, uint32_t* dOutR, uint64_t capacity,
                            uint32_t* dSMarks, uint32_t* dRMarks)
{
    if (nPairs > 0xFFFFFFFFull || sRows > 0xFFFFFFFFull || rRows > 0xFFFFFFFFull)
        return fail(c, HJ_ERR_INVALID, fn, "nPairs, sRows or rRows above 2^32 - 1");
    if (const char* what = key_cols_error(cols, nCols, sRows != 0, rRows != 0)) return fail(c, HJ_ERR_INVALID, fn, what);
    if (nPairs && (!dMapS || !dMapR)) return fail(c, HJ_ERR_INVALID, fn, "a map NULL with nPairs > 0");
    if (nPairs && capacity && (!dOutS || !dOutR)) return fail(c, HJ_ERR_INVALID, fn, "an output pointer NULL with capacity > 0");
    KeyCols2SR k{};
    for (uint32_t i = 0; i < nCols; ++i) {
        const hj_key_col2 col = key_col2_of(cols[i]);
        k.s[i] = col.s; k.r[i] = col.r; k.sOff[i] = col.sOffsets; k.rOff[i] = col.rOffsets;
        k.sValid[i] = col.sValid; k.rValid[i] = col.rValid; k.width[i] = col.width; k.flags[i] = col.flags;
    }
    HJ_HIP(c, hipSetDevice(c->device));
    const PairsOut out{dOutS, dOutR, capacity, c->buf[B_VERIFY_CTR].as<unsigned long long>()};
    HJ_HIP(c, hipMemsetAsync(out.cursor, 0, 2 * sizeof(unsigned long long), c->stream));
    HJ_HIP(c, hipEventRecord(c->call[CALL_VERIFY].ev[0], c->stream));
    HJ_HIP(c, launch_pairs_verify2(dMapS, dMapR, nPairs, sRowBase, (uint32_t)sRows, (uint32_t)rRows, k, nCols, out, dSMarks, dRMarks, c->stream));
    return call_end(c, CALL_VERIFY, capacity, nPairs);
}

}  // extern "C++"

int hj_key_hash_dev(hj_ctx* c, const hj_key_col* cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask, uint64_t* dOutTuples)
{
    HJ_ENTER(c, true);
    return key_hash_dev(c, "hj_key_hash_dev", cols, nCols, side, nRows, keyMask, dOutTuples);
}

int hj_key_hash_host(const hj_key_col* cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask, uint64_t* outTuples)
{
    return key_hash_on_host(cols, nCols, side, nRows, keyMask, outTuples);
}

int hj_pairs_verify_dev(hj_ctx* c, const uint32_t* dMapS, const uint32_t* dMapR, uint64_t nPairs, uint32_t sRowBase, uint64_t sRows,
                        uint64_t rRows, const hj_key_col* cols, uint32_t nCols, uint32_t* dOutS, uint32_t* dOutR, uint64_t capacity,
                        uint32_t* dSMarks, uint32_t* dRMarks)
{
    HJ_ENTER(c, true);
    return pairs_verify_dev(c, "hj_pairs_verify_dev", dMapS, dMapR, nPairs, sRowBase, sRows, rRows, cols, nCols, dOutS, dOutR, capacity, dSMarks,
                            dRMarks);
}

int hj_key_hash2_dev(hj_ctx* c, const hj_key_col2* cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask, uint64_t* dOutTuples)
{
    HJ_ENTER(c, true);
    return key_hash_dev(c, "hj_key_hash2_dev", cols, nCols, side, nRows, keyMask, dOutTuples);
}

int hj_key_hash2_host(const hj_key_col2* cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask, uint64_t* outTuples)
{
    return key_hash_on_host(cols, nCols, side, nRows, keyMask, outTuples);
}

int hj_pairs_verify2_dev(hj_ctx* c, const uint32_t* dMapS, const uint32_t* dMapR, uint64_t nPairs, uint32_t sRowBase, uint64_t sRows,
                         uint64_t rRows, const hj_key_col2* cols, uint32_t nCols, uint32_t* dOutS, uint32_t* dOutR, uint64_t capacity,
                         uint32_t* dSMarks, uint32_t* dRMarks)
{
    HJ_ENTER(c, true);
    return pairs_verify_dev(c, "hj_pairs_verify2_dev", dMapS, dMapR, nPairs, sRowBase, sRows, rRows, cols, nCols, dOutS, dOutR, capacity, dSMarks,
                            dRMarks);
}

int hj_verify_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    return call_info(c, c->call[CALL_VERIFY], c->buf[B_VERIFY_CTR].p, 16, out);     // pairs kept, candidates dropped
}

// ---- rows of one table grouped by their key columns (hj_groups.hip) ----------
// hj_key_groups_dev's and hj_key_groups_host's arguments -> the kernels' columns; the message of what is wrong, or nullptr
static const char* key_groups_args(const hj_key_col2* cols, uint32_t nCols, uint32_t side, uint64_t nRows, const uint32_t* rep,
                                   const uint32_t* group, const uint32_t* firstRows, uint64_t capacity, KeyCols2* k)
{
    if (side > HJ_KEY_SIDE_R) return "side must be HJ_KEY_SIDE_S or HJ_KEY_SIDE_R";
    if (nRows > 0xFFFFFFFEull) return "nRows above 2^32 - 2";
    if (const char* what = key_cols_error(cols, nCols, nRows && side == HJ_KEY_SIDE_S, nRows && side == HJ_KEY_SIDE_R)) return what;
    if (nRows && !rep) return "dRep NULL with nRows > 0";
    if (nRows && capacity && !firstRows) return "dFirstRows NULL with capacity > 0";
    if (!word_ptr_ok(rep) || !word_ptr_ok(group) || !word_ptr_ok(firstRows)) return "an output pointer that is not 4-byte aligned";
    key_side_cols(cols, nCols, side, k);
    return nullptr;
}

int hj_key_groups_dev(hj_ctx* c, const hj_key_col2* cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask, uint32_t* dRep,
                      uint32_t* dGroup, uint32_t* dFirstRows, uint64_t capacity)
{
    HJ_ENTER(c, true);
    KeyCols2 k{};
    if (const char* what = key_groups_args(cols, nCols, side, nRows, dRep, dGroup, dFirstRows, capacity, &k))
        return fail(c, HJ_ERR_INVALID, "hj_key_groups_dev", what);
    HJ_HIP(c, hipSetDevice(c->device));
    if (const int rc = c->buf[B_GROUPS_CTR].reserve(c, 4 * sizeof(unsigned long long))) return rc;
    if (nRows)
        if (const int rc = c->buf[B_GROUPS_WORK].reserve(c, key_groups_work_bytes(nRows))) return rc;
    HJ_HIP(c, hipEventRecord(c->call[CALL_GROUPS].ev[0], c->stream));          // the whole call: the table's fill too
    HJ_HIP(c, launch_key_groups(k, nCols, nRows, keyMask ? keyMask : 0xFFFFFFFFu, dRep, dGroup, dFirstRows, capacity, c->buf[B_GROUPS_WORK].p,
                                c->buf[B_GROUPS_CTR].as<unsigned long long>(), c->stream));
    return call_end(c, CALL_GROUPS, capacity, nRows);
}

int hj_key_groups_info(hj_ctx* c, uint64_t out[8])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_GROUPS];
    for (int i = 4; i < 8; ++i) out[i] = 0;
    // the word behind the sweep's block counts: the first rows it found (no row: no work was enqueued and there is no word)
    const uint32_t* const total = r.called && r.rows ? key_groups_total(c->buf[B_GROUPS_WORK].p, r.rows) : nullptr;
    if (const int rc = call_info(c, r, total, sizeof(uint32_t), out)) return rc;
    if (!r.called || !r.rows) return HJ_OK;
    unsigned long long ctr[4];
    HJ_HIP(c, hipMemcpy(ctr, c->buf[B_GROUPS_CTR].p, sizeof(ctr), hipMemcpyDeviceToHost));
    out[3] = ctr[2]; out[4] = key_groups_slots(r.rows); out[5] = ctr[0]; out[6] = ctr[1]; out[7] = ctr[3];
    return HJ_OK;
}

int hj_key_groups_host(const hj_key_col2* cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask, uint32_t* rep, uint32_t* group,
                       uint32_t* firstRows, uint64_t capacity, uint64_t out[8])
{
    KeyCols2 k{};
    if (!out || key_groups_args(cols, nCols, side, nRows, rep, group, firstRows, capacity, &k)) return HJ_ERR_INVALID;
    key_groups_host(k, nCols, nRows, keyMask ? keyMask : 0xFFFFFFFFu, rep, group, firstRows, capacity, out);
    return HJ_OK;
}

// ---- rows in the order of their columns (hj_sort.hip) -------------------------
// hj_sort_rows_dev's and hj_sort_rows_host's arguments -> the kernels' columns; the message of what is wrong, or nullptr
// the columns themselves: what hj_sort_rows_* and hj_window_rows_* (its order columns) refuse of one
static const char* sort_cols_error(const hj_sort_col* cols, uint32_t nCols, uint64_t nRows, SortCols* k)
{
    for (uint32_t i = 0; i < nCols; ++i) {
        const hj_sort_col& col = cols[i];
        if (col.type > HJ_VAL_FLOAT) return "type must be an hj_val_type";
        const bool widthOk = col.width == 4 || col.width == 8 || (col.type != HJ_VAL_FLOAT && (col.width == 1 || col.width == 2));
        if (!widthOk) return "a width that the type does not have (UINT / INT: 1, 2, 4, 8; FLOAT: 4, 8)";
        if (col.flags & ~(HJ_SORT_DESC | HJ_SORT_NULLS_FIRST)) return "hj_sort_col.flags has bits other than HJ_SORT_DESC and HJ_SORT_NULLS_FIRST";
        if (col.reserved) return "hj_sort_col.reserved must be 0";
        if (nRows && !col_ptr_ok(col.values, col.width)) return "a values pointer that is NULL or not aligned to its width";
        if (nRows && !word_ptr_ok(col.valid)) return "a validity pointer that is not 4-byte aligned";
        k->p[i] = col.values; k->valid[i] = col.valid; k->width[i] = col.width; k->type[i] = col.type; k->flags[i] = col.flags;
    }
    return nullptr;
}

static const char* sort_args(const hj_sort_col* cols, uint32_t nCols, uint64_t nRows, const uint32_t* perm, SortCols* k)
{
    if (nCols == 0 || nCols > HJ_SORT_MAX_COLS) return "nCols must be 1 .. HJ_SORT_MAX_COLS";
    if (!cols) return "cols NULL";
    if (nRows > 0xFFFFFFFEull) return "nRows above 2^32 - 2";
    if (const char* what = sort_cols_error(cols, nCols, nRows, k)) return what;
    if (nRows && (!perm || !word_ptr_ok(perm))) return "dPerm NULL or not 4-byte aligned";
    return nullptr;
}

int hj_sort_rows_dev(hj_ctx* c, const hj_sort_col* cols, uint32_t nCols, uint64_t nRows, uint32_t* dPerm)
{
    HJ_ENTER(c, true);
    SortCols k{};
    if (const char* what = sort_args(cols, nCols, nRows, dPerm, &k)) return fail(c, HJ_ERR_INVALID, "hj_sort_rows_dev", what);
    HJ_HIP(c, hipSetDevice(c->device));
    const SortLayout l = sort_layout(nRows, sort_key_bytes(k, nCols));
    if (nRows)
        if (const int rc = c->buf[B_SORT_WORK].reserve(c, l.bytes)) return rc;
    HJ_HIP(c, hipEventRecord(c->call[CALL_SORT].ev[0], c->stream));
    HJ_HIP(c, launch_sort_rows(k, nCols, nRows, dPerm, c->buf[B_SORT_WORK].p, c->stream));
    c->sort = {};
    if (nRows) c->sort = {sort_passes(k, nCols), l.chunks, l.chunkRows, l.bytes};
    return call_end(c, CALL_SORT, 0, nRows);
}

int hj_sort_rows_info(hj_ctx* c, uint64_t out[8])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_SORT];
    for (int i = 4; i < 8; ++i) out[i] = 0;
    if (const int rc = call_info(c, r, nullptr, 0, out)) return rc;
    if (!r.called || !r.rows) { out[2] = 0; return HJ_OK; }     // no row: nothing was enqueued between the two events
    out[0] = r.rows; out[1] = c->sort.passes; out[3] = 0;       // no pass is ever skipped
    out[4] = c->sort.chunks; out[5] = c->sort.chunkRows; out[6] = c->sort.bytes;
    return HJ_OK;
}

int hj_sort_rows_host(const hj_sort_col* cols, uint32_t nCols, uint64_t nRows, uint32_t* perm, uint64_t out[8])
{
    SortCols k{};
    if (sort_args(cols, nCols, nRows, perm, &k)) return HJ_ERR_INVALID;
    sort_rows_host(k, nCols, nRows, perm);
    if (!out) return HJ_OK;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (!nRows) return HJ_OK;
    const SortLayout l = sort_layout(nRows, sort_key_bytes(k, nCols));
    out[0] = nRows; out[1] = sort_passes(k, nCols); out[4] = l.chunks; out[5] = l.chunkRows; out[6] = l.bytes;
    return HJ_OK;
}

int hj_sort_layout_info(uint64_t nRows, uint64_t out[4])
{
    if (!out || nRows > 0xFFFFFFFEull) return HJ_ERR_INVALID;
    const SortLayout l = sort_layout(nRows, 8);
    out[0] = l.tileRows; out[1] = l.chunkRows; out[2] = l.chunks; out[3] = l.bytes;
    return HJ_OK;
}

// ---- window functions over the runs along a permutation (hj_window.hip) --------
// hj_window_rows_dev's and hj_window_rows_host's arguments -> the kernels' columns and functions; the message of what is wrong, or nullptr
static const char* window_args(const uint32_t* perm, uint64_t nPos, uint64_t nRows, const uint32_t* part, const hj_sort_col* order, uint32_t nOrder,
                               const hj_win_func* funcs, uint32_t nFuncs, SortCols* k, WinFuncs* w)
{
    if (nFuncs == 0 || nFuncs > HJ_WIN_MAX_FUNCS) return "nFuncs must be 1 .. HJ_WIN_MAX_FUNCS";
    if (!funcs) return "funcs NULL";
    if (nPos > 0xFFFFFFFEull || nRows > 0xFFFFFFFEull) return "nPos or nRows above 2^32 - 2";
    if (nOrder > HJ_SORT_MAX_COLS) return "nOrder above HJ_SORT_MAX_COLS";
    if (nOrder && !order) return "order NULL with nOrder > 0";
    if (const char* what = sort_cols_error(order, nOrder, nRows, k)) return what;
    if (!perm && nPos > nRows) return "dPerm NULL with nPos > nRows";
    if (!word_ptr_ok(perm) || !word_ptr_ok(part)) return "dPerm or dPart not 4-byte aligned";
    for (uint32_t i = 0; i < nFuncs; ++i) {
        const hj_win_func& f = funcs[i];
        if (f.op > HJ_WIN_RUN_MAX) return "op must be an hj_win_op";
        const bool run = f.op >= HJ_WIN_RUN_COUNT, reads = f.op > HJ_WIN_RUN_COUNT;
        const bool widthOk = reads ? (f.width == 4 || f.width == 8) : run ? (f.width == 0 || f.width == 4 || f.width == 8) : f.width == 0;
        if (!widthOk) return "a width that the op does not have (RUN_SUM / MIN / MAX: 4 or 8; RUN_COUNT: 0, 4 or 8; else 0)";
        if (f.flags & ~(run ? HJ_AGG_SIGNED : 0u)) return "hj_win_func.flags has bits other than HJ_AGG_SIGNED, or any outside RUN_*";
        if (f.offset && f.op != HJ_WIN_LAG && f.op != HJ_WIN_LEAD) return "offset != 0 outside LAG / LEAD";
        if (!col_ptr_ok(f.out, run ? 8 : 4)) return "an out that is NULL or not aligned to its entries";
        if (reads && nRows && !col_ptr_ok(f.src, f.width)) return "a src that is NULL or not aligned to its width";
        if (!word_ptr_ok(f.srcValid)) return "a srcValid that is not 4-byte aligned";
        w->src[i] = f.src; w->valid[i] = run ? f.srcValid : nullptr; w->out[i] = f.out;
        w->op[i] = f.op; w->width[i] = f.width; w->sgn[i] = f.flags & HJ_AGG_SIGNED; w->offset[i] = f.offset;
    }
    return nullptr;
}

int hj_window_rows_dev(hj_ctx* c, const uint32_t* dPerm, uint64_t nPos, uint64_t nRows, const uint32_t* dPart, const hj_sort_col* order,
                       uint32_t nOrder, const hj_win_func* funcs, uint32_t nFuncs)
{
    HJ_ENTER(c, true);
    SortCols k{};
    WinFuncs w{};
    if (const char* what = window_args(dPerm, nPos, nRows, dPart, order, nOrder, funcs, nFuncs, &k, &w))
        return fail(c, HJ_ERR_INVALID, "hj_window_rows_dev", what);
    HJ_HIP(c, hipSetDevice(c->device));
    const WindowLayout l = window_layout(nPos);
    if (const int rc = c->buf[B_WINDOW_CTR].reserve(c, 3 * sizeof(unsigned long long))) return rc;
    if (nPos)
        if (const int rc = c->buf[B_WINDOW_WORK].reserve(c, l.bytes)) return rc;
    HJ_HIP(c, hipEventRecord(c->call[CALL_WINDOW].ev[0], c->stream));
    HJ_HIP(c, launch_window_rows(dPerm, nPos, (uint32_t)nRows, dPart, k, nOrder, w, nFuncs, c->buf[B_WINDOW_WORK].p,
                                 c->buf[B_WINDOW_CTR].as<unsigned long long>(), c->stream));
    c->window = {};
    if (nPos) c->window = {l.chunks, l.bytes};
    return call_end(c, CALL_WINDOW, 0, nPos);
}

int hj_window_rows_info(hj_ctx* c, uint64_t out[8])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_WINDOW];
    for (int i = 4; i < 8; ++i) out[i] = 0;
    uint64_t t[4];
    if (const int rc = call_info(c, r, nullptr, 0, t)) return rc;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!r.called || !r.rows) return HJ_OK;                     // no position: nothing was enqueued between the two events
    unsigned long long totals[3];
    HJ_HIP(c, hipMemcpy(totals, c->buf[B_WINDOW_CTR].p, sizeof(totals), hipMemcpyDeviceToHost));
    out[0] = r.rows; out[1] = totals[0]; out[2] = totals[1]; out[3] = t[2]; out[4] = totals[2];
    out[5] = c->window.chunks; out[6] = c->window.bytes;
    return HJ_OK;
}

int hj_window_rows_host(const uint32_t* perm, uint64_t nPos, uint64_t nRows, const uint32_t* part, const hj_sort_col* order, uint32_t nOrder,
                        const hj_win_func* funcs, uint32_t nFuncs, uint64_t out[8])
{
    SortCols k{};
    WinFuncs w{};
    if (window_args(perm, nPos, nRows, part, order, nOrder, funcs, nFuncs, &k, &w)) return HJ_ERR_INVALID;
    uint64_t totals[3];
    window_rows_host(perm, nPos, (uint32_t)nRows, part, k, nOrder, w, nFuncs, totals);
    if (!out) return HJ_OK;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (!nPos) return HJ_OK;
    const WindowLayout l = window_layout(nPos);
    out[0] = nPos; out[1] = totals[0]; out[2] = totals[1]; out[4] = totals[2]; out[5] = l.chunks; out[6] = l.bytes;
    return HJ_OK;
}

int hj_window_layout_info(uint64_t nPos, uint64_t out[4])
{
    if (!out || nPos > 0xFFFFFFFEull) return HJ_ERR_INVALID;
    const WindowLayout l = window_layout(nPos);
    out[0] = l.tilePos; out[1] = l.chunkPos; out[2] = l.chunks; out[3] = l.bytes;
    return HJ_OK;
}

// ---- join conditions beyond equality (hj_where.hip) --------------------------
// hj_pairs_where_dev's and hj_pairs_where_host's arguments -> the kernel's terms; the message of what is wrong, or nullptr
static const char* where_args(const uint32_t* mapS, const uint32_t* mapR, uint64_t nPairs, uint64_t sRows, uint64_t rRows,
                              const hj_where_term* terms, uint32_t nTerms, const uint32_t* outS, const uint32_t* outR, uint64_t capacity,
                              WhereTerms* k)
{
    if (nPairs > 0xFFFFFFFFull || sRows > 0xFFFFFFFFull || rRows > 0xFFFFFFFFull) return "nPairs, sRows or rRows above 2^32 - 1";
    if (nTerms == 0 || nTerms > HJ_WHERE_MAX_TERMS) return "nTerms must be 1 .. HJ_WHERE_MAX_TERMS";
    if (!terms) return "terms NULL";
    for (uint32_t i = 0; i < nTerms; ++i) {
        const hj_where_term& t = terms[i];
        if (t.type > HJ_VAL_FLOAT) return "type must be an hj_val_type";
        if (t.op > HJ_CMP_GE) return "op must be an hj_cmp_op";
        const bool widthOk = t.width == 4 || t.width == 8 || (t.type != HJ_VAL_FLOAT && (t.width == 1 || t.width == 2));
        if (!widthOk) return "a width that the type does not have (UINT / INT: 1, 2, 4, 8; FLOAT: 4, 8)";
        if (t.reserved) return "hj_where_term.reserved must be 0";
        if (sRows && !col_ptr_ok(t.s, t.width)) return "an s pointer that is NULL or not aligned to its width";
        if (rRows && !col_ptr_ok(t.r, t.width)) return "an r pointer that is NULL or not aligned to its width";
        if (!word_ptr_ok(t.sValid) || !word_ptr_ok(t.rValid)) return "a validity pointer that is not 4-byte aligned";
        k->s[i] = t.s; k->r[i] = t.r; k->sValid[i] = t.sValid; k->rValid[i] = t.rValid;
        k->width[i] = t.width; k->type[i] = t.type; k->op[i] = t.op;
    }
    if (nPairs && (!mapS || !mapR)) return "a map NULL with nPairs > 0";
    if (nPairs && capacity && (!outS || !outR)) return "an output pointer NULL with capacity > 0";
    return nullptr;
}

int hj_pairs_where_dev(hj_ctx* c, const uint32_t* dMapS, const uint32_t* dMapR, uint64_t nPairs, uint32_t sRowBase, uint64_t sRows,
                       uint64_t rRows, const hj_where_term* terms, uint32_t nTerms, uint32_t* dOutS, uint32_t* dOutR, uint64_t capacity,
                       uint32_t* dSMarks, uint32_t* dRMarks)
{
    HJ_ENTER(c, true);
    WhereTerms k{};
    if (const char* what = where_args(dMapS, dMapR, nPairs, sRows, rRows, terms, nTerms, dOutS, dOutR, capacity, &k))
        return fail(c, HJ_ERR_INVALID, "hj_pairs_where_dev", what);
    HJ_HIP(c, hipSetDevice(c->device));
    const PairsOut out{dOutS, dOutR, capacity, c->buf[B_WHERE_CTR].as<unsigned long long>()};
    HJ_HIP(c, hipMemsetAsync(out.cursor, 0, 2 * sizeof(unsigned long long), c->stream));
    HJ_HIP(c, hipEventRecord(c->call[CALL_WHERE].ev[0], c->stream));
    HJ_HIP(c, launch_pairs_where(dMapS, dMapR, nPairs, sRowBase, (uint32_t)sRows, (uint32_t)rRows, k, nTerms, out, dSMarks, dRMarks, c->stream));
    return call_end(c, CALL_WHERE, capacity, nPairs);
}

int hj_where_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    return call_info(c, c->call[CALL_WHERE], c->buf[B_WHERE_CTR].p, 16, out);       // pairs kept, pairs dropped
}

int hj_pairs_where_host(const uint32_t* mapS, const uint32_t* mapR, uint64_t nPairs, uint32_t sRowBase, uint64_t sRows, uint64_t rRows,
                        const hj_where_term* terms, uint32_t nTerms, uint32_t* outS, uint32_t* outR, uint64_t capacity, uint32_t* sMarks,
                        uint32_t* rMarks, uint64_t info[4])
{
    WhereTerms k{};
    if (where_args(mapS, mapR, nPairs, sRows, rRows, terms, nTerms, outS, outR, capacity, &k)) return HJ_ERR_INVALID;
    pairs_where_host(mapS, mapR, nPairs, sRowBase, (uint32_t)sRows, (uint32_t)rRows, k, nTerms, outS, outR, capacity, sMarks, rMarks, info);
    return HJ_OK;
}

// ---- as-of joins (hj_asof.hip) -----------------------------------------------
// hj_pairs_asof_dev's and hj_pairs_asof_host's arguments -> the kernels' term; the message of what is wrong, or nullptr
static const char* asof_args(const uint32_t* mapS, const uint32_t* mapR, uint64_t nPairs, uint64_t sRows, uint64_t rRows, const hj_asof_term* t,
                             const uint64_t* bestVal, const uint32_t* bestRow, const uint32_t* outS, const uint32_t* outR, uint64_t capacity,
                             AsofTerm* k)
{
    if (nPairs > 0xFFFFFFFFull || sRows > 0xFFFFFFFFull || rRows > 0xFFFFFFFFull) return "nPairs, sRows or rRows above 2^32 - 1";
    if (!t) return "term NULL";
    if (t->type > HJ_VAL_FLOAT) return "type must be an hj_val_type";
    if (t->op != HJ_CMP_GE && t->op != HJ_CMP_GT && t->op != HJ_CMP_LE && t->op != HJ_CMP_LT)
        return "op must be HJ_CMP_GE, HJ_CMP_GT, HJ_CMP_LE or HJ_CMP_LT";
    const bool widthOk = t->width == 4 || t->width == 8 || (t->type != HJ_VAL_FLOAT && (t->width == 1 || t->width == 2));
    if (!widthOk) return "a width that the type does not have (UINT / INT: 1, 2, 4, 8; FLOAT: 4, 8)";
    if (t->reserved) return "hj_asof_term.reserved must be 0";
    if (sRows && !col_ptr_ok(t->s, t->width)) return "an s pointer that is NULL or not aligned to its width";
    if (rRows && !col_ptr_ok(t->r, t->width)) return "an r pointer that is NULL or not aligned to its width";
    if (!word_ptr_ok(t->sValid) || !word_ptr_ok(t->rValid)) return "a validity pointer that is not 4-byte aligned";
    if (!bestVal || (reinterpret_cast<uintptr_t>(bestVal) & 7u)) return "dBestVal NULL or not 8-byte aligned";
    if (!bestRow || !word_ptr_ok(bestRow)) return "dBestRow NULL or not 4-byte aligned";
    if (nPairs && (!mapS || !mapR)) return "a map NULL with nPairs > 0";
    if (nPairs && capacity && (!outS || !outR)) return "an output pointer NULL with capacity > 0";
    *k = AsofTerm{t->s, t->r, t->sValid, t->rValid, t->width, t->type, t->op};
    return nullptr;
}

int hj_pairs_asof_dev(hj_ctx* c, const uint32_t* dMapS, const uint32_t* dMapR, uint64_t nPairs, uint32_t sRowBase, uint64_t sRows,
                      uint64_t rRows, const hj_asof_term* term, uint64_t* dBestVal, uint32_t* dBestRow, uint32_t* dOutS, uint32_t* dOutR,
                      uint64_t capacity, uint32_t* dSMarks, uint32_t* dRMarks)
{
    HJ_ENTER(c, true);
    AsofTerm k{};
    if (const char* what = asof_args(dMapS, dMapR, nPairs, sRows, rRows, term, dBestVal, dBestRow, dOutS, dOutR, capacity, &k))
        return fail(c, HJ_ERR_INVALID, "hj_pairs_asof_dev", what);
    HJ_HIP(c, hipSetDevice(c->device));
    const PairsOut out{dOutS, dOutR, capacity, c->buf[B_ASOF_CTR].as<unsigned long long>()};
    HJ_HIP(c, hipEventRecord(c->call[CALL_ASOF].ev[0], c->stream));          // the whole call: the initialisations too
    HJ_HIP(c, hipMemsetAsync(out.cursor, 0, 2 * sizeof(unsigned long long), c->stream));
    HJ_HIP(c, launch_pairs_asof(dMapS, dMapR, nPairs, sRowBase, (uint32_t)sRows, (uint32_t)rRows, k, reinterpret_cast<unsigned long long*>(dBestVal),
                                dBestRow, out, dSMarks, dRMarks, c->stream));
    return call_end(c, CALL_ASOF, capacity, nPairs);
}

int hj_asof_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    return call_info(c, c->call[CALL_ASOF], c->buf[B_ASOF_CTR].p, 16, out);        // pairs kept, pairs dropped
}

int hj_pairs_asof_host(const uint32_t* mapS, const uint32_t* mapR, uint64_t nPairs, uint32_t sRowBase, uint64_t sRows, uint64_t rRows,
                       const hj_asof_term* term, uint64_t* bestVal, uint32_t* bestRow, uint32_t* outS, uint32_t* outR, uint64_t capacity,
                       uint32_t* sMarks, uint32_t* rMarks, uint64_t info[4])
{
    AsofTerm k{};
    if (asof_args(mapS, mapR, nPairs, sRows, rRows, term, bestVal, bestRow, outS, outR, capacity, &k)) return HJ_ERR_INVALID;
    pairs_asof_host(mapS, mapR, nPairs, sRowBase, (uint32_t)sRows, (uint32_t)rRows, k, bestVal, bestRow, outS, outR, capacity, sMarks, rMarks, info);
    return HJ_OK;
}

// ---- the reduction over a pair list (hj_agg.hip) ----------------------------
int hj_pairs_agg_dev(hj_ctx* c, const uint32_t* dMapG, const uint32_t* dMapV, uint64_t nPairs, uint32_t gBase, uint64_t gRows, uint32_t vBase,
                     uint64_t vRows, const hj_agg_col* cols, uint32_t nCols, uint64_t* dCount)
{
    HJ_ENTER(c, true);
    const char* const fn = "hj_pairs_agg_dev";
    if (nCols > HJ_AGG_MAX_COLS) return fail(c, HJ_ERR_INVALID, fn, "more than HJ_AGG_MAX_COLS columns");
    if (nCols && !cols) return fail(c, HJ_ERR_INVALID, fn, "cols NULL with nCols > 0");
    if (!nCols && !dCount) return fail(c, HJ_ERR_INVALID, fn, "neither a column nor dCount");
    if (nPairs > 0xFFFFFFFFull || gRows > 0xFFFFFFFFull || vRows > 0xFFFFFFFFull)
        return fail(c, HJ_ERR_INVALID, fn, "nPairs, gRows or vRows above 2^32 - 1");
    if (nPairs && !dMapG) return fail(c, HJ_ERR_INVALID, fn, "dMapG NULL with nPairs > 0");
    if (reinterpret_cast<uintptr_t>(dCount) & 7u) return fail(c, HJ_ERR_INVALID, fn, "dCount not 8-byte aligned");
    PairAggCols k{};
    for (uint32_t i = 0; i < nCols; ++i) {
        const hj_agg_col& col = cols[i];
        if (col.op > HJ_AGG_MAX) return fail(c, HJ_ERR_INVALID, fn, "op must be an hj_agg_op");
        if (col.op == HJ_AGG_COUNT ? col.width != 0 : (col.width != 4 && col.width != 8))
            return fail(c, HJ_ERR_INVALID, fn, "a width that is not 4 or 8 (HJ_AGG_COUNT: 0)");
        if (col.flags & ~HJ_AGG_SIGNED) return fail(c, HJ_ERR_INVALID, fn, "hj_agg_col.flags has bits other than HJ_AGG_SIGNED");
        if (col.reserved) return fail(c, HJ_ERR_INVALID, fn, "hj_agg_col.reserved must be 0");
        if (!col.acc || (reinterpret_cast<uintptr_t>(col.acc) & 7u)) return fail(c, HJ_ERR_INVALID, fn, "an acc that is NULL or not 8-byte aligned");
        if (!word_ptr_ok(col.srcValid)) return fail(c, HJ_ERR_INVALID, fn, "a srcValid that is not 4-byte aligned");
        if (col.width && vRows && !col_ptr_ok(col.src, col.width)) return fail(c, HJ_ERR_INVALID, fn, "a src that is NULL or not aligned to its width");
        if (nPairs && !dMapV && (col.width || col.srcValid)) return fail(c, HJ_ERR_INVALID, fn, "dMapV NULL with a column that reads S values or validity");
        k.src.p[i] = col.src; k.src.valid[i] = col.srcValid; k.acc[i] = static_cast<unsigned long long*>(col.acc);
        k.ops.op[i] = col.op; k.ops.width[i] = col.width; k.ops.sgn[i] = col.flags & HJ_AGG_SIGNED;
    }
    HJ_HIP(c, hipSetDevice(c->device));
    if (const int rc = c->buf[B_PAIRS_AGG_CTR].reserve(c, 2 * sizeof(unsigned long long))) return rc;
    unsigned long long* const counts = c->buf[B_PAIRS_AGG_CTR].as<unsigned long long>();
    HJ_HIP(c, hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), c->stream));
    HJ_HIP(c, hipEventRecord(c->call[CALL_PAIRS_AGG].ev[0], c->stream));
    HJ_HIP(c, launch_pairs_agg(dMapG, dMapV, nPairs, gBase, (uint32_t)gRows, vBase, (uint32_t)vRows, k, nCols,
                               reinterpret_cast<unsigned long long*>(dCount), counts, c->stream));
    return call_end(c, CALL_PAIRS_AGG, 0, nPairs);
}

int hj_pairs_agg_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_PAIRS_AGG];  // pairs applied, pairs skipped
    if (const int rc = call_info(c, r, c->buf[B_PAIRS_AGG_CTR].p, 16, out)) return rc;
    out[1] = out[0]; out[0] = r.called ? r.rows : 0;
    return HJ_OK;
}

int hj_mark_rows_dev(hj_ctx* c, const uint32_t* dMarks, uint64_t rows, uint32_t rowBase, uint32_t which, uint32_t* dOut, uint64_t capacity)
{
    HJ_ENTER(c, true);
    if (which > HJ_R_MATCHED) return fail(c, HJ_ERR_INVALID, "hj_mark_rows_dev: which must be HJ_R_UNMATCHED or HJ_R_MATCHED");
    if (rows > 0xFFFFFFFFull || (uint64_t)rowBase + rows > 0xFFFFFFFFull)
        return fail(c, HJ_ERR_INVALID, "hj_mark_rows_dev: rows or rowBase + rows above 2^32 - 1");
    if (rows && !dMarks) return fail(c, HJ_ERR_INVALID, "hj_mark_rows_dev: dMarks NULL with rows > 0");
    if (rows && capacity && !dOut) return fail(c, HJ_ERR_INVALID, "hj_mark_rows_dev: output pointer NULL with capacity > 0");
    HJ_HIP(c, hipSetDevice(c->device));
    if (const int rc = c->buf[B_MARK_SWEEP].reserve(c, r_sweep_count_words(rows) * sizeof(uint32_t))) return rc;
    HJ_HIP(c, hipEventRecord(c->call[CALL_MARK_ROWS].ev[0], c->stream));
    // the sweep reads the plane and never writes it
    const RMarks mk{const_cast<uint32_t*>(dMarks), rowBase, (uint32_t)rows};
    HJ_HIP(c, launch_r_sweep(mk, which == HJ_R_MATCHED, dOut, capacity, c->buf[B_MARK_SWEEP].as<uint32_t>(), c->stream));
    return call_end(c, CALL_MARK_ROWS, capacity, rows);
}

int hj_mark_rows_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    // the word behind the block counts: their total after the scan (no block: no row)
    const CallRecord& r = c->call[CALL_MARK_ROWS];
    const uint32_t* const total = r.rows ? c->buf[B_MARK_SWEEP].as<uint32_t>() + r_sweep_blocks(r.rows) : nullptr;
    if (const int rc = call_info(c, r, total, sizeof(uint32_t), out)) return rc;
    out[3] = r.rows;
    return HJ_OK;
}

}  // extern "C"
