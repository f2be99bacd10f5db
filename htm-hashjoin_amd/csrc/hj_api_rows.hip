// hj_api_rows.hip -- the C ABI's calls on rows: the R-side match marks and their sweep, the gather through a row map, the
// joins on real key columns (hash, verify, sweep of a caller's plane), the rows of one table grouped by their key columns
// and sorted by them, the window functions along a permutation and their sliding frames, the join conditions beyond
// equality, the as-of step, the range joins without an equality key, the reduction over a pair list, and the *_info entry
// point of every call that has a record (hj_host.h: CallRecord).
// Host-side glue only, and the same three parts for every recorded call: its checks, which give the message of the first
// thing wrong; recorded_call, the one frame around its launch; call_info, the one reader of what it left.
#include "hj_host.h"

using namespace hjapi;

extern "C" {

// Waits for the stream. The last call of kind `which` in the common form of the *_info entry points: out[0] = the call's
// first counter word, out[1] = min(out[0], capacity), out[2] = its device time in microseconds, out[3] = the second word.
// words (kCallWords of them, or nullptr: the kind counts nothing): the kind's block (call_words) as the call left it,
// copied to the host once and whole; a caller that reports more than two words reads the rest there. dTotal (or nullptr): the
// first word is this 32-bit total in a workspace instead, and out[3] is 0. All 0, words too, for a call that was never
// made, or forgotten since.
static int call_info(hj_ctx* c, Call which, const uint32_t* dTotal, unsigned long long* words, uint64_t out[4])
{
    const CallRecord& rec = c->call[which];
    HJ_HIP(c, hipSetDevice(c->device));
    HJ_HIP(c, hipStreamSynchronize(c->stream));
    out[0] = out[1] = out[2] = out[3] = 0;
    for (uint32_t i = 0; words && i < kCallWords; ++i) words[i] = 0;
    if (!rec.called) return HJ_OK;
    uint32_t total = 0;
    if (dTotal) HJ_HIP(c, hipMemcpy(&total, dTotal, sizeof(total), hipMemcpyDeviceToHost));
    if (words) HJ_HIP(c, hipMemcpy(words, call_words(c, which), kCallWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    float ms = 0;
    if (!rec.timed || hipEventElapsedTime(&ms, rec.ev[0], rec.ev[1]) != hipSuccess) ms = 0;
    out[0] = dTotal ? total : words ? words[0] : 0;
    out[1] = out[0] < rec.capacity ? out[0] : rec.capacity;
    out[2] = (uint64_t)((double)ms * 1000.0 + 0.5);
    out[3] = !dTotal && words ? words[1] : 0;
    return HJ_OK;
}
// the kinds whose block holds the two words and nothing else
static int call_info(hj_ctx* c, Call which, uint64_t out[4])
{
    unsigned long long words[kCallWords];       // copied and not looked at again
    return call_info(c, which, nullptr, words, out);
}

// The one frame of a recorded call, in the order every entry point has always made its HIP calls: the device; the call's
// workspace grown (work.bytes 0: it has none); `zero` words of the kind's block zeroed on the stream (0: the launcher zeroes
// its own, or the kind counts nothing); ev[0]; launch(the kind's block); ev[1] and what *_info is to report (call_end, extra).
// init says on which side of the zeroing ev[0] stands. INIT_TIMED, in front of it: the calls whose time is "the whole call" --
// as-of, whose launcher goes on to initialise the caller's best planes, and groups and window, whose launchers fill their
// workspace and zero their own words. INIT_UNTIMED, behind it: all the others, whose time is their kernels'. The intervals
// are what the benchmark write-ups under profiles/ report, so a call keeps its side.
enum Init { INIT_UNTIMED, INIT_TIMED };
struct Work { Buf b; size_t bytes; };
constexpr Work kNoWork{B_COUNT, 0};
struct Facts { uint64_t capacity, rows, extra[4]; };
extern "C++" {
template <class Launch>
static int recorded_call(hj_ctx* c, Call which, uint32_t zero, Init init, Work work, const Facts& facts, Launch&& launch)
{
    CallRecord& r = c->call[which];
    unsigned long long* const words = call_words(c, which);
    HJ_HIP(c, hipSetDevice(c->device));
    if (work.bytes)
        if (const int rc = c->buf[work.b].reserve(c, work.bytes)) return rc;
    if (init == INIT_TIMED) HJ_HIP(c, hipEventRecord(r.ev[0], c->stream));
    if (zero) HJ_HIP(c, hipMemsetAsync(words, 0, zero * sizeof(unsigned long long), c->stream));
    if (init == INIT_UNTIMED) HJ_HIP(c, hipEventRecord(r.ev[0], c->stream));
    HJ_HIP(c, launch(words));
    if (const int rc = call_end(c, which, facts.capacity, facts.rows)) return rc;
    for (int i = 0; i < 4; ++i) r.extra[i] = facts.extra[i];
    return HJ_OK;
}
}  // extern "C++"

int hj_pairs_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_PAIRS];      // the cursor = rows found; LEFT's unmatched S tuples
    if (const int rc = call_info(c, CALL_PAIRS, out)) return rc;
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
    const RMarks mk{c->buf[B_R_MARKS].as<uint32_t>(), (uint32_t)c->marks.base, (uint32_t)c->marks.rows};
    return recorded_call(c, CALL_R_ROWS, 0, INIT_UNTIMED, kNoWork, Facts{capacity, c->marks.rows}, [&](unsigned long long*) {
        return launch_r_sweep(mk, which == HJ_R_MATCHED, dOutR, capacity, c->buf[B_R_SWEEP].as<uint32_t>(), c->stream);
    });
}

int hj_r_rows_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    if (const int rc = marks_state(c, "hj_r_rows_info")) return rc;
    // the word behind the block counts: their total after the scan
    if (const int rc = call_info(c, CALL_R_ROWS, c->buf[B_R_SWEEP].as<uint32_t>() + r_sweep_blocks(c->marks.rows), nullptr, out)) return rc;
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
    return recorded_call(c, CALL_GATHER, 2, INIT_UNTIMED, kNoWork, Facts{0, nRows},
                         [&](unsigned long long* counts) { return launch_gather(dMap, nRows, rowBase, srcRows, k, nCols, dValid, counts, c->stream); });
}

int hj_gather_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_GATHER];     // NULL rows, out-of-range entries
    if (const int rc = call_info(c, CALL_GATHER, out)) return rc;
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
    bool varlen = false;
    for (uint32_t i = 0; i < nCols; ++i) varlen = varlen || !k.col[i].width;
    const Work work{B_GATHER2_WORK, varlen ? gather2_work_words(nRows) * sizeof(uint32_t) : 0};
    return recorded_call(c, CALL_GATHER2, 2, INIT_UNTIMED, work, Facts{0, nRows}, [&](unsigned long long* counts) {
        return launch_gather2(dMap, nRows, rowBase, srcRows, k, nCols, dValid, counts, counts + 2, c->buf[B_GATHER2_WORK].as<uint32_t>(), c->stream);
    });
}

int hj_gather2_info(hj_ctx* c, uint64_t out[4 + HJ_GATHER_MAX_COLS])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_GATHER2];
    unsigned long long words[kCallWords];
    for (uint32_t i = 0; i < HJ_GATHER_MAX_COLS; ++i) out[4 + i] = 0;
    if (const int rc = call_info(c, CALL_GATHER2, nullptr, words, out)) return rc;
    out[1] = out[0]; out[0] = r.called ? r.rows : 0;
    for (uint32_t i = 0; i < HJ_GATHER_MAX_COLS; ++i) out[4 + i] = words[2 + i];
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

// The pair list and its sink as hj_pairs_verify*_dev, hj_pairs_where_* and hj_pairs_asof_* take them. Checked in two halves,
// sizes_error in front of a call's columns or terms and ptrs_error behind them: that is the order in which every one of these
// entry points refuses, and for any combination of bad arguments the first refusal reported is to stay what it was.
struct PairArgs {
    const uint32_t *mapS, *mapR; uint64_t nPairs; uint32_t sRowBase; uint64_t sRows, rRows;
    uint32_t *outS, *outR; uint64_t capacity; uint32_t *sMarks, *rMarks;
    const char* sizes_error() const
    {
        return nPairs > 0xFFFFFFFFull || sRows > 0xFFFFFFFFull || rRows > 0xFFFFFFFFull ? "nPairs, sRows or rRows above 2^32 - 1" : nullptr;
    }
    const char* ptrs_error() const
    {
        if (nPairs && (!mapS || !mapR)) return "a map NULL with nPairs > 0";
        if (nPairs && capacity && (!outS || !outR)) return "an output pointer NULL with capacity > 0";
        return nullptr;
    }
    // as the launchers and the host twins take them, once the sizes are checked (the host twins have no cursor)
    PairList list() const { return PairList{mapS, mapR, nPairs, sRowBase, (uint32_t)sRows, (uint32_t)rRows}; }
    PairSink sink(unsigned long long* cursor = nullptr) const { return PairSink{PairsOut{outS, outR, capacity, cursor}, sMarks, rMarks}; }
};

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
    HJ_HIP(c, launch_key_hash2(k, nCols, nRows, effective_mask(keyMask), dOutTuples, c->stream));
    return HJ_OK;
}

template <class Col>
static int key_hash_on_host(const Col* cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask, uint64_t* outTuples)
{
    KeyCols2 k{};
    if (key_hash_args(cols, nCols, side, nRows, outTuples, &k)) return HJ_ERR_INVALID;
    key_hash2_host(k, nCols, nRows, effective_mask(keyMask), outTuples);
    return HJ_OK;
}

// hj_pairs_verify_dev and hj_pairs_verify2_dev behind their names: one call record and one cursor (hj_verify_info reports
// the last call of either)
template <class Col>
static int pairs_verify_dev(hj_ctx* c, const char* fn, const PairArgs& a, const Col* cols, uint32_t nCols)
{
    if (const char* what = a.sizes_error()) return fail(c, HJ_ERR_INVALID, fn, what);
    if (const char* what = key_cols_error(cols, nCols, a.sRows != 0, a.rRows != 0)) return fail(c, HJ_ERR_INVALID, fn, what);
    if (const char* what = a.ptrs_error()) return fail(c, HJ_ERR_INVALID, fn, what);
    KeyCols2SR k{};
    for (uint32_t i = 0; i < nCols; ++i) {
        const hj_key_col2 col = key_col2_of(cols[i]);
        k.s[i] = col.s; k.r[i] = col.r; k.sOff[i] = col.sOffsets; k.rOff[i] = col.rOffsets;
        k.sValid[i] = col.sValid; k.rValid[i] = col.rValid; k.width[i] = col.width; k.flags[i] = col.flags;
    }
    return recorded_call(c, CALL_VERIFY, 2, INIT_UNTIMED, kNoWork, Facts{a.capacity, a.nPairs},
                         [&](unsigned long long* cursor) { return launch_pairs_verify2(a.list(), k, nCols, a.sink(cursor), c->stream); });
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
    const PairArgs a{dMapS, dMapR, nPairs, sRowBase, sRows, rRows, dOutS, dOutR, capacity, dSMarks, dRMarks};
    return pairs_verify_dev(c, "hj_pairs_verify_dev", a, cols, nCols);
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
    const PairArgs a{dMapS, dMapR, nPairs, sRowBase, sRows, rRows, dOutS, dOutR, capacity, dSMarks, dRMarks};
    return pairs_verify_dev(c, "hj_pairs_verify2_dev", a, cols, nCols);
}

int hj_verify_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    return call_info(c, CALL_VERIFY, out);          // pairs kept, candidates dropped
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
    const Work work{B_GROUPS_WORK, nRows ? key_groups_work_bytes(nRows) : 0};
    return recorded_call(c, CALL_GROUPS, 0, INIT_TIMED, work, Facts{capacity, nRows}, [&](unsigned long long* ctr) {
        return launch_key_groups(k, nCols, nRows, effective_mask(keyMask), dRep, dGroup, dFirstRows, capacity, c->buf[B_GROUPS_WORK].p, ctr, c->stream);
    });
}

int hj_key_groups_info(hj_ctx* c, uint64_t out[8])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_GROUPS];
    for (int i = 4; i < 8; ++i) out[i] = 0;
    // the word behind the sweep's block counts: the first rows it found (no row: no work was enqueued and there is no word)
    const uint32_t* const total = r.called && r.rows ? key_groups_total(c->buf[B_GROUPS_WORK].p, r.rows) : nullptr;
    unsigned long long ctr[kCallWords];
    if (const int rc = call_info(c, CALL_GROUPS, total, total ? ctr : nullptr, out)) return rc;
    if (!total) return HJ_OK;
    out[3] = ctr[2]; out[4] = key_groups_slots(r.rows); out[5] = ctr[0]; out[6] = ctr[1]; out[7] = ctr[3];
    return HJ_OK;
}

int hj_key_groups_host(const hj_key_col2* cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask, uint32_t* rep, uint32_t* group,
                       uint32_t* firstRows, uint64_t capacity, uint64_t out[8])
{
    KeyCols2 k{};
    if (!out || key_groups_args(cols, nCols, side, nRows, rep, group, firstRows, capacity, &k)) return HJ_ERR_INVALID;
    key_groups_host(k, nCols, nRows, effective_mask(keyMask), rep, group, firstRows, capacity, out);
    return HJ_OK;
}

// ---- typed value columns: the sort's, and the terms of where and as-of --------
// A column of hj_val_type values and the widths the type has. opError: a term's own refusal of its op, which ranks between
// the two checks; nullptr for a column, and for a term whose op is in order.
static const char* val_col_error(uint32_t type, uint32_t width, const char* opError = nullptr)
{
    if (type > HJ_VAL_FLOAT) return "type must be an hj_val_type";
    if (opError) return opError;
    const bool widthOk = width == 4 || width == 8 || (type != HJ_VAL_FLOAT && (width == 1 || width == 2));
    return widthOk ? nullptr : "a width that the type does not have (UINT / INT: 1, 2, 4, 8; FLOAT: 4, 8)";
}

// ---- rows in the order of their columns (hj_sort.hip) -------------------------
// hj_sort_rows_dev's and hj_sort_rows_host's arguments -> the kernels' columns; the message of what is wrong, or nullptr
// the columns themselves: what hj_sort_rows_* and hj_window_rows_* (its order columns) refuse of one
static const char* sort_cols_error(const hj_sort_col* cols, uint32_t nCols, uint64_t nRows, SortCols* k)
{
    for (uint32_t i = 0; i < nCols; ++i) {
        const hj_sort_col& col = cols[i];
        if (const char* what = val_col_error(col.type, col.width)) return what;
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
    const SortLayout l = sort_layout(nRows, sort_key_bytes(k, nCols));
    const Facts facts = nRows ? Facts{0, nRows, {sort_passes(k, nCols), l.chunks, l.chunkRows, l.bytes}} : Facts{};
    return recorded_call(c, CALL_SORT, 0, INIT_UNTIMED, Work{B_SORT_WORK, nRows ? l.bytes : 0}, facts,
                         [&](unsigned long long*) { return launch_sort_rows(k, nCols, nRows, dPerm, c->buf[B_SORT_WORK].p, c->stream); });
}

int hj_sort_rows_info(hj_ctx* c, uint64_t out[8])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_SORT];
    for (int i = 4; i < 8; ++i) out[i] = 0;
    if (const int rc = call_info(c, CALL_SORT, nullptr, nullptr, out)) return rc;
    if (!r.called || !r.rows) { out[2] = 0; return HJ_OK; }     // no row: nothing was enqueued between the two events
    out[0] = r.rows; out[1] = r.extra[0]; out[3] = 0;           // the passes: none is ever skipped
    out[4] = r.extra[1]; out[5] = r.extra[2]; out[6] = r.extra[3];
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
    const WindowLayout l = window_layout(nPos);
    const Facts facts = nPos ? Facts{0, nPos, {l.chunks, l.bytes}} : Facts{};
    return recorded_call(c, CALL_WINDOW, 0, INIT_TIMED, Work{B_WINDOW_WORK, nPos ? l.bytes : 0}, facts, [&](unsigned long long* totals) {
        return launch_window_rows(dPerm, nPos, (uint32_t)nRows, dPart, k, nOrder, w, nFuncs, c->buf[B_WINDOW_WORK].p, totals, c->stream);
    });
}

int hj_window_rows_info(hj_ctx* c, uint64_t out[8])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_WINDOW];
    for (int i = 4; i < 8; ++i) out[i] = 0;
    uint64_t t[4];
    unsigned long long totals[kCallWords];
    if (const int rc = call_info(c, CALL_WINDOW, nullptr, r.rows ? totals : nullptr, t)) return rc;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!r.called || !r.rows) return HJ_OK;                     // no position: nothing was enqueued between the two events
    out[0] = r.rows; out[1] = totals[0]; out[2] = totals[1]; out[3] = t[2]; out[4] = totals[2];
    out[5] = r.extra[0]; out[6] = r.extra[1];
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

// ---- sliding window frames over the same runs (hj_frames.hip) -------------------
// hj_window_frames_dev's and hj_window_frames_host's arguments -> the kernels' functions; the message of what is wrong, or nullptr
static const char* frames_args(const uint32_t* perm, uint64_t nPos, uint64_t nRows, const uint32_t* part, const hj_frame_func* funcs, uint32_t nFuncs,
                               FrameFunc* w)
{
    constexpr int64_t kMaxOffset = 0xFFFFFFFFll;
    if (nFuncs == 0 || nFuncs > HJ_FRAME_MAX_FUNCS) return "nFuncs must be 1 .. HJ_FRAME_MAX_FUNCS";
    if (!funcs) return "funcs NULL";
    if (nPos > 0xFFFFFFFEull || nRows > 0xFFFFFFFEull) return "nPos or nRows above 2^32 - 2";
    if (!perm && nPos > nRows) return "dPerm NULL with nPos > nRows";
    if (!word_ptr_ok(perm) || !word_ptr_ok(part)) return "dPerm or dPart not 4-byte aligned";
    for (uint32_t i = 0; i < nFuncs; ++i) {
        const hj_frame_func& f = funcs[i];
        if (f.op > HJ_AGG_MAX) return "op must be an hj_agg_op";
        const bool reads = f.op != HJ_AGG_COUNT;
        if (!(f.width == 4 || f.width == 8 || (!reads && f.width == 0))) return "a width that the op does not have (SUM / MIN / MAX: 4 or 8; COUNT: 0, 4 or 8)";
        if (f.flags & ~(HJ_AGG_SIGNED | HJ_FRAME_UNBOUNDED_LO | HJ_FRAME_UNBOUNDED_HI))
            return "hj_frame_func.flags has bits other than HJ_AGG_SIGNED, HJ_FRAME_UNBOUNDED_LO and HJ_FRAME_UNBOUNDED_HI";
        if (f.reserved) return "hj_frame_func.reserved must be 0";
        const bool unbLo = f.flags & HJ_FRAME_UNBOUNDED_LO, unbHi = f.flags & HJ_FRAME_UNBOUNDED_HI;
        if (f.lo < -kMaxOffset || f.lo > kMaxOffset || f.hi < -kMaxOffset || f.hi > kMaxOffset) return "lo or hi outside [-(2^32 - 1), 2^32 - 1]";
        if ((unbLo && f.lo) || (unbHi && f.hi)) return "a non-zero offset beside its HJ_FRAME_UNBOUNDED flag";
        if (!unbLo && !unbHi && f.lo > f.hi) return "lo > hi";
        if (!col_ptr_ok(f.out, 8)) return "an out that is NULL or not 8-byte aligned";
        if (reads && nRows && !col_ptr_ok(f.src, f.width)) return "a src that is NULL or not aligned to its width";
        if (!word_ptr_ok(f.srcValid)) return "a srcValid that is not 4-byte aligned";
        w[i] = FrameFunc{f.src, f.srcValid, f.out, f.lo, f.hi, f.op, f.width, f.flags & HJ_AGG_SIGNED, unbLo, unbHi};
    }
    return nullptr;
}

int hj_window_frames_dev(hj_ctx* c, const uint32_t* dPerm, uint64_t nPos, uint64_t nRows, const uint32_t* dPart, const hj_frame_func* funcs, uint32_t nFuncs)
{
    HJ_ENTER(c, true);
    FrameFunc w[kFrameMaxFuncs];
    if (const char* what = frames_args(dPerm, nPos, nRows, dPart, funcs, nFuncs, w)) return fail(c, HJ_ERR_INVALID, "hj_window_frames_dev", what);
    const FramesLayout l = frames_layout(nPos);
    const Facts facts = nPos ? Facts{0, nPos, {l.chunks, l.bytes}} : Facts{};
    return recorded_call(c, CALL_FRAMES, 0, INIT_TIMED, Work{B_FRAMES_WORK, nPos ? l.bytes : 0}, facts, [&](unsigned long long* totals) {
        return launch_window_frames(dPerm, nPos, (uint32_t)nRows, dPart, w, nFuncs, c->buf[B_FRAMES_WORK].p, totals, c->stream);
    });
}

int hj_window_frames_info(hj_ctx* c, uint64_t out[8])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_FRAMES];
    for (int i = 4; i < 8; ++i) out[i] = 0;
    uint64_t t[4];
    unsigned long long totals[kCallWords];
    if (const int rc = call_info(c, CALL_FRAMES, nullptr, r.rows ? totals : nullptr, t)) return rc;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!r.called || !r.rows) return HJ_OK;                     // no position: nothing was enqueued between the two events
    out[0] = r.rows; out[1] = totals[0]; out[3] = t[2]; out[4] = totals[2];
    out[5] = r.extra[0]; out[6] = r.extra[1];
    return HJ_OK;
}

int hj_window_frames_host(const uint32_t* perm, uint64_t nPos, uint64_t nRows, const uint32_t* part, const hj_frame_func* funcs, uint32_t nFuncs,
                          uint64_t out[8])
{
    FrameFunc w[kFrameMaxFuncs];
    if (frames_args(perm, nPos, nRows, part, funcs, nFuncs, w)) return HJ_ERR_INVALID;
    uint64_t totals[3];
    window_frames_host(perm, nPos, (uint32_t)nRows, part, w, nFuncs, totals);
    if (!out) return HJ_OK;
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (!nPos) return HJ_OK;
    const FramesLayout l = frames_layout(nPos);
    out[0] = nPos; out[1] = totals[0]; out[4] = totals[2]; out[5] = l.chunks; out[6] = l.bytes;
    return HJ_OK;
}

int hj_frames_layout_info(uint64_t nPos, uint64_t out[4])
{
    if (!out || nPos > 0xFFFFFFFEull) return HJ_ERR_INVALID;
    const FramesLayout l = frames_layout(nPos);
    out[0] = l.tilePos; out[1] = l.chunkPos; out[2] = l.chunks; out[3] = l.bytes;
    return HJ_OK;
}

// ---- join conditions beyond equality (hj_where.hip) --------------------------
// What the condition step and the as-of step refuse of one term: hj_asof_term has hj_where_term's fields. opError: the step's
// own rule for the op (val_col_error); reservedError: the text with the step's struct name.
extern "C++" {
template <class Term>
static const char* term_error(const Term& t, const char* opError, const char* reservedError, const PairArgs& a)
{
    if (const char* what = val_col_error(t.type, t.width, opError)) return what;
    if (t.reserved) return reservedError;
    if (a.sRows && !col_ptr_ok(t.s, t.width)) return "an s pointer that is NULL or not aligned to its width";
    if (a.rRows && !col_ptr_ok(t.r, t.width)) return "an r pointer that is NULL or not aligned to its width";
    if (!word_ptr_ok(t.sValid) || !word_ptr_ok(t.rValid)) return "a validity pointer that is not 4-byte aligned";
    return nullptr;
}
}  // extern "C++"

// hj_pairs_where_dev's and hj_pairs_where_host's arguments -> the kernel's terms; the message of what is wrong, or nullptr
static const char* where_args(const PairArgs& a, const hj_where_term* terms, uint32_t nTerms, WhereTerms* k)
{
    if (const char* what = a.sizes_error()) return what;
    if (nTerms == 0 || nTerms > HJ_WHERE_MAX_TERMS) return "nTerms must be 1 .. HJ_WHERE_MAX_TERMS";
    if (!terms) return "terms NULL";
    for (uint32_t i = 0; i < nTerms; ++i) {
        const hj_where_term& t = terms[i];
        if (const char* what = term_error(t, t.op > HJ_CMP_GE ? "op must be an hj_cmp_op" : nullptr, "hj_where_term.reserved must be 0", a)) return what;
        k->s[i] = t.s; k->r[i] = t.r; k->sValid[i] = t.sValid; k->rValid[i] = t.rValid;
        k->width[i] = t.width; k->type[i] = t.type; k->op[i] = t.op;
    }
    return a.ptrs_error();
}

int hj_pairs_where_dev(hj_ctx* c, const uint32_t* dMapS, const uint32_t* dMapR, uint64_t nPairs, uint32_t sRowBase, uint64_t sRows,
                       uint64_t rRows, const hj_where_term* terms, uint32_t nTerms, uint32_t* dOutS, uint32_t* dOutR, uint64_t capacity,
                       uint32_t* dSMarks, uint32_t* dRMarks)
{
    HJ_ENTER(c, true);
    const PairArgs a{dMapS, dMapR, nPairs, sRowBase, sRows, rRows, dOutS, dOutR, capacity, dSMarks, dRMarks};
    WhereTerms k{};
    if (const char* what = where_args(a, terms, nTerms, &k)) return fail(c, HJ_ERR_INVALID, "hj_pairs_where_dev", what);
    return recorded_call(c, CALL_WHERE, 2, INIT_UNTIMED, kNoWork, Facts{capacity, nPairs},
                         [&](unsigned long long* cursor) { return launch_pairs_where(a.list(), k, nTerms, a.sink(cursor), c->stream); });
}

int hj_where_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    return call_info(c, CALL_WHERE, out);           // pairs kept, pairs dropped
}

int hj_pairs_where_host(const uint32_t* mapS, const uint32_t* mapR, uint64_t nPairs, uint32_t sRowBase, uint64_t sRows, uint64_t rRows,
                        const hj_where_term* terms, uint32_t nTerms, uint32_t* outS, uint32_t* outR, uint64_t capacity, uint32_t* sMarks,
                        uint32_t* rMarks, uint64_t info[4])
{
    const PairArgs a{mapS, mapR, nPairs, sRowBase, sRows, rRows, outS, outR, capacity, sMarks, rMarks};
    WhereTerms k{};
    if (where_args(a, terms, nTerms, &k)) return HJ_ERR_INVALID;
    pairs_where_host(a.list(), k, nTerms, a.sink(), info);
    return HJ_OK;
}

// ---- as-of joins (hj_asof.hip) -----------------------------------------------
// hj_pairs_asof_dev's and hj_pairs_asof_host's arguments -> the kernels' term; the message of what is wrong, or nullptr
static const char* asof_args(const PairArgs& a, const hj_asof_term* t, const uint64_t* bestVal, const uint32_t* bestRow, AsofTerm* k)
{
    if (const char* what = a.sizes_error()) return what;
    if (!t) return "term NULL";
    const bool opOk = t->op == HJ_CMP_GE || t->op == HJ_CMP_GT || t->op == HJ_CMP_LE || t->op == HJ_CMP_LT;
    if (const char* what = term_error(*t, opOk ? nullptr : "op must be HJ_CMP_GE, HJ_CMP_GT, HJ_CMP_LE or HJ_CMP_LT", "hj_asof_term.reserved must be 0", a))
        return what;
    if (!bestVal || (reinterpret_cast<uintptr_t>(bestVal) & 7u)) return "dBestVal NULL or not 8-byte aligned";
    if (!bestRow || !word_ptr_ok(bestRow)) return "dBestRow NULL or not 4-byte aligned";
    if (const char* what = a.ptrs_error()) return what;
    *k = AsofTerm{t->s, t->r, t->sValid, t->rValid, t->width, t->type, t->op};
    return nullptr;
}

int hj_pairs_asof_dev(hj_ctx* c, const uint32_t* dMapS, const uint32_t* dMapR, uint64_t nPairs, uint32_t sRowBase, uint64_t sRows,
                      uint64_t rRows, const hj_asof_term* term, uint64_t* dBestVal, uint32_t* dBestRow, uint32_t* dOutS, uint32_t* dOutR,
                      uint64_t capacity, uint32_t* dSMarks, uint32_t* dRMarks)
{
    HJ_ENTER(c, true);
    const PairArgs a{dMapS, dMapR, nPairs, sRowBase, sRows, rRows, dOutS, dOutR, capacity, dSMarks, dRMarks};
    AsofTerm k{};
    if (const char* what = asof_args(a, term, dBestVal, dBestRow, &k)) return fail(c, HJ_ERR_INVALID, "hj_pairs_asof_dev", what);
    return recorded_call(c, CALL_ASOF, 2, INIT_TIMED, kNoWork, Facts{capacity, nPairs}, [&](unsigned long long* cursor) {
        return launch_pairs_asof(a.list(), k, reinterpret_cast<unsigned long long*>(dBestVal), dBestRow, a.sink(cursor), c->stream);
    });
}

int hj_asof_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    return call_info(c, CALL_ASOF, out);            // pairs kept, pairs dropped
}

int hj_pairs_asof_host(const uint32_t* mapS, const uint32_t* mapR, uint64_t nPairs, uint32_t sRowBase, uint64_t sRows, uint64_t rRows,
                       const hj_asof_term* term, uint64_t* bestVal, uint32_t* bestRow, uint32_t* outS, uint32_t* outR, uint64_t capacity,
                       uint32_t* sMarks, uint32_t* rMarks, uint64_t info[4])
{
    const PairArgs a{mapS, mapR, nPairs, sRowBase, sRows, rRows, outS, outR, capacity, sMarks, rMarks};
    AsofTerm k{};
    if (asof_args(a, term, bestVal, bestRow, &k)) return HJ_ERR_INVALID;
    pairs_asof_host(a.list(), k, bestVal, bestRow, a.sink(), info);
    return HJ_OK;
}

// ---- range joins without an equality key (hj_range.hip) ------------------------
// hj_range_index_dev's and hj_range_index_host's arguments -> the kernels' column; the message of what is wrong, or nullptr
static const char* range_index_args(const hj_sort_col* col, uint64_t nRows, const uint32_t* perm, const void* keys, const uint32_t* head, SortCols* k)
{
    if (!col) return "col NULL";
    if (nRows > 0xFFFFFFFEull) return "nRows above 2^32 - 2";
    if (col->flags) return "hj_sort_col.flags must be 0: the index is ascending with its NULLs last";
    if (const char* what = sort_cols_error(col, 1, nRows, k)) return what;
    if (nRows && (!perm || !word_ptr_ok(perm))) return "dPerm NULL or not 4-byte aligned";
    if (nRows && !col_ptr_ok(keys, col->width == 8 ? 8 : 4)) return "dKeys NULL or not aligned to its key bytes";
    if (!head || !word_ptr_ok(head)) return "dHead NULL or not 4-byte aligned";
    return nullptr;
}

int hj_range_index_dev(hj_ctx* c, const hj_sort_col* col, uint64_t nRows, uint32_t* dPerm, void* dKeys, uint32_t* dHead)
{
    HJ_ENTER(c, true);
    SortCols k{};
    if (const char* what = range_index_args(col, nRows, dPerm, dKeys, dHead, &k)) return fail(c, HJ_ERR_INVALID, "hj_range_index_dev", what);
    const SortLayout l = sort_layout(nRows, sort_key_bytes(k, 1));
    const Facts facts{0, nRows, {(uint64_t)reinterpret_cast<uintptr_t>(dHead)}};
    return recorded_call(c, CALL_RANGE_INDEX, 0, INIT_UNTIMED, Work{B_SORT_WORK, nRows ? l.bytes : 0}, facts, [&](unsigned long long*) {
        return launch_range_index(k, nRows, dPerm, dKeys, dHead, c->buf[B_SORT_WORK].p, c->stream);
    });
}

int hj_range_index_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_RANGE_INDEX];
    if (const int rc = call_info(c, CALL_RANGE_INDEX, nullptr, nullptr, out)) return rc;
    if (!r.called) return HJ_OK;
    uint32_t head[4];                                           // the caller's plane, as the call left it
    HJ_HIP(c, hipMemcpy(head, reinterpret_cast<const void*>((uintptr_t)r.extra[0]), sizeof(head), hipMemcpyDeviceToHost));
    out[0] = head[0]; out[1] = head[1]; out[3] = head[2];
    return HJ_OK;
}

int hj_range_index_host(const hj_sort_col* col, uint64_t nRows, uint32_t* perm, void* keys, uint32_t head[4])
{
    SortCols k{};
    if (range_index_args(col, nRows, perm, keys, head, &k)) return HJ_ERR_INVALID;
    range_index_host(k, nRows, perm, keys, head);
    return HJ_OK;
}

int hj_range_layout_info(uint64_t nRows, uint64_t sRows, uint64_t out[8])
{
    if (!out || nRows > 0xFFFFFFFEull || sRows > 0xFFFFFFFEull) return HJ_ERR_INVALID;
    const RangeLayout l = range_layout(nRows, sRows);
    out[0] = l.pivots; out[1] = l.stride; out[2] = l.tilePairs; out[3] = l.bytes; out[4] = l.chunkRows; out[5] = l.chunks; out[6] = l.ldsBytes;
    out[7] = 0;
    return HJ_OK;
}

// hj_range_pairs_dev's and hj_range_pairs_host's arguments -> the kernels' term; the message of what is wrong, or nullptr
static const char* range_args(const void* keys, const uint32_t* perm, const uint32_t* head, uint64_t rRows, const hj_range_term* t, uint64_t sRows,
                              const uint32_t* outS, const uint32_t* outR, uint64_t capacity, const uint32_t* sMarks, const uint32_t* rMarks, RangeTerm* k)
{
    if (sRows > 0xFFFFFFFEull || rRows > 0xFFFFFFFEull) return "sRows or rRows above 2^32 - 2";
    if (capacity > 0xFFFFFFFFull) return "capacity above 2^32 - 1";
    if (!t) return "term NULL";
    if (!t->lo && !t->hi) return "lo and hi both NULL: a range has a bound";
    if (const char* what = val_col_error(t->type, t->width)) return what;
    if (t->flags & ~(HJ_RANGE_LO_OPEN | HJ_RANGE_HI_OPEN)) return "hj_range_term.flags has bits other than HJ_RANGE_LO_OPEN and HJ_RANGE_HI_OPEN";
    if (t->pick > HJ_RANGE_LAST) return "pick must be an hj_range_pick";
    if ((reinterpret_cast<uintptr_t>(t->lo) | reinterpret_cast<uintptr_t>(t->hi)) & (t->width - 1)) return "a bound pointer that is not aligned to its width";
    if (!word_ptr_ok(t->loValid) || !word_ptr_ok(t->hiValid)) return "a validity pointer that is not 4-byte aligned";
    if (rRows && (!perm || !word_ptr_ok(perm))) return "dPerm NULL or not 4-byte aligned";
    if (rRows && !col_ptr_ok(keys, t->width == 8 ? 8 : 4)) return "dKeys NULL or not aligned to its key bytes";
    if (rRows && (!head || !word_ptr_ok(head))) return "dHead NULL or not 4-byte aligned";
    if (!word_ptr_ok(outS) || !word_ptr_ok(outR) || !word_ptr_ok(sMarks) || !word_ptr_ok(rMarks)) return "an output or mark pointer that is not 4-byte aligned";
    if (sRows && rRows && capacity && (!outS || !outR)) return "an output pointer NULL with capacity > 0";
    *k = RangeTerm{t->lo, t->hi, t->loValid, t->hiValid, t->width, t->type, t->flags, t->pick};
    return nullptr;
}

int hj_range_pairs_dev(hj_ctx* c, const void* dKeys, const uint32_t* dPerm, const uint32_t* dHead, uint64_t rRows, const hj_range_term* term,
                       uint64_t sRows, uint32_t sRowBase, uint32_t* dOutS, uint32_t* dOutR, uint64_t capacity, uint32_t* dSMarks, uint32_t* dRMarks)
{
    HJ_ENTER(c, true);
    RangeTerm k{};
    if (const char* what = range_args(dKeys, dPerm, dHead, rRows, term, sRows, dOutS, dOutR, capacity, dSMarks, dRMarks, &k))
        return fail(c, HJ_ERR_INVALID, "hj_range_pairs_dev", what);
    const RangeLayout l = range_layout(rRows, sRows);
    const PairSink to{PairsOut{dOutS, dOutR, capacity, nullptr}, dSMarks, dRMarks};
    return recorded_call(c, CALL_RANGE, 4, INIT_UNTIMED, Work{B_RANGE_WORK, l.bytes}, Facts{capacity, sRows}, [&](unsigned long long* words) {
        return launch_range_pairs(dKeys, dPerm, dHead, (uint32_t)rRows, k, (uint32_t)sRows, sRowBase, to, c->buf[B_RANGE_WORK].p, words, c->stream);
    });
}

int hj_range_pairs_info(hj_ctx* c, uint64_t out[8])
{
    HJ_ENTER(c, out);
    for (int i = 4; i < 8; ++i) out[i] = 0;
    unsigned long long words[kCallWords];
    if (const int rc = call_info(c, CALL_RANGE, nullptr, words, out)) return rc;       // pairs, written, time, S rows with a pair
    out[4] = words[2]; out[5] = words[3];
    return HJ_OK;
}

int hj_range_pairs_host(const void* keys, const uint32_t* perm, const uint32_t* head, uint64_t rRows, const hj_range_term* term, uint64_t sRows,
                        uint32_t sRowBase, uint32_t* outS, uint32_t* outR, uint64_t capacity, uint32_t* sMarks, uint32_t* rMarks, uint64_t info[8])
{
    RangeTerm k{};
    if (range_args(keys, perm, head, rRows, term, sRows, outS, outR, capacity, sMarks, rMarks, &k)) return HJ_ERR_INVALID;
    if (rRows && head[3] != (k.width == 8 ? 8u : 4u)) return HJ_ERR_INVALID;              // the index is of another key width
    const PairSink to{PairsOut{outS, outR, capacity, nullptr}, sMarks, rMarks};
    range_pairs_host(keys, perm, head, (uint32_t)rRows, k, (uint32_t)sRows, sRowBase, to, info);
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
    return recorded_call(c, CALL_PAIRS_AGG, 2, INIT_UNTIMED, kNoWork, Facts{0, nPairs}, [&](unsigned long long* counts) {
        return launch_pairs_agg(dMapG, dMapV, nPairs, gBase, (uint32_t)gRows, vBase, (uint32_t)vRows, k, nCols,
                                reinterpret_cast<unsigned long long*>(dCount), counts, c->stream);
    });
}

int hj_pairs_agg_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    const CallRecord& r = c->call[CALL_PAIRS_AGG];  // pairs applied, pairs skipped
    if (const int rc = call_info(c, CALL_PAIRS_AGG, out)) return rc;
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
    // the sweep reads the plane and never writes it
    const RMarks mk{const_cast<uint32_t*>(dMarks), rowBase, (uint32_t)rows};
    const Work work{B_MARK_SWEEP, r_sweep_count_words(rows) * sizeof(uint32_t)};
    return recorded_call(c, CALL_MARK_ROWS, 0, INIT_UNTIMED, work, Facts{capacity, rows}, [&](unsigned long long*) {
        return launch_r_sweep(mk, which == HJ_R_MATCHED, dOut, capacity, c->buf[B_MARK_SWEEP].as<uint32_t>(), c->stream);
    });
}

int hj_mark_rows_info(hj_ctx* c, uint64_t out[4])
{
    HJ_ENTER(c, out);
    // the word behind the block counts: their total after the scan (no block: no row)
    const CallRecord& r = c->call[CALL_MARK_ROWS];
    const uint32_t* const total = r.rows ? c->buf[B_MARK_SWEEP].as<uint32_t>() + r_sweep_blocks(r.rows) : nullptr;
    if (const int rc = call_info(c, CALL_MARK_ROWS, total, nullptr, out)) return rc;
    out[3] = r.rows;
    return HJ_OK;
}

}  // extern "C"
