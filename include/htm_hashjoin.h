/*
 * htm_hashjoin.h -- C ABI of libhtmjoin_hip.so, the MI355X (gfx950) hash-join
 * build+probe engine.
 *
 * This is the drop-in boundary for the hot path of anilshanbhag/HTM-HashJoin.
 * The reference has no FFI layer: its operator interface is a set of C++ free
 * functions picked by a string compare in main (main.cpp:99-108 with probe,
 * :115-122 build only), plus mc's function-pointer table
 * (mc/src/main.c:262-301).  Each entry point below names the reference
 * interface it replaces.  Plain pointers and sizes only; no HIP, torch or C++
 * types cross this boundary.  INTEGRATION.md shows the reference-side binding.
 *
 * Tuple layout (A0): one uint64_t per tuple whose value is the key; seen as
 * little-endian {uint32 key; uint32 payload=0} it is mc's tuple_t
 * (include/DataGen.hpp:29, mc/src/types.h:34-37).
 *
 * Error behaviour: the reference returns void and exits on allocation failure
 * (HTMHashBuild.hpp:66-70, mc MALLOC_CHECK).  This library never exits: every
 * call returns HJ_OK (0) or a negative hj_status; hj_last_error() gives text.
 * There is NO CPU fallback: without a usable gfx950 device hj_create fails
 * with HJ_ERR_NO_DEVICE.
 */
#ifndef HTM_HASHJOIN_H
#define HTM_HASHJOIN_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HJ_ABI_VERSION 4

typedef enum {
    HJ_OK                  = 0,
    HJ_ERR_INVALID         = -1,  /* bad argument / unsupported size           */
    HJ_ERR_NO_DEVICE       = -2,  /* no HIP device / not gfx950                */
    HJ_ERR_HIP             = -3,  /* a HIP runtime call failed                 */
    HJ_ERR_OOM             = -4,  /* device allocation failed                  */
    HJ_ERR_KEY_RANGE       = -5,  /* a tuple has non-zero payload bits or is 0 */
    HJ_ERR_UNKNOWN_ALGO    = -6,
    HJ_ERR_STATE           = -7   /* call order violated (e.g. probe w/o build)*/
} hj_status;

/* Which reference operator the call stands in for. NOCC and ATOMIC run the same
 * order-deterministic open-addressing kernels (the racy store and the CAS loop
 * replaced outright) and differ only in which checksum quirk outputSum follows
 * (see hj_result). HTM builds the reference's OTHER table: 32-byte buckets of
 * three tuples, bucket = (key / 3) & (numBuckets - 1), numBuckets =
 * nextpow2(rSize / 3 + 1), tuples beyond the third ("conflicts") chained into
 * overflow buckets, probe = bucket + chain (HTMHashBuild.hpp:41-45, 61-62, 176-183,
 * 231-279, 291-305); Intel TSX is replaced outright by the index-priority fill,
 * so a bucket holds its three lowest-indexed tuples whatever the scheduling. */
typedef enum {
    HJ_ALGO_NOCC   = 0,  /* NoCCHashBuild   (NoCCHashBuild.hpp:13-151)   */
    HJ_ALGO_ATOMIC = 1,  /* AtomicHashBuild (AtomicHashBuild.hpp:14-157) */
    HJ_ALGO_HTM    = 2,  /* HTMHashBuild    (HTMHashBuild.hpp:54-464): bucketised table + overflow chains;
                            rSize need not be a power of two; totalMatches = true join cardinality */
    HJ_ALGO_PRJ    = 3,  /* mc PRO          (mc/src/parallel_radix_join.c:1305) */
    HJ_ALGO_AUTO   = 4   /* the reference's adaptive idea (README.md:6, the sampling pre-round of
                            HTMHashBuild.hpp:98-154 and its 0.4 % / 2 % thresholds :209-210): sample R for
                            locality; with locality run the no-partition path (HJ_ALGO_ATOMIC, LDS-window
                            build), otherwise the radix join (HJ_ALGO_PRJ) -- also when rSize is not a power of
                            two, which the table join does not take. hj_result.algoUsed says which;
                            totalMatches agrees between the two whenever R has unique keys */
} hj_algo;

/* Mirrors the trailing arguments of the reference signatures
 * (NoCCHashBuild.hpp:13-19; HTMHashBuild.hpp:54-60) and mc's compile-time
 * NUM_RADIX_BITS (mc/src/prj_params.h:16). Zero means "reference default". */
typedef struct {
    uint32_t algo;            /* hj_algo                                        */
    uint32_t scaleOutput;     /* accepted, unused: tableSize is 2*rSize
                                 (main.cpp:59-60, NoCCHashBuild.hpp:20)         */
    uint32_t numPartitions;   /* default 64 (main.cpp:84); informational        */
    uint32_t probeLength;     /* default 4  (main.cpp:80)                       */
    uint32_t transactionSize; /* default 16 (main.cpp:82); echoed for htm       */
    uint32_t radixBits;       /* PRJ only. 0 = auto (>= 14 so that every
                                 R partition fits one LDS table)                */
    uint32_t buildVariant;    /* 0 = auto (samples R for locality, like the pre-round of
                                 HTMHashBuild.hpp:100-154); 1 = global atomicMin kernel;
                                 2 = block-ownership + workgroup LDS-window kernel (locality
                                 up to a shuffle window of ~2000 positions);
                                 3 = wavefront-private LDS rings over statically owned slot
                                 ranges (tight locality, the reference's default
                                 --shuffleRange 16);
                                 4 = the same rings writing a COMPACT table (4-byte keys: the
                                 index words that order the inserts never leave the LDS; no
                                 deferred phase; if the input needs one, 3 redoes the table,
                                 decided on the device) -- what 0 picks where 3 would do;
                                 all give the same table (hj_export_table) and counters    */
    uint32_t prjMode;         /* PRJ: 0 = partition large relations without histograms (fragments
                                 sized for uniform low key bits, checked; the exact passes of
                                 parallel_radix_join.c:586-626 run instead when one overflows);
                                 1 = exact passes only; 2 = as 0 at any size that can be laid out   */
    uint32_t flags;           /* HJ_FLAG_* bits; 0 = none                        */
    uint32_t reserved[3];
} hj_params;

/* hj_params.flags. Open addressing: never leave the table in the compact 4-byte format, so that every slot keeps the
 * input index of its tuple for hj_probe_pairs_dev (buildVariant 4 runs as 3; buildVariant 0 neither enqueues nor picks
 * 4; buildVariant 3 writes its packed 8-byte slots instead of a key plane and an index plane, hj_wave_planar_info).
 * No effect on HJ_ALGO_HTM, whose table always keeps the indices.
 * Resident radix join (hj_reserve with HJ_ALGO_PRJ or HJ_ALGO_AUTO): hj_prj_build_dev keeps R resident as 8-byte
 * {key, row} elements (row = position in dR; the input's own upper word is dropped) instead of bare 4-byte keys, for
 * hj_prj_probe_pairs_dev. Row ids travel through the exact passes only: prjPath and the paths of hj_prj_resident_info
 * report 0, and R costs 8 bytes per tuple of resident memory. hj_prj_probe_dev keeps working and counts the same.
 * No effect on the one-shot hj_prj_join_dev. */
#define HJ_FLAG_KEEP_ROW_IDS 0x1u
/* hj_params.flags. R-side match marks: the context remembers which R rows have appeared in a row of a materialising probe
 * since the last build, across probe calls (R is built once, S arrives in slices), and hj_r_rows_dev turns that memory
 * into rows -- what right outer, full outer, right semi and right anti joins need (see hj_r_rows_dev).
 * hj_reserve also allocates the mark plane: one bit per R row of the reserved rSize, in 32-bit words. The marks are
 * indexed by R row, so on open addressing and on HJ_ALGO_PRJ / HJ_ALGO_AUTO the flag is accepted only together with
 * HJ_FLAG_KEEP_ROW_IDS (hj_reserve: HJ_ERR_INVALID otherwise); HJ_ALGO_HTM, whose table always keeps the rows, takes it
 * alone. hj_build_keys_dev on such a context returns HJ_ERR_STATE (the sharded path keeps no marks). */
#define HJ_FLAG_TRACK_R_MATCHES 0x2u
/* hj_params.flags. Open addressing, hj_build_dev through the classic rings (buildVariant 3, or 0 picking it) on a context
 * without HJ_FLAG_KEEP_ROW_IDS: leave the table as one CODE BYTE per slot (table format 2, hj_slot_codes_info) whatever the
 * table's size. Without the flag that format is taken exactly where a byte holds any 32-bit key -- (32 - log2(tableSize))
 * + ceil(log2(probeLength)) <= 7, i.e. tables of 2^27 slots and more at probeLength 4 -- and smaller tables keep 4-byte
 * keys. With it, a build that meets a key whose bits above the table size do not fit hands over to the 8-byte build
 * (cause 4 of hj_slot_codes_info); results are the same on every road. For tests of the format at small sizes.
 * hj_reserve refuses it (HJ_ERR_INVALID) together with HJ_FLAG_KEEP_ROW_IDS, on an algo other than HJ_ALGO_NOCC /
 * HJ_ALGO_ATOMIC, and with a probeLength above 128. hj_build_keys_dev ignores it. */
#define HJ_FLAG_SLOT_CODES 0x4u

/* Everything the reference prints in its JSON line (NoCCHashBuild.hpp:127-146,
 * AtomicHashBuild.hpp:133-152) plus device timings. */
typedef struct {
    uint64_t rSize, sSize, tableSize;
    uint64_t conflicts;       /* tuples that exhausted probeLength ("conflicts") */
    uint64_t totalMatches;
    uint64_t inputSum;        /* sum of R                                        */
    uint64_t tableSumHalf;    /* sum of table[0..rSize)                          */
    uint64_t tableSumFull;    /* sum of table[0..tableSize)                      */
    uint64_t conflictSum;     /* sum of dropped keys                             */
    uint64_t outputSum;       /* nocc:  tableSumHalf + conflictSum (the
                                 NoCCHashBuild.hpp:94 quirk, kept for log parity);
                                 atomic/htm: tableSumFull + conflictSum           */
    uint64_t prjChecksum;     /* PRJ: sum of bucket idx == mc PRO "Results"
                                 (parallel_radix_join.c:256) when radixBits=14    */
    uint64_t prjPartitions;   /* PRJ: number of final partitions                  */
    uint32_t radixBits;       /* PRJ: bits actually used                          */
    uint32_t buildVariant;    /* kernel actually used (4 only if the compact build held) */
    /* device time of the last call of each phase, from HIP events on the
     * context's stream, in microseconds */
    double clear_us, build_us, probe_us, partition_us, join_us, total_us;
    double h2d_us;            /* hj_run only: host->device copies (reported
                                 separately, never part of total_us)              */
    uint64_t buildDeferred;   /* buildVariant 2: tuples that left the LDS window and
                                 were finished by the global-atomic phase            */
    double   buildPhaseA_us;  /* buildVariant 2: device time of k_build_own alone
                                 (build_us also covers k_clear_unowned and
                                 k_build_deferred)                                   */
    uint32_t algoUsed;        /* hj_algo that produced this result (differs from
                                 hj_params.algo only for HJ_ALGO_AUTO)               */
    uint32_t prjPath;         /* PRJ: 0 = exact (histogram) passes; 1 = histogram-free passes;
                                 2 = histogram-free passes overflowed, exact passes redid the join */
    uint64_t foreignTuples;   /* hj_set_shard_check: build + probe tuples whose
                                 destination is another shard (0 when the check is off) */
    double   prjScatterPass1R_us; /* PRJ: device time of the pass-1 scatter of R alone (the
                                 dominant kernel: 8 B read + 4 B written per tuple)      */
    /* HJ_ALGO_HTM: conflicts = the reference's conflictCount (tuples that found their
     * bucket full, HTMHashBuild.hpp:181-183, :225-228), tableSumFull = sum of the tuples in
     * primary buckets, outputSum = tableSumFull + htmOverflowSum (== inputSum) */
    uint64_t htmBuckets;          /* numBuckets                                           */
    uint64_t htmOverflowBuckets;  /* overflow buckets linked into chains (:231-279)       */
    uint64_t htmOverflowSum;      /* sum of the tuples they hold (== conflictSum)         */
    uint64_t compactFallback;     /* open addressing: 0 = the compact ring build (buildVariant 4) held or was not
                                     tried; else why it handed over to the classic build -- bit 0: a tuple outside
                                     ring and range (no locality there), bit 1: more than 64 walks across one seam,
                                     bit 2: key 0xFFFFFFFF, bit 3: a tuple below its chunk's range in the tile that holds
                                     the chunk's tail zone (in any other tile past the head zone such a tuple is
                                     outside the ring: bit 0), bit 4: a seam's two sides disagree (the shadow granule
                                     missed a tuple, or a walk entered it from below).
                                     HJ_ALGO_HTM: bit 8 = the chain phase could not run in LDS behind the ring build (key
                                     range of a chunk or its conflicts too large for the LDS image) and the generic
                                     chain kernels redid it                                                            */
} hj_result;

typedef struct hj_ctx hj_ctx;

/* ---- context ------------------------------------------------------------- */
int  hj_abi_version(void);
int  hj_device_count(int *count);
/* Binds to `device`, checks it is gfx950, creates a private stream. */
int  hj_create(int device, hj_ctx **out);
/* Same, but launches on the caller's stream (a hipStream_t passed as void*;
 * NULL = the default stream). Lets a host that owns streams (PyTorch) time and
 * order the kernels itself. */
int  hj_create_on_stream(int device, void *hip_stream, hj_ctx **out);
void hj_destroy(hj_ctx *ctx);
const char *hj_strerror(int status);
const char *hj_last_error(const hj_ctx *ctx);
int  hj_synchronize(hj_ctx *ctx);

/* ---- one-shot operator, host buffers ------------------------------------- */
/* Replaces NoCCHashBuild/AtomicHashBuild/HTMHashBuild(relR, rSize, relS, sSize,
 * ...) as called at main.cpp:99-104, and mc's PRO(relR, relS, nthreads)
 * (mc/src/main.c:292-301) for HJ_ALGO_PRJ. relS may be NULL / sSize 0 for the
 * build-only variant (main.cpp:115-120, ENABLE_PROBE 0). Inputs are read-only
 * and stay host-owned; device memory is owned by ctx. Like the reference
 * (NoCCHashBuild.hpp:24-34) allocation, host->device copies and checksums are
 * outside total_us. */
int hj_run(hj_ctx *ctx, const hj_params *params,
           const uint64_t *relR, uint64_t rSize,
           const uint64_t *relS, uint64_t sSize, hj_result *out);

/* ---- split operator, device-resident buffers ------------------------------ */
/* Allocate the table / partition workspace for these sizes (the `new[]` block
 * of NoCCHashBuild.hpp:24-31). Idempotent; grows only. */
int hj_reserve(hj_ctx *ctx, const hj_params *params, uint64_t rSize, uint64_t sSize);
/* HOT LOOP 1 (NoCCHashBuild.hpp:37-62 / AtomicHashBuild.hpp:37-67): clears the
 * table and inserts dR[0..rSize). Asynchronous on the context's stream, also
 * with buildVariant 0: the locality pre-round's decision is taken and acted on
 * by the device (no read-back), hj_result.buildVariant reports it afterwards.
 * Not so under HJ_ALGO_HTM: that build waits for the stream once, to read the
 * conflict count back and size the overflow area (with buildVariant 0 once
 * more, for the locality sample). INTEGRATION.md, "Stream contract", says for
 * every entry point whether it waits.
 * idxBase = global index of dR[0] (0 unless R is a shard of a larger input). */
int hj_build_dev(hj_ctx *ctx, const uint64_t *dR, uint64_t rSize, uint64_t idxBase);
/* HOT LOOP 2 (NoCCHashBuild.hpp:66-80): probes dS[0..sSize) against the table
 * of the last hj_build_dev and accumulates totalMatches. Asynchronous. */
int hj_probe_dev(hj_ctx *ctx, const uint64_t *dS, uint64_t sSize);
/* HOT LOOP 2 with its result kept: probes dS[0..sSize) like hj_probe_dev and, for every match it counts, writes one
 * pair  dOutS[k] = sIdxBase + (position in dS),  dOutR[k] = global input index of the matching R tuple
 * (idxBase + position, as given to hj_build_dev). The two arrays are gather maps into S and R: row k of the join is
 * (S[dOutS[k]], R[dOutR[k]]). Pairs fill dOut*[0 .. written) without holes; every call starts at 0; pairs beyond
 * `capacity` are counted but not written. The order of the pairs is unspecified; the multiset is exact. What an S
 * tuple matches is what hj_probe_dev counts for it: open addressing = the reference's walk (at most probeLength slots
 * from the home slot, stop at the first empty one), HJ_ALGO_HTM = bucket plus whole chain, i.e. the complete
 * equi-join. Adds to totalMatches and sSize exactly as hj_probe_dev does. Asynchronous.
 * HJ_ERR_STATE: no table; a PRJ context; an open-addressing context reserved without HJ_FLAG_KEEP_ROW_IDS.
 * HJ_ERR_INVALID: an output pointer NULL with capacity > 0, or sIdxBase + sSize > 2^32 - 1. sSize 0 is a no-op. */
int hj_probe_pairs_dev(hj_ctx *ctx, const uint64_t *dS, uint64_t sSize, uint64_t sIdxBase,
                       uint32_t *dOutS, uint32_t *dOutR, uint64_t capacity);
/* The join kinds of the materialising probes. S, the probe side, is the preserved side; a "match" is exactly what the
 * pairs probe of that path emits (above: the walk, the bucket plus its chain, or, for the radix join, the complete
 * equi-join on the key word). An S tuple is unmatched when that probe emits no pair for it -- on the table paths this
 * includes tuples outside the DataGen layout and tuples whose home lies outside the slots the build defined.
 *   HJ_JOIN_INNER  one row per match                                                   planes S, R
 *   HJ_JOIN_LEFT   one row per match; for a tuple without one, one row with R row = HJ_NO_ROW   planes S, R
 *   HJ_JOIN_SEMI   one row for a tuple with at least one match, however many            plane S only
 *   HJ_JOIN_ANTI   one row for a tuple without a match                                  plane S only
 * R-preserving results (right / full outer, right semi / anti) are no fifth kind: they are the INNER or LEFT calls of a
 * context reserved with HJ_FLAG_TRACK_R_MATCHES plus hj_r_rows_dev (below). */
typedef enum { HJ_JOIN_INNER = 0, HJ_JOIN_LEFT = 1, HJ_JOIN_SEMI = 2, HJ_JOIN_ANTI = 3 } hj_join_kind;
/* The R row of an HJ_JOIN_LEFT row whose S tuple has no match. No real row takes the value: S rows stay below it by the
 * check on sIdxBase + sSize, R rows by the builds' own checks (idxBase + rSize <= 2^32 - 1; PRJ: rSize < 2^32 - 1). */
#define HJ_NO_ROW 0xFFFFFFFFu
/* hj_probe_pairs_dev for any join kind (hj_probe_pairs_dev is its HJ_JOIN_INNER case). Same preconditions, same errors,
 * same output contract with "row" for "pair": the planes fill from 0 without holes on every call, rows at or beyond
 * `capacity` are counted and not written, the order is unspecified, the multiset is exact. For HJ_JOIN_SEMI / ANTI
 * dOutR is ignored: it may be NULL with capacity > 0 and is never written. totalMatches and sSize grow exactly as under
 * hj_probe_dev -- by the INNER matches, whatever the kind -- so a context ends with the same hj_result as one driven
 * through the counting probe. HJ_ERR_INVALID also for kind > 3. Asynchronous. */
int hj_probe_join_dev(hj_ctx *ctx, uint32_t kind, const uint64_t *dS, uint64_t sSize, uint64_t sIdxBase,
                      uint32_t *dOutS, uint32_t *dOutR, uint64_t capacity);
/* Waits for the stream. About the last hj_probe_pairs_dev / hj_probe_join_dev / hj_prj_probe_pairs_dev /
 * hj_prj_probe_join_dev: out[0] = rows it produced, out[1] = rows it wrote (= min(out[0], capacity)), out[2] = its device
 * time in microseconds (rounded), out[3] = S tuples of the call without a match for a kind other than HJ_JOIN_INNER
 * (0 after an INNER call). */
int hj_pairs_info(hj_ctx *ctx, uint64_t out[4]);
/* ---- R-side match marks (contexts reserved with HJ_FLAG_TRACK_R_MATCHES) ----
 * One bit per R row of the last build. hj_build_dev and hj_prj_build_dev clear the plane on the stream. Every later
 * hj_probe_join_dev / hj_prj_probe_join_dev call of kind HJ_JOIN_INNER or HJ_JOIN_LEFT (hj_probe_pairs_dev and
 * hj_prj_probe_pairs_dev included) sets the bit of every R row that appears in a row it produces -- whether the row is
 * written or not: rows at or beyond `capacity` mark too, so a call with capacity 0 and NULL planes is a mark-only pass.
 * HJ_NO_ROW marks nothing. HJ_JOIN_SEMI and HJ_JOIN_ANTI calls, hj_probe_dev and hj_prj_probe_dev never touch the marks
 * and run the kernels they run without the flag. Bit index: table paths, R row - idxBase of the last build; PRJ, the
 * position in dR. hj_result and hj_pairs_info are what the same calls give on a context without the flag.
 * "Matched" is exactly "some produced row named this R row", as an S tuple is unmatched when the probe emits no pair for
 * it: on open addressing an R tuple the build dropped (a conflict: probeLength exhausted) is unmatched, and so is a
 * tuple behind the reach of the probe's walk.
 *   right outer = the rows of the HJ_JOIN_INNER calls, plus (HJ_NO_ROW, r) for every unmatched r
 *   full outer  = the rows of the HJ_JOIN_LEFT calls, plus the same tail
 *   right semi  = the matched rows                       right anti = the unmatched rows */
#define HJ_R_UNMATCHED 0u
#define HJ_R_MATCHED   1u
/* Zeroes the marks without rebuilding. Asynchronous. HJ_ERR_STATE as for hj_r_rows_dev. */
int hj_r_marks_clear(hj_ctx *ctx);
/* Writes the R rows of the last build whose bit is clear (HJ_R_UNMATCHED) or set (HJ_R_MATCHED), as the pairs report them
 * (idxBase + position; PRJ: the position in dR), in ASCENDING order from dOutR[0] without holes. Rows at or beyond
 * `capacity` are counted and not written, so a truncated call yields the first `capacity` rows; capacity 0 (dOutR may be
 * NULL) only counts. Changes no mark and no counter of hj_result. Asynchronous.
 * HJ_ERR_STATE: context reserved without HJ_FLAG_TRACK_R_MATCHES; no build yet, or the last build was not hj_build_dev /
 * hj_prj_build_dev. HJ_ERR_INVALID: which > 1; dOutR NULL with capacity > 0. */
int hj_r_rows_dev(hj_ctx *ctx, uint32_t which, uint32_t *dOutR, uint64_t capacity);
/* Waits for the stream. About the last hj_r_rows_dev since the build: out[0] = rows it produced, out[1] = rows it wrote
 * (= min(out[0], capacity)), out[2] = its device time in microseconds (rounded) -- all 0 when there was none --, out[3] =
 * R rows of the build. HJ_ERR_STATE as for hj_r_rows_dev. */
int hj_r_rows_info(hj_ctx *ctx, uint64_t out[4]);
/* ---- payload columns through the row maps ----
 * The planes of hj_probe_join_dev / hj_prj_probe_join_dev and the rows of hj_r_rows_dev are gather maps; hj_gather_dev is
 * the step from a map to the joined rows: for output row k and e = dMap[k],
 *   e == HJ_NO_ROW (the raw entry, whatever rowBase is)     a NULL row: every column gets its fill, validity bit 0
 *   i = e - rowBase, unsigned, >= srcRows                   out of range: never dereferenced; fill and bit 0 like a NULL
 *                                                           row, and counted apart (hj_gather_info out[3])
 *   otherwise                                               dst[k] = src[i] in every column, validity bit 1
 * rowBase is the idxBase / sIdxBase the map was written with (S slices: the slice's sIdxBase with the slice's columns).
 * The library's own maps over the relation they were made from have no out-of-range entry. The map is taken as it is:
 * it is neither sorted nor bucketed, so a random map fetches one cache line per element. */
#define HJ_GATHER_MAX_COLS 8
typedef struct {
    const void *src;     /* device: srcRows elements of `width` bytes (may be NULL when srcRows == 0) */
    void       *dst;     /* device: nRows elements of `width` bytes                                   */
    uint32_t    width;   /* 1, 2, 4, 8 or 16; src and dst aligned to it                               */
    uint32_t    reserved;/* 0                                                                          */
    uint64_t    fill[2]; /* the low `width` bytes are what a NULL row gets                            */
} hj_gather_col;         /* 40 bytes */
/* Gathers nCols (0 .. HJ_GATHER_MAX_COLS) columns through dMap[0..nRows), one pass over the map per element width
 * among them. `cols` is host memory and is read before the call returns. dValid (may be NULL): the validity plane in the Arrow layout, bit k & 31 of 32-bit
 * word k >> 5, 1 = valid; words 0 .. ceil(nRows / 32) - 1 are written whole (the bits at or behind nRows are 0), nothing
 * behind them. nCols 0 with a dValid gives the plane alone. Needs no table, no hj_reserve and no particular state; touches
 * no counter of hj_result, hj_pairs_info or hj_r_rows_info. Asynchronous on the context's stream. nRows 0 is a no-op.
 * HJ_ERR_INVALID (nothing is enqueued): nCols > HJ_GATHER_MAX_COLS; a width other than 1, 2, 4, 8, 16; reserved != 0; a
 * dst, or with srcRows > 0 a src, that is NULL or not aligned to its width; dMap NULL with nRows > 0; cols NULL with
 * nCols > 0; nRows or srcRows above 2^32 - 1; nCols == 0 and dValid == NULL with nRows > 0. */
int hj_gather_dev(hj_ctx *ctx, const uint32_t *dMap, uint64_t nRows, uint32_t rowBase, uint64_t srcRows,
                  const hj_gather_col *cols, uint32_t nCols, uint32_t *dValid);
/* Waits for the stream. About the last hj_gather_dev that enqueued work: out[0] = its rows, out[1] = its NULL rows
 * (HJ_NO_ROW entries), out[2] = its device time in microseconds (rounded), out[3] = its out-of-range entries. All 0 before
 * the first one. */
int hj_gather_info(hj_ctx *ctx, uint64_t out[4]);
/* ---- payload columns in the Arrow layout: source NULLs and variable-length (string) columns ----
 * hj_gather2_dev is hj_gather_dev on a second column descriptor, modelled on hj_key_col2 (below): per column an optional
 * source validity plane and optional 32-bit offsets, both gathered on the device. The map semantics are hj_gather_dev's,
 * word for word: the raw entry HJ_NO_ROW is a NULL row whatever rowBase is; an entry with e - rowBase >= srcRows is never
 * dereferenced in ANY buffer of any column (values, offsets, validity), gives what a NULL row gives and is counted apart;
 * dValid stays the call-level plane "row has a source row". Per column, an ELEMENT is valid when its row has a source row
 * i and the column has no srcValid or bit i of it is 1:
 *   fixed width       a row with a valid element gets src[i], every other row the fill; the bytes under a source NULL are
 *                     never read
 *   variable length   a row with a valid element gets the bytes [srcOffsets[i], srcOffsets[i + 1]) of src, every other row
 *                     is empty. dstOffsets[0 .. nRows] is always written in full: dstOffsets[0] = 0, dstOffsets[k + 1] -
 *                     dstOffsets[k] = the bytes of row k, dstOffsets[nRows] = the bytes the rows take. Output bytes at
 *                     positions at or behind dstCapacity are counted and not written (the library's contract for rows,
 *                     applied to bytes); the cut is byte-granular: every byte below min(total, dstCapacity) is exact and
 *                     no byte at or behind it is touched. dstCapacity 0 (dst may be NULL) is the sizing pass: offsets and
 *                     totals only
 *   dstValid          (either kind; may be NULL) bit k = row k has a valid element; ceil(nRows / 32) words written whole,
 *                     the bits at or behind nRows 0, nothing behind them
 * The totals are exact in 64 bits (hj_gather2_info). A column whose rows take more than 2^32 - 1 bytes cannot be laid out
 * with 32-bit offsets: none of its bytes are written, its dstOffsets are unspecified, its total says so; nothing faults.
 * What is read: the map; of a row with a source row the validity word of its element and, if that is valid, its two
 * offsets; of a valid non-empty element the aligned 32-bit words that hold one of its bytes (the rule of hj_key_hash2_dev)
 * and no byte outside them; of an empty or ungathered element nothing. What is written: the ranges named above and nothing
 * else. A call whose columns are all fixed without srcValid and dstValid runs the kernels of hj_gather_dev and costs what
 * that call costs. */
typedef struct {
    const void     *src;        /* fixed width: srcRows elements. Variable length: the bytes buffer (any alignment). May
                                   be NULL when srcRows == 0                                                              */
    void           *dst;        /* fixed: nRows elements. Variable length: dstCapacity bytes (any alignment); may be NULL
                                   when dstCapacity == 0                                                                  */
    const uint32_t *srcOffsets; /* NULL: fixed width. Else srcRows + 1 offsets into src (Arrow Binary / Utf8): non-decreasing,
                                   srcOffsets[0] need not be 0. Caller's contract, not checked on the device             */
    uint32_t       *dstOffsets; /* variable length: nRows + 1 offsets out                                                */
    const uint32_t *srcValid;   /* NULL: the source has no NULLs. Else the plane hj_gather_dev writes, bit i = source row i,
                                   ceil(srcRows / 32) words                                                              */
    uint32_t       *dstValid;   /* NULL, or ceil(nRows / 32) words out                                                   */
    uint64_t        dstCapacity;/* variable length: the bytes of dst. Fixed width: 0                                     */
    uint32_t        width;      /* 1, 2, 4, 8 or 16 (src and dst aligned to it); 0 for a variable-length column          */
    uint32_t        flags;      /* 0                                                                                     */
    uint64_t        fill[2];    /* fixed width: the low `width` bytes are what a row without a valid element gets        */
} hj_gather_col2;               /* 80 bytes */
/* Gathers nCols (0 .. HJ_GATHER_MAX_COLS) columns through dMap[0..nRows). `cols` is host memory and is read before the
 * call returns. Asynchronous on the context's stream; needs no table, no hj_reserve and no state; touches no counter of
 * hj_result and no other *_info, hj_gather_info included. The scan workspace of the variable-length columns belongs to the
 * context and grows with nRows (as for hj_mark_rows_dev). A variable-length column is three steps -- the rows' lengths
 * into dstOffsets with a 64-bit partial sum per workgroup, the library's exclusive scan over the nRows + 1 words in place,
 * the copy -- so its cost is two passes over the map and three over dstOffsets besides the bytes. nRows 0 is a no-op.
 * HJ_ERR_INVALID (nothing is enqueued; also for a NULL context): everything hj_gather_dev refuses (for a variable-length
 * column src and dst need no alignment, and dst may be NULL with dstCapacity 0); width 0 without srcOffsets or without
 * dstOffsets; srcOffsets or dstOffsets with a width other than 0; any flag bit; an offsets or validity pointer that is not
 * 4-byte aligned; dstCapacity > 0 with dst NULL; dstCapacity != 0 on a fixed column; a variable-length dst whose
 * dstCapacity bytes overlap another output of the call (a column's dst over its nRows elements or its dstCapacity bytes,
 * a dstOffsets, a dstValid, dValid) -- as far as the host can tell from the pointers. */
int hj_gather2_dev(hj_ctx *ctx, const uint32_t *dMap, uint64_t nRows, uint32_t rowBase, uint64_t srcRows,
                   const hj_gather_col2 *cols, uint32_t nCols, uint32_t *dValid);
/* Waits for the stream. About the last hj_gather2_dev that enqueued work (hj_gather_info keeps reporting hj_gather_dev
 * alone, and the other way round): out[0 .. 3] as hj_gather_info -- rows, NULL rows, device time in microseconds,
 * out-of-range entries --, out[4 + c] = the bytes the rows of column c take, exact in 64 bits, 0 for a fixed column and for
 * c at or behind the call's nCols. A total above 2^32 - 1 is the report that the column was not written. All 0 before the
 * first call. */
int hj_gather2_info(hj_ctx *ctx, uint64_t out[4 + HJ_GATHER_MAX_COLS]);
/* ---- joins on real key columns: hash, candidate join, verify ----
 * Every join above matches on one 32-bit word. A key of 64 bits, of several columns or of 16 bytes is joined in three steps:
 * hj_key_hash_dev hashes the key columns of each row to a 32-bit join word, written as the 8-byte tuple the resident radix
 * join takes; hj_prj_probe_join_dev(HJ_JOIN_INNER) on those tuples gives CANDIDATE pairs; hj_pairs_verify_dev compares the
 * real key bytes of every candidate, keeps the equal ones and records which S rows and which R rows took part in a kept
 * pair in two caller-owned bit planes. hj_mark_rows_dev turns such a plane into rows, and all eight join kinds follow from
 * the kept pairs and two sweeps. A context's own HJ_FLAG_TRACK_R_MATCHES marks are of no use here: a candidate the
 * verify step rejects would have set them.
 * A key column is one element of `width` bytes per row, the S side's and the R side's elements of a column having the
 * same width; keys are equal when every column is BYTEWISE equal (floats: -0.0 != 0.0, a NaN equals the same bit pattern).
 *
 * The hash (a test may restate it): MurmurHash3_x86_32 with seed 0 over the row's key columns in column order. An element
 * of width 1 or 2 is zero-extended to one 32-bit word; a wider element contributes its little-endian 32-bit words in
 * order. `len`, the value xored in before the finaliser, is 4 x the number of words. The join word is h & keyMask, keyMask
 * 0 meaning 0xFFFFFFFF. That is, with h = 0 and for every word k in order:
 *   k *= 0xcc9e2d51; k = rotl32(k, 15); k *= 0x1b873593; h ^= k; h = rotl32(h, 13); h = h * 5 + 0xe6546b64;
 * then h ^= len; h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16. (One 4-byte column holding 0
 * hashes to 0x2362F9DE.) keyMask exists so that tests and users can force collisions: the join's result does not depend
 * on the hash's quality, only its speed does. */
#define HJ_KEY_MAX_COLS 4
typedef struct {
    const void *s;       /* the S side's column: sRows elements of `width` bytes (NULL where that side is not in use) */
    const void *r;       /* the R side's column: rRows elements of `width` bytes                                    */
    uint32_t    width;   /* 1, 2, 4, 8 or 16; the pointer of a side in use aligned to it                             */
    uint32_t    reserved;/* 0                                                                                         */
} hj_key_col;            /* 24 bytes */
#define HJ_KEY_SIDE_S 0u
#define HJ_KEY_SIDE_R 1u
/* dOutTuples[i] = (uint64_t)(join word of row i) for i in [0, nRows), from the `side` pointers of cols[0 .. nCols): an
 * 8-byte tuple as hj_prj_build_dev and hj_prj_probe_join_dev take it. Device pointers; `cols` is host memory and is read
 * before the call returns. Coalesced loads of every column, one 8-byte store per row, no atomics. Asynchronous on the
 * context's stream; nRows 0 is a no-op. Needs no hj_reserve, no table and no state; touches no counter and no *_info.
 * HJ_ERR_INVALID (nothing is enqueued; also for a NULL context): nCols 0 or above HJ_KEY_MAX_COLS, cols NULL; a width
 * other than 1, 2, 4, 8, 16; reserved != 0; side > 1; with nRows > 0 a column pointer of the side that is NULL or not
 * aligned to its width, or dOutTuples NULL; nRows above 2^32 - 1. */
int hj_key_hash_dev(hj_ctx *ctx, const hj_key_col *cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask,
                    uint64_t *dOutTuples);
/* The same function on host pointers: no context, no device (the kernel and this loop share one body). For hosts that
 * pre-hash, and so that the hash can be tested anywhere. HJ_ERR_INVALID as hj_key_hash_dev. */
int hj_key_hash_host(const hj_key_col *cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask,
                     uint64_t *outTuples);
/* Candidate pairs -> exact pairs. For candidate k in [0, nPairs): s = dMapS[k] - sRowBase, r = dMapR[k] (the planes of an
 * hj_prj_probe_join_dev(HJ_JOIN_INNER) call with sIdxBase = sRowBase). A candidate whose raw entry is HJ_NO_ROW on either
 * side, or with s >= sRows or r >= rRows, is never dereferenced: it is dropped and counted apart (hj_verify_info out[3]).
 * Otherwise the pair is kept iff cols[c].s[s] and cols[c].r[r] are bytewise equal in every column c. Kept pairs go to
 * dOutS / dOutR under the output contract of hj_probe_pairs_dev: dOutS[j] is the original entry dMapS[k], base included;
 * the planes fill from 0 without holes; pairs at or beyond `capacity` are counted and not written; the order is
 * unspecified, the multiset is exact. Every kept pair, written or cut by the capacity, sets bit s of dSMarks and bit r of
 * dRMarks where those are not NULL: bit i & 31 of 32-bit word i >> 5, words 0 .. ceil(rows / 32) - 1, nothing behind
 * them. Bits only go 0 -> 1: the caller clears the planes (per S slice, once per R). capacity 0 with NULL outputs is a
 * mark-only pass. dOutS / dOutR must not alias dMapS / dMapR, each other, or the planes. `cols` is host memory, read
 * before the call returns. Asynchronous; needs no hj_reserve, no table and no state; touches no counter of hj_result,
 * hj_pairs_info, hj_r_rows_info or hj_gather_info.
 * HJ_ERR_INVALID (nothing is enqueued; also for a NULL context): the column errors of hj_key_hash_dev, for the s pointers
 * with sRows > 0 and the r pointers with rRows > 0; a map NULL with nPairs > 0; an output NULL with nPairs > 0 and
 * capacity > 0; nPairs, sRows or rRows above 2^32 - 1. nPairs 0 is a call that kept nothing. */
int hj_pairs_verify_dev(hj_ctx *ctx, const uint32_t *dMapS, const uint32_t *dMapR, uint64_t nPairs, uint32_t sRowBase,
                        uint64_t sRows, uint64_t rRows, const hj_key_col *cols, uint32_t nCols, uint32_t *dOutS,
                        uint32_t *dOutR, uint64_t capacity, uint32_t *dSMarks, uint32_t *dRMarks);
/* Waits for the stream. About the last hj_pairs_verify_dev: out[0] = pairs kept, out[1] = pairs written (= min(out[0],
 * capacity)), out[2] = its device time in microseconds (rounded), out[3] = candidates dropped as NULL or out of range.
 * Rejected candidates = nPairs - out[0] - out[3]. All 0 before the first call. */
int hj_verify_info(hj_ctx *ctx, uint64_t out[4]);
/* ---- key columns in the Arrow layout: NULL keys and variable-length (string) keys ----
 * hj_key_hash2_dev / hj_key_hash2_host / hj_pairs_verify2_dev are the three calls above on a second column descriptor: a
 * values buffer, an optional validity plane and an optional 32-bit offsets buffer per side. The candidate join, the
 * marks, the sweeps, the gather and the eight kinds are untouched. A column's two sides agree in kind: both fixed with
 * the same width, or both variable-length. An element is NULL when its side has a validity plane and its bit is 0.
 *
 * The hash (a test may restate it): the MurmurHash3_x86_32 above, seed 0, over the row's columns in order. A valid fixed
 * element contributes what it contributes to hj_key_hash_dev. A valid variable-length element of L bytes contributes one
 * word L, then its bytes as ceil(L / 4) little-endian words, the last one zero-padded. A NULL element of a column with
 * HJ_KEY_NULLS_EQUAL contributes the single word 0xFFFFFFFF. `len` is 4 x the words mixed for that row. A row is
 * NULL-KEYED when some column WITHOUT HJ_KEY_NULLS_EQUAL is NULL in it: it can match nothing, and so that such rows do not
 * pile up on one join word, its word ignores the columns: mm3_final(mm3_mix(0x4E554C4C, (uint32_t)i), 4) & keyMask, i the
 * row's position in the call, mm3_mix the block step and mm3_final(h, len) the xor of len and the finaliser above. With
 * no offsets, no validity and flags 0 the tuples are exactly those of hj_key_hash_dev / hj_key_hash_host.
 *
 * The verify: for candidate (s, r), column c is equal when -- either element NULL: both are NULL and the column has
 * HJ_KEY_NULLS_EQUAL; otherwise, fixed width: bytewise; otherwise: same length and the same bytes. The pair is kept when
 * every column is equal. The bytes of a NULL element are never compared; its offsets are valid offsets (Arrow's rule)
 * and may be read.
 *
 * What is read: of a fixed column, the elements (those under a NULL too: they exist). Of a variable-length element, the
 * device code may read the aligned 32-bit words that contain its first and its last byte and those between them, and no
 * byte outside those words; of an empty element nothing. (So up to three bytes in front of the first element and behind
 * the last are read where the buffer does not start and end on a 4-byte address: device allocations do, or reach
 * further.) hj_key_hash2_host reads the element's bytes only. */
#define HJ_KEY_NULLS_EQUAL 0x1u   /* hj_key_col2.flags: in this column a NULL equals a NULL (IS NOT DISTINCT FROM) */
typedef struct {
    const void     *s, *r;               /* fixed width: the elements. Variable length: the bytes buffer            */
    const uint32_t *sOffsets, *rOffsets; /* NULL: fixed width. Else rows + 1 offsets into the bytes buffer (Arrow
                                            Binary/Utf8 layout): element i = bytes [off[i], off[i+1]); non-decreasing;
                                            off[0] need not be 0. Caller's contract, not checked on the device       */
    const uint32_t *sValid, *rValid;     /* NULL: that side has no NULLs. Else the plane hj_gather_dev writes: bit
                                            i & 31 of 32-bit word i >> 5, 1 = valid                                   */
    uint32_t width;                      /* 1, 2, 4, 8, 16; 0 for a variable-length column                           */
    uint32_t flags;                      /* HJ_KEY_NULLS_EQUAL or 0                                                   */
} hj_key_col2;                           /* 56 bytes */
/* hj_key_hash_dev on hj_key_col2 columns, from the `side` pointers (values, offsets, validity) of cols[0 .. nCols): the
 * hash above. Coalesced loads of every fixed column and of the offsets, a validity word read once per 32 rows, one
 * 8-byte store per row, no atomics. Asynchronous on the context's stream; nRows 0 is a no-op. Needs no hj_reserve, no
 * table and no state; touches no counter and no *_info. The validity plane of the side holds ceil(nRows / 32) words.
 * HJ_ERR_INVALID (nothing is enqueued; also for a NULL context): what hj_key_hash_dev refuses (a width that is neither 0
 * nor 1, 2, 4, 8, 16; a values pointer of the side that is NULL or, fixed width, not aligned to its width, ...); width 0
 * without offsets on a side in use; offsets on either side with width != 0; flag bits other than HJ_KEY_NULLS_EQUAL; an
 * offsets or validity pointer that is not 4-byte aligned. */
int hj_key_hash2_dev(hj_ctx *ctx, const hj_key_col2 *cols, uint32_t nCols, uint32_t side, uint64_t nRows,
                     uint32_t keyMask, uint64_t *dOutTuples);
/* The same function on host pointers: no context, no device (one body, the host reading bytewise). HJ_ERR_INVALID as
 * hj_key_hash2_dev; a refused call writes nothing. */
int hj_key_hash2_host(const hj_key_col2 *cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask,
                      uint64_t *outTuples);
/* hj_pairs_verify_dev on hj_key_col2 columns, column equality as stated above. Everything else is hj_pairs_verify_dev's,
 * word for word: a candidate whose raw entry is HJ_NO_ROW on either side, or with s >= sRows or r >= rRows, is never
 * dereferenced, dropped and counted apart; kept pairs go to dOutS / dOutR under the output contract of
 * hj_probe_pairs_dev (dOutS[j] the original entry, base included; no holes; pairs at or beyond `capacity` counted and not
 * written; order unspecified, multiset exact); every kept pair, written or cut, sets bit s of dSMarks and bit r of
 * dRMarks where those are not NULL, bits only going 0 -> 1; capacity 0 with NULL outputs is a mark-only pass; dOutS /
 * dOutR must not alias the maps, each other or the planes. sValid / sOffsets are indexed by s (the base is off), so they
 * hold ceil(sRows / 32) words and sRows + 1 offsets. hj_verify_info reports the last call of either verify entry.
 * HJ_ERR_INVALID (nothing is enqueued; also for a NULL context): the column errors of hj_key_hash2_dev, for the s
 * pointers with sRows > 0 and the r pointers with rRows > 0; a map NULL with nPairs > 0; an output NULL with nPairs > 0
 * and capacity > 0; nPairs, sRows or rRows above 2^32 - 1. nPairs 0 is a call that kept nothing. */
int hj_pairs_verify2_dev(hj_ctx *ctx, const uint32_t *dMapS, const uint32_t *dMapR, uint64_t nPairs, uint32_t sRowBase,
                         uint64_t sRows, uint64_t rRows, const hj_key_col2 *cols, uint32_t nCols, uint32_t *dOutS,
                         uint32_t *dOutR, uint64_t capacity, uint32_t *dSMarks, uint32_t *dRMarks);
/* ---- the rows of ONE table grouped by their key columns: DISTINCT, GROUP BY key, a dense group id ----
 * Which rows of a table have the same key? For row i in [0, nRows), from the `side` pointers of cols[0 .. nCols) (as
 * hj_key_hash2_dev reads them):
 *   dRep[i]    the LOWEST row whose key equals row i's -- column equality exactly as hj_pairs_verify2_dev defines it: fixed
 *              width bytewise; variable length the same length and the same bytes; a NULL equals a NULL only in a column
 *              with HJ_KEY_NULLS_EQUAL.
 *   dFirstRows the rows with dRep[i] == i, ascending, from 0 without holes: one row per distinct key (DISTINCT ON, in
 *              order of first occurrence). Rows at or beyond `capacity` are counted and not written; capacity 0 with
 *              NULL is the count alone.
 *   dGroup[i]  the position of dRep[i] in the COMPLETE ascending list of first rows, whatever `capacity` is: a dense
 *              group id in order of first occurrence (pandas.factorize, torch.unique(return_inverse) up to the order).
 * A NULL-keyed row (some column WITHOUT HJ_KEY_NULLS_EQUAL is NULL in it, as above) belongs to no group: dRep[i] =
 * dGroup[i] = HJ_NO_ROW, it is counted apart (hj_key_groups_info out[3]) and its key bytes are never compared. With the
 * flag on every column no row is NULL-keyed and the NULLs form groups (SQL's GROUP BY). dGroup and dFirstRows may be
 * NULL (not wanted); dRep may not be NULL when nRows > 0. dGroup with HJ_NO_ROW entries is a dMapG that hj_pairs_agg_dev
 * takes as it stands: those pairs are skipped.
 * The result is exact and depends neither on keyMask (which only forces collisions, as in hj_key_hash2_dev), nor on the
 * slot a key lands in, nor on scheduling. Method: a hash table of >= 2 * nRows 8-byte slots (join word << 32 | row),
 * filled with EMPTY on the stream at the start of every call; an insert with the priority rule "the lowest row of a key
 * wins" (CAS into an empty slot, the real keys compared where the words agree, a 64-bit atomicMin only while the slot's row is
 * above i); a second launch that turns slots into rows and marks the first rows; the ordered sweep of hj_mark_rows_dev
 * for dFirstRows and the library's scan for the ids. No lane waits for another, and the probe loop is bounded by the
 * slot count: a row that exceeded it would set the failure word (out[7]) and end as HJ_NO_ROW -- the host never waits on it.
 * What is read of the columns: what hj_key_hash2_dev reads, and the elements again where two rows are compared.
 * Asynchronous on the context's stream; nRows 0 enqueues no kernel. Needs no hj_reserve, no table and no state; touches
 * no counter and no other *_info. The workspace (the table, one bit per row, one word per 32 rows, the sweep's counts)
 * belongs to the context and only grows: a call that needs more waits for the stream once. `cols` is host memory and is
 * read before the call returns. The outputs must not alias each other or the columns.
 * HJ_ERR_INVALID (nothing is enqueued; also for a NULL context): the column errors of hj_key_hash2_dev; side > 1; nRows
 * above 2^32 - 2; dRep NULL with nRows > 0; dFirstRows NULL with nRows > 0 and capacity > 0; an output pointer that is not
 * 4-byte aligned. */
int hj_key_groups_dev(hj_ctx *ctx, const hj_key_col2 *cols, uint32_t nCols, uint32_t side, uint64_t nRows,
                      uint32_t keyMask, uint32_t *dRep, uint32_t *dGroup, uint32_t *dFirstRows, uint64_t capacity);
/* Waits for the stream. About the last hj_key_groups_dev: out[0] = groups (= first rows found), out[1] = first rows
 * written (= min(out[0], capacity)), out[2] = the device time of the whole call in microseconds (rounded), out[3] =
 * NULL-keyed rows, out[4] = table slots, out[5] = probe steps beyond the home slot, summed over the rows, out[6] = key
 * compares that found a different key (word collisions), summed, out[7] = the device-side failure word, 0 on success.
 * out[5] and out[6] depend on scheduling (they describe the table, not the result). All 0 before the first call and
 * after a call with nRows 0. */
int hj_key_groups_info(hj_ctx *ctx, uint64_t out[8]);
/* The same function on host pointers: no context, no device (the hash and the compare are the kernels' bodies, around a
 * sequential table). out[0], out[1] and out[3] as above, the rest 0; out may not be NULL. HJ_ERR_INVALID as
 * hj_key_groups_dev; a refused call writes nothing. */
int hj_key_groups_host(const hj_key_col2 *cols, uint32_t nCols, uint32_t side, uint64_t nRows, uint32_t keyMask,
                       uint32_t *rep, uint32_t *group, uint32_t *firstRows, uint64_t capacity, uint64_t out[8]);
/* hj_r_rows_dev on a caller's plane: the rows rowBase + i, i in [0, rows), whose bit i of dMarks is clear (which =
 * HJ_R_UNMATCHED) or set (HJ_R_MATCHED), ascending, into dOut[0 ..) without holes; rows at or beyond `capacity` are counted
 * and not written (capacity 0: the count alone). The plane is read, never changed; the sweep's count workspace belongs to
 * the context and grows with `rows`. Asynchronous; needs no hj_reserve and no state; touches no counter of hj_result,
 * hj_pairs_info, hj_r_rows_info or hj_gather_info.
 * HJ_ERR_INVALID (nothing is enqueued; also for a NULL context): which > 1; dMarks NULL with rows > 0; dOut NULL with
 * rows > 0 and capacity > 0; rows or rowBase + rows above 2^32 - 1. */
int hj_mark_rows_dev(hj_ctx *ctx, const uint32_t *dMarks, uint64_t rows, uint32_t rowBase, uint32_t which, uint32_t *dOut,
                     uint64_t capacity);
/* Waits for the stream. About the last hj_mark_rows_dev: out[0] = rows produced, out[1] = rows written (= min(out[0],
 * capacity)), out[2] = its device time in microseconds (rounded), out[3] = its `rows`. All 0 before the first call. */
int hj_mark_rows_info(hj_ctx *ctx, uint64_t out[4]);
/* ---- join conditions beyond equality: typed comparisons on the matched pair ----
 * ... ON S.k = R.k AND S.ts >= R.valid_from AND S.ts < R.valid_to: an equi-join plus a condition on the pair. For the
 * kinds other than INNER the condition belongs to the match -- an S row whose pairs all fail it is an unmatched row of a
 * left or anti join, and the same goes for R -- so it cannot be a filter behind the join, and the context's own
 * HJ_FLAG_TRACK_R_MATCHES marks are of no use: a pair the condition rejects would have set them. hj_pairs_where_dev is one
 * more step of the flow above: pairs in (an INNER probe's, or hj_pairs_verify_dev's kept ones), the pairs that pass out,
 * and their rows marked in two caller-owned planes, from which hj_mark_rows_dev gives all eight kinds.
 * A condition is the AND of 1 to HJ_WHERE_MAX_TERMS terms  s[si] OP r[ri], both sides of a term of one type and width.
 * A pair is kept iff every term holds. A term with a NULL on either side does not hold (SQL's unknown), HJ_CMP_NE
 * included; the bytes under a NULL are never compared (they are read: they exist). HJ_VAL_UINT / HJ_VAL_INT compare as
 * integers of that width and signedness. HJ_VAL_FLOAT compares as IEEE-754 binary32 / binary64, which is NOT the bytewise
 * equality of the key columns above: -0.0 == +0.0, and with a NaN on either side EQ, LT, LE, GT and GE are false and NE
 * is true. No constants, no arithmetic, no OR, no ordering of strings, no 16-bit floats. */
#define HJ_WHERE_MAX_TERMS 4
typedef enum { HJ_CMP_EQ = 0, HJ_CMP_NE = 1, HJ_CMP_LT = 2, HJ_CMP_LE = 3, HJ_CMP_GT = 4, HJ_CMP_GE = 5 } hj_cmp_op;
typedef enum { HJ_VAL_UINT = 0, HJ_VAL_INT = 1, HJ_VAL_FLOAT = 2 } hj_val_type;
typedef struct {
    const void     *s, *r;            /* sRows / rRows elements of `width` bytes, aligned to it            */
    const uint32_t *sValid, *rValid;  /* NULL: no NULLs. Else the plane hj_gather_dev writes, 1 = valid    */
    uint32_t width;                   /* UINT / INT: 1, 2, 4, 8.  FLOAT: 4, 8                              */
    uint32_t type;                    /* hj_val_type, the same on both sides                               */
    uint32_t op;                      /* hj_cmp_op: the term is  s[si] OP r[ri]                            */
    uint32_t reserved;                /* 0                                                                 */
} hj_where_term;                      /* 48 bytes */
/* Pairs -> the pairs whose terms all hold. Pairs, output and marks are hj_pairs_verify_dev's, word for word: for pair k in
 * [0, nPairs): s = dMapS[k] - sRowBase, r = dMapR[k]. A pair whose raw entry is HJ_NO_ROW on either side, or with
 * s >= sRows or r >= rRows, is never dereferenced: it is dropped and counted apart (hj_where_info out[3]). Kept pairs go to
 * dOutS / dOutR under the output contract of hj_probe_pairs_dev: dOutS[j] is the original entry dMapS[k], base included;
 * the planes fill from 0 without holes; pairs at or beyond `capacity` are counted and not written; the order is
 * unspecified, the multiset is exact. Every kept pair, written or cut by the capacity, sets bit s of dSMarks and bit r of
 * dRMarks where those are not NULL: bit i & 31 of 32-bit word i >> 5, words 0 .. ceil(rows / 32) - 1, nothing behind
 * them. Bits only go 0 -> 1: the caller clears the planes. capacity 0 with NULL outputs is a mark-only pass. dOutS / dOutR
 * must not alias dMapS / dMapR, each other, or the planes. sValid is indexed by s (the base is off): ceil(sRows / 32)
 * words; rValid holds ceil(rRows / 32). `terms` is host memory, read before the call returns. Asynchronous on the
 * context's stream; needs no hj_reserve, no table and no state; touches no counter of hj_result and no other *_info.
 * HJ_ERR_INVALID (nothing is enqueued; also for a NULL context): nTerms 0 or above HJ_WHERE_MAX_TERMS, terms NULL; a type
 * above HJ_VAL_FLOAT, an op above HJ_CMP_GE, a width the type does not have; reserved != 0; with sRows > 0 an s pointer that
 * is NULL or not aligned to its width, likewise r with rRows > 0; a validity pointer that is not 4-byte aligned; a map
 * NULL with nPairs > 0; an output NULL with nPairs > 0 and capacity > 0; nPairs, sRows or rRows above 2^32 - 1. nPairs 0 is
 * a call that kept nothing. */
int hj_pairs_where_dev(hj_ctx *ctx, const uint32_t *dMapS, const uint32_t *dMapR, uint64_t nPairs, uint32_t sRowBase,
                       uint64_t sRows, uint64_t rRows, const hj_where_term *terms, uint32_t nTerms, uint32_t *dOutS,
                       uint32_t *dOutR, uint64_t capacity, uint32_t *dSMarks, uint32_t *dRMarks);
/* Waits for the stream. About the last hj_pairs_where_dev: out[0] = pairs kept, out[1] = pairs written (= min(out[0],
 * capacity)), out[2] = its device time in microseconds (rounded), out[3] = pairs dropped as HJ_NO_ROW or out of range.
 * Rejected pairs = nPairs - out[0] - out[3]. All 0 before the first call. */
int hj_where_info(hj_ctx *ctx, uint64_t out[4]);
/* The same function on host pointers: no context, no device (the kernel and this loop evaluate a term with one body).
 * The kept pairs are written in input order; `info` (may be NULL) is filled as hj_where_info fills out, info[2] = 0.
 * HJ_ERR_INVALID as hj_pairs_where_dev; a refused call writes nothing. */
int hj_pairs_where_host(const uint32_t *mapS, const uint32_t *mapR, uint64_t nPairs, uint32_t sRowBase, uint64_t sRows,
                        uint64_t rRows, const hj_where_term *terms, uint32_t nTerms, uint32_t *outS, uint32_t *outR,
                        uint64_t capacity, uint32_t *sMarks, uint32_t *rMarks, uint64_t info[4]);
/* ---- as-of joins: one best match per S row ----
 * ... ON S.k = R.k AND S.ts >= R.ts, and of the R rows that qualify the LATEST one: the price in force, the last quote
 * before a trade (pandas.merge_asof, DuckDB's ASOF JOIN). R carries one timestamp per version, not an interval, so no
 * condition on the pair alone expresses it: whether a pair survives depends on the other pairs of its S row. The as-of
 * step is an arg-max per S row over the matched pairs and sits behind hj_pairs_where_dev as that sits behind the verify
 * step: pairs in (an INNER probe's, the verify step's or the condition step's kept ones), per S row at most one pair out,
 * and the rows of the pairs that come out marked in two caller-owned planes, from which hj_mark_rows_dev gives all eight
 * kinds.
 * The term  s[si] OP r[ri]  is an hj_where_term's with OP one of HJ_CMP_GE, HJ_CMP_GT, HJ_CMP_LE, HJ_CMP_LT. A pair is
 * ELIGIBLE when the term holds with hj_pairs_where_dev's meaning: a NULL on either side does not hold, a NaN is unordered
 * and does not hold, -0.0 == 0.0. Per S row exactly one eligible pair is KEPT (none when it has no eligible pair): for
 * GE / GT the pair with the largest R value (backward: the latest at or before), for LE / LT the pair with the smallest
 * (forward). Ties on the R value -- -0.0 and 0.0 are one -- go to the lowest R row: the library's index-priority rule.
 * The result therefore depends neither on the order of the list nor on scheduling. */
typedef struct {
    const void     *s, *r;            /* sRows / rRows elements of `width` bytes, aligned to it            */
    const uint32_t *sValid, *rValid;  /* NULL: no NULLs. Else the plane hj_gather_dev writes, 1 = valid    */
    uint32_t width;                   /* UINT / INT: 1, 2, 4, 8.  FLOAT: 4, 8                              */
    uint32_t type;                    /* hj_val_type, the same on both sides                               */
    uint32_t op;                      /* HJ_CMP_GE, HJ_CMP_GT (backward), HJ_CMP_LE, HJ_CMP_LT (forward)    */
    uint32_t reserved;                /* 0                                                                 */
} hj_asof_term;                       /* 48 bytes */
/* Pairs -> per S row the as-of pair. Pairs, output and marks are hj_pairs_where_dev's: for pair k in [0, nPairs):
 * s = dMapS[k] - sRowBase, r = dMapR[k]; a pair whose raw entry is HJ_NO_ROW on either side, or with s >= sRows or
 * r >= rRows, is never dereferenced: it is dropped and counted apart (hj_asof_info out[3]). Kept pairs go to dOutS / dOutR
 * under the output contract of hj_probe_pairs_dev (dOutS[j] the original entry, base included; no holes; pairs at or beyond
 * `capacity` counted and not written; order unspecified, multiset exact). Every kept pair, written or cut by the capacity,
 * sets bit s of dSMarks and bit r of dRMarks where those are not NULL, bits only going 0 -> 1: the caller clears the
 * planes. An R row is marked only when it wins some S row: an eligible pair that loses marks nothing. capacity 0 with NULL
 * outputs is a mark-only pass. dOutS / dOutR must not alias the maps, each other, the mark planes or the best planes.
 * dBestVal (sRows 64-bit words, 8-byte aligned) and dBestRow (sRows 32-bit words) are caller-owned planes that the call
 * initialises itself, on the context's stream. dBestRow is an OUTPUT: after the call dBestRow[i] is the R row kept for S row
 * sRowBase + i, or HJ_NO_ROW -- the left-outer as-of map in S order. dBestVal is workspace (it ends as the order key of the
 * kept pair's R value, 0 without one).
 * ALL PAIRS OF AN S ROW MUST BE IN ONE CALL: the planes are reset per call, and the best pair of half a list is not the
 * best pair of the list. Each (s, r) occurs at most once in a join's pair list, so one pair per matched S row is kept; in
 * a list that repeats the winning pair each copy is kept and counted.
 * Three kernels behind the two initialisations, each reading the whole list (profiles/pairs_asof.md). `term` is host
 * memory, read before the call returns. Asynchronous on the context's stream; needs no hj_reserve, no table and no state;
 * touches no counter of hj_result and no other *_info.
 * HJ_ERR_INVALID (nothing is enqueued; also for a NULL context): term NULL; a type above HJ_VAL_FLOAT; an op that is not
 * GE, GT, LE or LT (EQ and NE order nothing); a width the type does not have; reserved != 0; with sRows > 0 an s pointer
 * that is NULL or not aligned to its width, likewise r with rRows > 0; a validity pointer that is not 4-byte aligned;
 * dBestVal NULL or not 8-byte aligned, dBestRow NULL or not 4-byte aligned; a map NULL with nPairs > 0; an output NULL with
 * nPairs > 0 and capacity > 0; nPairs, sRows or rRows above 2^32 - 1. nPairs 0 is a call that kept nothing (the planes are
 * initialised all the same). */
int hj_pairs_asof_dev(hj_ctx *ctx, const uint32_t *dMapS, const uint32_t *dMapR, uint64_t nPairs, uint32_t sRowBase,
                      uint64_t sRows, uint64_t rRows, const hj_asof_term *term, uint64_t *dBestVal, uint32_t *dBestRow,
                      uint32_t *dOutS, uint32_t *dOutR, uint64_t capacity, uint32_t *dSMarks, uint32_t *dRMarks);
/* Waits for the stream. About the last hj_pairs_asof_dev: out[0] = pairs kept, out[1] = pairs written (= min(out[0],
 * capacity)), out[2] = the device time of the whole call -- initialisations and all three kernels -- in microseconds
 * (rounded), out[3] = pairs dropped as HJ_NO_ROW or out of range. All 0 before the first call. */
int hj_asof_info(hj_ctx *ctx, uint64_t out[4]);
/* The same function on host pointers: no context, no device (the kernels and these loops compare and order with one
 * body). bestVal / bestRow are initialised and left as the device call leaves them. The kept pairs are written in input
 * order; `info` (may be NULL) is filled as hj_asof_info fills out, info[2] = 0. HJ_ERR_INVALID as hj_pairs_asof_dev; a
 * refused call writes nothing. */
int hj_pairs_asof_host(const uint32_t *mapS, const uint32_t *mapR, uint64_t nPairs, uint32_t sRowBase, uint64_t sRows,
                       uint64_t rRows, const hj_asof_term *term, uint64_t *bestVal, uint32_t *bestRow, uint32_t *outS,
                       uint32_t *outR, uint64_t capacity, uint32_t *sMarks, uint32_t *rMarks, uint64_t info[4]);
/* ---- the rows of ONE table in the order of their columns: ORDER BY ----
 * Every call above that returns rows leaves their order unspecified. hj_sort_rows_dev puts the rows of a table in order:
 * dPerm[0 .. nRows) is the permutation of the rows 0 .. nRows - 1 in ASCENDING LEXICOGRAPHIC order of cols[0 .. nCols),
 * cols[0] the most significant -- ORDER BY a DESC, b NULLS FIRST, c, d over typed, nullable columns in one call. A gather
 * through dPerm (hj_gather_dev / hj_gather2_dev) puts any column of the table, strings included, in that order.
 * Within a column two valid elements compare as a term of hj_pairs_where_dev compares them: HJ_VAL_UINT / HJ_VAL_INT as
 * integers of the width and signedness; HJ_VAL_FLOAT as IEEE-754 binary32 / binary64 values with -0.0 == 0.0. Where that
 * comparison has no opinion a sort must have one, and it is numpy's and pandas': every NaN, whatever its sign or payload,
 * equals every other NaN and is greater than +inf. HJ_SORT_DESC reverses the order of the column's valid elements, NaN
 * included (the NaNs then come first among them). A NULL equals a NULL, and the NULLs of a column stand BEHIND all its
 * valid elements, or in FRONT of them with HJ_SORT_NULLS_FIRST -- independently of HJ_SORT_DESC: pandas' na_position, not
 * PostgreSQL's default (where DESC implies NULLS FIRST). The bytes under a NULL are read (they exist) and never influence
 * the result. Rows equal in every column keep ascending row order: the sort is stable, the library's index-priority rule.
 * The result is therefore unique, independent of scheduling, and the same bit for bit on every run.
 * Method (hj_sort.hip): an LSD radix sort over (key, row) records, 8 bits per pass, the columns processed last
 * to first; 4-byte keys for elements of 1, 2 and 4 bytes -- a pass per element byte: an int16 column costs 2 passes, a
 * float32 column is not widened --, 8-byte keys for 8-byte elements, and one 2-bin pass more for a column with a validity
 * plane. A pass is a per-chunk histogram, the library's scan, and a stable scatter that ranks with ballots, without an
 * atomic. No workgroup waits for another (no look-back, no flag that is spun on); every loop is bounded by the chunk.
 * What it does NOT do: strings (as the condition step: no ordering of strings), 16-byte elements, collations, a row map
 * as input (gather first), top-k without the full sort, more than HJ_SORT_MAX_COLS columns in a call.
 * Asynchronous on the context's stream; nRows 0 enqueues no kernel. Needs no hj_reserve, no table and no state; touches no
 * counter and no other *_info. The workspace (two key planes and two row planes of nRows, a histogram of 256 words per
 * chunk, the scan's sums: hj_sort_layout_info) belongs to the context and only grows: a call that needs more waits for
 * the stream once. `cols` is host memory and is read before the call returns. dPerm must not alias a column or a plane.
 * Nothing is written outside dPerm[0 .. nRows).
 * HJ_ERR_INVALID (nothing is enqueued; also for a NULL context): nCols 0 or above HJ_SORT_MAX_COLS, cols NULL; a type
 * above HJ_VAL_FLOAT, a width the type does not have; flag bits other than the two defined; reserved != 0; with nRows > 0
 * a values pointer that is NULL or not aligned to its width, a validity pointer that is not 4-byte aligned, dPerm NULL or
 * not 4-byte aligned; nRows above 2^32 - 2. */
#define HJ_SORT_MAX_COLS   4
#define HJ_SORT_DESC        0x1u   /* this column descending */
#define HJ_SORT_NULLS_FIRST 0x2u   /* this column's NULLs before its values (default: after) */
typedef struct {
    const void     *values;   /* nRows elements of `width` bytes, aligned to it        */
    const uint32_t *valid;    /* NULL: no NULLs. Else the plane hj_gather_dev writes   */
    uint32_t width;           /* UINT / INT: 1, 2, 4, 8.  FLOAT: 4, 8                  */
    uint32_t type;            /* hj_val_type                                           */
    uint32_t flags;           /* HJ_SORT_DESC | HJ_SORT_NULLS_FIRST                    */
    uint32_t reserved;        /* 0                                                     */
} hj_sort_col;                /* 32 bytes */
int hj_sort_rows_dev(hj_ctx *ctx, const hj_sort_col *cols, uint32_t nCols, uint64_t nRows, uint32_t *dPerm);
/* Waits for the stream. About the last hj_sort_rows_dev: out[0] = rows, out[1] = radix passes launched (one per element
 * byte and one per validity plane), out[2] = the device time of the whole call in microseconds (rounded), out[3] = passes
 * skipped (always 0: no pass is skipped), out[4] = chunks, out[5] = chunk rows, out[6] = workspace bytes the call needed,
 * out[7] = 0. All 0 before the first call and after a call with nRows 0. */
int hj_sort_rows_info(hj_ctx *ctx, uint64_t out[8]);
/* The same function on host pointers: no context, no device (the order key is the kernels' body, around one stable sort
 * per column). `out` (may be NULL) is filled as hj_sort_rows_info fills it, out[2] = 0. HJ_ERR_INVALID as
 * hj_sort_rows_dev; a refused call writes nothing. */
int hj_sort_rows_host(const hj_sort_col *cols, uint32_t nCols, uint64_t nRows, uint32_t *perm, uint64_t out[8]);
/* How a pass cuts nRows rows; a pure function, no context and no device: out[0] = tile rows (what one workgroup ranks at
 * a time), out[1] = chunk rows (what one workgroup owns in a pass, a multiple of the tile; grows with nRows), out[2] =
 * chunks (at most 4096 at any nRows: the histogram of a pass is bounded by 256 x 4096 words = 4 MiB), out[3] = workspace
 * bytes with 8-byte keys (monotone in nRows). HJ_ERR_INVALID for out NULL or nRows above 2^32 - 2. */
int hj_sort_layout_info(uint64_t nRows, uint64_t out[4]);
/* ---- window functions over sorted rows: f(...) OVER (PARTITION BY keys ORDER BY cols) ----
 * The step between the sort and the gather: hj_key_groups_dev gives every row a dense partition id, hj_sort_rows_dev over
 * (id, order columns) puts every partition in order, and hj_window_rows_dev scans along that permutation: ROW_NUMBER, RANK,
 * DENSE_RANK, the rows of the partition, LAG / LEAD / first / last row as gather maps (hj_gather_dev / hj_gather2_dev turn
 * them into values with NULLs, strings included), and running COUNT / SUM / MIN / MAX.
 * Everything is defined on RUNS along dPerm, not on sortedness: the call is exact for any dPerm, and the host twin is one
 * sequential loop. For position p in [0, nPos), row(p) = dPerm[p]; dPerm NULL is the identity and needs nPos <= nRows.
 *   An entry that is HJ_NO_ROW or >= nRows is never dereferenced and writes nothing; it is counted apart (info out[4]). It
 *     ends the run in front of it, and the next position starts a new one. It is in no partition and no peer run.
 *   The partition of p, [start(p), end(p)], is the maximal run of in-range positions around p whose dPart[row] are equal.
 *     The ids are compared for equality only, HJ_NO_ROW is a value like any other; dPart NULL: one value everywhere.
 *   Two rows are peers when in every one of the nOrder columns both are NULL, or both are valid and their order keys are
 *     equal -- the sort's own tie: -0.0 == 0.0, every NaN equals every NaN, the bytes under a NULL are never compared. The
 *     column flags do not change equality. nOrder 0: all rows of a partition are peers. peerStart(p) is the lowest q in
 *     [start(p), p] such that q .. p are all peers of p.
 * out[row(p)] of a function:
 *   HJ_WIN_ROW_NUMBER  p - start + 1                      HJ_WIN_RANK       peerStart - start + 1
 *   HJ_WIN_DENSE_RANK  the peer runs that start in [start, p]      HJ_WIN_PART_ROWS  end - start + 1
 *   HJ_WIN_LAG         dPerm[p - offset] if p - offset >= start, else HJ_NO_ROW (no wrap for an offset above p)
 *   HJ_WIN_LEAD        dPerm[p + offset] if p + offset <= end, else HJ_NO_ROW (no wrap near 2^32)
 *   HJ_WIN_FIRST_ROW   dPerm[start]                       HJ_WIN_LAST_ROW   dPerm[end]
 *   HJ_WIN_RUN_*       COUNT / SUM / MIN / MAX over the valid elements src[row(q)], q in [start, p] -- the frame ROWS BETWEEN
 *     UNBOUNDED PRECEDING AND CURRENT ROW (pandas' cumsum), unique because the order along dPerm is fixed. Values, sign
 *     extension, wrap-around (SUM modulo 2^64) and the identity where the frame holds no valid element are
 *     hj_pairs_agg_dev's. RUN_COUNT counts the valid elements, or the positions when srcValid is NULL. There is no output
 *     validity: whether a SUM / MIN / MAX saw a value is RUN_COUNT of the same column > 0. Integers only.
 * A row that occurs at no position is not written: `out` keeps what the caller put there. A row that occurs at two
 * positions keeps one of its two results (unspecified); nothing else is affected.
 * Method (hj_window.hip): segmented scans over positions in five launches -- head bits, per-chunk summaries, one
 * workgroup over the at most 4096 summaries, end(p) from the back where a function needs it, and one pass that computes
 * every function of the call. No workgroup waits for another, no atomic; every loop is bounded by the chunk.
 * Cost: two scattered rows per position for the head bits; per RUN function two scattered reads of its source (fewer
 * where partitions are short); per function and position one scattered 4- or 8-byte store. With dPerm NULL all of it is
 * coalesced.
 * Asynchronous on the context's stream; nPos 0 enqueues nothing. Needs no hj_reserve, no table and no state; touches no
 * counter and no other *_info. The workspace (hj_window_layout_info) belongs to the context and only grows: a call that
 * needs more waits for the stream once. `funcs` and `order` are host memory and are read before the call returns. Outputs
 * must not alias each other, dPerm, dPart or a column. Nothing is written outside out[0 .. nRows) of each function.
 * HJ_ERR_INVALID (nothing is enqueued, nothing written; also for a NULL context): nFuncs 0 or above HJ_WIN_MAX_FUNCS, funcs
 * NULL; an op above HJ_WIN_RUN_MAX; a width the op does not have (RUN_SUM / MIN / MAX: 4 or 8; RUN_COUNT: 0, 4 or 8; else
 * 0); flags other than HJ_AGG_SIGNED on a RUN_* op, or any on another; offset != 0 outside LAG / LEAD; an out that is NULL
 * or not aligned to its entries (4 or 8 bytes); with nRows > 0 a src that is NULL or not aligned to its width where the
 * op reads one (RUN_SUM / MIN / MAX); a srcValid that is not 4-byte aligned; nOrder above HJ_SORT_MAX_COLS, order NULL
 * with nOrder > 0, or the column errors of hj_sort_rows_dev; dPerm NULL with nPos > nRows; dPerm or dPart not 4-byte
 * aligned; nPos or nRows above 2^32 - 2. */
#define HJ_WIN_MAX_FUNCS 8
typedef enum {
    HJ_WIN_ROW_NUMBER = 0, HJ_WIN_RANK = 1, HJ_WIN_DENSE_RANK = 2, HJ_WIN_PART_ROWS = 3,   /* out: uint32 per row   */
    HJ_WIN_LAG = 4, HJ_WIN_LEAD = 5, HJ_WIN_FIRST_ROW = 6, HJ_WIN_LAST_ROW = 7,            /* out: uint32 row map   */
    HJ_WIN_RUN_COUNT = 8, HJ_WIN_RUN_SUM = 9, HJ_WIN_RUN_MIN = 10, HJ_WIN_RUN_MAX = 11     /* out: 8 bytes per row  */
} hj_win_op;
typedef struct {
    const void     *src;       /* RUN_*: nRows elements of `width` bytes; else ignored (may be NULL)            */
    const uint32_t *srcValid;  /* RUN_*: NULL = no NULLs, else the plane hj_gather_dev writes                   */
    void           *out;       /* nRows entries INDEXED BY ROW: 4 bytes (ops 0..7) or 8 bytes (ops 8..11)       */
    uint32_t        op;        /* hj_win_op                                                                     */
    uint32_t        width;     /* RUN_SUM/MIN/MAX: 4 or 8; RUN_COUNT: 0, 4 or 8; else 0                         */
    uint32_t        flags;     /* HJ_AGG_SIGNED or 0 (RUN_* only)                                               */
    uint32_t        offset;    /* LAG / LEAD: k (0 .. 2^32 - 1); else 0                                         */
} hj_win_func;                 /* 40 bytes */
int hj_window_rows_dev(hj_ctx *ctx, const uint32_t *dPerm, uint64_t nPos, uint64_t nRows, const uint32_t *dPart,
                       const hj_sort_col *order, uint32_t nOrder, const hj_win_func *funcs, uint32_t nFuncs);
/* Waits for the stream. About the last hj_window_rows_dev: out[0] = positions, out[1] = partitions (runs of in-range
 * positions; a skipped entry is none), out[2] = peer runs, out[3] = the device time of the whole call in microseconds
 * (rounded), out[4] = entries skipped as HJ_NO_ROW or out of range, out[5] = chunks, out[6] = workspace bytes the call
 * needed, out[7] = 0. All 0 before the first call and after a call with nPos 0. */
int hj_window_rows_info(hj_ctx *ctx, uint64_t out[8]);
/* The same function on host pointers: no context, no device (the head test and the accumulate bodies are the kernels',
 * around one sequential loop). `out` (may be NULL) is filled as hj_window_rows_info fills it, out[3] = 0. HJ_ERR_INVALID
 * as hj_window_rows_dev; a refused call writes nothing. */
int hj_window_rows_host(const uint32_t *perm, uint64_t nPos, uint64_t nRows, const uint32_t *part,
                        const hj_sort_col *order, uint32_t nOrder, const hj_win_func *funcs, uint32_t nFuncs, uint64_t out[8]);
/* How a call cuts nPos positions; a pure function, no context and no device: out[0] = tile positions (what one workgroup
 * scans at a time), out[1] = chunk positions (what one workgroup owns, a multiple of the tile; grows with nPos), out[2] =
 * chunks (at most 4096 at any nPos: one workgroup scans their summaries), out[3] = workspace bytes (one head byte and one
 * 4-byte end per position, and the chunk summaries; monotone in nPos). HJ_ERR_INVALID for out NULL or nPos above 2^32 - 2. */
int hj_window_layout_info(uint64_t nPos, uint64_t out[4]);
/* ---- sliding window frames: f(x) OVER (PARTITION BY keys ORDER BY cols ROWS BETWEEN lo AND hi) ----
 * hj_window_rows_dev knows one frame, UNBOUNDED PRECEDING to CURRENT ROW. hj_window_frames_dev computes COUNT / SUM / MIN /
 * MAX over a frame of ROWS around every position: the 7-day moving sum (lo -6, hi 0), the rolling maximum of the last 100
 * ticks, the centred window, a frame that leaves the current row out (lo -3, hi -1), and with both sides unbounded the
 * partition's total next to every row (pandas' groupby().rolling(w) and groupby().transform()).
 * Positions, rows, partitions and skipped entries are EXACTLY hj_window_rows_dev's: for position p in [0, nPos), row(p) =
 * dPerm[p] (dPerm NULL: the identity, needs nPos <= nRows); the partition of p, [start, end], is the maximal run of in-range
 * positions around p whose dPart[row] are equal (dPart NULL: one value); an entry that is HJ_NO_ROW or >= nRows is never
 * dereferenced, writes nothing, is counted (info out[4]) and cuts the run. The call is exact for any dPerm. Peers play no
 * part: there are no order columns.
 * THE FRAME of position p is [max(start, p + lo), min(end, p + hi)]: lo and hi are signed offsets relative to p, lo <= hi,
 * both in [-(2^32 - 1), 2^32 - 1]; (0, 0) is the element itself. HJ_FRAME_UNBOUNDED_LO / _HI put start / end in the place of
 * that side, and its offset must be 0; both: the whole partition. p + lo and p + hi are formed in 64 bits: nothing wraps.
 * A frame with L > R is empty.
 * out[row(p)], 8 bytes per row: the op (an hj_agg_op) over the valid elements src[row(q)], q in the frame. Values, sign
 * extension of 4-byte elements (HJ_AGG_SIGNED), wrap-around (SUM modulo 2^64) and the identity of an empty frame or of one
 * without a valid element are hj_pairs_agg_dev's; COUNT counts the valid elements, or the positions when srcValid is NULL,
 * and is 0 for an empty frame. There is no output validity: whether a SUM / MIN / MAX saw a value is COUNT of the same
 * column and frame > 0. Integers only. A row that occurs at no position keeps the caller's bytes; a row at two positions
 * keeps one of its two results.
 * Method (hj_frames.hip): positions are cut into blocks of W = hi - lo + 1; one forward and one backward
 * segmented scan whose segments end at the partition's AND the block's borders give G and H, and a frame, which touches
 * at most two blocks, is op(H[L], G[R]) -- O(1) per position whatever W, for MIN and MAX too. Per function: one scattered
 * read of src through dPerm into a position-indexed plane, two coalesced scans over it (one with an unbounded side), one
 * coalesced combine with a scattered 8-byte store. No workgroup waits for another, no atomic, every loop bounded by the chunk.
 * WORKSPACE (hj_frames_layout_info): one head byte, one 4-byte end and TWO 8-byte planes per position, which the functions
 * of a call share one after another, plus the chunk summaries (192 KiB): 21 bytes per position, and never more than 32 bytes
 * per position plus 1 MiB, whatever nFuncs. It belongs to the context, apart from hj_window_rows_dev's, and only grows: a
 * call that needs more waits for the stream once.
 * Asynchronous on the context's stream; nPos 0 enqueues nothing. Needs no hj_reserve, no table and no state; touches no
 * counter and no other *_info. `funcs` is host memory and is read before the call returns. Outputs must not alias each
 * other, dPerm, dPart or a column. Nothing is written outside out[0 .. nRows) of each function.
 * HJ_ERR_INVALID (nothing is enqueued, nothing written; also for a NULL context): nFuncs 0 or above HJ_FRAME_MAX_FUNCS, funcs
 * NULL; an op above HJ_AGG_MAX; a width the op does not have (SUM / MIN / MAX: 4 or 8; COUNT: 0, 4 or 8); flags other than
 * HJ_AGG_SIGNED and the two HJ_FRAME_UNBOUNDED_*; reserved != 0; an offset outside [-(2^32 - 1), 2^32 - 1]; a non-zero offset
 * beside its unbounded flag; lo > hi with both sides bounded; an out that is NULL or not 8-byte aligned; with nRows > 0 a
 * src that is NULL or not aligned to its width where the op reads one (SUM / MIN / MAX); a srcValid that is not 4-byte
 * aligned; dPerm NULL with nPos > nRows; dPerm or dPart not 4-byte aligned; nPos or nRows above 2^32 - 2. */
#define HJ_FRAME_MAX_FUNCS 8
#define HJ_FRAME_UNBOUNDED_LO 0x2u   /* hj_frame_func.flags: the frame starts at the partition's first position; lo must be 0 */
#define HJ_FRAME_UNBOUNDED_HI 0x4u   /* ... ends at the partition's last position; hi must be 0                              */
typedef struct {
    const void     *src;       /* nRows elements of `width` bytes; COUNT: ignored (may be NULL)                 */
    const uint32_t *srcValid;  /* NULL = no NULLs, else the plane hj_gather_dev writes                          */
    void           *out;       /* nRows entries of 8 bytes INDEXED BY ROW                                       */
    int64_t         lo;        /* the frame's first position relative to p (negative: preceding)                */
    int64_t         hi;        /* the frame's last position relative to p                                       */
    uint32_t        op;        /* hj_agg_op                                                                     */
    uint32_t        width;     /* SUM / MIN / MAX: 4 or 8; COUNT: 0, 4 or 8                                     */
    uint32_t        flags;     /* HJ_AGG_SIGNED | HJ_FRAME_UNBOUNDED_LO | HJ_FRAME_UNBOUNDED_HI                 */
    uint32_t        reserved;  /* must be 0                                                                     */
} hj_frame_func;               /* 56 bytes */
int hj_window_frames_dev(hj_ctx *ctx, const uint32_t *dPerm, uint64_t nPos, uint64_t nRows, const uint32_t *dPart,
                         const hj_frame_func *funcs, uint32_t nFuncs);
/* Waits for the stream. About the last hj_window_frames_dev, in hj_window_rows_info's places: out[0] = positions, out[1] =
 * partitions (runs of in-range positions; a skipped entry is none), out[2] = 0 (no peer runs), out[3] = the device time of
 * the whole call in microseconds (rounded), out[4] = entries skipped as HJ_NO_ROW or out of range, out[5] = chunks, out[6] =
 * workspace bytes the call needed, out[7] = 0. All 0 before the first call and after a call with nPos 0. */
int hj_window_frames_info(hj_ctx *ctx, uint64_t out[8]);
/* The same function on host pointers: no context, no device, and ANOTHER ALGORITHM on purpose -- one sequential loop per
 * function, COUNT / SUM by a running window (add the entering element, subtract the leaving one, modulo 2^64), MIN / MAX by
 * a monotonic deque; no blocks, no scans; O(nPos) per function whatever W. Twin and kernels are two independent computations
 * of one definition. `out` (may be NULL) is filled as hj_window_frames_info fills it, out[3] = 0. HJ_ERR_INVALID as
 * hj_window_frames_dev; a refused call writes nothing. */
int hj_window_frames_host(const uint32_t *perm, uint64_t nPos, uint64_t nRows, const uint32_t *part,
                          const hj_frame_func *funcs, uint32_t nFuncs, uint64_t out[8]);
/* How a call cuts nPos positions; a pure function, no context and no device: out[0] = tile positions, out[1] = chunk
 * positions (both hj_window_layout_info's), out[2] = chunks (at most 4096), out[3] = workspace bytes (monotone in nPos; at
 * most 32 bytes per position plus 1 MiB). HJ_ERR_INVALID for out NULL or nPos above 2^32 - 2. */
int hj_frames_layout_info(uint64_t nPos, uint64_t out[4]);
/* ---- range joins without an equality key: ... ON R.y BETWEEN S.lo AND S.hi ----
 * Every join above starts from an equality on a join word. These two calls join on an ORDER condition alone: events
 * against sessions, packets against address blocks, readings against calibration periods, one bound (R.y < S.x), and the
 * as-of join without a `by` key (hj_range_pick). The same join with the sides swapped (S.x BETWEEN R.lo AND R.hi) is this
 * one with S's points indexed and R's intervals probing.
 *
 * THE INDEX of R's column is the caller's: three device planes, built once by hj_range_index_dev and probed by any number
 * of hj_range_pairs_dev calls, one per slice of S.
 *   dPerm[0 .. nRows)  hj_sort_rows_dev's ascending, stable permutation of the one column (NULLs last, every NaN above
 *                      +inf in front of them); col->flags must be 0: HJ_SORT_DESC and HJ_SORT_NULLS_FIRST are refused
 *   dKeys[0 .. nRows)  the order key of the element of row dPerm[q], in a plane of 4-byte words (widths 1, 2 and 4) or of
 *                      8-byte words (width 8)
 *   dHead[0 .. 4)      rows indexed, NULL rows, NaN rows, key bytes (4 or 8)
 * The indexed rows are the leading positions whose element is valid and no NaN: a NULL or a NaN lies in no range, and the
 * ascending order puts them last, so the indexed rows are a prefix and dHead[0] is its length. The CONTENT of the three
 * planes belongs to the library: a caller that edits them gets undefined pairs (never a write outside the outputs: the
 * range call takes no more than rRows rows of them whatever dHead says). Asynchronous on the context's stream; the
 * workspace is hj_sort_rows_dev's; needs no hj_reserve, no table and no state. HJ_ERR_INVALID: what hj_sort_rows_dev
 * refuses of one column, flags other than 0, nRows above 2^32 - 2, dKeys NULL or not aligned to its key bytes with
 * nRows > 0, dHead NULL or not 4-byte aligned. nRows 0 writes dHead alone. */
int hj_range_index_dev(hj_ctx *ctx, const hj_sort_col *col, uint64_t nRows, uint32_t *dPerm, void *dKeys, uint32_t *dHead);
/* Waits for the stream. About the last hj_range_index_dev, whose dHead must still be allocated: out[0] = rows indexed,
 * out[1] = NULL rows, out[2] = the device time of the call in microseconds (rounded), out[3] = NaN rows. All 0 before
 * the first call. */
int hj_range_index_info(hj_ctx *ctx, uint64_t out[4]);
/* The same index on host pointers: no context, no device (the order key is the kernels', the order hj_sort_rows_host's).
 * HJ_ERR_INVALID as hj_range_index_dev; a refused call writes nothing. */
int hj_range_index_host(const hj_sort_col *col, uint64_t nRows, uint32_t *perm, void *keys, uint32_t head[4]);
/* How the range call cuts an index of nRows rows probed by sRows S rows; a pure function, no context and no device:
 * out[0] = pivots (every out[1]-th key of the index, searched in LDS), out[1] = the pivot stride (a power of two, at least
 * 16: what is left of a search runs over stride - 1 keys in global memory), out[2] = the pair tile (output positions one
 * workgroup of the expansion owns), out[3] = workspace bytes (monotone in both arguments), out[4] = chunk rows (S rows one
 * workgroup takes to their bounds), out[5] = chunks, out[6] = the LDS bytes the pivots may take (8 * out[0] at most),
 * out[7] = 0. HJ_ERR_INVALID for out NULL or a row count above 2^32 - 2. */
int hj_range_layout_info(uint64_t nRows, uint64_t sRows, uint64_t out[8]);
/* THE RANGE STEP. For S row i, i in [0, sRows), the pairs are (sRowBase + i, r) for every indexed R row r whose value
 * lies in [lo[i], hi[i]], the brackets as the flags say. The comparison is hj_pairs_where_dev's: integers by width and
 * signedness, floats as IEEE-754 values with -0.0 == 0.0. A NULL or a NaN bound makes the row match nothing; such rows are
 * counted apart. An empty interval (lo > hi, or lo == hi with an open side) matches nothing. An open bound is a search
 * for the other end of the run of equal keys, never +-1 on the value: x < UINT64_MAX and x > INT64_MIN are right.
 *   HJ_RANGE_ALL    every pair
 *   HJ_RANGE_FIRST  per S row the one pair with the smallest R value in the range
 *   HJ_RANGE_LAST   ... with the largest; with lo NULL this is the backward as-of join without a key
 * Ties on the value go to the lowest R row, as in hj_pairs_asof_dev.
 * Output and marks are hj_probe_pairs_dev's and hj_pairs_where_dev's: the planes fill from 0 without holes; pairs at or
 * beyond `capacity` are counted and not written; the order is unspecified, the multiset exact; dOutS[j] carries the base.
 * Bit i of dSMarks is set when S row i has at least one pair, bit r of dRMarks when some S row of the call has r in its
 * range (FIRST / LAST: when r is the picked row), written or cut by the capacity alike. Bits only go 0 -> 1; nothing is
 * written behind word ceil(rows / 32) - 1; either plane may be NULL. The R marks cost O(sRows + rRows) whatever the pairs.
 * Capacity 0 with NULL outputs is the sizing or mark-only pass. THE TOTAL IS EXACT IN 64 BITS and can exceed 2^32.
 * dHead is read ON THE DEVICE: an index and its probes are enqueued back to back with no host wait in between. An index
 * whose key bytes are not the term's (dHead[3]) counts as empty. Asynchronous on the context's stream; `term` is read
 * before the call returns; needs no hj_reserve, no table and no state, and touches no other call's counters; the
 * workspace belongs to the context and grows with rRows and sRows (hj_range_layout_info).
 * HJ_ERR_INVALID: sRows or rRows above 2^32 - 2; capacity above 2^32 - 1; term NULL; lo and hi both NULL; a type that is
 * no hj_val_type or a width the type does not have; flags with other bits; pick above HJ_RANGE_LAST; a bound not aligned
 * to its width; a validity, output or mark pointer not 4-byte aligned; with rRows > 0: dPerm, dKeys or dHead NULL or
 * misaligned; with rows on both sides and capacity > 0: an output pointer NULL.
 * OUT OF SCOPE: strings; an equality key in the same step (that is where= behind a key join); conditions on two
 * different R columns in one step (an interval on R's side is the same call with the sides swapped); general
 * two-inequality joins; a sorted output order; more than one device. */
#define HJ_RANGE_LO_OPEN 0x1u     /* lo <  R.y  instead of  lo <= R.y */
#define HJ_RANGE_HI_OPEN 0x2u     /* R.y <  hi  instead of  R.y <= hi */
typedef enum { HJ_RANGE_ALL = 0, HJ_RANGE_FIRST = 1, HJ_RANGE_LAST = 2 } hj_range_pick;
typedef struct {
    const void     *lo, *hi;            /* sRows elements each; NULL: no bound on that side (not both)     */
    const uint32_t *loValid, *hiValid;  /* one bit per S row; NULL: no NULLs                               */
    uint32_t        width, type;        /* the indexed column's                                            */
    uint32_t        flags, pick;        /* HJ_RANGE_*_OPEN; an hj_range_pick                               */
} hj_range_term;                        /* 48 bytes */
int hj_range_pairs_dev(hj_ctx *ctx, const void *dKeys, const uint32_t *dPerm, const uint32_t *dHead, uint64_t rRows,
                       const hj_range_term *term, uint64_t sRows, uint32_t sRowBase,
                       uint32_t *dOutS, uint32_t *dOutR, uint64_t capacity, uint32_t *dSMarks, uint32_t *dRMarks);
/* Waits for the stream. About the last hj_range_pairs_dev: out[0] = pairs (64 bits, exact), out[1] = pairs written
 * (min(out[0], capacity)), out[2] = the device time of the call in microseconds (rounded), out[3] = S rows with a pair,
 * out[4] = S rows with a NULL or NaN bound, out[5] = rows indexed, out[6] = out[7] = 0. All 0 before the first call. */
int hj_range_pairs_info(hj_ctx *ctx, uint64_t out[8]);
/* The same step on host pointers: no context, no device (the order key is the kernels', around std::lower_bound and
 * std::upper_bound); the pairs in S-row order, ascending index positions inside a row. `info` (may be NULL) is filled as
 * hj_range_pairs_info fills it, info[2] = 0. HJ_ERR_INVALID as hj_range_pairs_dev, and for an index whose key bytes
 * (head[3]) are not the term's; a refused call writes nothing. */
int hj_range_pairs_host(const void *keys, const uint32_t *perm, const uint32_t *head, uint64_t rRows,
                        const hj_range_term *term, uint64_t sRows, uint32_t sRowBase,
                        uint32_t *outS, uint32_t *outR, uint64_t capacity, uint32_t *sMarks, uint32_t *rMarks, uint64_t info[8]);
/* PRJ (parallel_radix_join.c:808-1122): radix-partitions dR and dS and joins
 * each partition pair in LDS. Asynchronous. dS may be NULL (fork behaviour:
 * R-side only, checksum only). */
int hj_prj_join_dev(hj_ctx *ctx, const uint64_t *dR, uint64_t rSize,
                    const uint64_t *dS, uint64_t sSize);
/* PRJ with a resident build side. Sizing: hj_reserve(params{algo = PRJ or AUTO}, rSize, sliceSize); radixBits is fixed
 * at the build and used by every probe.
 * Partition dR once (the passes of hj_prj_join_dev's R side) and keep the partitions resident in ctx.
 * dR may be freed or overwritten after the call. Resets the counters; prjChecksum = R's PRO checksum. Async. */
int hj_prj_build_dev(hj_ctx *ctx, const uint64_t *dR, uint64_t rSize);
/* Radix-partition dS[0..sSize) with the resident R's radix bits and join it against R's partitions. Adds to
 * totalMatches and sSize, like hj_probe_dev. Any sSize up to the one given to hj_reserve. Async.
 * HJ_ERR_STATE without a resident R (no hj_prj_build_dev yet, or hj_prj_join_dev / hj_build_dev / hj_join_dev / an
 * hj_reserve that reallocated since) or for an sSize above the reserved one. sSize 0 is a no-op. */
int hj_prj_probe_dev(hj_ctx *ctx, const uint64_t *dS, uint64_t sSize);
/* hj_prj_probe_dev with its result kept, against an R built on a context reserved with HJ_FLAG_KEEP_ROW_IDS: partitions
 * dS[0..sSize) with its row ids and writes one pair  dOutS[k] = sIdxBase + (position in dS),  dOutR[k] = position of the
 * matching tuple in the dR given to hj_prj_build_dev  per match, under the output contract of hj_probe_pairs_dev: the
 * planes fill from 0 without holes on every call, pairs beyond `capacity` are counted but not written, the order is
 * unspecified, the multiset is exact. The join is hj_prj_probe_dev's: the complete equi-join on the key word (the low 32
 * bits of a tuple; upper bits are ignored and key 0 is an ordinary key), duplicate keys on both sides included. Adds to
 * totalMatches and sSize exactly as hj_prj_probe_dev does; hj_pairs_info reports the call. Asynchronous.
 * HJ_ERR_STATE: no resident R; a resident R built without the flag; sSize above the reserved one.
 * HJ_ERR_INVALID: an output pointer NULL with capacity > 0, or sIdxBase + sSize > 2^32 - 1. sSize 0 is a no-op. */
int hj_prj_probe_pairs_dev(hj_ctx *ctx, const uint64_t *dS, uint64_t sSize, uint64_t sIdxBase,
                           uint32_t *dOutS, uint32_t *dOutR, uint64_t capacity);
/* hj_prj_probe_pairs_dev for any hj_join_kind (hj_prj_probe_pairs_dev is its HJ_JOIN_INNER case), as hj_probe_join_dev is
 * for the table probes: the same rows per S tuple, dOutR ignored and never written for HJ_JOIN_SEMI / ANTI, totalMatches
 * and sSize growing as under hj_prj_probe_dev whatever the kind, HJ_ERR_INVALID also for kind > 3. Under HJ_JOIN_LEFT and
 * HJ_JOIN_ANTI the S tuples of a partition that holds no R tuple are rows as well. Asynchronous. */
int hj_prj_probe_join_dev(hj_ctx *ctx, uint32_t kind, const uint64_t *dS, uint64_t sSize, uint64_t sIdxBase,
                          uint32_t *dOutS, uint32_t *dOutR, uint64_t capacity);
/* ---- aggregating joins: COUNT / SUM / MIN / MAX of S values per R row, without the pairs ----
 * A join that feeds GROUP BY <R row> needs no pair: the resident radix join has R's partition in an LDS table while the S
 * tuples of that partition stream past it, so the per-R-row accumulators are updated in LDS and leave for memory once per
 * work item. hj_prj_agg_begin names the columns and allocates the accumulators, hj_prj_probe_agg_dev adds one S slice to
 * them (R is built once, S arrives in slices), hj_prj_agg_rows_dev writes them out by R row, at any time.
 * Integer columns only: every accumulator is 64 bits wide, a 4-byte value is sign-extended (HJ_AGG_SIGNED) or zero-extended
 * to it, SUM wraps modulo 2^64, and every result is independent of the order of the adds -- exact, like everything else
 * this library returns. Floating-point columns are out of scope for that reason: an atomic float sum depends on the order
 * its terms arrive in, and no tolerance is offered instead. Values of 1 or 2 bytes are widened by the caller. */
#define HJ_AGG_MAX_COLS 4
typedef enum { HJ_AGG_COUNT = 0, HJ_AGG_SUM = 1, HJ_AGG_MIN = 2, HJ_AGG_MAX = 3 } hj_agg_op;
#define HJ_AGG_SIGNED 0x1u   /* hj_agg_spec.flags / hj_agg_col.flags: the values are signed (extension of 4-byte values; MIN and MAX) */
typedef struct {
    uint32_t op;         /* hj_agg_op                                                        */
    uint32_t width;      /* bytes of a source element: 4 or 8; 0 for HJ_AGG_COUNT            */
    uint32_t flags;      /* HJ_AGG_SIGNED or 0                                               */
    uint32_t reserved;   /* 0                                                                */
} hj_agg_spec;           /* 16 bytes */
typedef struct {
    const void     *src;      /* device: one element of the spec's width per S tuple of the slice, indexed by the position in
                                 dS; aligned to the width. HJ_AGG_COUNT: ignored, may be NULL                               */
    const uint32_t *srcValid; /* NULL: no NULLs. Else the plane hj_gather_dev writes: bit i & 31 of word i >> 5, 1 = valid,
                                 ceil(sSize / 32) words                                                                     */
} hj_agg_src;                 /* 16 bytes */
/* Starts an aggregation of nCols (1 .. HJ_AGG_MAX_COLS) columns over the resident R, which must have been built on a
 * context reserved with HJ_FLAG_KEEP_ROW_IDS. Allocates the context-owned accumulators (a buffer that only grows): one
 * 64-bit match-count plane and nCols 64-bit accumulator planes of rSize entries each, indexed by RESIDENT POSITION -- the
 * tuple's place in the partitioned R -- not by R row, so that the entries a work item updates are one contiguous range.
 * Initialises them on the stream: COUNT and SUM 0; MIN INT64_MAX with HJ_AGG_SIGNED, else UINT64_MAX; MAX INT64_MIN with
 * HJ_AGG_SIGNED, else 0. A second begin starts over. hj_prj_build_dev, hj_prj_join_dev, hj_build_dev (every call that
 * starts a new operation) and an hj_reserve that reallocates end the aggregation. `specs` is host memory, read before the
 * call returns. Asynchronous.
 * HJ_ERR_STATE: no resident R, or one built without HJ_FLAG_KEEP_ROW_IDS. HJ_ERR_INVALID: nCols 0 or above
 * HJ_AGG_MAX_COLS; specs NULL; an op above HJ_AGG_MAX; a width other than 4 or 8 (HJ_AGG_COUNT: other than 0); a flag bit
 * other than HJ_AGG_SIGNED; reserved != 0. */
int hj_prj_agg_begin(hj_ctx *ctx, const hj_agg_spec *specs, uint32_t nCols);
/* hj_prj_probe_dev with its matches reduced: the complete equi-join of dS[0..sSize) with the resident R on the key word,
 * duplicate keys on both sides included, key 0 an ordinary key. For every match (s, r) and column c:
 * acc[c][r] op= value(src[c][s]), and the match count of r grows by 1. An S element whose srcValid bit is 0 contributes
 * nothing to that column and its bytes are never read; the bytes of an S element without a match are never read either.
 * HJ_AGG_COUNT with a srcValid counts the valid elements (COUNT(col)), without one the matches (COUNT(*)). The
 * accumulators persist across calls. totalMatches and sSize grow exactly as under hj_prj_probe_dev; hj_pairs_info, the R
 * marks and every other *_info but hj_prj_resident_info (whose work items are those of the last probe of any kind) are
 * untouched. `srcs` is host memory, read before the call returns. Asynchronous. sSize 0 is a no-op.
 * Cost: the slice's row-id passes as under hj_prj_probe_pairs_dev; one scattered read per matched valid element and
 * column; per work item one 64-bit global atomic per R tuple that was hit and column, at contiguous addresses. An R
 * partition larger than one LDS build (hj_prj_agg_layout_info: fewer tuples the more columns) is probed once per build.
 * HJ_ERR_STATE: no resident R; no hj_prj_agg_begin since the last build; sSize above the reserved one. HJ_ERR_INVALID:
 * nCols differs from the begin's; srcs NULL; a src that is NULL (but for HJ_AGG_COUNT) or not aligned to its width; a
 * srcValid that is not 4-byte aligned. */
int hj_prj_probe_agg_dev(hj_ctx *ctx, const uint64_t *dS, uint64_t sSize, const hj_agg_src *srcs, uint32_t nCols);
/* Resident order -> R rows: for every resident position pos, with row = the tuple's position in the dR given to
 * hj_prj_build_dev, dOut[c][row] = acc[c][pos] for the begin's nCols columns and, unless NULL, dOutCount[row] = the match
 * count. dOut: host array of nCols device pointers to planes of rSize x 8 bytes. Plain stores; every R row is written
 * exactly once, nothing behind rSize entries. A row that never matched holds count 0 and the identities of the begin.
 * Changes no accumulator: a later slice and a later call keep working. Asynchronous.
 * HJ_ERR_STATE as hj_prj_probe_agg_dev. HJ_ERR_INVALID: dOut NULL; a plane that is NULL or not 8-byte aligned. */
int hj_prj_agg_rows_dev(hj_ctx *ctx, void *const *dOut, uint64_t *dOutCount);
/* Waits for the stream. out[0] = matches of the last hj_prj_probe_agg_dev since the begin, out[1] = its device time in
 * microseconds (rounded), out[2] = nCols, out[3] = probes since the begin, out[4] = R tuples the planes hold, out[5..7] = 0.
 * All 0 without an aggregation. */
int hj_prj_agg_info(hj_ctx *ctx, uint64_t out[8]);
/* Host-only arithmetic, no context: the LDS layout of the aggregating join for nCols columns. out[0] = table slots, out[1] =
 * R tuples per LDS build (at most 0.75 x slots), out[2] = S elements per round of a workgroup, out[3] = S tuples per work
 * item at most. Per build the LDS holds out[1] x (4 + 8 nCols) bytes of counts and accumulators and out[0] x 6 bytes of
 * table (a 4-byte key remainder and a 2-byte position per slot), within 160 KiB. HJ_ERR_INVALID: nCols 0 or above
 * HJ_AGG_MAX_COLS; out NULL. */
int hj_prj_agg_layout_info(uint32_t nCols, uint64_t out[4]);
/* The same reduction over a pair list, for the joins whose pairs must exist first: hj_pairs_verify_dev's kept pairs
 * (joins on real key columns) and the planes of the table probes. */
typedef struct {
    const void     *src;      /* device: vRows elements of `width` bytes, aligned to it. HJ_AGG_COUNT: ignored, may be NULL */
    const uint32_t *srcValid; /* NULL: no NULLs. Else one bit per element of src, ceil(vRows / 32) words                    */
    void           *acc;      /* device: gRows accumulators of 8 bytes, owned AND INITIALISED by the caller                 */
    uint32_t        op;       /* hj_agg_op                                                                                   */
    uint32_t        width;    /* 4 or 8; 0 for HJ_AGG_COUNT                                                                  */
    uint32_t        flags;    /* HJ_AGG_SIGNED or 0                                                                          */
    uint32_t        reserved; /* 0                                                                                           */
} hj_agg_col;                 /* 40 bytes */
/* For pair k in [0, nPairs), with g = dMapG[k] - gBase and v = dMapV[k] - vBase: acc[c][g] op= value(src[c][v]) for every
 * column c whose element v is valid, and dCount[g] += 1 (dCount may be NULL; gRows x 8 bytes, the caller's, initialised by
 * the caller). Either map may be the S plane or the R plane of a pairs call: grouping by S row while aggregating R values
 * is the same call with the maps swapped. A pair whose raw entry is HJ_NO_ROW on either side, or with g >= gRows or v >=
 * vRows, is never dereferenced: it is skipped and counted apart (hj_pairs_agg_info out[3]), as in hj_pairs_verify_dev.
 * dMapV may be NULL when no column reads a value or a validity (HJ_AGG_COUNT without srcValid, or nCols 0 with a dCount).
 * Values, ops and exactness as for hj_prj_probe_agg_dev. `cols` is host memory, read before the call returns. Needs no
 * table, no hj_reserve and no state; touches no counter of hj_result and no other *_info. Asynchronous.
 * Cost, stated plainly: neighbouring lanes of a wavefront whose pairs name the same g combine their values first (a
 * segmented reduction over 64 pairs) and the last lane of such a run issues the atomic, so the call costs ONE MEMORY-SIDE
 * ATOMIC REQUEST PER RUN AND COLUMN, each its own scattered 64-byte request. The radix join emits a hot R row's pairs in
 * runs; a list without runs pays one request per pair and column, the worst shape this chip has for global atomics.
 * Where the join is on the key word itself, hj_prj_probe_agg_dev avoids both the pairs and these requests.
 * HJ_ERR_INVALID (nothing is enqueued; also for a NULL context): nCols above HJ_AGG_MAX_COLS; cols NULL with nCols > 0;
 * nCols 0 and dCount NULL; the op, width, flags and reserved errors of hj_prj_agg_begin; an acc that is NULL or not 8-byte
 * aligned; with vRows > 0 a src that is NULL (but for HJ_AGG_COUNT) or not aligned to its width; a srcValid that is not
 * 4-byte aligned; dMapG NULL with nPairs > 0; dMapV NULL with nPairs > 0 and a column that has a width or a srcValid;
 * dCount not 8-byte aligned; nPairs, gRows or vRows above 2^32 - 1. nPairs 0 is a call that applied nothing. */
int hj_pairs_agg_dev(hj_ctx *ctx, const uint32_t *dMapG, const uint32_t *dMapV, uint64_t nPairs, uint32_t gBase, uint64_t gRows,
                     uint32_t vBase, uint64_t vRows, const hj_agg_col *cols, uint32_t nCols, uint64_t *dCount);
/* Waits for the stream. About the last hj_pairs_agg_dev: out[0] = its nPairs, out[1] = pairs applied, out[2] = its device
 * time in microseconds (rounded), out[3] = pairs skipped as HJ_NO_ROW or out of range. All 0 before the first call. */
int hj_pairs_agg_info(hj_ctx *ctx, uint64_t out[4]);
/* Host-visible facts about the resident build and the last probe (waits for the stream), out[8]:
 * [0] R's path (0 exact, 1 histogram-free, 2 fell back), [1] last probe's S path (same coding),
 * [2] join work items of the last probe (after an HJ_JOIN_LEFT / HJ_JOIN_ANTI call they include the items of partitions
 * with S tuples and no R tuple; unchanged for every other call), [3] partitions whose S side was split over > 1 item,
 * [4] largest S partition of the last probe, [5] resident bytes held for R, [6..7] reserved (0). */
int hj_prj_resident_info(hj_ctx *ctx, uint64_t out[8]);
/* Build + probe of dR x dS by whatever hj_reserve was given: HJ_ALGO_NOCC/ATOMIC/HTM = hj_build_dev(idxBase 0) then
 * hj_probe_dev; HJ_ALGO_PRJ = hj_prj_join_dev; HJ_ALGO_AUTO = one locality pre-round over dR (k_sample_locality, one
 * small device->host read-back) and then one of the two. Asynchronous apart from that read-back and, under HJ_ALGO_HTM,
 * the read-back of hj_build_dev. */
int hj_join_dev(hj_ctx *ctx, const uint64_t *dR, uint64_t rSize,
                const uint64_t *dS, uint64_t sSize);
/* The untimed reductions of NoCCHashBuild.hpp:85-113 (table sums). Async. */
int hj_checksums_dev(hj_ctx *ctx);
/* Waits for the stream and returns counters + timings of the calls above. */
int hj_fetch_result(hj_ctx *ctx, hj_result *out);
/* Copies the open-addressing table to host in the reference's format
 * (tableSize slots, value = key, 0 = empty). */
int hj_export_table(hj_ctx *ctx, uint64_t *host_table, uint64_t tableSize);
/* HJ_ALGO_HTM: copies the bucket table to host as the reference's `struct Bucket
 * {uint64_t tuples[3]; uint32_t count; uint32_t nextIndex;}` (HTMHashBuild.hpp:41-45,
 * 32 bytes): host_buckets[numBuckets] and host_overflows[0 .. *nOverflow] (index 0
 * unused, nextIndex is 1-based, 0 = end of chain; overflowCap >= *nOverflow + 1
 * entries; pass NULL / 0 to learn *nOverflow first). A chain's head is its newest
 * overflow bucket, as in the reference; the physical overflow indices are this
 * library's (a bucket's overflow buckets are neighbours), not the reference's
 * creation order. `count` of a bucket with a chain, and of every overflow bucket,
 * is the count word the build stored next to the link; of a bucket without a
 * chain, its tuple slots in use. */
int hj_export_buckets(hj_ctx *ctx, void *host_buckets, uint64_t numBuckets,
                      void *host_overflows, uint64_t overflowCap, uint64_t *nOverflow);

/* ---- multi-GPU sharding helpers (new design) ---------------- */
/* dest(key) = ((key - b) >> d) & (nShards-1), nShards a power of two <= 64, with d = mode & 0xFF the bit position
 * of the radix digit and b = 1 if mode has HJ_SHARD_ONE_BASED set, else 0: HASH_BIT_MODULO(key, MASK, R) of
 * parallel_radix_join.c:59 with R = d. d = 0 takes the low key bits: balanced for any key distribution, but on a
 * relation whose pieces are contiguous key ranges (the reference's near-sorted inputs, held piecewise) all but
 * 1/nShards of the tuples change GPU. d = (bits of the key domain) - log2(nShards) takes the HIGH bits, i.e. a
 * range split: such pieces mostly stay where they are and only what does not fit a rank's range moves
 * (HJ_SHARD_ONE_BASED makes the ranges of DataGen's keys 1..N come out even). Both relations of a join must use
 * the same mode. */
#define HJ_SHARD_ONE_BASED 0x100u
/* Counts tuples per destination into dCounts[nShards] (device, uint64) and keeps
 * the per-chunk write cursors for the scatter of the same input. Async. */
int hj_shard_histogram_dev(hj_ctx *ctx, const uint64_t *dIn, uint64_t n,
                           uint32_t nShards, uint32_t mode, uint64_t *dCounts);
/* Scatter of the n tuples of dIn, grouped by destination, into dOutKeys as bare
 * 32-bit keys (a DataGen tuple is its key, DataGen.hpp:29: the exchange then
 * moves 4 bytes per tuple instead of 8). Must follow hj_shard_histogram_dev on
 * the same (dIn, n). The input order is preserved inside every destination
 * (scan-based cursors, no atomics across workgroups). That is what carries the
 * reference's insertion order through the exchange: when rank g holds the g-th
 * contiguous piece of the relation and the receiver lays the pieces out in rank
 * order, position in the received buffer IS global input order, so no index
 * has to travel. Async. */
int hj_shard_scatter_dev(hj_ctx *ctx, const uint64_t *dIn, uint64_t n,
                         uint32_t nShards, uint32_t mode,
                         const uint64_t *dCounts, uint32_t *dOutKeys);
/* hj_build_dev / hj_probe_dev for bare keys (the received side of the exchange):
 * tuple i of dKeys has index i; table of tableSize slots (a power of two,
 * reserved via hj_reserve(rSize = tableSize/2)); home slot of a key =
 * (key >> homeShift) & (tableSize-1) with homeShift = log2(nShards): inside a
 * shard the low key bits are the same for every key and would leave all but
 * every nShards-th slot unused. */
int hj_build_keys_dev(hj_ctx *ctx, const uint32_t *dKeys, uint64_t n,
                      uint32_t homeShift, uint64_t tableSize);
int hj_probe_keys_dev(hj_ctx *ctx, const uint32_t *dKeys, uint64_t n);
/* Optimistic joining in place: under a range split the pieces a rank holds are often already its shards. While a
 * check is set (nShards > 0), every later build and probe on this context also counts, at no extra pass over the
 * data, the tuples whose destination under (nShards, mode) is NOT shardId -> hj_result.foreignTuples. A caller
 * joins its pieces in place with hj_build_dev / hj_probe_dev and takes the result if the count is 0 on every
 * rank, else redoes the step with split + exchange. nShards = 0 switches the check off. */
int hj_set_shard_check(hj_ctx *ctx, uint32_t nShards, uint32_t mode, uint32_t shardId);

/* Host-only arithmetic (no device needed): how hj_reserve sizes the PRJ histogram workspace for (rSize, sSize,
 * radixBits; 0 = auto). out[0] = workspace bytes, out[1] = histogram entries planned, out[2] / out[3] = entries the
 * passes over R / over S write. Each relation is chunked by its own size (mc's per-thread slices,
 * parallel_radix_join.c:586-617, become per-chunk histograms), so out[1] >= max(out[2], out[3]) must hold. */
int hj_prj_workspace_info(uint64_t rSize, uint64_t sSize, uint32_t radixBits, uint64_t out[4]);
/* Host-only arithmetic: the fragment geometry of the histogram-free passes for (rSize, sSize, radixBits, prjMode).
 * out[0] = 1 when those passes would be enqueued (both relations qualify), else 0 (exact passes only);
 * out[1..5] = R's chunks of pass 1, slots per pass-1 fragment, tuples per pass-1 chunk, chunks of pass 2 per pass-1
 * partition (= fragments per final partition), slots per pass-2 fragment; out[6..10] = the same for S; out[11], out[12] =
 * radix bits of pass 1 and pass 2. A relation with out[1] (out[6]) == 0 does not qualify. */
int hj_prj_fragment_info(uint64_t rSize, uint64_t sSize, uint32_t radixBits, uint32_t prjMode, uint64_t out[13]);

/* Planning facts of the ring builds (buildVariant 3 and 4), the counterpart of hj_prj_fragment_info: how a relation of n
 * tuples is cut into chunks, one per wavefront, and the constants the zones around every chunk seam are made of, reported
 * from the kernel's own constants. ctx == NULL: host-only arithmetic for a device of `computeUnits` compute units (no
 * device needed); otherwise the compute units of the context's device are used and computeUnits is ignored.
 * out[0] = chunk length in tuples (the nominal seam of chunk c is c * out[0]), out[1] = chunks, out[2] = slice length (a
 * chunk's share of the deferred queue), out[3] = tuples per tile, out[4] = slots per granule, out[5] = granules per ring,
 * out[6] = look (positions from the nominal seam among which the pre-pass places the real one), out[7] = overlap (positions
 * past its end a wavefront reads = head zone of the next), out[8] = shadow (positions before its seam the compact build
 * reads), out[9] = tail (positions before the nominal seam whose next-range tuples the next wavefront inserts), out[10] =
 * walks across one seam the compact build lists at most, out[11] = the largest probeLength the compact build takes,
 * out[12] = compute units used, out[13..15] = 0. HJ_ERR_INVALID: out NULL, n > 2^32 - 1, no context and computeUnits 0. */
int hj_wave_layout_info(const hj_ctx *ctx, uint32_t computeUnits, uint64_t n, uint64_t out[16]);
/* What the ring pre-pass of the last build decided (waits for the stream): chunk c holds the positions
 * [starts[c], starts[c + 1]) of the input and owns the granules [bounds[c], bounds[c + 1]) of the table; both arrays take
 * *nChunks + 1 entries (starts[*nChunks] = n, bounds[*nChunks] = granules of the table). pcounts (may be NULL) takes
 * *nChunks entries: the walks chunk c let in across its lower seam -- defined only when the compact build held
 * (hj_result.buildVariant == 4). capacity = entries each array has room for; *nChunks is set whenever the call gets as far
 * as knowing it. HJ_ERR_STATE: the last build on this context did not run the ring pre-pass (no build, buildVariant 1 or
 * 2, or buildVariant 0 picking one of them). HJ_ERR_INVALID: capacity < *nChunks + 1, or a NULL argument. */
int hj_wave_seams(hj_ctx *ctx, uint32_t *starts, uint32_t *bounds, uint32_t *pcounts, uint64_t capacity,
                  uint64_t *nChunks);
/* The planar retire of the classic ring build (waits for the stream). On a context reserved WITHOUT HJ_FLAG_KEEP_ROW_IDS,
 * buildVariant 3 leaves the table as 4-byte keys (what the probe reads) with the input indices in a plane of their own,
 * which only its deferred phase reads; an input it cannot take is redone by the packed classic build, decided on the
 * device, and hj_result.buildVariant says 3 either way. out[0] = 1 if the last build's table is the planar one, out[1] =
 * why the planar build handed over, 0 = it did not or was not tried (bit 0: a chunk's log of slots the deferred phase
 * changed did not fit -- an input that defers nearly everything; bit 1: key 0xFFFFFFFF, the 4-byte empty pattern),
 * out[2] = table format (0 = 8-byte slots, 1 = 4-byte keys, 2 = slot codes: hj_slot_codes_info; out[0] is 0 then and out[1]
 * may carry that road's cause 4), out[3] = 0. hj_result.compactFallback does not speak of this.
 * HJ_ERR_STATE: no open-addressing table. */
int hj_wave_planar_info(hj_ctx *ctx, uint64_t out[4]);
/* Slot codes (table format 2: one byte per slot instead of a 4-byte key; see HJ_FLAG_SLOT_CODES). Slot s holds the code
 * (hi << dbits) | d of the key with home slot s - d and bits above the table size hi; 0xFF = empty; codes use 7 bits.
 * Host-only arithmetic for a table of tableSize slots (a power of two up to 2^32) at probeLength -- ctx may be NULL:
 * out[0] = 1 if a build of this table takes the format by itself (every 32-bit key has a code), out[1] = dbits =
 * ceil(log2(probeLength)), out[2] = hiCap = 2^(7 - dbits) (0: no code at this probeLength), out[3] = log2(tableSize).
 * With a context whose last build made a table of that size (tableSize 0: that table, at the context's probeLength; waits
 * for the stream): out[4] = 1 if that table is in slot codes, out[5] = why the road handed over to the 8-byte build, 0 =
 * it did not or was not taken (the bits of hj_wave_planar_info's out[1], and bit 2, value 4: a key whose high bits no code
 * holds), out[6] = road the host chose (0 none, 1 by the size rule, 2 forced by the flag), out[7] = table format. Otherwise
 * out[4..7] = 0. HJ_ERR_INVALID: out NULL, tableSize no power of two or above 2^32, probeLength 0. HJ_ERR_STATE: tableSize 0
 * without an open-addressing table. */
int hj_slot_codes_info(hj_ctx *ctx, uint64_t tableSize, uint32_t probeLength, uint64_t out[8]);
/* Ring words (host-only arithmetic; for tests): what a slot of a wavefront's LDS ring holds while a build on the slot-code
 * road runs, word = (rel << 7) | code, rel = the tuple's offset from the first position its wavefront reads; all ones =
 * empty. For the tuple with that rel and key in a table of tableSize slots at probeLength, after `steps` steps from its home
 * slot: out[0] = the word, out[1] = the key read back out of (slot, word), out[2] = tries the tuple has left, this slot
 * included (probeLength - steps), out[3] = rel and out[4] = code read back out of the word (the code is the one the slot
 * ends with: hj_slot_codes_info), out[5] = the layout rule's bound (a rel must be below it), out[6] = the empty pattern,
 * out[7] = the slot. HJ_ERR_INVALID: what the road never makes -- out NULL, a bad table size or probeLength (as
 * hj_slot_codes_info), no code at this probeLength, a key without a code, rel at or above the bound, steps >= probeLength
 * (out[5] and out[6] are set whenever out, tableSize and probeLength are good). */
int hj_ring_word_layout_info(uint64_t tableSize, uint32_t probeLength, uint32_t rel, uint32_t key, uint32_t steps, uint64_t out[8]);
/* The table of the last hj_build_dev / hj_build_keys_dev as its readers see it (waits for the stream; for tests). An LDS
 * build (buildVariant 2, 3, 4, also under HJ_ALGO_HTM) writes only the slots some tuple can reach: out[0], out[1] = the
 * valid slot range [validLo, validHiEx) -- a home slot outside it matches nothing, the slots [validLo, validHiEx + 512)
 * hold defined contents, and everything else in the buffer is whatever an earlier build on this context left there, in
 * that build's format. out[2] = table format (0 = 8-byte slots, 1 = 4-byte keys, 2 = one code byte per slot; HJ_ALGO_HTM:
 * always 0), out[3] = slots of
 * the live table (HJ_ALGO_HTM: 4 per bucket), out[4] = device address of the table buffer, out[5] = its size in bytes
 * (hj_reserve only grows it). With out[4], hj_copy_d2h reads the raw table words. Changes nothing.
 * HJ_ERR_STATE: no table (no build yet, or the last operation was a radix join). */
int hj_table_debug(hj_ctx *ctx, uint64_t out[6]);
/* The chain phase of the bucketised table behind the ring build (HJ_ALGO_HTM, buildVariant 3): every overflow chain is
 * built in LDS, one workgroup per PART of a chunk's slice of the conflict list; an input that does not fit hands over to
 * the generic chain kernels (hj_result.compactFallback bit 8). hj_htm_chain_layout_info is the counterpart of
 * hj_wave_layout_info (ctx == NULL: host-only arithmetic for computeUnits compute units; else the context's device, and
 * computeUnits is ignored), for 0 < n < 2^32 tuples: out[0] = slices (= chunks), out[1] = sliceLen (places per slice),
 * out[2] = parts per slice, out[3] = kChainCountCap (buckets a slice's conflicts may span), out[4] = kChainCap (buckets
 * per part; tuple slots of a part's overflow image, i.e. kChainCap / 3 overflow buckets), out[5] = kChainMaxParts,
 * out[6] = positions of a slice per part (parts = ceil(sliceLen / out[6]), at most out[5]), out[7] = 1 when a build of
 * n tuples that asks for buildVariant 3 tries the LDS phase, else 0: the ring build must take the table at all (at least
 * one ring of slots, hj_wave_layout_info's ringGranules x granuleSlots; below that buildVariant 3 becomes 2 or 1 and the
 * phase is not tried), and the phase's scratch must fit two per-bucket arrays (slices x parts + 1 and
 * 2 x slices x (1 + parts) words, each at most the number of buckets). Every table the rings take has room for the
 * scratch, so the first condition alone decides. */
int hj_htm_chain_layout_info(const hj_ctx *ctx, uint32_t computeUnits, uint64_t n, uint64_t out[8]);
/* What the chain phase of the last hj_build_dev under HJ_ALGO_HTM did (waits for the stream; changes nothing).
 * out[0] = 0: the LDS phase was not tried (another build variant, or a relation too small for it), 1: it held, 2: it
 * handed over to the generic chain kernels -- exactly when hj_result.compactFallback has bit 8. out[1] = why it handed
 * over, else 0: bit 0 = a slice took more conflicts than sliceLen, bit 1 = a conflict lay outside its slice's bucket
 * range, bit 2 = a slice's conflicts span more than kChainCountCap buckets, bit 3 = a part covers more than kChainCap
 * buckets, bit 4 = a part needs more than kChainCap / 3 overflow buckets. Workgroups that start after the first cause was
 * raised return at once: the mask is a non-empty subset of the causes the input holds. out[2] = overflow buckets the
 * parts asked for when the phase held (= hj_result.htmOverflowBuckets), else 0. out[3] = 0.
 * HJ_ERR_STATE: no htm table. */
int hj_htm_chain_info(hj_ctx *ctx, uint64_t out[4]);
/* Planning facts of the workgroup-window build (buildVariant 2, also under HJ_ALGO_HTM), the counterpart of
 * hj_wave_layout_info, for 0 < n < 2^32 tuples, reported from the kernel's own constants. ctx == NULL: host-only arithmetic
 * for a device of `computeUnits` compute units; otherwise the context's device, and computeUnits is ignored.
 * out[0] = chunk length in tuples (chunk c = positions [c * out[0], (c + 1) * out[0]) of the input, one workgroup each),
 * out[1] = chunks, out[2] = tuples per build tile, out[3] = slots per table block (the unit of ownership), out[4] = blocks
 * per LDS window, out[5] = blocks the window keeps behind a tile's lowest home block, out[6] = the seam-tile divisor (in a
 * chunk's first and last tile a block is claimed only if it holds at least 1/out[6] of what the tile's fullest block
 * holds), out[7] = slots of the smallest table the build takes (one window; below it buildVariant 2 becomes 1), out[8] =
 * workgroups per chunk's slice of the deferred queue in the deferred phase, out[9] = the largest probeLength for which
 * the build's valid slot range is right (not enforced: hj_reserve and the builds take any probeLength) = out[3] + 1: a
 * walk, the deferred phase's included, must end at most one block past the block it starts in, because the valid slot
 * range is "the blocks claimed or deferred into, plus one" and a walk that straddles a block end asks for one next block,
 * out[10] = compute units used, out[11..15] = 0.
 * HJ_ERR_INVALID: out NULL, n == 0 or n > 2^32 - 1, no context and computeUnits 0. */
int hj_own_layout_info(const hj_ctx *ctx, uint32_t computeUnits, uint64_t n, uint64_t out[16]);
/* What the last workgroup-window build left (waits for the stream; changes nothing; for tests): owner[b] = 0 when nobody
 * claimed table block b, else (chunk + 1) of the workgroup that did, for the out[0] blocks of the table; deferCounts[c] =
 * tuples chunk c's workgroup handed to the deferred phase, for the out[1] chunks; out[2] = their sum (=
 * hj_result.buildDeferred), out[3] = 0. ownerCapacity / countsCapacity = entries the arrays have room for; out[0] and
 * out[1] are set whenever the call gets as far as knowing them. HJ_ERR_STATE: the last build on this context did not run
 * the window build (no build, a radix join, buildVariant 1, 3, 4, or buildVariant 0 picking one of them), or hj_reserve
 * has replaced the owner table since -- the only call between two builds that touches what is reported here.
 * HJ_ERR_INVALID: a NULL argument, or a capacity below out[0] / out[1]. */
int hj_own_info(hj_ctx *ctx, uint32_t *owner, uint64_t ownerCapacity, uint32_t *deferCounts, uint64_t countsCapacity,
                uint64_t out[4]);

/* ---- device memory for hosts without a HIP runtime of their own ----------- */
int hj_dev_alloc(hj_ctx *ctx, uint64_t bytes, void **dptr);
int hj_dev_free(hj_ctx *ctx, void *dptr);
int hj_copy_h2d(hj_ctx *ctx, void *dst_dev, const void *src_host, uint64_t bytes);
int hj_copy_d2h(hj_ctx *ctx, void *dst_host, const void *src_dev, uint64_t bytes);

/* ---- input layer ---------------------------------------------------------- */
/* generate_data(dist, n, distinct, window) of include/DataGen.hpp:26-122 into a
 * caller-owned host buffer: same glibc rand() stream after srand(0), same
 * distributions ("uniform","random","sorted","shuffle","local_shuffle").
 * "zipf" (an empty stub in the reference, :72-77) draws keys over [1,distinct]
 * with the LUT method of mc/src/genzipf.c:60-158, theta = zipfTheta.
 * Returns HJ_ERR_INVALID for an unknown distribution (the reference exits). */
int hj_generate_data(const char *dist, uint64_t n, uint64_t distinct, int window,
                     double zipfTheta, uint64_t *out);

/* Streaming Zipf generator for probe sides too large to generate and copy in one piece (BASELINE config 5:
 * |S| = 4 * 10^9 draws over 2^28 keys). hj_zipf_open builds gen_zipf's alphabet permutation and cumulative table
 * (mc/src/genzipf.c:28-93) after srand(seed) and keeps them on the device; every hj_zipf_next_dev(n) continues the SAME
 * rand() stream where the last call stopped and writes the next n draws to dOut as 8-byte tuples: the host produces
 * only the serial rand() values, the binary search of genzipf.c:118-151 runs on the GPU. The concatenation of the
 * slices equals hj_generate_relation("zipf", total, alphabet, 0, theta, seed, ...) element for element (seed 0:
 * hj_generate_data("zipf")). The work is enqueued on the context's stream, but the call is not asynchronous: the host draws
 * the rand() values itself into one of two pinned buffers and, before it reuses one, waits for the event behind the call that
 * used it last -- so a third call in a row blocks until the first has run on the device. hj_zipf_open and hj_zipf_close wait
 * for the stream. */
int hj_zipf_open(hj_ctx *ctx, uint64_t alphabetSize, double theta, unsigned seed);
int hj_zipf_next_dev(hj_ctx *ctx, uint64_t n, uint64_t *dOut);
int hj_zipf_close(hj_ctx *ctx);

/* The relation generators of the reference's mc/ comparison code (mc/src/generator.c), serial forms, same glibc
 * rand() stream after srand(seed) (seed_generator, :56-61; mc/src/main.c:337-338 seeds R with 12345, S with 54321),
 * written as 8-byte tuples {key, payload = 0}:
 *   "pk"          create_relation_pk (:241-261): keys 1..n, Knuth shuffle (:83-93)
 *   "pk_lshuffle" create_relation_pk_lshuffle (:263-284): keys 1..n, lshuffle(window) (:96-110)
 *   "fk"          create_relation_fk (:408-445): foreign keys into 1..maxid: n / maxid shuffled copies of 1..maxid,
 *                 then a shuffled 1..(n % maxid)  -- workload A/B of mc/src/main.c:171-215
 *   "nonunique"   create_relation_nonunique (:494-509): key = RAND_RANGE(maxid), 0 .. maxid-1. Key 0 is the table
 *                 paths' empty marker (HJ_ERR_KEY_RANGE there); HJ_ALGO_PRJ takes it
 *   "zipf"        create_relation_zipf (:521-538): gen_zipf(n, maxid, theta) of mc/src/genzipf.c
 * Returns HJ_ERR_INVALID for an unknown kind or arguments the reference would divide by zero on. */
int hj_generate_relation(const char *kind, uint64_t n, uint64_t maxid, int window, double theta,
                         unsigned seed, uint64_t *out);

#ifdef __cplusplus
}
#endif
#endif /* HTM_HASHJOIN_H */
