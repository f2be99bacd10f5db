"""Host-side mirror of the reference's operator interface.

    reference (C++)                                   here
    ------------------------------------------------  ---------------------------------
    generate_data(dist, n, distinct, window)          generate_data(...)      DataGen.hpp:26
    NoCCHashBuild(relR,rSize,relS,sSize,scale,P,pl)    NoCCHashBuild(...)      NoCCHashBuild.hpp:13
    AtomicHashBuild(... same ...)                      AtomicHashBuild(...)    AtomicHashBuild.hpp:14
    HTMHashBuild(relR,rSize,relS,sSize,tSize,...)      HTMHashBuild(...)       HTMHashBuild.hpp:54
    PRO(relR, relS, nthreads)                          PRO(...)                mc/src/parallel_radix_join.c:1305

The reference functions return void and print one JSON line; these return the
same fields as a dict. Every operator runs on the GPU through the C ABI; without
a gfx950 device they raise HashJoinError(HJ_ERR_NO_DEVICE).

This module is the mirror of the C ABI: errors, parameter and descriptor packers, HashJoinContext, the layout functions,
the operators and the generators. The relational layer built on it lives in columns, conditions, joins, key_joins,
aggregates and groups, each of which imports only from this module and from those named before it.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib, hj_params, hj_result


# struct Bucket, HTMHashBuild.hpp:41-45 (32 bytes)
BUCKET_DTYPE = np.dtype([("tuples", np.uint64, 3), ("count", np.uint32), ("nextIndex", np.uint32)])

# HJ_NO_ROW: the R row of a left-outer row whose S tuple has no match
NO_ROW = _lib.HJ_NO_ROW


def _vp(d):
    """a device or host address as the C ABI takes it; 0 is NULL"""
    return C.c_void_p(d) if d else None


class HashJoinError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        msg = lib.hj_strerror(status).decode()
        super().__init__(f"{msg} [{status}]" + (f": {detail}" if detail else ""))


def device_count():
    n = C.c_int(0)
    lib.hj_device_count(C.byref(n))
    return n.value


def generate_data(dist, size_in_tuples, distinct_keys=None, local_shuffle_range=16, zipf_theta=0.9):
    """include/DataGen.hpp:26 -- returns a numpy uint64 array of size_in_tuples tuples."""
    if distinct_keys is None:
        distinct_keys = size_in_tuples
    out = np.empty(size_in_tuples, dtype=np.uint64)
    rc = lib.hj_generate_data(dist.encode(), size_in_tuples, distinct_keys, int(local_shuffle_range),
                              float(zipf_theta), out.ctypes.data)
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, f"Unknown distribution {dist!r}")
    return out


def generate_relation(kind, num_tuples, maxid=None, local_shuffle_range=0, zipf_param=0.0, seed=12345):
    """mc/src/generator.c: kind = pk | pk_lshuffle | fk | nonunique | zipf (create_relation_*), srand(seed) first
    (mc seeds R with 12345 and S with 54321, mc/src/main.c:337-338)."""
    out = np.empty(num_tuples, dtype=np.uint64)
    rc = lib.hj_generate_relation(kind.encode(), num_tuples, num_tuples if maxid is None else maxid,
                                  int(local_shuffle_range), float(zipf_param), int(seed), out.ctypes.data)
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, f"hj_generate_relation({kind!r})")
    return out


_WAVE_LAYOUT_FIELDS = ("chunkLen", "nChunks", "sliceLen", "tileTuples", "granuleSlots", "ringGranules", "look", "overlap",
                       "shadow", "tail", "crosserCap", "compactMaxProbeLength", "computeUnits")


def _wave_layout(handle, compute_units, n):
    out = (C.c_uint64 * 16)()
    rc = lib.hj_wave_layout_info(handle, compute_units, n, out)
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, f"hj_wave_layout_info(n={n}, computeUnits={compute_units})")
    return {k: int(out[i]) for i, k in enumerate(_WAVE_LAYOUT_FIELDS)}


def wave_layout_info(n, compute_units):
    """hj_wave_layout_info without a context (host-only arithmetic): how the ring builds cut n tuples into chunks on a
    device of compute_units compute units, and the constants of the seam zones (look, overlap, shadow, tail, crosserCap,
    compactMaxProbeLength, tileTuples, granuleSlots, ringGranules), as a dict."""
    return _wave_layout(None, int(compute_units), n)


_HTM_CHAIN_LAYOUT_FIELDS = ("slices", "sliceLen", "parts", "chainCountCap", "chainCap", "chainMaxParts", "partTuples", "tries")


def _htm_chain_layout(handle, compute_units, n):
    out = (C.c_uint64 * 8)()
    rc = lib.hj_htm_chain_layout_info(handle, compute_units, n, out)
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, f"hj_htm_chain_layout_info(n={n}, computeUnits={compute_units})")
    return {k: int(out[i]) for i, k in enumerate(_HTM_CHAIN_LAYOUT_FIELDS)}


def htm_chain_layout_info(n, compute_units):
    """hj_htm_chain_layout_info without a context (host-only arithmetic): the slices and parts the LDS chain phase of the
    bucketised table cuts n tuples' conflicts into on a device of compute_units compute units, the kernel's caps
    (chainCountCap, chainCap, chainMaxParts, partTuples) and whether the host tries the phase at this size, as a dict."""
    return _htm_chain_layout(None, int(compute_units), n)


_OWN_LAYOUT_FIELDS = ("chunkLen", "nChunks", "tileTuples", "blockSlots", "windowBlocks", "backBlocks", "seamDivisor",
                      "minTableSlots", "deferredParts", "maxProbeLength", "computeUnits")


def _own_layout(handle, compute_units, n):
    out = (C.c_uint64 * 16)()
    rc = lib.hj_own_layout_info(handle, compute_units, n, out)
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, f"hj_own_layout_info(n={n}, computeUnits={compute_units})")
    return {k: int(out[i]) for i, k in enumerate(_OWN_LAYOUT_FIELDS)}


def own_layout_info(n, compute_units):
    """hj_own_layout_info without a context (host-only arithmetic): how the workgroup-window build (buildVariant 2) cuts n
    tuples into chunks on a device of compute_units compute units, and its kernels' constants (tileTuples, blockSlots,
    windowBlocks, backBlocks, seamDivisor, minTableSlots, deferredParts, maxProbeLength), as a dict."""
    return _own_layout(None, int(compute_units), n)


_SLOT_CODES_FIELDS = ("fitsAuto", "dbits", "hiCap", "tableBits", "codes", "cause", "road", "tableFormat")


def _slot_codes(handle, table_size, probe_length):
    out = (C.c_uint64 * 8)()
    rc = lib.hj_slot_codes_info(handle, table_size, probe_length, out)
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, f"hj_slot_codes_info(tableSize={table_size}, probeLength={probe_length})")
    d = {k: int(out[i]) for i, k in enumerate(_SLOT_CODES_FIELDS)}
    d["fitsAuto"], d["codes"] = bool(d["fitsAuto"]), bool(d["codes"])
    return d


def slot_codes_info(table_size, probe_length=4):
    """hj_slot_codes_info without a context (host-only arithmetic): whether a ring build of a table of table_size slots
    at probe_length leaves one code byte per slot by itself (fitsAuto), the displacement's bits (dbits) and the high parts
    a code holds (hiCap), as a dict; the fields about a build (codes, cause, road, tableFormat) are 0."""
    return _slot_codes(None, int(table_size), int(probe_length))


_RING_WORD_FIELDS = ("word", "key", "triesLeft", "rel", "code", "relCap", "empty", "slot")


def ring_word_info(table_size, probe_length, rel, key, steps=0):
    """hj_ring_word_layout_info (host-only arithmetic): the 4-byte ring word of the tuple with offset rel and that key after
    `steps` steps from its home slot, and what reads back out of it, as a dict (word, key, triesLeft, rel, code, relCap,
    empty, slot). HashJoinError(HJ_ERR_INVALID) for what the slot-code road never makes; its relCap and empty are then in
    the error's .partial dict when the table size and probe length were good."""
    out = (C.c_uint64 * 8)()
    rc = lib.hj_ring_word_layout_info(int(table_size), int(probe_length), int(rel), int(key), int(steps), out)
    d = {k: int(out[i]) for i, k in enumerate(_RING_WORD_FIELDS)}
    if rc != _lib.HJ_OK:
        err = HashJoinError(rc, f"hj_ring_word_layout_info(tableSize={table_size}, probeLength={probe_length}, rel={rel}, key={key}, steps={steps})")
        err.partial = d
        raise err
    return d


def _params(algo, scaleOutput=2, numPartitions=64, probeLength=4, transactionSize=16, radixBits=0,
            buildVariant=0, prjMode=0, keepRowIds=False, trackRMatches=False, slotCodes=False):
    p = hj_params()
    p.algo = _lib.ALGO_IDS[algo]
    p.scaleOutput, p.numPartitions, p.probeLength = scaleOutput, numPartitions, probeLength
    p.transactionSize, p.radixBits, p.buildVariant = transactionSize, radixBits, buildVariant
    p.prjMode = prjMode
    p.flags = ((_lib.HJ_FLAG_KEEP_ROW_IDS if keepRowIds else 0) | (_lib.HJ_FLAG_TRACK_R_MATCHES if trackRMatches else 0) |
               (_lib.HJ_FLAG_SLOT_CODES if slotCodes else 0))
    return p


SHARD_ONE_BASED = 0x100


_KEY_GROUPS_INFO = ("groups", "written", "us", "null_rows", "slots", "probe_steps", "collisions", "failure")
_SORT_ROWS_INFO = ("rows", "passes", "us", "skipped", "chunks", "chunk_rows", "workspace_bytes", "reserved")
_WINDOW_ROWS_INFO = ("positions", "partitions", "peer_runs", "us", "skipped", "chunks", "workspace_bytes", "reserved")


def _sort_cols(cols):
    """[(values_ptr, valid_ptr, width, type, flags)] -> (hj_sort_col array, its length)"""
    cols = list(cols)
    arr = (_lib.hj_sort_col * max(len(cols), 1))()
    for c, (values, valid, width, type_, flags) in zip(arr, cols):
        c.values, c.valid, c.width, c.type, c.flags, c.reserved = values or None, valid or None, width, type_, flags, 0
    return arr, len(cols)


def _win_funcs(funcs):
    """[(op, out_ptr, src_ptr, valid_ptr, width, flags, offset)], whatever follows the out pointer optional (0) -> (hj_win_func
    array, its length)"""
    funcs = [tuple(f) + (0,) * (7 - len(f)) for f in funcs]
    arr = (_lib.hj_win_func * max(len(funcs), 1))()
    for a, (op, out, src, valid, width, flags, offset) in zip(arr, funcs):
        a.src, a.srcValid, a.out = src or None, valid or None, out or None
        a.op, a.width, a.flags, a.offset = op, width, flags, offset
    return arr, len(funcs)


def window_layout_info(n_pos):
    """hj_window_layout_info: how hj_window_rows_dev cuts n_pos positions -- tile positions, chunk positions, chunks,
    workspace bytes. Host-only; no device."""
    out = (C.c_uint64 * 4)()
    rc = lib.hj_window_layout_info(int(n_pos), out)
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, "hj_window_layout_info")
    return {"tile": int(out[0]), "chunk": int(out[1]), "chunks": int(out[2]), "workspace_bytes": int(out[3])}


def _frame_funcs(funcs):
    """[(op, out_ptr, lo, hi[, src_ptr, valid_ptr, width, flags])], lo / hi integers or None (unbounded: the flag is set and
    the offset 0), whatever follows hi optional (0) -> (hj_frame_func array, its length)"""
    funcs = [tuple(f) + (0,) * (8 - len(f)) for f in funcs]
    arr = (_lib.hj_frame_func * max(len(funcs), 1))()
    for a, (op, out, lo, hi, src, valid, width, flags) in zip(arr, funcs):
        a.src, a.srcValid, a.out = src or None, valid or None, out or None
        a.lo, a.hi = 0 if lo is None else int(lo), 0 if hi is None else int(hi)
        a.op, a.width, a.reserved = op, width, 0
        a.flags = flags | (_lib.HJ_FRAME_UNBOUNDED_LO if lo is None else 0) | (_lib.HJ_FRAME_UNBOUNDED_HI if hi is None else 0)
    return arr, len(funcs)


def frames_layout_info(n_pos):
    """hj_frames_layout_info: how hj_window_frames_dev cuts n_pos positions -- tile positions, chunk positions, chunks,
    workspace bytes (at most 32 per position plus 1 MiB, whatever the functions). Host-only; no device."""
    out = (C.c_uint64 * 4)()
    rc = lib.hj_frames_layout_info(int(n_pos), out)
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, "hj_frames_layout_info")
    return {"tile": int(out[0]), "chunk": int(out[1]), "chunks": int(out[2]), "workspace_bytes": int(out[3])}


def _key_cols(cols):
    """[(s_ptr, r_ptr, width)] -> (hj_key_col array, its length)"""
    cols = list(cols)
    arr = (_lib.hj_key_col * max(len(cols), 1))()
    for c, (s, r, width) in zip(arr, cols):
        c.s, c.r, c.width, c.reserved = s or None, r or None, width, 0
    return arr, len(cols)


def _key_cols2(cols):
    """[(s_ptr, r_ptr, width, s_offsets, r_offsets, s_valid, r_valid, flags)], whatever follows the width optional (0)
    -> (hj_key_col2 array, its length)"""
    cols = [tuple(c) + (0,) * (8 - len(c)) for c in cols]
    arr = (_lib.hj_key_col2 * max(len(cols), 1))()
    for c, (s, r, width, s_off, r_off, s_valid, r_valid, flags) in zip(arr, cols):
        c.s, c.r, c.sOffsets, c.rOffsets, c.sValid, c.rValid = (p or None for p in (s, r, s_off, r_off, s_valid, r_valid))
        c.width, c.flags = width, flags
    return arr, len(cols)


def _terms_arr(terms, struct=_lib.hj_where_term):
    """[(s_ptr, r_ptr, width, type, op, s_valid, r_valid)], the two planes optional (0) -> (array of `struct`, its length);
    struct: hj_where_term, or hj_asof_term, which has its fields (the array of one term is what hj_pairs_asof_* take)"""
    terms = [tuple(t) + (0,) * (7 - len(t)) for t in terms]
    arr = (struct * max(len(terms), 1))()
    for a, (s, r, width, type_, op, s_valid, r_valid) in zip(arr, terms):
        a.s, a.r, a.sValid, a.rValid = (p or None for p in (s, r, s_valid, r_valid))
        a.width, a.type, a.op, a.reserved = width, type_, op, 0
    return arr, len(terms)


def _agg_specs(specs):
    """[(op, width, flags[, reserved])] -> (hj_agg_spec array, its length)"""
    specs = [tuple(s) + (0,) * (4 - len(s)) for s in specs]
    arr = (_lib.hj_agg_spec * max(len(specs), 1))()
    for a, (op, width, flags, reserved) in zip(arr, specs):
        a.op, a.width, a.flags, a.reserved = op, width, flags, reserved
    return arr, len(specs)


def prj_agg_layout_info(n_cols):
    """hj_prj_agg_layout_info: the LDS layout of the aggregating radix join for n_cols columns -- table slots, R tuples per
    LDS build, S elements per round of a workgroup, S tuples per work item. Host-only; no device."""
    out = (C.c_uint64 * 4)()
    rc = lib.hj_prj_agg_layout_info(n_cols, out)
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, "hj_prj_agg_layout_info")
    return {"slots": int(out[0]), "blockTuples": int(out[1]), "roundS": int(out[2]), "itemS": int(out[3])}


class HashJoinContext:
    """One engine context bound to one GPU (hj_ctx). ``stream`` is a raw hipStream_t
    handle (e.g. torch.cuda.current_stream().cuda_stream); None = private stream."""

    def __init__(self, device=0, stream=None):
        self._h = C.c_void_p()
        if stream is None:
            rc = lib.hj_create(device, C.byref(self._h))
        else:
            rc = lib.hj_create_on_stream(device, C.c_void_p(stream), C.byref(self._h))
        if rc != _lib.HJ_OK:
            self._h = None
            raise HashJoinError(rc)
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            lib.hj_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != _lib.HJ_OK:
            raise HashJoinError(rc, lib.hj_last_error(self._h).decode())

    def _info(self, fn, n=4):
        """the n 64-bit words an hj_*_info function reports about this context, as a tuple of ints"""
        out = (C.c_uint64 * n)()
        self._check(fn(self._h, out))
        return tuple(int(x) for x in out)

    # ---- one-shot, host buffers -------------------------------------------
    def run(self, algo, relR, relS=None, **kw):
        relR = np.ascontiguousarray(relR, dtype=np.uint64)
        if relS is not None:
            relS = np.ascontiguousarray(relS, dtype=np.uint64)
        p = _params(algo, **kw)
        r = hj_result()
        self._check(lib.hj_run(self._h, C.byref(p), relR.ctypes.data, relR.size,
                               relS.ctypes.data if relS is not None else None,
                               relS.size if relS is not None else 0, C.byref(r)))
        return r.as_dict()

    # ---- split API, device pointers ---------------------------------------
    def reserve(self, algo, rSize, sSize, **kw):
        """hj_reserve. Keywords: the fields of hj_params, slotCodes (HJ_FLAG_SLOT_CODES), keepRowIds (HJ_FLAG_KEEP_ROW_IDS) and trackRMatches
        (HJ_FLAG_TRACK_R_MATCHES: one bit per R row, set by the inner / left probe_pairs and prj_probe_pairs calls for the
        R rows they produce, read by r_rows; needs keepRowIds except on "htm")."""
        p = _params(algo, **kw)
        self._check(lib.hj_reserve(self._h, C.byref(p), rSize, sSize))

    def build(self, dR_ptr, rSize, idx_base=0):
        self._check(lib.hj_build_dev(self._h, C.c_void_p(dR_ptr), rSize, idx_base))

    def probe(self, dS_ptr, sSize):
        self._check(lib.hj_probe_dev(self._h, C.c_void_p(dS_ptr), sSize))

    def probe_pairs(self, dS_ptr, sSize, d_out_s, d_out_r, capacity, s_idx_base=0, kind=0):
        """hj_probe_join_dev: the probe with its result kept. For every match the probe counts, one pair
        d_out_s[k] = s_idx_base + position in dS, d_out_r[k] = global input index of the matching R tuple (two device
        uint32 arrays of `capacity` entries; pairs beyond it are counted, not written). Open addressing needs
        reserve(..., keepRowIds=True). Adds to totalMatches and sSize like probe().
        kind (HJ_JOIN_*): 0 inner (the above), 1 left outer (an S tuple without a match gives one row with R row NO_ROW),
        2 semi / 3 anti (one S row per tuple with / without a match; d_out_r is ignored and may be 0). totalMatches
        grows by the inner matches whatever the kind."""
        self._check(lib.hj_probe_join_dev(self._h, kind, _vp(dS_ptr), sSize, s_idx_base, _vp(d_out_s), _vp(d_out_r), capacity))

    def pairs_info(self):
        """hj_pairs_info (waits for the stream): (rows the last probe_pairs / prj_probe_pairs found, rows it wrote, its
        device time in microseconds, its S tuples without a match for a kind other than inner -- 0 after an inner call)."""
        return self._info(lib.hj_pairs_info)

    # ---- R-side match marks (reserve(..., trackRMatches=True)) ----------------
    def r_rows(self, which, d_out_r, capacity):
        """hj_r_rows_dev: the R rows of the last build that no inner / left probe since has produced (which = 0,
        HJ_R_UNMATCHED) or that one has (1, HJ_R_MATCHED), ascending, into the device uint32 array d_out_r of `capacity`
        entries; rows beyond it are counted, not written (capacity 0, d_out_r 0: count only). Changes no mark."""
        self._check(lib.hj_r_rows_dev(self._h, which, _vp(d_out_r), capacity))

    def r_rows_info(self):
        """hj_r_rows_info (waits for the stream): (rows the last r_rows produced, rows it wrote, its device time in
        microseconds, R rows of the build)."""
        return self._info(lib.hj_r_rows_info)

    def r_marks_clear(self):
        """hj_r_marks_clear: every R row unmatched again, without rebuilding."""
        self._check(lib.hj_r_marks_clear(self._h))

    # ---- payload columns through a row map ---------------------------------
    def gather(self, d_map, n_rows, src_rows, cols, d_valid=0, row_base=0):
        """hj_gather_dev: for every output row k < n_rows and e = d_map[k] (a device uint32 map as probe_pairs,
        prj_probe_pairs and r_rows write them), dst[k] = src[e - row_base] in every column; a row whose entry is NO_ROW, or
        lies at or behind src_rows once the base is off, reads nothing and gets the column's fill. cols: up to
        HJ_GATHER_MAX_COLS tuples (src_ptr, dst_ptr, width, fill), width 1, 2, 4, 8 or 16 bytes, fill an int or bytes (its
        low `width` bytes count). d_valid (0: none): device uint32 words, bit k & 31 of word k >> 5 = row k has a source
        row. Asynchronous; needs no reserve and no table."""
        cols = list(cols)
        arr = (_lib.hj_gather_col * max(len(cols), 1))()
        for c, (src, dst, width, fill) in zip(arr, cols):
            if isinstance(fill, (bytes, bytearray)):
                fill = int.from_bytes(bytes(fill[:16]), "little")
            c.src, c.dst, c.width, c.reserved = src or None, dst or None, width, 0
            c.fill[0], c.fill[1] = fill & 0xFFFFFFFFFFFFFFFF, (fill >> 64) & 0xFFFFFFFFFFFFFFFF
        self._check(lib.hj_gather_dev(self._h, _vp(d_map), n_rows, row_base, src_rows,
                                      arr if cols else None, len(cols), _vp(d_valid)))

    def gather_info(self):
        """hj_gather_info (waits for the stream): (rows of the last gather, its NULL rows, its device time in
        microseconds, its out-of-range entries); all 0 before the first one."""
        return self._info(lib.hj_gather_info)

    def gather2(self, d_map, n_rows, src_rows, cols, d_valid=0, row_base=0):
        """hj_gather2_dev: gather on columns in the Arrow layout. cols: up to HJ_GATHER_MAX_COLS dicts with the fields of
        hj_gather_col2 as keys, whatever is left out being 0 -- src, dst, width (0: variable length), fill (an int or
        bytes), src_offsets / dst_offsets (variable length: src_rows + 1 offsets in, n_rows + 1 out), src_valid (the
        source's validity plane), dst_valid (n_rows bits out: the row has a source row and its element is valid),
        dst_capacity (variable length: the bytes of dst; 0 is the sizing pass) -- all pointers device pointers. The map,
        row_base and d_valid (the call-level plane "row has a source row") are gather's. Asynchronous; needs no reserve and
        no table. gather2_info() gives the bytes each column's rows take."""
        cols = list(cols)
        arr = (_lib.hj_gather_col2 * max(len(cols), 1))()
        for c, d in zip(arr, cols):
            unknown = set(d) - {"src", "dst", "width", "fill", "src_offsets", "dst_offsets", "src_valid", "dst_valid", "dst_capacity", "flags"}
            if unknown:
                raise ValueError(f"gather2: unknown column fields {sorted(unknown)}")
            fill = d.get("fill", 0)
            if isinstance(fill, (bytes, bytearray)):
                fill = int.from_bytes(bytes(fill[:16]), "little")
            c.src, c.dst, c.srcOffsets, c.dstOffsets, c.srcValid, c.dstValid = (
                d.get(k) or None for k in ("src", "dst", "src_offsets", "dst_offsets", "src_valid", "dst_valid"))
            c.dstCapacity, c.width, c.flags = d.get("dst_capacity", 0), d.get("width", 0), d.get("flags", 0)
            c.fill[0], c.fill[1] = fill & 0xFFFFFFFFFFFFFFFF, (fill >> 64) & 0xFFFFFFFFFFFFFFFF
        self._check(lib.hj_gather2_dev(self._h, _vp(d_map), n_rows, row_base, src_rows,
                                       arr if cols else None, len(cols), _vp(d_valid)))

    def gather2_info(self):
        """hj_gather2_info (waits for the stream): (rows of the last gather2, its NULL rows, its device time in
        microseconds, its out-of-range entries, then per column the bytes its rows take -- exact in 64 bits, 0 for a fixed
        column; above 2^32 - 1 the column was not written); all 0 before the first one. gather_info() reports gather()
        alone, and the other way round."""
        return self._info(lib.hj_gather2_info, 4 + _lib.HJ_GATHER_MAX_COLS)

    # ---- joins on real key columns: hash, candidate join, verify ---------------
    def key_hash(self, cols, side, n_rows, d_out, key_mask=0):
        """hj_key_hash_dev: d_out[i] = the 32-bit join word of row i < n_rows as an 8-byte tuple (what prj_build and
        prj_probe_pairs take), hashed from the key columns cols = 1 to HJ_KEY_MAX_COLS tuples (s_ptr, r_ptr, width) of
        device pointers, width 1, 2, 4, 8 or 16 bytes; side (HJ_KEY_SIDE_S / HJ_KEY_SIDE_R) says which pointers are read,
        the others may be 0. The hash is MurmurHash3_x86_32 over the row's columns (include/htm_hashjoin.h), & key_mask
        (0: all 32 bits). Asynchronous; needs no reserve and no table."""
        arr, n = _key_cols(cols)
        self._check(lib.hj_key_hash_dev(self._h, arr, n, side, n_rows, key_mask, _vp(d_out)))

    def pairs_verify(self, d_map_s, d_map_r, n_pairs, s_row_base, s_rows, r_rows, cols, d_out_s, d_out_r, capacity,
                     d_s_marks=0, d_r_marks=0):
        """hj_pairs_verify_dev: of the n_pairs candidate pairs (d_map_s[k] - s_row_base, d_map_r[k]) -- the planes of a
        prj_probe_pairs(kind=0) call on hashed keys -- keeps those whose key columns (cols as in key_hash, both pointers
        of every column in use) are bytewise equal, and writes them to d_out_s / d_out_r as probe_pairs writes its pairs
        (d_out_s keeps the base; pairs beyond `capacity` are counted, not written; capacity 0 with 0 outputs marks only).
        Every kept pair sets bit s of d_s_marks and bit r of d_r_marks (device uint32 words, bit i & 31 of word i >> 5;
        0: no plane), which the caller has cleared. A candidate that is NO_ROW or outside s_rows / r_rows is dropped
        unread. The outputs must not alias the maps. Asynchronous; needs no reserve and no table."""
        arr, n = _key_cols(cols)
        self._check(lib.hj_pairs_verify_dev(self._h, _vp(d_map_s), _vp(d_map_r), n_pairs, s_row_base, s_rows, r_rows, arr, n,
                                            _vp(d_out_s), _vp(d_out_r), capacity, _vp(d_s_marks), _vp(d_r_marks)))

    def key_hash2(self, cols, side, n_rows, d_out, key_mask=0):
        """hj_key_hash2_dev: key_hash on key columns in the Arrow layout. cols = 1 to HJ_KEY_MAX_COLS tuples (s_ptr,
        r_ptr, width, s_offsets, r_offsets, s_valid, r_valid, flags) of device pointers, whatever follows the width
        optional (0). A fixed column has width 1, 2, 4, 8 or 16 and no offsets; a variable-length one width 0, the bytes
        buffer as its pointer and n_rows + 1 uint32 offsets into it. s_valid / r_valid: the validity plane of that side
        (uint32 words, bit i & 31 of word i >> 5, 1 = valid; 0: no NULLs). flags: HJ_KEY_NULLS_EQUAL or 0. The hash and
        the word of a NULL-keyed row: include/htm_hashjoin.h. Asynchronous; needs no reserve and no table."""
        arr, n = _key_cols2(cols)
        self._check(lib.hj_key_hash2_dev(self._h, arr, n, side, n_rows, key_mask, _vp(d_out)))

    def pairs_verify2(self, d_map_s, d_map_r, n_pairs, s_row_base, s_rows, r_rows, cols, d_out_s, d_out_r, capacity,
                      d_s_marks=0, d_r_marks=0):
        """hj_pairs_verify2_dev: pairs_verify on key columns in the Arrow layout (cols as in key_hash2, both sides of
        every column in use; the S side's offsets and validity are indexed by the S row with s_row_base off, like its
        column). A column is equal when -- either element NULL: both are and the column has HJ_KEY_NULLS_EQUAL;
        otherwise fixed width: bytewise; otherwise: the same length and the same bytes. Outputs, marks, dropped
        candidates and aliasing as in pairs_verify; verify_info reports the last call of either."""
        arr, n = _key_cols2(cols)
        self._check(lib.hj_pairs_verify2_dev(self._h, _vp(d_map_s), _vp(d_map_r), n_pairs, s_row_base, s_rows, r_rows, arr, n,
                                             _vp(d_out_s), _vp(d_out_r), capacity, _vp(d_s_marks), _vp(d_r_marks)))

    def verify_info(self):
        """hj_verify_info (waits for the stream): (pairs the last pairs_verify kept, pairs it wrote, its device time in
        microseconds, candidates it dropped as NO_ROW or out of range); rejected = n_pairs - kept - dropped."""
        return self._info(lib.hj_verify_info)

    # ---- the rows of one table grouped by their key columns ----------------------------
    def key_groups(self, cols, side, n_rows, d_rep, d_group=0, d_first_rows=0, capacity=0, key_mask=0):
        """hj_key_groups_dev: which rows of ONE table have the same key. cols as in key_hash2, read from the `side`
        pointers. d_rep[i] (n_rows device uint32) = the lowest row whose key equals row i's, column equality as in
        pairs_verify2; d_first_rows (device uint32, `capacity` entries; 0 with capacity 0: the count alone) = the rows with
        d_rep[i] == i, ascending, rows beyond the capacity counted and not written; d_group[i] (0: not wanted) = the position
        of d_rep[i] among ALL first rows, a dense group id in order of first occurrence. A NULL-keyed row is in no group:
        NO_ROW in both planes. Exact, whatever key_mask and the scheduling. Asynchronous; needs no reserve and no table;
        the context's workspace grows with n_rows."""
        arr, n = _key_cols2(cols)
        self._check(lib.hj_key_groups_dev(self._h, arr, n, side, n_rows, key_mask, _vp(d_rep), _vp(d_group), _vp(d_first_rows), capacity))

    def key_groups_info(self):
        """hj_key_groups_info (waits for the stream), about the last key_groups: groups, first rows written, the device time
        of the call in microseconds, NULL-keyed rows, table slots, probe steps beyond the home slot, key compares that found
        a different key (word collisions), the device-side failure word (0 on success)."""
        return dict(zip(_KEY_GROUPS_INFO, self._info(lib.hj_key_groups_info, 8)))

    # ---- rows in the order of their columns ----------------------------------------
    def sort_rows(self, desc, n, d_perm):
        """hj_sort_rows_dev: d_perm[0 .. n) = the rows 0 .. n - 1 of ONE table in ascending lexicographic order of its key
        columns, stable (ORDER BY). desc = 1 to HJ_SORT_MAX_COLS tuples (values_ptr, valid_ptr, width, type, flags) of device
        pointers, the most significant column first: elements of `width` bytes read as HJ_VAL_UINT / HJ_VAL_INT (1, 2, 4, 8)
        or HJ_VAL_FLOAT (4, 8: -0.0 == 0.0, every NaN one value above +inf), valid_ptr the validity plane or 0, flags
        HJ_SORT_DESC | HJ_SORT_NULLS_FIRST (NULLs stand last without it, whatever the direction). Asynchronous; needs no
        reserve and no table; the workspace belongs to the context and grows with n."""
        arr, k = _sort_cols(desc)
        self._check(lib.hj_sort_rows_dev(self._h, arr, k, n, _vp(d_perm)))

    def sort_rows_info(self):
        """hj_sort_rows_info (waits for the stream), about the last sort_rows: rows, radix passes, the device time of the
        whole call (us), passes skipped (always 0), chunks, chunk_rows, workspace_bytes"""
        return dict(zip(_SORT_ROWS_INFO, self._info(lib.hj_sort_rows_info, 8)))

    # ---- window functions over the runs along a permutation --------------------------
    def window_rows(self, d_perm, n_pos, n_rows, d_part, order, funcs):
        """hj_window_rows_dev: f(...) OVER (PARTITION BY .. ORDER BY ..) along d_perm[0 .. n_pos) (0: the identity). A
        partition is a maximal run of positions whose d_part[row] are equal (0: one value), peers are the rows that tie in
        every column of `order` (tuples as sort_rows takes them; the flags do not matter). funcs = 1 to HJ_WIN_MAX_FUNCS
        tuples (op, out_ptr[, src_ptr, valid_ptr, width, flags, offset]): op an hj_win_op, out n_rows entries INDEXED BY
        ROW -- uint32 for the numbering ops and the row maps (LAG / LEAD by `offset`, first, last: gather maps with NO_ROW
        holes), 8 bytes for the running COUNT / SUM / MIN / MAX over src (width 4 or 8, flags HJ_AGG_SIGNED, valid_ptr the
        validity plane). An entry of d_perm that is NO_ROW or >= n_rows writes nothing and ends the run; a row at no
        position keeps what its out entries held. Asynchronous; needs no reserve and no table; the workspace belongs to
        the context and grows with n_pos."""
        o_arr, n_order = _sort_cols(order)
        f_arr, n_funcs = _win_funcs(funcs)
        self._check(lib.hj_window_rows_dev(self._h, _vp(d_perm), n_pos, n_rows, _vp(d_part), o_arr, n_order, f_arr, n_funcs))

    def window_rows_info(self):
        """hj_window_rows_info (waits for the stream), about the last window_rows: positions, partitions, peer_runs, the
        device time of the whole call (us), skipped entries, chunks, workspace_bytes"""
        return dict(zip(_WINDOW_ROWS_INFO, self._info(lib.hj_window_rows_info, 8)))

    # ---- sliding window frames over the same runs -------------------------------------
    def window_frames(self, d_perm, n_pos, n_rows, d_part, funcs):
        """hj_window_frames_dev: COUNT / SUM / MIN / MAX OVER (PARTITION BY .. ORDER BY .. ROWS BETWEEN lo AND hi) along
        d_perm[0 .. n_pos) (0: the identity); positions, partitions (runs of equal d_part[row], 0: one value) and skipped
        entries are window_rows'. funcs = 1 to HJ_FRAME_MAX_FUNCS tuples (op, out_ptr, lo, hi[, src_ptr, valid_ptr, width,
        flags]): op an hj_agg_op, out n_rows entries of 8 bytes INDEXED BY ROW, lo <= hi the frame's ends relative to the
        position (negative: preceding; None: unbounded on that side), the frame clamped to the partition; src of width 4
        or 8 (flags HJ_AGG_SIGNED), valid_ptr the validity plane. An empty frame gives the op's identity and COUNT 0. A row
        at no position keeps what its out entries held. Asynchronous; needs no reserve and no table; the workspace belongs
        to the context (apart from window_rows') and grows with n_pos."""
        f_arr, n_funcs = _frame_funcs(funcs)
        self._check(lib.hj_window_frames_dev(self._h, _vp(d_perm), n_pos, n_rows, _vp(d_part), f_arr, n_funcs))

    def window_frames_info(self):
        """hj_window_frames_info (waits for the stream), about the last window_frames, under window_rows_info's names:
        positions, partitions, peer_runs (always 0), the device time of the whole call (us), skipped entries, chunks,
        workspace_bytes"""
        return dict(zip(_WINDOW_ROWS_INFO, self._info(lib.hj_window_frames_info, 8)))

    # ---- join conditions beyond equality ------------------------------------------
    def pairs_where(self, d_map_s, d_map_r, n_pairs, s_row_base, s_rows, r_rows, terms, d_out_s, d_out_r, capacity,
                    d_s_marks=0, d_r_marks=0):
        """hj_pairs_where_dev: of the n_pairs pairs (d_map_s[k] - s_row_base, d_map_r[k]) -- the planes of an inner probe, or
        the kept pairs of pairs_verify -- keeps those for which every term holds. terms = 1 to HJ_WHERE_MAX_TERMS tuples
        (s_ptr, r_ptr, width, type, op, s_valid, r_valid) of device pointers, the two validity planes optional (0: no
        NULLs): the term is s[si] op r[ri] with op an hj_cmp_op (CMP_OPS) and the elements of `width` bytes read as type
        HJ_VAL_UINT / HJ_VAL_INT (1, 2, 4, 8 bytes) or HJ_VAL_FLOAT (4, 8: IEEE-754, -0.0 == 0.0, a NaN is unordered). A
        term with a NULL on either side does not hold. Outputs, marks, dropped pairs and aliasing as in pairs_verify.
        Asynchronous; needs no reserve and no table."""
        arr, n = _terms_arr(terms)
        self._check(lib.hj_pairs_where_dev(self._h, _vp(d_map_s), _vp(d_map_r), n_pairs, s_row_base, s_rows, r_rows, arr, n,
                                           _vp(d_out_s), _vp(d_out_r), capacity, _vp(d_s_marks), _vp(d_r_marks)))

    def where_info(self):
        """hj_where_info (waits for the stream): (pairs the last pairs_where kept, pairs it wrote, its device time in
        microseconds, pairs it dropped as NO_ROW or out of range); rejected = n_pairs - kept - dropped."""
        return self._info(lib.hj_where_info)

    # ---- as-of joins: one best match per S row ------------------------------------
    def pairs_asof(self, d_map_s, d_map_r, n_pairs, s_row_base, s_rows, r_rows, term, d_best_val, d_best_row, d_out_s, d_out_r,
                   capacity, d_s_marks=0, d_r_marks=0):
        """hj_pairs_asof_dev: of the n_pairs pairs (d_map_s[k] - s_row_base, d_map_r[k]) keeps, per S row, the one eligible
        pair whose R value is nearest on the permitted side. term = (s_ptr, r_ptr, width, type, op, s_valid, r_valid) as a
        term of pairs_where, op out of ASOF_OPS: a pair is eligible when s[si] op r[ri] holds (a NULL or a NaN on either
        side: it does not); ">=" / ">" keep the pair with the largest R value, "<=" / "<" the one with the smallest; ties go
        to the lowest R row. d_best_val (s_rows 64-bit words) and d_best_row (s_rows 32-bit words) are the caller's planes,
        initialised by the call: d_best_row[i] ends as the R row kept for S row s_row_base + i, or NO_ROW. Outputs, marks
        (set by the kept pairs alone), dropped pairs and aliasing as in pairs_where. All pairs of an S row must be in one
        call. Asynchronous; needs no reserve and no table."""
        self._check(lib.hj_pairs_asof_dev(self._h, _vp(d_map_s), _vp(d_map_r), n_pairs, s_row_base, s_rows, r_rows,
                                          _terms_arr([term], _lib.hj_asof_term)[0], _vp(d_best_val), _vp(d_best_row), _vp(d_out_s), _vp(d_out_r),
                                          capacity, _vp(d_s_marks), _vp(d_r_marks)))

    def asof_info(self):
        """hj_asof_info (waits for the stream): (pairs the last pairs_asof kept, pairs it wrote, the device time of the whole
        call in microseconds, pairs it dropped as NO_ROW or out of range)."""
        return self._info(lib.hj_asof_info)

    # ---- range joins without an equality key -----------------------------------------
    def range_index(self, col, n, d_perm, d_keys, d_head):
        """hj_range_index_dev: the index of ONE column for range_pairs. col = (values_ptr, valid_ptr, width, type) of device
        pointers as a column of sort_rows (no flags: ascending, NULLs last). d_perm: n uint32 (the ascending, stable
        permutation), d_keys: n order keys of 4 bytes (widths 1, 2, 4) or 8, d_head: 4 uint32 -- rows indexed (valid and no
        NaN: a prefix of the order), NULL rows, NaN rows, key bytes. The three planes are the caller's, their content the
        library's. Asynchronous; needs no reserve and no table; the workspace is sort_rows'."""
        arr, _ = _sort_cols([tuple(col)[:4] + (0,)])
        self._check(lib.hj_range_index_dev(self._h, arr, n, _vp(d_perm), _vp(d_keys), _vp(d_head)))

    def range_index_info(self):
        """hj_range_index_info (waits for the stream), about the last range_index, whose d_head must still be allocated:
        (rows indexed, NULL rows, the device time of the call in microseconds, NaN rows)."""
        return self._info(lib.hj_range_index_info)

    def range_pairs(self, d_keys, d_perm, d_head, r_rows, term, s_rows, s_row_base, d_out_s, d_out_r, capacity, d_s_marks=0, d_r_marks=0):
        """hj_range_pairs_dev: for S row i < s_rows the pairs (s_row_base + i, r) of every indexed R row r whose value lies
        between lo[i] and hi[i]. term = (lo_ptr, hi_ptr, width, type[, flags, pick, lo_valid, hi_valid]) of device pointers:
        a bound of 0 is no bound on that side (not both), flags HJ_RANGE_LO_OPEN | HJ_RANGE_HI_OPEN, pick HJ_RANGE_ALL /
        FIRST (the smallest R value in the range) / LAST (the largest; ties to the lowest R row). The index (range_index)
        is read on the device: no wait in between. A NULL or NaN bound matches nothing. Outputs and marks as pairs_where;
        capacity 0 with outputs 0 sizes or marks only; the total is exact in 64 bits. Asynchronous; needs no reserve."""
        t = tuple(term) + (0,) * (8 - len(term))
        arr = _lib.hj_range_term()
        arr.lo, arr.hi, arr.width, arr.type, arr.flags, arr.pick = t[0] or None, t[1] or None, t[2], t[3], t[4], t[5]
        arr.loValid, arr.hiValid = t[6] or None, t[7] or None
        self._check(lib.hj_range_pairs_dev(self._h, _vp(d_keys), _vp(d_perm), _vp(d_head), r_rows, C.byref(arr), s_rows, s_row_base,
                                           _vp(d_out_s), _vp(d_out_r), capacity, _vp(d_s_marks), _vp(d_r_marks)))

    def range_pairs_info(self):
        """hj_range_pairs_info (waits for the stream), about the last range_pairs: (pairs, pairs written, its device time in
        microseconds, S rows with a pair, S rows with a NULL or NaN bound, rows indexed, 0, 0)."""
        return self._info(lib.hj_range_pairs_info, 8)

    def mark_rows(self, d_marks, rows, row_base, which, d_out, capacity):
        """hj_mark_rows_dev: r_rows on a caller's plane. The rows row_base + i, i < rows, whose bit i of d_marks is clear
        (which = 0, HJ_R_UNMATCHED) or set (1, HJ_R_MATCHED), ascending, into the device uint32 array d_out of `capacity`
        entries; rows beyond it are counted, not written (capacity 0, d_out 0: count only). Changes no mark."""
        self._check(lib.hj_mark_rows_dev(self._h, _vp(d_marks), rows, row_base, which, _vp(d_out), capacity))

    def mark_rows_info(self):
        """hj_mark_rows_info (waits for the stream): (rows the last mark_rows produced, rows it wrote, its device time in
        microseconds, the rows of its plane)."""
        return self._info(lib.hj_mark_rows_info)

    def prj_join(self, dR_ptr, rSize, dS_ptr, sSize):
        self._check(lib.hj_prj_join_dev(self._h, C.c_void_p(dR_ptr), rSize,
                                        _vp(dS_ptr), sSize))

    # ---- PRJ with a resident R: partition R once, probe S slice by slice ----
    def prj_build(self, dR_ptr, rSize):
        """Radix-partitions dR once and keeps the partitions in the context (dR may be freed afterwards); resets the
        counters, prjChecksum = R's checksum. Sizing: reserve("prj" or "auto", rSize, largest slice)."""
        self._check(lib.hj_prj_build_dev(self._h, C.c_void_p(dR_ptr), rSize))

    def prj_probe(self, dS_ptr, sSize):
        """Partitions one S slice and joins it against the resident R; totalMatches and sSize add up over the slices."""
        self._check(lib.hj_prj_probe_dev(self._h, _vp(dS_ptr), sSize))

    def prj_probe_pairs(self, dS_ptr, sSize, d_out_s, d_out_r, capacity, s_idx_base=0, kind=0):
        """hj_prj_probe_join_dev: prj_probe with its result kept, against an R built after reserve("prj" or "auto", ...,
        keepRowIds=True). For every match one pair d_out_s[k] = s_idx_base + position in dS, d_out_r[k] = position of
        the R tuple in the relation given to prj_build (two device uint32 arrays of `capacity` entries; pairs beyond it
        are counted, not written). The complete equi-join on the key word. pairs_info() reports the call.
        kind (HJ_JOIN_*): as in probe_pairs."""
        self._check(lib.hj_prj_probe_join_dev(self._h, kind, _vp(dS_ptr), sSize, s_idx_base, _vp(d_out_s), _vp(d_out_r), capacity))

    def prj_resident_info(self):
        """hj_prj_resident_info (waits for the stream): R's and the last slice's partitioning path, the last probe's join
        work items, its partitions split over several items, its largest S partition, bytes held for R."""
        out = self._info(lib.hj_prj_resident_info, 8)
        return {"rPath": out[0], "sPath": out[1], "items": out[2], "splitPartitions": out[3],
                "maxSPartition": out[4], "residentBytes": out[5]}

    # ---- aggregating joins: COUNT / SUM / MIN / MAX per R row, without the pairs ----
    def prj_agg_begin(self, specs):
        """hj_prj_agg_begin: starts an aggregation over the resident R (built after reserve(..., keepRowIds=True)).
        specs: 1 to HJ_AGG_MAX_COLS tuples (op, width, flags[, reserved]) -- op an HJ_AGG_* value, width 4 or 8 (0 for
        HJ_AGG_COUNT), flags HJ_AGG_SIGNED or 0. Allocates and initialises the context's accumulators: 0 for COUNT and
        SUM, the largest value of the type for MIN, the smallest for MAX."""
        arr, n = _agg_specs(specs)
        self._check(lib.hj_prj_agg_begin(self._h, arr, n))

    def prj_probe_agg(self, dS_ptr, sSize, srcs):
        """hj_prj_probe_agg_dev: prj_probe with its matches reduced. srcs: one tuple (src_ptr, valid_ptr) per column of
        the begin -- device pointers, src one element per S tuple of the slice (0 for a COUNT), valid_ptr the validity
        words of those elements or 0. For every match (s, r): the accumulator of r op= src[s] where s is valid, and r's
        match count + 1. The accumulators persist across calls; totalMatches and sSize grow as under prj_probe."""
        srcs = list(srcs)
        arr = (_lib.hj_agg_src * max(len(srcs), 1))()
        for a, (src, valid) in zip(arr, srcs):
            a.src, a.srcValid = src or None, valid or None
        self._check(lib.hj_prj_probe_agg_dev(self._h, _vp(dS_ptr), sSize, arr, len(srcs)))

    def prj_agg_rows(self, d_outs, d_count=0):
        """hj_prj_agg_rows_dev: the accumulators by R row. d_outs: one device pointer per column of the begin, each a plane
        of rSize 8-byte entries; d_count (0: none): the same for the match counts. Every R row is written once; the
        accumulators stay as they are."""
        d_outs = list(d_outs)
        arr = (C.c_void_p * max(len(d_outs), 1))(*[_vp(p) for p in d_outs])
        self._check(lib.hj_prj_agg_rows_dev(self._h, arr if d_outs else None, _vp(d_count)))

    def prj_agg_info(self):
        """hj_prj_agg_info (waits for the stream): the matches of the last prj_probe_agg, its device time in microseconds,
        the columns of the aggregation, the probes since prj_agg_begin, the R tuples its planes hold."""
        return dict(zip(("matches", "us", "nCols", "probes", "rows"), self._info(lib.hj_prj_agg_info, 8)))

    def pairs_agg(self, d_map_g, d_map_v, n_pairs, g_base, g_rows, v_base, v_rows, cols, d_count=0):
        """hj_pairs_agg_dev: the reduction over a pair list. For pair k, g = d_map_g[k] - g_base and v = d_map_v[k] -
        v_base: acc[g] op= src[v] in every column, d_count[g] += 1. cols: up to HJ_AGG_MAX_COLS tuples (src_ptr, valid_ptr,
        acc_ptr, op, width, flags[, reserved]); the accumulators (g_rows x 8 bytes each) and d_count are the caller's,
        initialised by the caller. A pair that is NO_ROW or out of range on either side is skipped unread. d_map_v may be
        0 when no column reads a value. One memory-side atomic per run of equal g within a wavefront and column."""
        cols = [tuple(c) + (0,) * (7 - len(c)) for c in cols]
        arr = (_lib.hj_agg_col * max(len(cols), 1))()
        for a, (src, valid, acc, op, width, flags, reserved) in zip(arr, cols):
            a.src, a.srcValid, a.acc = src or None, valid or None, acc or None
            a.op, a.width, a.flags, a.reserved = op, width, flags, reserved
        self._check(lib.hj_pairs_agg_dev(self._h, _vp(d_map_g), _vp(d_map_v), n_pairs, g_base, g_rows, v_base, v_rows,
                                         arr if cols else None, len(cols), _vp(d_count)))

    def pairs_agg_info(self):
        """hj_pairs_agg_info (waits for the stream): (pairs of the last pairs_agg, pairs it applied, its device time in
        microseconds, pairs it skipped as NO_ROW or out of range)."""
        return self._info(lib.hj_pairs_agg_info)

    def join(self, dR_ptr, rSize, dS_ptr, sSize):
        """Build + probe by the reserved algo; "auto" samples R for locality and picks atomic or prj."""
        self._check(lib.hj_join_dev(self._h, C.c_void_p(dR_ptr), rSize,
                                    _vp(dS_ptr), sSize))

    def checksums(self):
        self._check(lib.hj_checksums_dev(self._h))

    def fetch(self):
        r = hj_result()
        self._check(lib.hj_fetch_result(self._h, C.byref(r)))
        return r.as_dict()

    def wave_layout_info(self, n):
        """hj_wave_layout_info for this context's device (see engine.wave_layout_info)."""
        return _wave_layout(self._h, 0, n)

    def wave_seams(self):
        """hj_wave_seams (waits for the stream): what the ring pre-pass of the last build decided, as numpy uint32 arrays
        starts[nChunks + 1], bounds[nChunks + 1] (granules) and pcounts[nChunks] (walks let in across each chunk's lower
        seam; defined only when the compact build held). HJ_ERR_STATE when that build did not run the rings."""
        n_chunks = C.c_uint64(0)
        cap = 1
        while True:
            starts, bounds = np.empty(cap, dtype=np.uint32), np.empty(cap, dtype=np.uint32)
            pcounts = np.empty(cap, dtype=np.uint32)
            rc = lib.hj_wave_seams(self._h, starts.ctypes.data, bounds.ctypes.data, pcounts.ctypes.data, cap,
                                   C.byref(n_chunks))
            if rc == _lib.HJ_ERR_INVALID and n_chunks.value + 1 > cap:
                cap = n_chunks.value + 1
                continue
            self._check(rc)
            k = n_chunks.value
            return starts[:k + 1], bounds[:k + 1], pcounts[:k]

    def wave_planar_info(self):
        """hj_wave_planar_info (waits for the stream): whether the last build left the planar table of the classic rings
        (4-byte keys + an index plane), and why that build handed over to the packed one (0: it did not)."""
        out = self._info(lib.hj_wave_planar_info)
        return {"planar": bool(out[0]), "planarFallback": out[1], "tableFormat": out[2]}

    def slot_codes_info(self):
        """hj_slot_codes_info for the table of the last build (waits for the stream): slot_codes_info()'s fields, and codes
        (the table is one code byte per slot), cause (why the road handed over to the 8-byte build; 0: it did not or was not
        taken; 4 = a key no code holds), road (0 not taken, 1 by the size rule, 2 forced by reserve(..., slotCodes=True)),
        tableFormat."""
        return _slot_codes(self._h, 0, 0)

    def table_debug(self):
        """hj_table_debug (waits for the stream; for tests): the valid slot range [validLo, validHiEx) of the last build,
        its table format (0 = 8-byte slots, 1 = 4-byte keys), the slots of the live table (htm: 4 per bucket), and the
        table buffer's device address and size in bytes -- with copy_d2h, the raw table words."""
        return dict(zip(("validLo", "validHiEx", "tableFormat", "tableSlots", "tableAddr", "tableBytes"),
                        self._info(lib.hj_table_debug, 6)))

    def htm_chain_layout_info(self, n):
        """hj_htm_chain_layout_info for this context's device (see engine.htm_chain_layout_info)."""
        return _htm_chain_layout(self._h, 0, n)

    def htm_chain_info(self):
        """hj_htm_chain_info (waits for the stream): state 0 = the last htm build did not try the LDS chain phase, 1 = it
        held, 2 = it handed over (compactFallback bit 8); cause = the mask of why (a non-empty subset of the causes the
        input holds); groups = overflow buckets the parts asked for where it held."""
        return dict(zip(("state", "cause", "groups"), self._info(lib.hj_htm_chain_info)))

    def own_layout_info(self, n):
        """hj_own_layout_info for this context's device (see engine.own_layout_info)."""
        return _own_layout(self._h, 0, n)

    def own_info(self):
        """hj_own_info (waits for the stream): what the last workgroup-window build left, as numpy uint32 arrays
        owner[table blocks] (0, or chunk + 1) and deferCounts[chunks], and the sum of the counts. HJ_ERR_STATE when that
        build did not run the window build."""
        out = (C.c_uint64 * 4)()
        owner, counts = np.empty(1, dtype=np.uint32), np.empty(1, dtype=np.uint32)
        rc = lib.hj_own_info(self._h, owner.ctypes.data, owner.size, counts.ctypes.data, counts.size, out)
        if rc == _lib.HJ_ERR_INVALID and (out[0] > owner.size or out[1] > counts.size):
            owner, counts = np.empty(int(out[0]), dtype=np.uint32), np.empty(int(out[1]), dtype=np.uint32)
            rc = lib.hj_own_info(self._h, owner.ctypes.data, owner.size, counts.ctypes.data, counts.size, out)
        self._check(rc)
        return owner[:int(out[0])], counts[:int(out[1])], int(out[2])

    def synchronize(self):
        self._check(lib.hj_synchronize(self._h))

    def export_table(self, tableSize):
        out = np.empty(tableSize, dtype=np.uint64)
        self._check(lib.hj_export_table(self._h, out.ctypes.data, tableSize))
        return out

    def export_buckets(self, numBuckets):
        """HTM table as the reference's Bucket structs: (buckets[numBuckets], overflows[1 + used]); overflows[0] is unused,
        nextIndex is 1-based (HTMHashBuild.hpp:41-45, 231-279)."""
        used = C.c_uint64(0)
        buckets = np.zeros(numBuckets, dtype=BUCKET_DTYPE)
        # first call learns the number of overflow buckets (no overflow buffer handed over), second one copies them
        rc = lib.hj_export_buckets(self._h, buckets.ctypes.data, numBuckets, None, 0, C.byref(used))
        if rc != _lib.HJ_OK and used.value == 0:
            self._check(rc)
        overflows = np.zeros(used.value + 1, dtype=BUCKET_DTYPE)
        self._check(lib.hj_export_buckets(self._h, buckets.ctypes.data, numBuckets, overflows.ctypes.data,
                                          overflows.size, C.byref(used)))
        return buckets, overflows

    # ---- raw device memory (hosts without a HIP runtime of their own) -------
    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        self._check(lib.hj_dev_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def dev_free(self, ptr):
        self._check(lib.hj_dev_free(self._h, C.c_void_p(ptr)))

    def copy_h2d(self, dst_ptr, src_np):
        src_np = np.ascontiguousarray(src_np)
        self._check(lib.hj_copy_h2d(self._h, C.c_void_p(dst_ptr), src_np.ctypes.data, src_np.nbytes))

    def copy_d2h(self, dst_np, src_ptr):
        self._check(lib.hj_copy_d2h(self._h, dst_np.ctypes.data, C.c_void_p(src_ptr), dst_np.nbytes))

    # ---- streaming Zipf generator (probe sides that do not fit one host buffer) -------------------------------
    def zipf_open(self, alphabet_size, theta, seed=0):
        self._check(lib.hj_zipf_open(self._h, alphabet_size, float(theta), int(seed)))

    def zipf_next(self, n, d_out):
        """the next n draws of the stream, as 8-byte tuples at device pointer d_out"""
        self._check(lib.hj_zipf_next_dev(self._h, n, C.c_void_p(d_out)))

    def zipf_close(self):
        self._check(lib.hj_zipf_close(self._h))

    def shard_histogram(self, d_in, n, n_shards, d_counts, mode=0):
        """mode = bit position of the radix digit (0 = low key bits), | SHARD_ONE_BASED for (key - 1)"""
        self._check(lib.hj_shard_histogram_dev(self._h, C.c_void_p(d_in), n, n_shards, mode, C.c_void_p(d_counts)))

    def shard_scatter(self, d_in, n, n_shards, d_counts, d_out_keys, mode=0):
        """tuples in, bare 32-bit keys out, grouped by destination in input order"""
        self._check(lib.hj_shard_scatter_dev(self._h, C.c_void_p(d_in), n, n_shards, mode, C.c_void_p(d_counts),
                                             C.c_void_p(d_out_keys)))

    def build_keys(self, d_keys, n, home_shift, table_size):
        self._check(lib.hj_build_keys_dev(self._h, C.c_void_p(d_keys), n, home_shift, table_size))

    def probe_keys(self, d_keys, n):
        self._check(lib.hj_probe_keys_dev(self._h, C.c_void_p(d_keys), n))

    def set_shard_check(self, n_shards, mode=0, shard_id=0):
        """later builds/probes also count tuples whose destination is another shard (result["foreignTuples"]); 0 = off"""
        self._check(lib.hj_set_shard_check(self._h, n_shards, mode, shard_id))


def _operator(algo, relR, rSize, relS, sSize, device, **kw):
    relR = np.asarray(relR, dtype=np.uint64)[:rSize]
    if relS is not None:
        relS = np.asarray(relS, dtype=np.uint64)[:sSize]
    with HashJoinContext(device) as ctx:
        r = ctx.run(algo, relR, relS, **kw)
    out = {"algo": algo, "rSize": r["rSize"], "probeLength": kw.get("probeLength", 4),
           "hashBuildTimeInMicroseconds": int(r["total_us"]), "conflicts": r["conflicts"]}
    if relS is not None:
        out["totalMatches"] = r["totalMatches"]
    out["inputSum"] = r["inputSum"]
    out["outputSum"] = r["outputSum"]
    out["detail"] = r
    return out


def NoCCHashBuild(relR, rSize, relS=None, sSize=0, scaleOutput=2, numPartitions=64, probeLength=4, device=0):
    """NoCCHashBuild.hpp:13-19. outputSum keeps the [0, rSize) quirk of :94."""
    return _operator("nocc", relR, rSize, relS, sSize, device, scaleOutput=scaleOutput,
                     numPartitions=numPartitions, probeLength=probeLength)


def AtomicHashBuild(relR, rSize, relS=None, sSize=0, scaleOutput=2, numPartitions=64, probeLength=4, device=0):
    """AtomicHashBuild.hpp:14-20."""
    return _operator("atomic", relR, rSize, relS, sSize, device, scaleOutput=scaleOutput,
                     numPartitions=numPartitions, probeLength=probeLength)


def HTMHashBuild(relR, rSize, relS=None, sSize=0, transactionSize=16, scaleOutput=2, numPartitions=64,
                 probeLength=4, device=0):
    """HTMHashBuild.hpp:54-60: the bucketised table (three tuples per 32-byte bucket, bucket = (key/3) & mask, conflicts
    chained into overflow buckets). The TSX transaction groups are replaced outright by the index-priority fill, so
    there are no aborted transactions to report (failedTransactions = 0); transactionSize is accepted and echoed. Returns
    the reference's JSON fields (:417-452) in its order."""
    relR = np.asarray(relR, dtype=np.uint64)[:rSize]
    if relS is not None:
        relS = np.asarray(relS, dtype=np.uint64)[:sSize]
    with HashJoinContext(device) as ctx:
        r = ctx.run("htm", relR, relS, scaleOutput=scaleOutput, numPartitions=numPartitions, probeLength=probeLength,
                    transactionSize=transactionSize)
    out = {"algo": "htm", "rSize": r["rSize"], "transactionSize": transactionSize, "probeLength": probeLength,
           "hashBuildTimeInMicroseconds": int(r["total_us"]), "firstRoundTime": 0, "firstRoundFailureFraction": 0.0,
           "conflictCount": r["conflicts"], "failedTransactions": 0, "failedTransactionPercentage": 0.0,
           "totalFailedPercentage": r["conflicts"] / max(r["rSize"], 1)}
    if relS is not None:
        out["totalMatches"] = r["totalMatches"]
    out["inputSum"] = r["inputSum"]
    out["outputSum"] = r["outputSum"]
    out["detail"] = r
    return out


def PRO(
relR, relS=None, nthreads=0, radixBits=0, device=0):
    """mc/src/parallel_radix_join.c:1305 (algos[] entry, mc/src/main.c:292-301).
    Returns the join cardinality and the fork's printed checksum ("Results")."""
    relR = np.asarray(relR, dtype=np.uint64)
    if relS is not None:
        relS = np.asarray(relS, dtype=np.uint64)
    with HashJoinContext(device) as ctx:
        r = ctx.run("prj", relR, relS, radixBits=radixBits)
    return {"algo": "PRO", "matches": r["totalMatches"], "results": r["prjChecksum"],
            "radixBits": r["radixBits"], "detail": r}
