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
"""
import ctypes as C
import functools

import numpy as np

from . import _lib
from ._lib import lib, hj_params, hj_result


# struct Bucket, HTMHashBuild.hpp:41-45 (32 bytes)
BUCKET_DTYPE = np.dtype([("tuples", np.uint64, 3), ("count", np.uint32), ("nextIndex", np.uint32)])

# HJ_NO_ROW: the R row of a left-outer row whose S tuple has no match
NO_ROW = _lib.HJ_NO_ROW


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


def _where_terms_arr(terms):
    """[(s_ptr, r_ptr, width, type, op, s_valid, r_valid)], the two planes optional (0) -> (hj_where_term array, its length)"""
    terms = [tuple(t) + (0,) * (7 - len(t)) for t in terms]
    arr = (_lib.hj_where_term * max(len(terms), 1))()
    for a, (s, r, width, type_, op, s_valid, r_valid) in zip(arr, terms):
        a.s, a.r, a.sValid, a.rValid = (p or None for p in (s, r, s_valid, r_valid))
        a.width, a.type, a.op, a.reserved = width, type_, op, 0
    return arr, len(terms)


def _asof_term_arr(term):
    """(s_ptr, r_ptr, width, type, op, s_valid, r_valid), the two planes optional (0) -> one hj_asof_term"""
    s, r, width, type_, op, s_valid, r_valid = tuple(term) + (0,) * (7 - len(term))
    a = _lib.hj_asof_term()
    a.s, a.r, a.sValid, a.rValid = (p or None for p in (s, r, s_valid, r_valid))
    a.width, a.type, a.op, a.reserved = width, type_, op, 0
    return a


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
        self._check(lib.hj_probe_join_dev(self._h, kind, C.c_void_p(dS_ptr) if dS_ptr else None, sSize, s_idx_base,
                                          C.c_void_p(d_out_s) if d_out_s else None,
                                          C.c_void_p(d_out_r) if d_out_r else None, capacity))

    def pairs_info(self):
        """hj_pairs_info (waits for the stream): (rows the last probe_pairs / prj_probe_pairs found, rows it wrote, its
        device time in microseconds, its S tuples without a match for a kind other than inner -- 0 after an inner call)."""
        out = (C.c_uint64 * 4)()
        self._check(lib.hj_pairs_info(self._h, out))
        return tuple(int(x) for x in out)

    # ---- R-side match marks (reserve(..., trackRMatches=True)) ----------------
    def r_rows(self, which, d_out_r, capacity):
        """hj_r_rows_dev: the R rows of the last build that no inner / left probe since has produced (which = 0,
        HJ_R_UNMATCHED) or that one has (1, HJ_R_MATCHED), ascending, into the device uint32 array d_out_r of `capacity`
        entries; rows beyond it are counted, not written (capacity 0, d_out_r 0: count only). Changes no mark."""
        self._check(lib.hj_r_rows_dev(self._h, which, C.c_void_p(d_out_r) if d_out_r else None, capacity))

    def r_rows_info(self):
        """hj_r_rows_info (waits for the stream): (rows the last r_rows produced, rows it wrote, its device time in
        microseconds, R rows of the build)."""
        out = (C.c_uint64 * 4)()
        self._check(lib.hj_r_rows_info(self._h, out))
        return tuple(int(x) for x in out)

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
        self._check(lib.hj_gather_dev(self._h, C.c_void_p(d_map) if d_map else None, n_rows, row_base, src_rows,
                                      arr if cols else None, len(cols), C.c_void_p(d_valid) if d_valid else None))

    def gather_info(self):
        """hj_gather_info (waits for the stream): (rows of the last gather, its NULL rows, its device time in
        microseconds, its out-of-range entries); all 0 before the first one."""
        out = (C.c_uint64 * 4)()
        self._check(lib.hj_gather_info(self._h, out))
        return tuple(int(x) for x in out)

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
        self._check(lib.hj_gather2_dev(self._h, C.c_void_p(d_map) if d_map else None, n_rows, row_base, src_rows,
                                       arr if cols else None, len(cols), C.c_void_p(d_valid) if d_valid else None))

    def gather2_info(self):
        """hj_gather2_info (waits for the stream): (rows of the last gather2, its NULL rows, its device time in
        microseconds, its out-of-range entries, then per column the bytes its rows take -- exact in 64 bits, 0 for a fixed
        column; above 2^32 - 1 the column was not written); all 0 before the first one. gather_info() reports gather()
        alone, and the other way round."""
        out = (C.c_uint64 * (4 + _lib.HJ_GATHER_MAX_COLS))()
        self._check(lib.hj_gather2_info(self._h, out))
        return tuple(int(x) for x in out)

    # ---- joins on real key columns: hash, candidate join, verify ---------------
    def key_hash(self, cols, side, n_rows, d_out, key_mask=0):
        """hj_key_hash_dev: d_out[i] = the 32-bit join word of row i < n_rows as an 8-byte tuple (what prj_build and
        prj_probe_pairs take), hashed from the key columns cols = 1 to HJ_KEY_MAX_COLS tuples (s_ptr, r_ptr, width) of
        device pointers, width 1, 2, 4, 8 or 16 bytes; side (HJ_KEY_SIDE_S / HJ_KEY_SIDE_R) says which pointers are read,
        the others may be 0. The hash is MurmurHash3_x86_32 over the row's columns (include/htm_hashjoin.h), & key_mask
        (0: all 32 bits). Asynchronous; needs no reserve and no table."""
        arr, n = _key_cols(cols)
        self._check(lib.hj_key_hash_dev(self._h, arr, n, side, n_rows, key_mask, C.c_void_p(d_out) if d_out else None))

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
        p = lambda d: C.c_void_p(d) if d else None       # noqa: E731
        self._check(lib.hj_pairs_verify_dev(self._h, p(d_map_s), p(d_map_r), n_pairs, s_row_base, s_rows, r_rows, arr, n,
                                            p(d_out_s), p(d_out_r), capacity, p(d_s_marks), p(d_r_marks)))

    def key_hash2(self, cols, side, n_rows, d_out, key_mask=0):
        """hj_key_hash2_dev: key_hash on key columns in the Arrow layout. cols = 1 to HJ_KEY_MAX_COLS tuples (s_ptr,
        r_ptr, width, s_offsets, r_offsets, s_valid, r_valid, flags) of device pointers, whatever follows the width
        optional (0). A fixed column has width 1, 2, 4, 8 or 16 and no offsets; a variable-length one width 0, the bytes
        buffer as its pointer and n_rows + 1 uint32 offsets into it. s_valid / r_valid: the validity plane of that side
        (uint32 words, bit i & 31 of word i >> 5, 1 = valid; 0: no NULLs). flags: HJ_KEY_NULLS_EQUAL or 0. The hash and
        the word of a NULL-keyed row: include/htm_hashjoin.h. Asynchronous; needs no reserve and no table."""
        arr, n = _key_cols2(cols)
        self._check(lib.hj_key_hash2_dev(self._h, arr, n, side, n_rows, key_mask, C.c_void_p(d_out) if d_out else None))

    def pairs_verify2(self, d_map_s, d_map_r, n_pairs, s_row_base, s_rows, r_rows, cols, d_out_s, d_out_r, capacity,
                      d_s_marks=0, d_r_marks=0):
        """hj_pairs_verify2_dev: pairs_verify on key columns in the Arrow layout (cols as in key_hash2, both sides of
        every column in use; the S side's offsets and validity are indexed by the S row with s_row_base off, like its
        column). A column is equal when -- either element NULL: both are and the column has HJ_KEY_NULLS_EQUAL;
        otherwise fixed width: bytewise; otherwise: the same length and the same bytes. Outputs, marks, dropped
        candidates and aliasing as in pairs_verify; verify_info reports the last call of either."""
        arr, n = _key_cols2(cols)
        p = lambda d: C.c_void_p(d) if d else None       # noqa: E731
        self._check(lib.hj_pairs_verify2_dev(self._h, p(d_map_s), p(d_map_r), n_pairs, s_row_base, s_rows, r_rows, arr, n,
                                             p(d_out_s), p(d_out_r), capacity, p(d_s_marks), p(d_r_marks)))

    def verify_info(self):
        """hj_verify_info (waits for the stream): (pairs the last pairs_verify kept, pairs it wrote, its device time in
        microseconds, candidates it dropped as NO_ROW or out of range); rejected = n_pairs - kept - dropped."""
        out = (C.c_uint64 * 4)()
        self._check(lib.hj_verify_info(self._h, out))
        return tuple(int(x) for x in out)

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
        p = lambda d: C.c_void_p(d) if d else None       # noqa: E731
        self._check(lib.hj_key_groups_dev(self._h, arr, n, side, n_rows, key_mask, p(d_rep), p(d_group), p(d_first_rows), capacity))

    def key_groups_info(self):
        """hj_key_groups_info (waits for the stream), about the last key_groups: groups, first rows written, the device time
        of the call in microseconds, NULL-keyed rows, table slots, probe steps beyond the home slot, key compares that found
        a different key (word collisions), the device-side failure word (0 on success)."""
        out = (C.c_uint64 * 8)()
        self._check(lib.hj_key_groups_info(self._h, out))
        return dict(zip(_KEY_GROUPS_INFO, (int(x) for x in out)))

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
        arr, n = _where_terms_arr(terms)
        p = lambda d: C.c_void_p(d) if d else None       # noqa: E731
        self._check(lib.hj_pairs_where_dev(self._h, p(d_map_s), p(d_map_r), n_pairs, s_row_base, s_rows, r_rows, arr, n,
                                           p(d_out_s), p(d_out_r), capacity, p(d_s_marks), p(d_r_marks)))

    def where_info(self):
        """hj_where_info (waits for the stream): (pairs the last pairs_where kept, pairs it wrote, its device time in
        microseconds, pairs it dropped as NO_ROW or out of range); rejected = n_pairs - kept - dropped."""
        out = (C.c_uint64 * 4)()
        self._check(lib.hj_where_info(self._h, out))
        return tuple(int(x) for x in out)

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
        p = lambda d: C.c_void_p(d) if d else None       # noqa: E731
        self._check(lib.hj_pairs_asof_dev(self._h, p(d_map_s), p(d_map_r), n_pairs, s_row_base, s_rows, r_rows,
                                          C.byref(_asof_term_arr(term)), p(d_best_val), p(d_best_row), p(d_out_s), p(d_out_r),
                                          capacity, p(d_s_marks), p(d_r_marks)))

    def asof_info(self):
        """hj_asof_info (waits for the stream): (pairs the last pairs_asof kept, pairs it wrote, the device time of the whole
        call in microseconds, pairs it dropped as NO_ROW or out of range)."""
        out = (C.c_uint64 * 4)()
        self._check(lib.hj_asof_info(self._h, out))
        return tuple(int(x) for x in out)

    def mark_rows(self, d_marks, rows, row_base, which, d_out, capacity):
        """hj_mark_rows_dev: r_rows on a caller's plane. The rows row_base + i, i < rows, whose bit i of d_marks is clear
        (which = 0, HJ_R_UNMATCHED) or set (1, HJ_R_MATCHED), ascending, into the device uint32 array d_out of `capacity`
        entries; rows beyond it are counted, not written (capacity 0, d_out 0: count only). Changes no mark."""
        self._check(lib.hj_mark_rows_dev(self._h, C.c_void_p(d_marks) if d_marks else None, rows, row_base, which,
                                         C.c_void_p(d_out) if d_out else None, capacity))

    def mark_rows_info(self):
        """hj_mark_rows_info (waits for the stream): (rows the last mark_rows produced, rows it wrote, its device time in
        microseconds, the rows of its plane)."""
        out = (C.c_uint64 * 4)()
        self._check(lib.hj_mark_rows_info(self._h, out))
        return tuple(int(x) for x in out)

    def prj_join(self, dR_ptr, rSize, dS_ptr, sSize):
        self._check(lib.hj_prj_join_dev(self._h, C.c_void_p(dR_ptr), rSize,
                                        C.c_void_p(dS_ptr) if dS_ptr else None, sSize))

    # ---- PRJ with a resident R: partition R once, probe S slice by slice ----
    def prj_build(self, dR_ptr, rSize):
        """Radix-partitions dR once and keeps the partitions in the context (dR may be freed afterwards); resets the
        counters, prjChecksum = R's checksum. Sizing: reserve("prj" or "auto", rSize, largest slice)."""
        self._check(lib.hj_prj_build_dev(self._h, C.c_void_p(dR_ptr), rSize))

    def prj_probe(self, dS_ptr, sSize):
        """Partitions one S slice and joins it against the resident R; totalMatches and sSize add up over the slices."""
        self._check(lib.hj_prj_probe_dev(self._h, C.c_void_p(dS_ptr) if dS_ptr else None, sSize))

    def prj_probe_pairs(self, dS_ptr, sSize, d_out_s, d_out_r, capacity, s_idx_base=0, kind=0):
        """hj_prj_probe_join_dev: prj_probe with its result kept, against an R built after reserve("prj" or "auto", ...,
        keepRowIds=True). For every match one pair d_out_s[k] = s_idx_base + position in dS, d_out_r[k] = position of
        the R tuple in the relation given to prj_build (two device uint32 arrays of `capacity` entries; pairs beyond it
        are counted, not written). The complete equi-join on the key word. pairs_info() reports the call.
        kind (HJ_JOIN_*): as in probe_pairs."""
        self._check(lib.hj_prj_probe_join_dev(self._h, kind, C.c_void_p(dS_ptr) if dS_ptr else None, sSize, s_idx_base,
                                              C.c_void_p(d_out_s) if d_out_s else None,
                                              C.c_void_p(d_out_r) if d_out_r else None, capacity))

    def prj_resident_info(self):
        """hj_prj_resident_info (waits for the stream): R's and the last slice's partitioning path, the last probe's join
        work items, its partitions split over several items, its largest S partition, bytes held for R."""
        out = (C.c_uint64 * 8)()
        self._check(lib.hj_prj_resident_info(self._h, out))
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
        self._check(lib.hj_prj_probe_agg_dev(self._h, C.c_void_p(dS_ptr) if dS_ptr else None, sSize, arr, len(srcs)))

    def prj_agg_rows(self, d_outs, d_count=0):
        """hj_prj_agg_rows_dev: the accumulators by R row. d_outs: one device pointer per column of the begin, each a plane
        of rSize 8-byte entries; d_count (0: none): the same for the match counts. Every R row is written once; the
        accumulators stay as they are."""
        d_outs = list(d_outs)
        arr = (C.c_void_p * max(len(d_outs), 1))(*[C.c_void_p(p) if p else None for p in d_outs])
        self._check(lib.hj_prj_agg_rows_dev(self._h, arr if d_outs else None, C.c_void_p(d_count) if d_count else None))

    def prj_agg_info(self):
        """hj_prj_agg_info (waits for the stream): the matches of the last prj_probe_agg, its device time in microseconds,
        the columns of the aggregation, the probes since prj_agg_begin, the R tuples its planes hold."""
        out = (C.c_uint64 * 8)()
        self._check(lib.hj_prj_agg_info(self._h, out))
        return {"matches": int(out[0]), "us": int(out[1]), "nCols": int(out[2]), "probes": int(out[3]), "rows": int(out[4])}

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
        p = lambda d: C.c_void_p(d) if d else None       # noqa: E731
        self._check(lib.hj_pairs_agg_dev(self._h, p(d_map_g), p(d_map_v), n_pairs, g_base, g_rows, v_base, v_rows,
                                         arr if cols else None, len(cols), p(d_count)))

    def pairs_agg_info(self):
        """hj_pairs_agg_info (waits for the stream): (pairs of the last pairs_agg, pairs it applied, its device time in
        microseconds, pairs it skipped as NO_ROW or out of range)."""
        out = (C.c_uint64 * 4)()
        self._check(lib.hj_pairs_agg_info(self._h, out))
        return tuple(int(x) for x in out)

    def join(self, dR_ptr, rSize, dS_ptr, sSize):
        """Build + probe by the reserved algo; "auto" samples R for locality and picks atomic or prj."""
        self._check(lib.hj_join_dev(self._h, C.c_void_p(dR_ptr), rSize,
                                    C.c_void_p(dS_ptr) if dS_ptr else None, sSize))

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
        out = (C.c_uint64 * 4)()
        self._check(lib.hj_wave_planar_info(self._h, out))
        return {"planar": bool(out[0]), "planarFallback": int(out[1]), "tableFormat": int(out[2])}

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
        out = (C.c_uint64 * 6)()
        self._check(lib.hj_table_debug(self._h, out))
        return {"validLo": int(out[0]), "validHiEx": int(out[1]), "tableFormat": int(out[2]), "tableSlots": int(out[3]),
                "tableAddr": int(out[4]), "tableBytes": int(out[5])}

    def htm_chain_layout_info(self, n):
        """hj_htm_chain_layout_info for this context's device (see engine.htm_chain_layout_info)."""
        return _htm_chain_layout(self._h, 0, n)

    def htm_chain_info(self):
        """hj_htm_chain_info (waits for the stream): state 0 = the last htm build did not try the LDS chain phase, 1 = it
        held, 2 = it handed over (compactFallback bit 8); cause = the mask of why (a non-empty subset of the causes the
        input holds); groups = overflow buckets the parts asked for where it held."""
        out = (C.c_uint64 * 4)()
        self._check(lib.hj_htm_chain_info(self._h, out))
        return {"state": int(out[0]), "cause": int(out[1]), "groups": int(out[2])}

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


def _join_kind(fn, how):
    if how not in _lib.JOIN_KINDS:
        raise ValueError(f"{fn}: how must be inner, left, semi or anti, not {how!r}")
    return _lib.JOIN_KINDS[how]


def _join_without_device(kind, n_r, n_s):
    """the gather maps of a join with an empty side (None: the inputs need the device): no S, no rows; no R, every S row
    is unmatched"""
    if n_r and n_s:
        return None
    keeps = n_s if kind in (_lib.HJ_JOIN_LEFT, _lib.HJ_JOIN_ANTI) else 0
    s_idx = np.arange(keeps, dtype=np.uint32)
    return s_idx, (np.full(keeps, NO_ROW, dtype=np.uint32) if kind <= _lib.HJ_JOIN_LEFT else None)


class _Held:
    """device allocations of one wrapper call: alloc / free as it goes, close frees what is left"""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def alloc(self, nbytes):
        self.ptrs.append(self.ctx.dev_alloc(max(int(nbytes), 4)))
        return self.ptrs[-1]

    def put(self, a):
        d = self.alloc(a.nbytes)
        if a.nbytes:
            self.ctx.copy_h2d(d, a)
        return d

    def free(self, *ptrs):
        for p in ptrs:
            self.ptrs.remove(p)
            self.ctx.dev_free(p)

    def close(self):
        for p in self.ptrs:
            self.ctx.dev_free(p)
        self.ptrs = []


def _fetch_map(ctx, d_map, n):
    idx = np.empty(n, dtype=np.uint32)
    if n:
        ctx.copy_d2h(idx, d_map)
    return idx



def _drive_join(relR, relS, path, kind, which, step, on_maps, device, probeLength=4, radixBits=0, fill=None, after=None):
    """The host sequence of every materialising wrapper, once: reserve, upload R, build, then relS in slices of `step`
    tuples -- upload, probe, hand the slice's maps to on_maps -- then the counters and the sweep of the R marks.
    path: "htm" | "atomic" | "nocc", the table probes (step = len(relS): all of S in one call from row 0; the fetch at
    the end raises HJ_ERR_KEY_RANGE for R tuples outside the DataGen layout, as the operators do), or "radix", the
    resident radix join on the key word.
    kind: the hj_join_kind of the probes; None: mark-only passes (INNER, capacity 0, NULL planes).
    which: HJ_R_UNMATCHED / HJ_R_MATCHED, the R rows swept after the probes (the context tracks R's matches), or None.
    Sizing: the planes start with `step` entries each (exact for a foreign-key join); a slice whose probe reports more
    rows gets planes of the reported count and is probed once more.
    on_maps(ctx, held, lo, n_s, d_s, d_r, rows): the device maps of the `rows` rows of the slice relS[lo:lo + n_s] (d_r
    is 0 for a kind without an R plane); after the probes once more with lo None and d_s 0, d_r being the sweep's map.
    The maps are valid until on_maps returns; what it allocates from `held` and does not free lives to the end.
    fill(ctx, held, d_tuples, lo, n) (join_on): the tuples are made on the device instead of copied there -- all n of R's
    with lo None, right after the reserve, then those of the slice relS[lo:lo + n] before its probe; relR and relS are
    then read for their lengths alone. after(ctx, held): runs behind the last slice, the context still open."""
    radix = path == "radix"
    plane_r = kind is not None and kind <= _lib.HJ_JOIN_LEFT
    with HashJoinContext(device) as ctx:
        held = _Held(ctx)
        try:
            ctx.reserve("prj" if radix else path, relR.size, step, probeLength=probeLength, radixBits=radixBits,
                        keepRowIds=True, trackRMatches=which is not None)
            if fill is None:
                dR = held.put(relR)
            else:
                dR = held.alloc(8 * relR.size)
                fill(ctx, held, dR, None, relR.size)
            if radix:
                ctx.prj_build(dR, relR.size)
            else:
                ctx.build(dR, relR.size)
            probe = ctx.prj_probe_pairs if radix else ctx.probe_pairs
            dS = held.alloc(8 * step)
            capacity = step if kind is not None else 0
            d_s, d_r = (held.alloc(4 * capacity), held.alloc(4 * capacity) if plane_r else 0) if capacity else (0, 0)
            for lo in range(0, relS.size, step):
                part = relS[lo:lo + step]
                if fill is None:
                    ctx.copy_h2d(dS, part)
                else:
                    fill(ctx, held, dS, lo, part.size)
                probe(dS, part.size, d_s, d_r, capacity, s_idx_base=lo, kind=kind or 0)
                if kind is None:
                    continue
                found, written = ctx.pairs_info()[:2]
                if found > capacity:
                    held.free(*(p for p in (d_s, d_r) if p))
                    capacity = found
                    d_s, d_r = held.alloc(4 * capacity), (held.alloc(4 * capacity) if plane_r else 0)
                    probe(dS, part.size, d_s, d_r, capacity, s_idx_base=lo, kind=kind)
                    found, written = ctx.pairs_info()[:2]
                on_maps(ctx, held, lo, part.size, d_s, d_r, written)
            if not radix:
                ctx.fetch()
            if which is not None:
                d_rows = held.alloc(4 * relR.size)
                ctx.r_rows(which, d_rows, relR.size)
                on_maps(ctx, held, None, 0, 0, d_rows, ctx.r_rows_info()[1])
            if after is not None:
                after(ctx, held)
        finally:
            held.close()


def _join_maps(relR, relS, path, kind, which, step, device, **kw):
    """_drive_join with every map copied to the host: ([S maps], [R maps]), one per slice, the sweep's map the last of R's"""
    s_parts, r_parts = [], []

    def to_host(ctx, held, lo, n_s, d_s, d_r, rows):
        if d_s:
            s_parts.append(_fetch_map(ctx, d_s, rows))
        if d_r:
            r_parts.append(_fetch_map(ctx, d_r, rows))

    _drive_join(relR, relS, path, kind, which, step, to_host, device, **kw)
    return s_parts, r_parts


def _slice_step(fn, n_s, slice_tuples):
    step = n_s if not slice_tuples else min(int(slice_tuples), n_s)
    if step < 1:
        raise ValueError(f"{fn}: slice_tuples must be positive, not {slice_tuples!r}")
    return step


def join_pairs(relR, relS, algo="htm", probeLength=4, device=0, how="inner"):
    """The join as two gather maps: (s_idx, r_idx), numpy uint32 arrays of equal length, row k of the result being
    (relS[s_idx[k]], relR[r_idx[k]]). The order of the rows is unspecified. algo = "htm" (the default): the complete
    equi-join, duplicate keys included, any len(relR). "atomic" / "nocc": the reference's budgeted open-addressing
    semantics (an R tuple that ran out of probeLength is not in the table, a walk ends at the first empty slot;
    len(relR) a power of two).
    Sizing: the outputs start with len(relS) entries each (exact for a foreign-key join); if the probe reports more
    pairs than that, they are enlarged to the reported count and the probe runs once more.
    how = "inner" | "left" | "semi" | "anti", relS being the preserved side: "left" adds one row (s, NO_ROW) for every S
    tuple without a match; "semi" / "anti" return the S rows with / without a match, once each, and r_idx is None."""
    if algo not in ("htm", "atomic", "nocc"):
        raise ValueError(f"join_pairs: algo must be htm, atomic or nocc, not {algo!r}")
    kind = _join_kind("join_pairs", how)
    relR = np.ascontiguousarray(relR, dtype=np.uint64)
    relS = np.ascontiguousarray(relS, dtype=np.uint64)
    trivial = _join_without_device(kind, relR.size, relS.size)
    if trivial is not None:
        return trivial
    s_parts, r_parts = _join_maps(relR, relS, algo, kind, None, relS.size, device, probeLength=probeLength)
    return np.concatenate(s_parts), (np.concatenate(r_parts) if r_parts else None)


def radix_join_pairs(relR, relS, radixBits=0, slice_tuples=None, device=0, how="inner"):
    """The complete equi-join on the key word (the low 32 bits of a tuple) through the resident radix join, as two gather
    maps like join_pairs: (s_idx, r_idx), numpy uint32 arrays, row k of the result being (relS[s_idx[k]], relR[r_idx[k]]),
    in no particular order. The path for a scattered or skewed relS. R is partitioned once with its row ids; relS is
    probed in slices of slice_tuples (default: all of it at once).
    Sizing, per slice, as in join_pairs: the outputs start with one entry per S tuple of the slice; if the probe reports
    more pairs than that, they are enlarged to the reported count and the slice is probed once more.
    how: as in join_pairs (r_idx is None for "semi" and "anti", and carries NO_ROW in the unmatched rows of "left")."""
    kind = _join_kind("radix_join_pairs", how)
    relR = np.ascontiguousarray(relR, dtype=np.uint64)
    relS = np.ascontiguousarray(relS, dtype=np.uint64)
    trivial = _join_without_device(kind, relR.size, relS.size)
    if trivial is not None:
        return trivial
    step = _slice_step("radix_join_pairs", relS.size, slice_tuples)
    s_parts, r_parts = _join_maps(relR, relS, "radix", kind, None, step, device, radixBits=radixBits)
    return np.concatenate(s_parts), (np.concatenate(r_parts) if r_parts else None)


# the R-preserving results: the kind of the probe calls (None: a mark-only pass, capacity 0) and which R rows follow
_OUTER_KINDS = {"right": (_lib.HJ_JOIN_INNER, _lib.HJ_R_UNMATCHED), "full": (_lib.HJ_JOIN_LEFT, _lib.HJ_R_UNMATCHED),
                "right_semi": (None, _lib.HJ_R_MATCHED), "right_anti": (None, _lib.HJ_R_UNMATCHED)}


def _outer_kind(fn, how):
    if not isinstance(how, str) or how not in _OUTER_KINDS:
        raise ValueError(f"{fn}: how must be right, full, right_semi or right_anti, not {how!r}")
    return _OUTER_KINDS[how]


def _outer_result(kind, s_parts, r_parts, r_only):
    """(s_idx, r_idx) of an R-preserving join: the probe's rows, then one (NO_ROW, r) row per R-only row; the rows alone
    for right_semi / right_anti"""
    if kind is None:
        return None, r_only
    return (np.concatenate(s_parts + [np.full(r_only.size, NO_ROW, dtype=np.uint32)]),
            np.concatenate(r_parts + [r_only]))


def _outer_without_device(kind, which, n_r, n_s):
    """an R-preserving join with an empty side (None: the inputs need the device). No S: no R row is matched. No R: the
    rows of the probe side alone."""
    if n_r and n_s:
        return None
    none = np.empty(0, dtype=np.uint32)
    s_idx, r_idx = (none, none) if kind is None else _join_without_device(kind, n_r, n_s)
    r_only = np.arange(n_r, dtype=np.uint32) if which == _lib.HJ_R_UNMATCHED else none
    return _outer_result(kind, [s_idx], [r_idx], r_only)


def outer_join_pairs(relR, relS, algo="htm", probeLength=4, device=0, how="right"):
    """The joins that preserve relR, the build side, as gather maps like join_pairs (same algo, same meaning of a match).
    how = "right": (s_idx, r_idx), the inner rows first, then one row (NO_ROW, r) for every R row no inner row names, r
    ascending. "full": the same with the left-outer rows in front (an S tuple without a match is (s, NO_ROW)).
    "right_semi" / "right_anti": (None, r_idx), the R rows some / no inner row names, ascending. With "atomic" / "nocc"
    an R tuple that ran out of probeLength is not in the table and therefore unmatched."""
    if algo not in ("htm", "atomic", "nocc"):
        raise ValueError(f"outer_join_pairs: algo must be htm, atomic or nocc, not {algo!r}")
    kind, which = _outer_kind("outer_join_pairs", how)
    relR = np.ascontiguousarray(relR, dtype=np.uint64)
    relS = np.ascontiguousarray(relS, dtype=np.uint64)
    trivial = _outer_without_device(kind, which, relR.size, relS.size)
    if trivial is not None:
        return trivial
    s_parts, r_parts = _join_maps(relR, relS, algo, kind, which, relS.size, device, probeLength=probeLength)
    return _outer_result(kind, s_parts, r_parts[:-1], r_parts[-1])


def radix_outer_join_pairs(relR, relS, radixBits=0, slice_tuples=None, device=0, how="right"):
    """outer_join_pairs through the resident radix join (the complete equi-join on the key word, as radix_join_pairs): R is
    partitioned once with its row ids, relS is probed in slices of slice_tuples, and the marks the slices leave on R's
    rows become the R-only rows at the end. how and the result as in outer_join_pairs."""
    kind, which = _outer_kind("radix_outer_join_pairs", how)
    relR = np.ascontiguousarray(relR, dtype=np.uint64)
    relS = np.ascontiguousarray(relS, dtype=np.uint64)
    trivial = _outer_without_device(kind, which, relR.size, relS.size)
    if trivial is not None:
        return trivial
    step = _slice_step("radix_outer_join_pairs", relS.size, slice_tuples)
    s_parts, r_parts = _join_maps(relR, relS, "radix", kind, which, step, device, radixBits=radixBits)
    return _outer_result(kind, s_parts, r_parts[:-1], r_parts[-1])


# ---- the joined rows themselves: payload columns through the maps, on the device --------------------------------------
_TABLE_HOWS = tuple(_lib.JOIN_KINDS) + tuple(_OUTER_KINDS)
_GATHER_WIDTHS = (1, 2, 4, 8, 16)


def _table_columns(fn, side, cols, n):
    """the payload columns of one side as {name: contiguous 1-D array, or KeyColumn}; ValueError for what the gather cannot take"""
    out = {}
    for name, col in (cols or {}).items():
        if isinstance(col, KeyColumn):
            if col.rows != n:
                raise ValueError(f"{fn}: {side} column {name!r} must have {n} rows, not {col.rows}")
            out[name] = col
            continue
        a = np.asarray(col)
        if a.ndim != 1 or a.shape[0] != n:
            raise ValueError(f"{fn}: {side} column {name!r} must be 1-D with {n} elements, not shape {a.shape}")
        if a.dtype.itemsize not in _GATHER_WIDTHS:
            raise ValueError(f"{fn}: {side} column {name!r} has {a.dtype.itemsize}-byte elements; 1, 2, 4, 8 or 16 can be gathered")
        out[name] = np.ascontiguousarray(a)
    return out


def _slice_bytes(c, n, step):
    """the most bytes a slice of `step` rows of the KeyColumn c, of n rows, takes"""
    if c.offsets is None:
        return step * c.width
    los = np.arange(0, n, step)
    return int((c.offsets[np.minimum(los + step, n)].astype(np.int64) - c.offsets[los]).max()) if los.size else 0


def _take_key_column(col, idx):
    """the rows idx of a KeyColumn, on the host: NO_ROW gives a NULL (fixed: all-zero bytes; variable length: empty)"""
    valid = idx != NO_ROW
    if col.valid is not None:
        valid[valid] = col.valid[idx[valid]]
    src = idx[valid].astype(np.int64)
    if col.offsets is None:
        values = np.zeros(idx.size, dtype=col.values.dtype)
        values[valid] = col.values[src]
        return KeyColumn(values, None if valid.all() else valid, col.nulls_equal)
    off = col.offsets.astype(np.int64)
    lens = np.zeros(idx.size, dtype=np.int64)
    lens[valid] = off[src + 1] - off[src]
    data = np.concatenate([col.values[off[i]:off[i + 1]] for i in src]) if src.size else np.empty(0, dtype=np.uint8)
    return KeyColumn.varlen(np.concatenate([[0], np.cumsum(lens)]), data, None if valid.all() else valid, col.nulls_equal)


def _concat_key_columns(parts, like):
    """the KeyColumns of the calls of one side, one behind the other; `like`: the source column (its kind, for no part at all)"""
    valid = np.concatenate([np.ones(0, dtype=bool)] + [p.valid if p.valid is not None else np.ones(p.rows, dtype=bool) for p in parts])
    valid = None if valid.all() else valid
    if like.offsets is None:
        return KeyColumn(np.concatenate([np.empty(0, dtype=like.values.dtype)] + [p.values for p in parts]), valid, like.nulls_equal)
    data, offsets, base = [np.empty(0, dtype=np.uint8)], [np.zeros(1, dtype=np.int64)], 0
    for p in parts:
        off = p.offsets.astype(np.int64)
        data.append(p.values[off[0]:off[-1]])
        offsets.append(off[1:] - off[0] + base)
        base += int(off[-1] - off[0])
    return KeyColumn.varlen(np.concatenate(offsets), np.concatenate(data), valid, like.nulls_equal)


def _take_on_host(cols, idx):
    """a side of a join that needed no device (an input is empty, so idx is all rows in order or all NO_ROW)"""
    valid = idx != NO_ROW
    out = {}
    for name, col in cols.items():
        if isinstance(col, KeyColumn):
            out[name] = _take_key_column(col, idx)
            continue
        out[name] = np.zeros(idx.size, dtype=col.dtype)
        out[name][valid] = col[idx[valid]]
    return out, valid


def _put_parts(ctx, held, parts, room=None):
    """what KeyColumn.take gave -- (values or bytes, offsets, validity words) -- to the device: into fresh allocations, or
    into `room`, three device pointers kept for a slice (0 where the column has no such part). A bytes buffer goes up in
    whole 32-bit words: the kernels read the aligned words of an element."""
    if room is None:
        room = tuple(held.alloc(a.nbytes + 3 & ~3) if a is not None else 0 for a in parts)
    for d, a in zip(room, parts):
        if a is not None and a.nbytes:
            ctx.copy_h2d(d, np.ascontiguousarray(a))
    return room


def _gather_key_columns(ctx, held, d_map, n_rows, row_base, src_rows, k_cols):
    """The KeyColumn columns of one side through HashJoinContext.gather2: k_cols = [(name, (device values, offsets,
    validity words), the source KeyColumn)] -> {name: KeyColumn of n_rows rows}. Variable-length columns are gathered as a
    sizing call (dst_capacity 0) followed by the copy call."""
    out = {}
    if not n_rows:
        return {name: _take_key_column(col, np.empty(0, dtype=np.uint32)) for name, _, col in k_cols}
    words = (n_rows + 31) // 32
    for i in range(0, len(k_cols), _lib.HJ_GATHER_MAX_COLS):
        part, descs = k_cols[i:i + _lib.HJ_GATHER_MAX_COLS], []
        for name, (d_values, d_offsets, d_valid), col in part:
            d = {"src": d_values, "width": col.width, "src_valid": d_valid, "dst_valid": held.alloc(4 * words), "dst": 0}
            if col.width:
                d["dst"] = held.alloc(n_rows * col.width)
            else:
                d["src_offsets"], d["dst_offsets"] = d_offsets, held.alloc(4 * (n_rows + 1))
            descs.append(d)
        sized = [d for d in descs if not d["width"]]
        if sized:
            ctx.gather2(d_map, n_rows, src_rows, sized, row_base=row_base)
            for d, total in zip(sized, ctx.gather2_info()[4:]):
                if total > 0xFFFFFFFF:
                    raise HashJoinError(_lib.HJ_ERR_INVALID, f"a variable-length column's {n_rows} result rows take {total} bytes, above 2^32 - 1")
                d["dst_capacity"], d["dst"] = total, held.alloc(total) if total else 0
        ctx.gather2(d_map, n_rows, src_rows, descs, row_base=row_base)
        stray = ctx.gather2_info()[3]
        if stray:
            raise HashJoinError(_lib.HJ_ERR_STATE, f"{stray} map entries outside the {src_rows} source rows from {row_base}")
        for (name, _, col), d in zip(part, descs):
            bits = np.zeros(words, dtype=np.uint32)
            ctx.copy_d2h(bits, d["dst_valid"])
            valid = np.unpackbits(bits.view(np.uint8), bitorder="little")[:n_rows].astype(bool)
            valid = None if valid.all() else valid
            if col.width:
                values = np.empty(n_rows, dtype=col.values.dtype)
                ctx.copy_d2h(values, d["dst"])
                out[name] = KeyColumn(values, valid, col.nulls_equal)
            else:
                offsets, data = np.empty(n_rows + 1, dtype=np.uint32), np.empty(d["dst_capacity"], dtype=np.uint8)
                ctx.copy_d2h(offsets, d["dst_offsets"])
                if data.size:
                    ctx.copy_d2h(data, d["dst"])
                out[name] = KeyColumn.varlen(offsets, data, valid, col.nulls_equal)
            held.free(*(d[k] for k in ("dst", "dst_offsets", "dst_valid") if d.get(k)))
    return out


def _gather_side(ctx, held, d_map, n_rows, row_base, src_rows, d_cols):
    """One side of n_rows result rows out of the device map d_map: d_cols = [(name, device source, dtype)] -> ({name:
    array}, valid). One gather call per HJ_GATHER_MAX_COLS columns, the validity plane with the first (alone when the
    side has no column). The library's own maps have no out-of-range entry: one is an error. A KeyColumn column -- (name,
    its three device parts, the KeyColumn) -- goes through _gather_key_columns behind the plain ones."""
    k_cols = [c for c in d_cols if isinstance(c[2], KeyColumn)]
    d_cols = [c for c in d_cols if not isinstance(c[2], KeyColumn)]
    out = {name: np.empty(n_rows, dtype=dt) for name, _, dt in d_cols}
    words = np.zeros((n_rows + 31) // 32, dtype=np.uint32)
    if n_rows:
        d_valid = held.alloc(words.nbytes)
        dsts = [held.alloc(n_rows * dt.itemsize) for _, _, dt in d_cols]
        calls = [(d_cols[i:i + _lib.HJ_GATHER_MAX_COLS], dsts[i:i + _lib.HJ_GATHER_MAX_COLS])
                 for i in range(0, len(d_cols), _lib.HJ_GATHER_MAX_COLS)] or [([], [])]
        for k, (part, part_dst) in enumerate(calls):
            ctx.gather(d_map, n_rows, src_rows, [(src, dst, dt.itemsize, 0) for (_, src, dt), dst in zip(part, part_dst)],
                       d_valid=0 if k else d_valid, row_base=row_base)
            stray = ctx.gather_info()[3]
            if stray:
                raise HashJoinError(_lib.HJ_ERR_STATE, f"{stray} map entries outside the {src_rows} source rows from {row_base}")
        ctx.copy_d2h(words, d_valid)
        for (name, _, _), dst in zip(d_cols, dsts):
            ctx.copy_d2h(out[name], dst)
        held.free(d_valid, *dsts)
    valid = np.unpackbits(words.view(np.uint8), bitorder="little")[:n_rows].astype(bool)
    out.update(_gather_key_columns(ctx, held, d_map, n_rows, row_base, src_rows, k_cols))
    return out, valid


def _concat_side(parts, cols):
    """[(columns, valid)] of the calls of one side -> (columns, valid)"""
    return ({name: _concat_key_columns([p[0][name] for p in parts], col) if isinstance(col, KeyColumn)
             else np.concatenate([p[0][name] for p in parts]) if parts else np.empty(0, dtype=col.dtype)
             for name, col in cols.items()},
            np.concatenate([p[1] for p in parts]) if parts else np.empty(0, dtype=bool))


class _TableRows:
    """The result of join_tables / join_on as it grows: every device map a call of add() is given is copied to the host
    for the result and feeds the gather of its side's payload columns where it lies."""

    def __init__(self, how, r_cols, s_cols, n_r, step, n_s=0):
        self.n_s = n_s
        self.outer = how in _OUTER_KINDS
        self.kind, self.which = _OUTER_KINDS[how] if self.outer else (_lib.JOIN_KINDS[how], None)
        self.plane_s = self.kind is not None                                # right_semi / right_anti: R rows alone
        self.plane_r = self.outer or self.kind <= _lib.HJ_JOIN_LEFT         # semi / anti: S rows alone
        self.r_cols, self.s_cols, self.n_r, self.step = r_cols, s_cols, n_r, step
        self.s_maps, self.r_maps, self.s_parts, self.r_parts, self.dev, self.s_lo = [], [], [], [], {}, None

    def result(self, s_idx, r_idx, s_side, r_side):
        return {"s_idx": s_idx, "r_idx": r_idx, "s": s_side[0] if self.plane_s else None, "r": r_side[0] if self.plane_r else None,
                "s_valid": s_side[1] if self.plane_s else None, "r_valid": r_side[1] if self.plane_r else None}

    def without_device(self, n_s):
        """the result of a join with an empty side; None: the inputs need the device"""
        trivial = (_outer_without_device(self.kind, self.which, self.n_r, n_s) if self.outer
                   else _join_without_device(self.kind, self.n_r, n_s))
        if trivial is None:
            return None
        s_idx, r_idx = trivial
        return self.result(s_idx, r_idx, _take_on_host(self.s_cols, s_idx) if self.plane_s else None,
                           _take_on_host(self.r_cols, r_idx) if self.plane_r else None)

    def add(self, ctx, held, lo, n_s, d_s, d_r, rows):
        """`rows` result rows: d_s their S rows out of the slice of n_s tuples from lo, d_r their R rows. The maps stay
        where the probe (or a sweep) left them and feed the gather there. A side the kind has a plane for and the rows
        have no map of (0) is NULL by construction: the S side of R-only rows, the R side of unmatched S rows."""
        if not self.dev:    # the first call: R's columns whole, room for a slice of S's
            self.dev["r"] = [(name, _put_parts(ctx, held, col.take(0, self.n_r)), col) if isinstance(col, KeyColumn)
                             else (name, held.put(col), col.dtype) for name, col in self.r_cols.items()] if self.plane_r else []
            self.dev["s"] = ([(name, self.slice_room(held, col), col) if isinstance(col, KeyColumn)
                              else (name, held.alloc(self.step * col.dtype.itemsize), col.dtype) for name, col in self.s_cols.items()]
                             if self.plane_s else [])
        for side, plane, d_map, maps, parts, cols in (("s", self.plane_s, d_s, self.s_maps, self.s_parts, self.s_cols),
                                                      ("r", self.plane_r, d_r, self.r_maps, self.r_parts, self.r_cols)):
            if not plane:
                continue
            if not d_map:
                maps.append(np.full(rows, NO_ROW, dtype=np.uint32))
                parts.append(_take_on_host(cols, maps[-1]))
                continue
            maps.append(_fetch_map(ctx, d_map, rows))
            if side == "r":
                parts.append(_gather_side(ctx, held, d_map, rows, 0, self.n_r, self.dev["r"]))
                continue
            if self.s_lo != lo:         # the slice's columns go up once, however many calls name rows of it
                for (name, d_col, kind) in self.dev["s"]:
                    if isinstance(kind, KeyColumn):
                        _put_parts(ctx, held, kind.take(lo, n_s), d_col)
                    else:
                        ctx.copy_h2d(d_col, self.s_cols[name][lo:lo + n_s])
                self.s_lo = lo
            parts.append(_gather_side(ctx, held, d_map, rows, lo, n_s, self.dev["s"]))

    def slice_room(self, held, col):
        """device room for the largest slice of the S-side KeyColumn col: (values or bytes, offsets, validity words)"""
        return (held.alloc(_slice_bytes(col, self.n_s, self.step) + 3 & ~3), held.alloc(4 * (self.step + 1)) if col.offsets is not None else 0,
                held.alloc(4 * ((self.step + 31) // 32)) if col.valid is not None else 0)

    def joined(self):
        return self.result(np.concatenate(self.s_maps) if self.plane_s else None, np.concatenate(self.r_maps) if self.plane_r else None,
                           _concat_side(self.s_parts, self.s_cols), _concat_side(self.r_parts, self.r_cols))


def _where_keyword(impl):
    """The keywords where= and asof= on a join: the decorated function keeps its parameters and, called with neither, runs as
    it is; a call with either goes to `impl`, the function of this module that takes the same arguments and the two."""
    def deco(fn):
        @functools.wraps(fn)
        def join(*args, where=None, asof=None, **kw):
            return fn(*args, **kw) if where is None and asof is None else globals()[impl](*args, where=where, asof=asof, **kw)
        return join
    return deco


@_where_keyword("_join_tables")
def join_tables(relR, relS, r_cols=None, s_cols=None, how="inner", path="htm", probeLength=4, radixBits=0, slice_tuples=None,
                device=0):
    """The joined rows: the key tuples relR / relS as join_pairs takes them, and payload columns of either side (r_cols /
    s_cols: {name: 1-D numpy array of len(rel) elements of 1, 2, 4, 8 or 16 bytes; structured dtypes welcome}) gathered
    through the join's maps on the device -- the maps go from the probe, or the sweep of the R marks, straight into
    HashJoinContext.gather and come to the host only as part of the result.
    how: inner | left | semi | anti (join_pairs) and right | full | right_semi | right_anti (outer_join_pairs).
    path: "htm" | "atomic" | "nocc", the table probes with their meaning of a match, or "radix", the resident radix join
    (radixBits; slice_tuples: relS and its columns are uploaded, probed and gathered in slices of that many tuples).
    Returns {"s_idx", "r_idx", "s", "r", "s_valid", "r_valid"}: the maps as the pairs wrappers give them, the gathered
    columns per side as {name: array of the input dtype} and one bool per row and side (False: the row has no tuple of
    that side, its columns are all-zero bytes). A side the kind has no plane for (R for semi / anti, S for right_semi /
    right_anti) is None in all three. For right / full the R-only rows follow the probe's rows, R ascending.
    where (keyword only): a condition on the matched pair beside the key's equality -- a sequence of 1 to HJ_WHERE_MAX_TERMS terms
    (s_values, op, r_values), op out of "==", "!=", "<", "<=", ">", ">=", the values 1-D numpy arrays of len(relS) / len(relR)
    elements (a numpy.ma.MaskedArray or a fixed-width KeyColumn brings NULLs) of one dtype out of uint8..uint64, int8..int64,
    float32, float64; there is no implicit cast. A pair is a match iff the keys are equal and every term holds; a term with
    a NULL on either side does not hold; floats compare as IEEE-754 (-0.0 == 0.0, a NaN is unordered). The condition
    belongs to the match: an S row whose pairs all fail it is an unmatched row of left / anti, and likewise R. The probe
    then gives the INNER pairs of the path, HashJoinContext.pairs_where keeps those that pass and marks their rows, and the
    kind follows from the kept pairs and the sweeps of the marks; the order of the rows is join_on's. None or an empty
    sequence: no condition.
    asof (keyword only): one term (s_values, op, r_values) with the values of a where term and op out of ">=", ">" (backward:
    the latest R row at or before / before the S value) and "<=", "<" (forward). A pair is then a match iff the keys are equal,
    every where term holds, and it is the AS-OF pair of its S row among such pairs: the one whose R value is the largest
    (backward) or smallest (forward) for which s op r holds -- a NULL or a NaN on either side never holds --, ties on the value
    going to the lowest R row. Every S row has at most one match; an S row without an eligible pair is an unmatched S row, an
    R row that wins no S row an unmatched R row, and all eight kinds follow (HashJoinContext.pairs_asof behind the condition
    step, which then keeps its pairs whatever the kind and marks nothing).
    Every path joins on one 32-bit word of a tuple; for a 64-bit key, a key of several columns or a 16-byte key: join_on."""
    return _join_tables(relR, relS, r_cols, s_cols, how, path, probeLength, radixBits, slice_tuples, device)


def _join_tables(relR, relS, r_cols=None, s_cols=None, how="inner", path="htm", probeLength=4, radixBits=0, slice_tuples=None,
                 device=0, where=None, asof=None):
    """join_tables, and join_tables with a condition or an as-of term (_where_keyword)"""
    fn = "join_tables"
    if not isinstance(how, str) or how not in _TABLE_HOWS:
        raise ValueError(f"{fn}: how must be one of {', '.join(_TABLE_HOWS)}, not {how!r}")
    if not isinstance(path, str) or path not in ("htm", "atomic", "nocc", "radix"):
        raise ValueError(f"{fn}: path must be htm, atomic, nocc or radix, not {path!r}")
    relR = np.ascontiguousarray(relR, dtype=np.uint64)
    relS = np.ascontiguousarray(relS, dtype=np.uint64)
    r_cols = _table_columns(fn, "R", r_cols, relR.size)
    s_cols = _table_columns(fn, "S", s_cols, relS.size)
    step = _slice_step(fn, relS.size, slice_tuples) if path == "radix" and relS.size else relS.size
    terms = _where_terms(fn, where, relS.size, relR.size)
    best = _asof_term(fn, asof, relS.size, relR.size)
    rows = _TableRows(how, r_cols, s_cols, relR.size, step, relS.size)
    trivial = rows.without_device(relS.size)
    if trivial is not None:
        return trivial
    if terms is not None or best is not None:
        # as in join_on: the probe is INNER whatever the kind, and the context's own R marks stay out of it -- a pair that
        # the condition rejects would have set them
        cond = _pair_steps(terms, best, rows, relR.size, relS.size, step)
        _drive_join(relR, relS, path, _lib.HJ_JOIN_INNER, None, step, cond.slice, device, probeLength=probeLength, radixBits=radixBits,
                    after=cond.r_only)
        return rows.joined()
    _drive_join(relR, relS, path, rows.kind, rows.which, step, rows.add, device, probeLength=probeLength, radixBits=radixBits)
    return rows.joined()


# ---- joins on real key columns: hash, candidate join, verify -------------------------------------------------------------
def _key_columns(fn, side, keys):
    """the key columns of one side as a list of contiguous 1-D arrays; ValueError for what the hash cannot take"""
    cols = [keys] if isinstance(keys, np.ndarray) else [np.asarray(k) for k in keys]
    if not 1 <= len(cols) <= _lib.HJ_KEY_MAX_COLS:
        raise ValueError(f"{fn}: {side} has {len(cols)} key columns; 1 to {_lib.HJ_KEY_MAX_COLS} can be joined on")
    for a in cols:
        if a.ndim != 1 or a.shape[0] != cols[0].shape[0]:
            raise ValueError(f"{fn}: the key columns of {side} must be 1-D and of one length, not shape {a.shape}")
        if a.dtype.itemsize not in _GATHER_WIDTHS:
            raise ValueError(f"{fn}: a key column of {side} has {a.dtype.itemsize}-byte elements; 1, 2, 4, 8 or 16 can be joined on")
    return [np.ascontiguousarray(a) for a in cols]


def _aligned(a):
    """a, or a copy of it whose first element lies at a multiple of the itemsize (the C ABI's rule for a column)"""
    width = a.dtype.itemsize
    if a.ctypes.data % width == 0:
        return a
    raw = np.empty(a.nbytes + width, dtype=np.uint8)
    off = -raw.ctypes.data % width
    out = raw[off:off + a.nbytes].view(a.dtype)
    out[...] = a
    return out


def key_hash_host(cols, key_mask=0):
    """hj_key_hash_host: the 32-bit join word of every row of the key columns `cols` (one 1-D numpy array, or a sequence of
    1 to HJ_KEY_MAX_COLS of them, elements of 1, 2, 4, 8 or 16 bytes) as a numpy uint64 array -- the tuples
    HashJoinContext.key_hash writes for the same columns on the device, computed by the same code on the host. The hash
    is MurmurHash3_x86_32 with seed 0 over the row's columns in order (include/htm_hashjoin.h), & key_mask (0: all 32
    bits). Needs no device."""
    cols = [_aligned(a) for a in _key_columns("key_hash_host", "cols", cols)]
    out = np.empty(cols[0].size, dtype=np.uint64)
    arr, n = _key_cols([(a.ctypes.data, 0, a.dtype.itemsize) for a in cols])
    rc = lib.hj_key_hash_host(arr, n, _lib.HJ_KEY_SIDE_S, out.size, int(key_mask), out.ctypes.data)
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, "hj_key_hash_host")
    return out


# which rows of the slice's S plane a kind adds to the kept pairs (left, full) or returns (semi, anti)
_ON_S_SWEEP = {_lib.HJ_JOIN_LEFT: _lib.HJ_R_UNMATCHED, _lib.HJ_JOIN_SEMI: _lib.HJ_R_MATCHED, _lib.HJ_JOIN_ANTI: _lib.HJ_R_UNMATCHED}


@_where_keyword("_join_on_arrays")
def join_on(r_keys, s_keys, r_cols=None, s_cols=None, how="inner", radixBits=0, slice_tuples=None, device=0, key_mask=0):
    """join_tables for keys that are not one 32-bit word: r_keys / s_keys are each one 1-D numpy array or a sequence of 1
    to HJ_KEY_MAX_COLS of them (all of a side of one length; column c of both sides of the same itemsize out of 1, 2, 4,
    8, 16 bytes -- 64-bit integers, several columns, 16-byte structured elements), and two rows match when every key
    column is BYTEWISE equal. For float keys that means -0.0 != 0.0, and a NaN equals the same NaN bit pattern.
    The method is hash, candidate join, verify, all on the device: the key columns are hashed to a 32-bit join word
    (HashJoinContext.key_hash), the resident radix join gives the candidate pairs on that word, pairs_verify compares
    the real key bytes of every candidate and marks the S and R rows of the pairs it keeps, and the kind follows from the
    kept pairs and the sweeps of those marks (mark_rows). key_mask (0: none) keeps only those bits of the join word: more
    candidates, the same result -- for tests; the result never depends on the hash's quality.
    how, r_cols / s_cols, radixBits, slice_tuples and the result -- {"s_idx", "r_idx", "s", "r", "s_valid", "r_valid"} -- as
    in join_tables(path="radix"). Per slice, left and full give the kept pairs first, then the slice's unmatched S rows
    ascending; semi and anti give their S rows ascending; for right / full the R-only rows come last, R ascending.
    where (keyword only): as in join_tables -- a pair is a match iff the keys are equal and every term holds. The verify step then runs
    without mark planes and with its pairs kept whatever the kind, and HashJoinContext.pairs_where over those pairs sets the
    marks and keeps the pairs of the result.
    asof (keyword only): as in join_tables -- per S row the one pair with equal keys, every where term holding, whose R value is
    nearest on the permitted side. The verify step and the condition step then keep their pairs and mark nothing, and
    HashJoinContext.pairs_asof sets the marks and keeps the pairs of the result."""
    return _join_on_arrays(r_keys, s_keys, r_cols, s_cols, how, radixBits, slice_tuples, device, key_mask)


def _join_on_arrays(r_keys, s_keys, r_cols=None, s_cols=None, how="inner", radixBits=0, slice_tuples=None, device=0, key_mask=0, where=None,
                    asof=None):
    """join_on, and join_on with a condition (_where_keyword): its own checks, then the driver of join_on_columns on the
    arrays as plain KeyColumns"""
    fn = "join_on"
    if not isinstance(how, str) or how not in _TABLE_HOWS:
        raise ValueError(f"{fn}: how must be one of {', '.join(_TABLE_HOWS)}, not {how!r}")
    r_keys, s_keys = _key_columns(fn, "R", r_keys), _key_columns(fn, "S", s_keys)
    widths = [a.dtype.itemsize for a in r_keys]
    if widths != [a.dtype.itemsize for a in s_keys]:
        raise ValueError(f"{fn}: the key columns of R have {widths}-byte elements, those of S {[a.dtype.itemsize for a in s_keys]}")
    return _join_key_columns(fn, [KeyColumn(a) for a in r_keys], [KeyColumn(a) for a in s_keys], False, r_cols, s_cols, how, radixBits,
                             slice_tuples, device, key_mask, where, asof)


# ---- key columns in the Arrow layout: NULL keys and variable-length (string) keys ------------------------------------------
class KeyColumn:
    """One key column of join_on_columns / key_hash2_host in the Arrow layout: the values, an optional validity and, for
    variable-length elements, 32-bit offsets.
    KeyColumn(values, valid=None): a fixed-width column, values a 1-D numpy array of 1, 2, 4, 8 or 16-byte elements. A
    numpy.ma.MaskedArray brings its validity along (its mask inverted).
    KeyColumn.varlen(offsets, data, valid=None): element i is the bytes data[offsets[i]:offsets[i + 1]] (Arrow Binary /
    Utf8: len(offsets) = rows + 1, non-decreasing, offsets[0] need not be 0).
    KeyColumn.from_list(items): a variable-length column out of bytes, str (as UTF-8) and None (NULL).
    valid: one bool per row, False = NULL -- what join_tables / join_on return as s_valid / r_valid; None: no NULLs. The
    values under a NULL are never compared. nulls_equal: in this column a NULL equals a NULL (HJ_KEY_NULLS_EQUAL); it is
    what key_hash2_host goes by. The flag belongs to the column of the JOIN, not to one side of it: join_on_columns sets
    it for column c when its own nulls_equal argument, R's column c or S's column c asks for it.
    ValueError for offsets that decrease or end behind the data, data above 2^32 - 1 bytes, and lengths that disagree."""

    def __init__(self, values, valid=None, nulls_equal=False):
        if isinstance(values, np.ma.MaskedArray):
            if valid is not None:
                raise ValueError("KeyColumn: a masked array brings its own validity")
            values, valid = np.ma.getdata(values), ~np.ma.getmaskarray(values)
        a = np.asarray(values)
        if a.ndim != 1:
            raise ValueError(f"KeyColumn: values must be 1-D, not shape {a.shape}")
        if a.dtype.hasobject or a.dtype.itemsize not in _GATHER_WIDTHS:
            raise ValueError(f"KeyColumn: {a.dtype} elements; 1, 2, 4, 8 or 16 bytes can be joined on (strings: KeyColumn.from_list)")
        self.values, self.offsets, self.width, self.rows = _aligned(np.ascontiguousarray(a)), None, a.dtype.itemsize, a.shape[0]
        self.valid, self.nulls_equal = self._validity(valid, self.rows), bool(nulls_equal)

    @classmethod
    def varlen(cls, offsets, data, valid=None, nulls_equal=False):
        off = np.asarray(offsets)
        if off.ndim != 1 or off.size < 1 or off.dtype.kind not in "iu":
            raise ValueError("KeyColumn.varlen: offsets must be a 1-D integer array of rows + 1 entries")
        data = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.asarray(data)
        if data.ndim != 1 or data.dtype.itemsize != 1:
            raise ValueError("KeyColumn.varlen: data must be bytes or a 1-D array of 1-byte elements")
        if data.size > 0xFFFFFFFF:
            raise ValueError("KeyColumn.varlen: more than 2^32 - 1 bytes of data")
        wide = off.astype(np.int64) if off.dtype != np.uint64 else off
        if (wide[1:] < wide[:-1]).any() or int(wide[0]) < 0:
            raise ValueError("KeyColumn.varlen: offsets must be non-negative and non-decreasing")
        if int(wide[-1]) > data.size:
            raise ValueError(f"KeyColumn.varlen: offsets end at {int(wide[-1])}, behind the {data.size} bytes of data")
        self = cls.__new__(cls)
        self.values, self.offsets = np.ascontiguousarray(data).view(np.uint8), np.ascontiguousarray(off, dtype=np.uint32)
        self.width, self.rows = 0, off.size - 1
        self.valid, self.nulls_equal = cls._validity(valid, self.rows), bool(nulls_equal)
        return self

    @classmethod
    def from_list(cls, items, nulls_equal=False):
        items = list(items)
        raw = []
        for x in items:
            if not (x is None or isinstance(x, (bytes, str))):
                raise ValueError(f"KeyColumn.from_list: bytes, str or None, not {type(x).__name__}")
            raw.append(b"" if x is None else x.encode("utf-8") if isinstance(x, str) else x)
        off = np.zeros(len(raw) + 1, dtype=np.int64)
        np.cumsum(np.array([len(b) for b in raw], dtype=np.int64), out=off[1:])
        valid = np.array([x is not None for x in items], dtype=bool)
        return cls.varlen(off, b"".join(raw), None if valid.all() else valid, nulls_equal)

    @staticmethod
    def _validity(valid, rows):
        if valid is None:
            return None
        v = np.asarray(valid)
        if v.dtype != np.bool_ or v.shape != (rows,):
            raise ValueError(f"KeyColumn: valid must be {rows} bools, not {v.dtype} of shape {v.shape}")
        return np.ascontiguousarray(v)

    def __len__(self):
        return self.rows

    def to_list(self):
        """the inverse of from_list: one `bytes | None` per row (None: NULL); a fixed element comes back as its bytes"""
        ok = self.valid if self.valid is not None else np.ones(self.rows, dtype=bool)
        if self.offsets is None:
            raw = np.ascontiguousarray(self.values).view(np.uint8).tobytes()
            return [raw[i * self.width:(i + 1) * self.width] if v else None for i, v in enumerate(ok)]
        raw, off = self.values.tobytes(), self.offsets
        return [raw[int(off[i]):int(off[i + 1])] if v else None for i, v in enumerate(ok)]

    def take(self, lo, n):
        """rows [lo, lo + n) as the C ABI takes a column: (values or bytes, offsets rebased to those bytes or None, the
        validity bits repacked from bit 0 as uint32 words or None)"""
        words = None
        if self.valid is not None:
            bits = np.packbits(self.valid[lo:lo + n], bitorder="little")
            words = np.zeros((n + 31) // 32 or 1, dtype=np.uint32)
            words.view(np.uint8)[:bits.size] = bits
        if self.offsets is None:
            return self.values[lo:lo + n], None, words
        off = self.offsets[lo:lo + n + 1]
        return self.values[int(off[0]):int(off[-1])], off - off[0], words


def _as_key_columns(fn, side, keys):
    """the key columns of one side as a list of KeyColumn of one length; ValueError for what cannot be joined on"""
    cols = [keys] if isinstance(keys, (KeyColumn, np.ndarray)) else list(keys)
    if not 1 <= len(cols) <= _lib.HJ_KEY_MAX_COLS:
        raise ValueError(f"{fn}: {side} has {len(cols)} key columns; 1 to {_lib.HJ_KEY_MAX_COLS} can be joined on")
    cols = [c if isinstance(c, KeyColumn) else KeyColumn(c) for c in cols]
    if any(c.rows != cols[0].rows for c in cols):
        raise ValueError(f"{fn}: the key columns of {side} have {[c.rows for c in cols]} rows")
    return cols


def key_hash2_host(cols, key_mask=0):
    """hj_key_hash2_host: key_hash_host on key columns in the Arrow layout -- cols is one KeyColumn (or plain / masked 1-D
    numpy array) or a sequence of 1 to HJ_KEY_MAX_COLS of them. Returns the join words as a numpy uint64 array, the tuples
    HashJoinContext.key_hash2 writes for the same columns on the device. A row with a NULL in a column that is not
    nulls_equal is NULL-keyed: its word is a hash of its position, not of its columns (include/htm_hashjoin.h). Needs no
    device."""
    cols = _as_key_columns("key_hash2_host", "cols", cols)
    if not 0 <= int(key_mask) <= 0xFFFFFFFF:
        raise ValueError(f"key_hash2_host: key_mask must fit 32 bits, not {key_mask!r}")
    n = cols[0].rows
    out = np.empty(n, dtype=np.uint64)
    held = [c.take(0, n) for c in cols]
    ptr = lambda a: a.ctypes.data if a is not None else 0       # noqa: E731
    arr, k = _key_cols2([(ptr(v), 0, c.width, ptr(off), 0, ptr(words), 0, _lib.HJ_KEY_NULLS_EQUAL if c.nulls_equal else 0)
                         for c, (v, off, words) in zip(cols, held)])
    rc = lib.hj_key_hash2_host(arr, k, _lib.HJ_KEY_SIDE_S, n, int(key_mask), out.ctypes.data)
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, "hj_key_hash2_host")
    return out


class _ColumnKeys:
    """What join_on, join_on_columns and aggregate_on share: the key columns of both sides on the device (R's whole, a slice of
    S's in the room kept for one), the hash of either side as _drive_join's `fill`, and the verify step of a slice's
    candidates. dev: "cols" (the hj_key_col2 tuples), "s_marks" / "r_marks" (the two mark planes)."""

    def __init__(self, r_keys, s_keys, nulls_equal, key_mask, step):
        self.r_keys, self.s_keys, self.key_mask, self.step = r_keys, s_keys, key_mask, step
        self.n_r, self.n_s = r_keys[0].rows, s_keys[0].rows
        self.widths = [c.width for c in r_keys]
        self.flags = [_lib.HJ_KEY_NULLS_EQUAL if nulls_equal or r.nulls_equal or s.nulls_equal else 0 for r, s in zip(r_keys, s_keys)]
        self.dev = {}

    @staticmethod
    def _put(ctx, d, a):
        if a is not None and a.nbytes:
            ctx.copy_h2d(d, a)

    def hash_keys(self, ctx, held, d_tuples, lo, n):
        """R's key columns go up whole, a slice's into the room kept for one; either is hashed where it lies"""
        dev, step = self.dev, self.step
        if lo is None:
            def up(a):      # a bytes buffer goes up in whole 32-bit words: the kernels read the aligned words of an element
                if a is None:
                    return 0
                d = held.alloc(a.nbytes + 3 & ~3)
                self._put(ctx, d, np.ascontiguousarray(a))
                return d

            r_dev = [tuple(up(a) for a in c.take(0, self.n_r)) for c in self.r_keys]
            dev["s"] = [(held.alloc(_slice_bytes(c, self.n_s, step) + 3 & ~3), held.alloc(4 * (step + 1)) if c.offsets is not None else 0,
                         held.alloc(4 * ((step + 31) // 32)) if c.valid is not None else 0) for c in self.s_keys]
            dev["r_marks"] = held.put(np.zeros((self.n_r + 31) // 32, dtype=np.uint32))
            dev["s_marks"] = held.alloc(4 * ((step + 31) // 32))
            dev["cols"] = [(s[0], r[0], w, s[1], r[1], s[2], r[2], f) for s, r, w, f in zip(dev["s"], r_dev, self.widths, self.flags)]
            ctx.key_hash2(dev["cols"], _lib.HJ_KEY_SIDE_R, n, d_tuples, self.key_mask)
        else:
            for d, c in zip(dev["s"], self.s_keys):
                for d_part, part in zip(d, c.take(lo, n)):
                    self._put(ctx, d_part, part)
            ctx.key_hash2(dev["cols"], _lib.HJ_KEY_SIDE_S, n, d_tuples, self.key_mask)

    def verify(self, ctx, held, lo, n, d_s, d_r, candidates, pairs, marks=True):
        """the slice's candidates -> (its kept pairs' S plane, R plane, their number) -- the planes allocated from held and
        the caller's to free; pairs False: a mark-only pass, (0, 0, 0) -- and the marks of both sides (marks False: no
        plane is touched -- a condition step behind this one sets its own)"""
        dev = self.dev
        if marks:
            ctx.copy_h2d(dev["s_marks"], np.zeros((n + 31) // 32, dtype=np.uint32))
        capacity = candidates if pairs else 0
        d_ks, d_kr = (held.alloc(4 * capacity), held.alloc(4 * capacity)) if pairs else (0, 0)
        ctx.pairs_verify2(d_s, d_r, candidates, lo, n, self.n_r, dev["cols"], d_ks, d_kr, capacity,
                          dev["s_marks"] if marks else 0, dev["r_marks"] if marks else 0)
        return d_ks, d_kr, (ctx.verify_info()[1] if pairs else 0)


@_where_keyword("_join_on_columns")
def join_on_columns(
r_keys, s_keys, r_cols=None, s_cols=None, how="inner", nulls_equal=False, radixBits=0, slice_tuples=None,
                    device=0, key_mask=0):
    """join_on for key columns that may hold NULLs and variable-length elements (strings): r_keys / s_keys are each one
    KeyColumn or a sequence of 1 to HJ_KEY_MAX_COLS of them, all of a side of one length; a plain 1-D numpy array stands
    for KeyColumn(array), a numpy.ma.MaskedArray brings its mask. Column c of both sides is of one kind: fixed with the
    same itemsize, or variable-length. Two rows match when every column is equal: fixed elements bytewise (as join_on),
    variable-length ones in length and bytes.
    NULLs: a row with a NULL in any key column is NULL-keyed and matches nothing, not even another NULL (SQL's =). A
    NULL-keyed S row is an unmatched S row: it appears in left, full and anti. A NULL-keyed R row is an unmatched R row:
    it appears in right, full and right_anti. nulls_equal=True sets HJ_KEY_NULLS_EQUAL on every column: a NULL equals a
    NULL and nothing else (the pandas reading); a column built with nulls_equal=True has it by itself.
    The method is join_on's with HashJoinContext.key_hash2 / pairs_verify2 in place of key_hash / pairs_verify; per S
    slice the validity bits are repacked from the slice's first row and the offsets rebased to the slice's own bytes.
    how, r_cols / s_cols, radixBits, slice_tuples, key_mask, where and asof (keyword only), the result dict and the order of its rows: as in join_on."""
    return _join_on_columns(r_keys, s_keys, r_cols, s_cols, how, nulls_equal, radixBits, slice_tuples, device, key_mask)


def _join_on_columns(r_keys, s_keys, r_cols=None, s_cols=None, how="inner", nulls_equal=False, radixBits=0, slice_tuples=None,
                     device=0, key_mask=0, where=None, asof=None):
    """join_on_columns, and join_on_columns with a condition or an as-of term (_where_keyword)"""
    fn = "join_on_columns"
    if not isinstance(how, str) or how not in _TABLE_HOWS:
        raise ValueError(f"{fn}: how must be one of {', '.join(_TABLE_HOWS)}, not {how!r}")
    r_keys, s_keys = _as_key_columns(fn, "R", r_keys), _as_key_columns(fn, "S", s_keys)
    widths = [c.width for c in r_keys]
    if widths != [c.width for c in s_keys]:
        raise ValueError(f"{fn}: the key columns of R have widths {widths} (0: variable-length), those of S {[c.width for c in s_keys]}")
    return _join_key_columns(fn, r_keys, s_keys, nulls_equal, r_cols, s_cols, how, radixBits, slice_tuples, device, key_mask, where, asof)


def _join_key_columns(fn, r_keys, s_keys, nulls_equal, r_cols, s_cols, how, radixBits, slice_tuples, device, key_mask, where, asof=None):
    """The driver of join_on (fn "join_on") and join_on_columns: hash, candidate join, verify, the rows of the kind. r_keys /
    s_keys: lists of KeyColumn, checked by the caller, column c of both sides of one width; `how` is one of _TABLE_HOWS."""
    if not 0 <= int(key_mask) <= 0xFFFFFFFF:
        raise ValueError(f"{fn}: key_mask must fit 32 bits, not {key_mask!r}")
    n_r, n_s = r_keys[0].rows, s_keys[0].rows
    if max(n_r, n_s) > 0xFFFFFFFF:
        raise ValueError(f"{fn}: a relation of more than 2^32 - 1 rows")
    r_cols = _table_columns(fn, "R", r_cols, n_r)
    s_cols = _table_columns(fn, "S", s_cols, n_s)
    step = _slice_step(fn, n_s, slice_tuples) if n_s else 0
    terms = _where_terms(fn, where, n_s, n_r)
    best = _asof_term(fn, asof, n_s, n_r)
    rows = _TableRows(how, r_cols, s_cols, n_r, step, n_s)
    trivial = rows.without_device(n_s)
    if trivial is not None:
        return trivial
    pairs = rows.kind is not None and rows.kind <= _lib.HJ_JOIN_LEFT        # the kept pairs are rows of the result
    s_sweep = _ON_S_SWEEP.get(rows.kind)
    keys = _ColumnKeys(r_keys, s_keys, nulls_equal, key_mask, step)
    cond = _pair_steps(terms, best, rows, n_r, n_s, step)
    dev = keys.dev

    def verify(ctx, held, lo, n, d_s, d_r, candidates):
        """the slice's candidates -> its kept pairs and the marks of both sides, then the rows of its kind"""
        d_ks, d_kr, kept = keys.verify(ctx, held, lo, n, d_s, d_r, candidates, pairs)      # right_semi / right_anti, semi / anti: a mark-only pass
        if pairs:
            rows.add(ctx, held, lo, n, d_ks, d_kr, kept)
            held.free(d_ks, d_kr)
        if s_sweep is not None:
            d_rows = held.alloc(4 * n)
            ctx.mark_rows(dev["s_marks"], n, lo, s_sweep, d_rows, n)
            rows.add(ctx, held, lo, n, d_rows, 0, ctx.mark_rows_info()[1])
            held.free(d_rows)

    def r_only(ctx, held):
        if rows.which is not None:
            d_rows = held.alloc(4 * n_r)
            ctx.mark_rows(dev["r_marks"], n_r, 0, rows.which, d_rows, n_r)
            rows.add(ctx, held, None, 0, 0, d_rows, ctx.mark_rows_info()[1])

    def verify_where(ctx, held, lo, n, d_s, d_r, candidates):
        """the slice's candidates -> the pairs with equal keys, no plane marked; the condition step takes it from there"""
        d_es, d_er, equal = keys.verify(ctx, held, lo, n, d_s, d_r, candidates, True, marks=False)
        cond.slice(ctx, held, lo, n, d_es, d_er, equal)
        held.free(d_es, d_er)

    # the candidate join is INNER whatever the kind, and the context's own R marks stay out of it: a candidate that the
    # verify step rejects would have set them. Its tuples are made on the device (_drive_join's fill): the two arrays stand
    # for the relations' lengths alone
    _drive_join(np.empty(n_r, dtype=np.uint8), np.empty(n_s, dtype=np.uint8), "radix", _lib.HJ_JOIN_INNER, None, step,
                verify if cond is None else verify_where, device, radixBits=radixBits, fill=keys.hash_keys,
                after=r_only if cond is None else cond.r_only)
    return rows.joined()


# ---- join conditions beyond equality: where= ------------------------------------------------------------------------------
_WHERE_TYPES = {"u": _lib.HJ_VAL_UINT, "i": _lib.HJ_VAL_INT, "f": _lib.HJ_VAL_FLOAT}


def _where_side(fn, side, values, n, what="a where term"):
    """one side of a term as a fixed-width KeyColumn of n rows; ValueError for what a term cannot compare"""
    col = values if isinstance(values, KeyColumn) else None
    if col is None:
        a = values if isinstance(values, np.ma.MaskedArray) else np.asarray(values)
        if a.ndim != 1:
            raise ValueError(f"{fn}: the {side} values of {what} must be 1-D, not shape {a.shape}")
        dt = a.dtype
    elif col.offsets is not None:
        raise ValueError(f"{fn}: {what} cannot compare a variable-length column ({side})")
    else:
        dt = col.values.dtype
    if dt.kind not in _WHERE_TYPES or dt.itemsize > 8 or (dt.kind == "f" and dt.itemsize < 4):
        raise ValueError(f"{fn}: {what} compares uint8..uint64, int8..int64, float32 or float64, not {dt} ({side})")
    col = KeyColumn(values) if col is None else col
    if n is not None and col.rows != n:
        raise ValueError(f"{fn}: the {side} values of {what} must have {n} elements, not {col.rows}")
    return col


def _where_terms(fn, where, n_s=None, n_r=None):
    """where= as a list of (S KeyColumn, hj_cmp_op, R KeyColumn, hj_val_type, width); None for None or an empty sequence"""
    if where is None:
        return None
    where = list(where)
    if not where:
        return None
    if len(where) > _lib.HJ_WHERE_MAX_TERMS:
        raise ValueError(f"{fn}: where has {len(where)} terms; 1 to {_lib.HJ_WHERE_MAX_TERMS} can be evaluated")
    out = []
    for term in where:
        if not isinstance(term, (tuple, list)) or len(term) != 3:
            raise ValueError(f"{fn}: a where term is (s_values, op, r_values), not {term!r}")
        s_values, op, r_values = term
        if not isinstance(op, str) or op not in _lib.CMP_OPS:
            raise ValueError(f"{fn}: the op of a where term must be one of {', '.join(_lib.CMP_OPS)}, not {op!r}")
        s, r = _where_side(fn, "S", s_values, n_s), _where_side(fn, "R", r_values, n_r)
        if s.values.dtype != r.values.dtype:
            raise ValueError(f"{fn}: a where term compares {s.values.dtype} (S) with {r.values.dtype} (R); there is no implicit cast")
        out.append((s, _lib.CMP_OPS[op], r, _WHERE_TYPES[s.values.dtype.kind], s.width))
    return out


def _asof_term(fn, asof, n_s=None, n_r=None):
    """asof= as (S KeyColumn, hj_cmp_op, R KeyColumn, hj_val_type, width), the shape of a where term; None for None"""
    if asof is None:
        return None
    what = "the asof term"
    if not isinstance(asof, (tuple, list)) or len(asof) != 3:
        raise ValueError(f"{fn}: asof is one term (s_values, op, r_values), not {asof!r}")
    s_values, op, r_values = asof
    if not isinstance(op, str) or op not in _lib.ASOF_OPS:
        raise ValueError(f"{fn}: the op of {what} must be one of {', '.join(_lib.ASOF_OPS)}, not {op!r}")
    s, r = _where_side(fn, "S", s_values, n_s, what), _where_side(fn, "R", r_values, n_r, what)
    if s.values.dtype != r.values.dtype:
        raise ValueError(f"{fn}: {what} compares {s.values.dtype} (S) with {r.values.dtype} (R); there is no implicit cast")
    return (s, _lib.ASOF_OPS[op], r, _WHERE_TYPES[s.values.dtype.kind], s.width)


def pairs_where_host(map_s, map_r, s_row_base, terms, capacity=None, marks=False):
    """hj_pairs_where_host: HashJoinContext.pairs_where on numpy arrays, computed by the same code on the host. map_s / map_r:
    the pairs as two uint32 arrays of one length; terms: 1 to HJ_WHERE_MAX_TERMS tuples (s_values, op, r_values) as the
    where= of the joins takes them, op out of CMP_OPS; the S side has len(s_values) rows from s_row_base, the R side
    len(r_values). capacity (None: every pair fits) cuts what is written, not what is counted or marked.
    Returns {"s_idx", "r_idx"} (the kept pairs written, in input order), "info" (kept, written, 0, dropped) and, with
    marks=True, "s_marks" / "r_marks": the two planes as uint32 words, zero before the call. Needs no device."""
    fn = "pairs_where_host"
    map_s, map_r = np.ascontiguousarray(map_s, dtype=np.uint32), np.ascontiguousarray(map_r, dtype=np.uint32)
    if map_s.ndim != 1 or map_s.shape != map_r.shape:
        raise ValueError(f"{fn}: the maps must be 1-D and of one length, not shapes {map_s.shape} and {map_r.shape}")
    cols = _where_terms(fn, terms)
    if cols is None:
        raise ValueError(f"{fn}: 1 to {_lib.HJ_WHERE_MAX_TERMS} terms, not none")
    n_s, n_r = cols[0][0].rows, cols[0][2].rows
    if any(s.rows != n_s or r.rows != n_r for s, _, r, _, _ in cols):
        raise ValueError(f"{fn}: the values of every term must have one length per side")
    capacity = map_s.size if capacity is None else int(capacity)
    held = [(s.take(0, n_s), r.take(0, n_r)) for s, _, r, _, _ in cols]
    ptr = lambda a: a.ctypes.data if a is not None else 0       # noqa: E731
    arr, k = _where_terms_arr([(ptr(sv), ptr(rv), width, type_, op, ptr(sw), ptr(rw))
                               for (_, op, _, type_, width), ((sv, _, sw), (rv, _, rw)) in zip(cols, held)])
    out_s, out_r = np.empty(min(capacity, map_s.size), dtype=np.uint32), np.empty(min(capacity, map_s.size), dtype=np.uint32)
    s_marks = np.zeros((n_s + 31) // 32, dtype=np.uint32) if marks else None
    r_marks = np.zeros((n_r + 31) // 32, dtype=np.uint32) if marks else None
    info = (C.c_uint64 * 4)()
    rc = lib.hj_pairs_where_host(map_s.ctypes.data, map_r.ctypes.data, map_s.size, int(s_row_base), n_s, n_r, arr, k,
                                 out_s.ctypes.data, out_r.ctypes.data, out_s.size, ptr(s_marks) or None, ptr(r_marks) or None, info)
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, "hj_pairs_where_host")
    info = tuple(int(x) for x in info)
    out = {"s_idx": out_s[:info[1]], "r_idx": out_r[:info[1]], "info": info}
    if marks:
        out["s_marks"], out["r_marks"] = s_marks, r_marks
    return out


def pairs_asof_host(map_s, map_r, s_row_base, term, capacity=None, marks=False):
    """hj_pairs_asof_host: HashJoinContext.pairs_asof on numpy arrays, computed by the same code on the host. map_s / map_r:
    the pairs as two uint32 arrays of one length; term: (s_values, op, r_values) as the asof= of the joins takes it; the S
    side has len(s_values) rows from s_row_base, the R side len(r_values). capacity (None: every pair fits) cuts what is
    written, not what is counted or marked.
    Returns {"s_idx", "r_idx"} (the kept pairs written, in input order), "best_row" (per S row the R row kept, or NO_ROW: the
    left-outer as-of map), "info" (kept, written, 0, dropped) and, with marks=True, "s_marks" / "r_marks": the two planes as
    uint32 words, zero before the call. Needs no device."""
    fn = "pairs_asof_host"
    map_s, map_r = np.ascontiguousarray(map_s, dtype=np.uint32), np.ascontiguousarray(map_r, dtype=np.uint32)
    if map_s.ndim != 1 or map_s.shape != map_r.shape:
        raise ValueError(f"{fn}: the maps must be 1-D and of one length, not shapes {map_s.shape} and {map_r.shape}")
    col = _asof_term(fn, term)
    if col is None:
        raise ValueError(f"{fn}: one term (s_values, op, r_values), not None")
    s, op, r, type_, width = col
    n_s, n_r = s.rows, r.rows
    capacity = map_s.size if capacity is None else int(capacity)
    (sv, _, sw), (rv, _, rw) = s.take(0, n_s), r.take(0, n_r)
    ptr = lambda a: a.ctypes.data if a is not None else 0       # noqa: E731
    arr = _asof_term_arr((ptr(sv), ptr(rv), width, type_, op, ptr(sw), ptr(rw)))
    out_s, out_r = np.empty(min(capacity, map_s.size), dtype=np.uint32), np.empty(min(capacity, map_s.size), dtype=np.uint32)
    best_val, best_row = np.empty(max(n_s, 1), dtype=np.uint64), np.empty(max(n_s, 1), dtype=np.uint32)
    s_marks = np.zeros((n_s + 31) // 32, dtype=np.uint32) if marks else None
    r_marks = np.zeros((n_r + 31) // 32, dtype=np.uint32) if marks else None
    info = (C.c_uint64 * 4)()
    rc = lib.hj_pairs_asof_host(map_s.ctypes.data, map_r.ctypes.data, map_s.size, int(s_row_base), n_s, n_r, C.byref(arr),
                                best_val.ctypes.data, best_row.ctypes.data, out_s.ctypes.data, out_r.ctypes.data, out_s.size,
                                ptr(s_marks) or None, ptr(r_marks) or None, info)
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, "hj_pairs_asof_host")
    info = tuple(int(x) for x in info)
    out = {"s_idx": out_s[:info[1]], "r_idx": out_r[:info[1]], "best_row": best_row[:n_s], "info": info}
    if marks:
        out["s_marks"], out["r_marks"] = s_marks, r_marks
    return out


class _WhereTerms:
    """What the joins share once they are given where=: the terms' R columns whole on the device and room for one slice of
    the S columns (uploaded once per slice), the two mark planes of the condition step, the step itself -- the pairs that
    agree on the key -> the pairs for which every term holds too, as rows of the result -- and the sweeps behind it. rows:
    the _TableRows the result grows in. slice() has the signature of _drive_join's on_maps, r_only() of its `after`."""

    def __init__(self, terms, rows, n_r, n_s, step):
        self.terms, self.rows, self.n_r, self.n_s, self.step = terms, rows, n_r, n_s, step
        self.pairs = rows.kind is not None and rows.kind <= _lib.HJ_JOIN_LEFT      # the kept pairs are rows of the result
        self.s_sweep = _ON_S_SWEEP.get(rows.kind)
        self.dev, self.lo = None, None

    def _put(self, ctx, held, lo, n):
        if self.dev is None:    # the first slice: R's columns whole, room for a slice of S's, the planes
            up = lambda a: held.put(np.ascontiguousarray(a)) if a is not None else 0       # noqa: E731
            r_dev = [tuple(up(a) for a in r.take(0, self.n_r)) for _, _, r, _, _ in self.terms]
            s_dev = [(held.alloc(self.step * s.width), 0, held.alloc(4 * ((self.step + 31) // 32)) if s.valid is not None else 0)
                     for s, _, _, _, _ in self.terms]
            self.dev = {"s": s_dev, "r_marks": held.put(np.zeros((self.n_r + 31) // 32, dtype=np.uint32)),
                        "s_marks": held.alloc(4 * ((self.step + 31) // 32)),
                        "terms": [(sd[0], rd[0], width, type_, op, sd[2], rd[2])
                                  for sd, rd, (_, op, _, type_, width) in zip(s_dev, r_dev, self.terms)]}
        if self.lo != lo:       # the slice's columns go up once
            for d, (s, _, _, _, _) in zip(self.dev["s"], self.terms):
                _put_parts(ctx, held, s.take(lo, n), d)
            self.lo = lo

    def slice(self, ctx, held, lo, n, d_s, d_r, n_pairs):
        """the n_pairs pairs of the slice [lo, lo + n) that agree on the key -> the rows of its kind"""
        self._put(ctx, held, lo, n)
        rows, dev = self.rows, self.dev
        ctx.copy_h2d(dev["s_marks"], np.zeros((n + 31) // 32, dtype=np.uint32))
        capacity = n_pairs if self.pairs else 0          # right_semi / right_anti, semi / anti: a mark-only pass
        d_ks, d_kr = (held.alloc(4 * capacity), held.alloc(4 * capacity)) if self.pairs else (0, 0)
        ctx.pairs_where(d_s, d_r, n_pairs, lo, n, self.n_r, dev["terms"], d_ks, d_kr, capacity, dev["s_marks"], dev["r_marks"])
        if self.pairs:
            rows.add(ctx, held, lo, n, d_ks, d_kr, ctx.where_info()[1])
            held.free(d_ks, d_kr)
        self.s_rows(ctx, held, lo, n)

    def s_rows(self, ctx, held, lo, n):
        """the rows a kind takes from the sweep of the slice's S plane"""
        if self.s_sweep is not None:
            d_rows = held.alloc(4 * n)
            ctx.mark_rows(self.dev["s_marks"], n, lo, self.s_sweep, d_rows, n)
            self.rows.add(ctx, held, lo, n, d_rows, 0, ctx.mark_rows_info()[1])
            held.free(d_rows)

    def r_only(self, ctx, held):
        if self.rows.which is not None:
            d_rows = held.alloc(4 * self.n_r)
            ctx.mark_rows(self.dev["r_marks"], self.n_r, 0, self.rows.which, d_rows, self.n_r)
            self.rows.add(ctx, held, None, 0, 0, d_rows, ctx.mark_rows_info()[1])


class _AsofStep(_WhereTerms):
    """_WhereTerms for a join that is given asof=, with or without where=: the as-of term's columns travel as one more term
    behind the condition's. slice() runs the condition step, where there is one, with its pairs kept whatever the kind and
    no mark plane, then HashJoinContext.pairs_asof over what it kept: that call sets the marks and gives the pairs of the
    result. The two best planes are sized for one slice; a slice's pair list is complete when it arrives here (_drive_join
    probes a slice again whose rows exceeded the planes), so every S row has all its pairs in one call."""

    def __init__(self, best, terms, rows, n_r, n_s, step):
        super().__init__(list(terms or []) + [best], rows, n_r, n_s, step)
        self.n_where = len(terms or [])

    def slice(self, ctx, held, lo, n, d_s, d_r, n_pairs):
        self._put(ctx, held, lo, n)
        rows, dev = self.rows, self.dev
        if "best_val" not in dev:
            dev["best_val"], dev["best_row"] = held.alloc(8 * self.step), held.alloc(4 * self.step)
        ctx.copy_h2d(dev["s_marks"], np.zeros((n + 31) // 32, dtype=np.uint32))
        mine = []
        if self.n_where:
            mine = [held.alloc(4 * n_pairs), held.alloc(4 * n_pairs)]
            ctx.pairs_where(d_s, d_r, n_pairs, lo, n, self.n_r, dev["terms"][:self.n_where], mine[0], mine[1], n_pairs)
            d_s, d_r, n_pairs = mine[0], mine[1], ctx.where_info()[1]
        capacity = min(n_pairs, n) if self.pairs else 0     # one pair per S row at most; semi / anti and R's kinds: a mark-only pass
        d_ks, d_kr = (held.alloc(4 * capacity), held.alloc(4 * capacity)) if self.pairs else (0, 0)
        ctx.pairs_asof(d_s, d_r, n_pairs, lo, n, self.n_r, dev["terms"][-1], dev["best_val"], dev["best_row"], d_ks, d_kr, capacity,
                       dev["s_marks"], dev["r_marks"])
        if self.pairs:
            rows.add(ctx, held, lo, n, d_ks, d_kr, ctx.asof_info()[1])
            held.free(d_ks, d_kr)
        held.free(*mine)
        self.s_rows(ctx, held, lo, n)


def _pair_steps(terms, best, rows, n_r, n_s, step):
    """the steps behind the pairs that agree on the key: none (None), the condition step, or the as-of step behind it"""
    if best is not None:
        return _AsofStep(best, terms, rows, n_r, n_s, step)
    return _WhereTerms(terms, rows, n_r, n_s, step) if terms is not None else None


# ---- aggregating joins: COUNT / SUM / MIN / MAX of S values per R row -----------------------------------------------------
_AGG_DTYPES = {np.dtype(np.int32): (4, _lib.HJ_AGG_SIGNED), np.dtype(np.uint32): (4, 0),
               np.dtype(np.int64): (8, _lib.HJ_AGG_SIGNED), np.dtype(np.uint64): (8, 0)}


def _agg_identity(op, signed):
    if op == _lib.HJ_AGG_MIN:
        return 0x7FFFFFFFFFFFFFFF if signed else 0xFFFFFFFFFFFFFFFF
    if op == _lib.HJ_AGG_MAX:
        return 0x8000000000000000 if signed else 0
    return 0


class _AggPlan:
    """The aggregates of radix_join_aggregate / aggregate_on, checked: cols -- the device columns, one dict each (op,
    source name or None, width, flags), the wrapper's own COUNT(col) of every nullable source of a SUM / MIN / MAX behind
    the caller's -- and how the result dict is put together from their planes. ValueError for what cannot be aggregated."""

    def __init__(self, fn, s_cols, aggs, n_s):
        self.fn, self.sources, self.cols, self.outputs = fn, {}, [], []
        for name, col in dict(s_cols or {}).items():
            c = col if isinstance(col, KeyColumn) else KeyColumn(col)
            if c.offsets is not None or np.asarray(c.values).dtype not in _AGG_DTYPES:
                raise ValueError(f"{fn}: column {name!r} is {np.asarray(c.values).dtype if c.offsets is None else 'variable-length'}; "
                                 "int32, uint32, int64 and uint64 can be aggregated (floating-point sums depend on their order)")
            if c.rows != n_s:
                raise ValueError(f"{fn}: column {name!r} has {c.rows} rows, S has {n_s}")
            self.sources[name] = c
        if not aggs:
            raise ValueError(f"{fn}: no aggregates")
        seen = {}            # nullable source -> the device column of its COUNT(col)
        for out, spec in dict(aggs).items():
            if out == "count":
                raise ValueError(f"{fn}: the output name 'count' is taken by the match counts")
            if not isinstance(spec, (tuple, list)) or len(spec) != 2:
                raise ValueError(f"{fn}: aggregate {out!r} must be (op, column name or None), not {spec!r}")
            op, src = spec
            if not isinstance(op, str) or op.lower() not in _lib.AGG_OPS:
                raise ValueError(f"{fn}: aggregate {out!r} has op {op!r}; count, sum, min and max exist")
            op = _lib.AGG_OPS[op.lower()]
            if src is None and op != _lib.HJ_AGG_COUNT:
                raise ValueError(f"{fn}: aggregate {out!r} needs a column")
            if src is not None and src not in self.sources:
                raise ValueError(f"{fn}: aggregate {out!r} names column {src!r}, which s_cols does not hold")
            self.outputs.append((out, op, src, self._col(op, src)))
        for out, op, src, _ in list(self.outputs):
            if op != _lib.HJ_AGG_COUNT and self.sources[src].valid is not None and src not in seen:
                seen[src] = self._col(_lib.HJ_AGG_COUNT, src)
        self.seen = seen

    def _col(self, op, src):
        width, flags = (0, 0) if op == _lib.HJ_AGG_COUNT else _AGG_DTYPES[np.asarray(self.sources[src].values).dtype]
        self.cols.append({"op": op, "src": src, "width": width, "flags": flags})
        return len(self.cols) - 1

    def rounds(self):
        """the device columns in runs of at most HJ_AGG_MAX_COLS"""
        return [list(range(i, min(i + _lib.HJ_AGG_MAX_COLS, len(self.cols)))) for i in range(0, len(self.cols), _lib.HJ_AGG_MAX_COLS)]

    def identity(self, i):
        return _agg_identity(self.cols[i]["op"], bool(self.cols[i]["flags"]))

    def result(self, count, planes):
        """count: the match counts (uint64 per R row); planes: one uint64 array per device column -> the result dict"""
        res = {"count": count}
        for out, op, src, i in self.outputs:
            if op == _lib.HJ_AGG_COUNT:
                res[out] = planes[i]
                continue
            valid = (planes[self.seen[src]] if src in self.seen else count) > 0
            values = np.where(valid, planes[i], np.uint64(0))
            res[out] = KeyColumn(values.view(np.int64) if self.cols[i]["flags"] else values, valid)
        return res

    def without_device(self, n_r):
        zeros = np.zeros(n_r, dtype=np.uint64)
        return self.result(zeros, [zeros.copy() for _ in self.cols])


class _AggSources:
    """the value columns of one S slice on the device: room for `step` elements and their validity words per source"""

    def __init__(self, held, plan, step):
        self.plan = plan
        self.dev = {name: (held.alloc(c.width * step), held.alloc(4 * ((step + 31) // 32)) if c.valid is not None else 0)
                    for name, c in plan.sources.items() if any(col["src"] == name for col in plan.cols)}

    def put(self, ctx, lo, n, names=None):
        for name, (d_v, d_valid) in self.dev.items():
            if names is not None and name not in names:
                continue
            values, _, words = self.plan.sources[name].take(lo, n)
            if values.nbytes:
                ctx.copy_h2d(d_v, np.ascontiguousarray(values))
            if d_valid:
                ctx.copy_h2d(d_valid, words)

    def pointers(self, i):
        """(src, valid) of device column i; a COUNT reads no value"""
        col = self.plan.cols[i]
        if col["src"] is None:
            return 0, 0
        d_v, d_valid = self.dev[col["src"]]
        return (0 if col["op"] == _lib.HJ_AGG_COUNT else d_v), d_valid


def _fetch_plane(ctx, d, n):
    a = np.empty(n, dtype=np.uint64)
    if n:
        ctx.copy_d2h(a, d)
    return a


def radix_join_aggregate(relR, relS, s_cols, aggs, radixBits=0, slice_tuples=None, device=0):
    """GROUP BY <R row> over the equi-join of relR and relS on the key word, without the pairs: the fused group-join of the
    resident radix join (hj_prj_probe_agg_dev). s_cols: {name: values}, one int32, uint32, int64 or uint64 element per S
    tuple, as a numpy array or a KeyColumn with a validity (False: NULL). aggs: {output name: (op, column name or None)},
    op "count" | "sum" | "min" | "max"; ("count", None) is COUNT(*), ("count", name) counts the valid elements.
    Returns a dict: "count", the matches of every R row (uint64, len(relR)); per COUNT a uint64 array; per SUM / MIN /
    MAX a KeyColumn of int64 (signed sources) or uint64 whose validity is "the group saw at least one valid value" -- an
    empty group is NULL, as in SQL -- and whose values under a NULL are 0. SUM wraps modulo 2^64. R is partitioned once;
    relS goes through in slices of slice_tuples (default: all at once), the accumulators adding up. More than
    HJ_AGG_MAX_COLS device columns (the wrapper adds a COUNT of its own per nullable source) take several rounds over
    the same resident R. ValueError for an unknown op, a column that is no 4- or 8-byte integer, a missing column, and
    lengths that disagree."""
    fn = "radix_join_aggregate"
    relR = np.ascontiguousarray(relR, dtype=np.uint64)
    relS = np.ascontiguousarray(relS, dtype=np.uint64)
    plan = _AggPlan(fn, s_cols, aggs, relS.size)
    if relR.size == 0 or relS.size == 0:
        return plan.without_device(relR.size)
    step = _slice_step(fn, relS.size, slice_tuples)
    n_r = relR.size
    planes = [None] * len(plan.cols)
    with HashJoinContext(device) as ctx:
        held = _Held(ctx)
        try:
            ctx.reserve("prj", n_r, step, radixBits=radixBits, keepRowIds=True)
            ctx.prj_build(held.put(relR), n_r)
            dS = held.alloc(8 * step)
            sources = _AggSources(held, plan, step)
            d_count = held.alloc(8 * n_r)
            d_out = [held.alloc(8 * n_r) for _ in range(min(len(plan.cols), _lib.HJ_AGG_MAX_COLS))]
            for cols in plan.rounds():
                ctx.prj_agg_begin([(plan.cols[i]["op"], plan.cols[i]["width"], plan.cols[i]["flags"]) for i in cols])
                names = {plan.cols[i]["src"] for i in cols}
                for lo in range(0, relS.size, step):
                    part = relS[lo:lo + step]
                    ctx.copy_h2d(dS, part)
                    sources.put(ctx, lo, part.size, names)
                    ctx.prj_probe_agg(dS, part.size, [sources.pointers(i) for i in cols])
                ctx.prj_agg_rows(d_out[:len(cols)], d_count)
                for i, d in zip(cols, d_out):
                    planes[i] = _fetch_plane(ctx, d, n_r)
            count = _fetch_plane(ctx, d_count, n_r)
        finally:
            held.close()
    return plan.result(count, planes)


def aggregate_on(r_keys, s_keys, s_cols, aggs, nulls_equal=False, radixBits=0, slice_tuples=None, device=0, key_mask=0):
    """radix_join_aggregate for joins on real key columns: GROUP BY <R row> over the inner join of join_on_columns(r_keys,
    s_keys, nulls_equal=...), by its method -- key_hash2, the candidate join on the hashed word, pairs_verify2 -- with
    hj_pairs_agg_dev over the KEPT pairs of each slice in place of the gather (a reduction over the candidates would
    count what the verify step rejects). r_keys / s_keys, nulls_equal, radixBits, slice_tuples, key_mask: as in
    join_on_columns; s_cols, aggs and the result dict: as in radix_join_aggregate, one entry per row of R."""
    fn = "aggregate_on"
    r_keys, s_keys = _as_key_columns(fn, "R", r_keys), _as_key_columns(fn, "S", s_keys)
    widths = [c.width for c in r_keys]
    if widths != [c.width for c in s_keys]:
        raise ValueError(f"{fn}: the key columns of R have widths {widths} (0: variable-length), those of S {[c.width for c in s_keys]}")
    if not 0 <= int(key_mask) <= 0xFFFFFFFF:
        raise ValueError(f"{fn}: key_mask must fit 32 bits, not {key_mask!r}")
    n_r, n_s = r_keys[0].rows, s_keys[0].rows
    if max(n_r, n_s) > 0xFFFFFFFF:
        raise ValueError(f"{fn}: a relation of more than 2^32 - 1 rows")
    plan = _AggPlan(fn, s_cols, aggs, n_s)
    if n_r == 0 or n_s == 0:
        return plan.without_device(n_r)
    step = _slice_step(fn, n_s, slice_tuples)
    keys = _ColumnKeys(r_keys, s_keys, nulls_equal, key_mask, step)
    dev, out = {}, {}

    def reduce(ctx, held, lo, n, d_s, d_r, candidates):
        """the slice's candidates -> its kept pairs -> the accumulators, grouped by the R plane"""
        if not dev:
            dev["sources"] = _AggSources(held, plan, step)
            dev["count"] = held.put(np.zeros(n_r, dtype=np.uint64))
            dev["acc"] = [held.put(np.full(n_r, plan.identity(i), dtype=np.uint64)) for i in range(len(plan.cols))]
        d_ks, d_kr, kept = keys.verify(ctx, held, lo, n, d_s, d_r, candidates, True)
        dev["sources"].put(ctx, lo, n)
        for k, cols in enumerate(plan.rounds()):
            ctx.pairs_agg(d_kr, d_ks, kept, 0, n_r, lo, n,
                          [dev["sources"].pointers(i) + (dev["acc"][i], plan.cols[i]["op"], plan.cols[i]["width"], plan.cols[i]["flags"])
                           for i in cols], dev["count"] if k == 0 else 0)
        held.free(d_ks, d_kr)

    def fetch(ctx, held):
        out["count"] = _fetch_plane(ctx, dev["count"], n_r)
        out["planes"] = [_fetch_plane(ctx, d, n_r) for d in dev["acc"]]

    _drive_join(np.empty(n_r, dtype=np.uint8), np.empty(n_s, dtype=np.uint8), "radix", _lib.HJ_JOIN_INNER, None, step, reduce, device,
                radixBits=radixBits, fill=keys.hash_keys, after=fetch)
    return plan.result(out["count"], out["planes"])


# ---- the rows of one table grouped by their key columns: DISTINCT, GROUP BY key, a dense group id ---------------------------
_GROUP_NULLS = ("group", "drop")


def _group_key_columns(fn, keys, nulls, key_mask):
    """the key columns of key_groups / distinct_on / group_by_columns, checked -> (list of KeyColumn, their flags)"""
    if not isinstance(nulls, str) or nulls not in _GROUP_NULLS:
        raise ValueError(f"{fn}: nulls must be 'group' or 'drop', not {nulls!r}")
    if isinstance(key_mask, bool) or not isinstance(key_mask, (int, np.integer)) or not 0 <= int(key_mask) <= 0xFFFFFFFF:
        raise ValueError(f"{fn}: key_mask must fit 32 bits, not {key_mask!r}")
    cols = _as_key_columns(fn, "keys", keys)
    if cols[0].rows > 0xFFFFFFFE:
        raise ValueError(f"{fn}: a table of more than 2^32 - 2 rows")
    return cols, [_lib.HJ_KEY_NULLS_EQUAL if nulls == "group" or c.nulls_equal else 0 for c in cols]


def _host_key_cols2(cols, flags):
    """(what the descriptors point to -- to be kept alive --, the hj_key_col2 array, its length) for host pointers, side S"""
    held = [c.take(0, c.rows) for c in cols]
    ptr = lambda a: a.ctypes.data if a is not None else 0       # noqa: E731
    arr, k = _key_cols2([(ptr(v), 0, c.width, ptr(off), 0, ptr(words), 0, f) for c, (v, off, words), f in zip(cols, held, flags)])
    return held, arr, k


def _groups_result(rep, group, first_rows, n_groups, null_rows):
    return {"rep": rep, "group": group, "first_rows": first_rows, "n_groups": int(n_groups), "null_rows": int(null_rows)}


def key_groups_host(keys, nulls="group", key_mask=0, capacity=None):
    """hj_key_groups_host: key_groups on the host, by the kernels' hash and compare around a sequential table; needs no
    device. keys, nulls and key_mask as in key_groups; capacity (None: every group) cuts first_rows as the C ABI's does --
    n_groups stays the number of groups. Returns the dict key_groups returns."""
    fn = "key_groups_host"
    cols, flags = _group_key_columns(fn, keys, nulls, key_mask)
    n = cols[0].rows
    if capacity is not None and (isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 0):
        raise ValueError(f"{fn}: capacity must be None or a count, not {capacity!r}")
    cap = n if capacity is None else min(int(capacity), n)
    rep, group, first = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32), np.empty(cap, dtype=np.uint32)
    held, arr, k = _host_key_cols2(cols, flags)
    out = (C.c_uint64 * 8)()
    rc = lib.hj_key_groups_host(arr, k, _lib.HJ_KEY_SIDE_S, n, int(key_mask), rep.ctypes.data if n else None, group.ctypes.data if n else None,
                                first.ctypes.data if cap else None, cap, out)
    del held
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, "hj_key_groups_host")
    return _groups_result(rep, group, first[:int(out[1])], out[0], out[3])


class _GroupedKeys:
    """What key_groups, distinct_on and group_by_columns share: the key columns of the table on the device, one
    hj_key_groups_dev over them, and what it left -- d_rep, d_group, d_first (device planes of n, n and n_groups entries),
    n_groups, null_rows. parts: the device parts of every key column, for a gather behind it."""

    def __init__(self, ctx, held, cols, flags, key_mask):
        n = cols[0].rows
        self.n, self.cols = n, cols
        self.parts = [_put_parts(ctx, held, c.take(0, n)) for c in cols]
        desc = [(d[0], 0, c.width, d[1], 0, d[2], 0, f) for d, c, f in zip(self.parts, cols, flags)]
        self.d_rep, self.d_group, self.d_first = held.alloc(4 * n), held.alloc(4 * n), held.alloc(4 * n)
        ctx.key_groups(desc, _lib.HJ_KEY_SIDE_S, n, self.d_rep, self.d_group, self.d_first, n, int(key_mask))
        info = ctx.key_groups_info()
        if info["failure"]:
            raise HashJoinError(_lib.HJ_ERR_STATE, f"hj_key_groups_dev: the device reported failure word {info['failure']}")
        self.n_groups, self.null_rows = info["groups"], info["null_rows"]

    def gather_keys(self, ctx, held):
        """the key columns of the first rows, one KeyColumn per key column"""
        k_cols = [(k, parts, c) for k, (parts, c) in enumerate(zip(self.parts, self.cols))]
        got = _gather_key_columns(ctx, held, self.d_first, self.n_groups, 0, self.n, k_cols)
        return [got[k] for k in range(len(self.cols))]


def _empty_keys(cols):
    return [_take_key_column(c, np.empty(0, dtype=np.uint32)) for c in cols]


def key_groups(keys, nulls="group", key_mask=0, device=0):
    """Which rows of ONE table have the same key (hj_key_groups_dev): DISTINCT, GROUP BY key and pandas.factorize in one
    call. keys: what join_on_columns takes for one side -- one KeyColumn or 1-D numpy array (a numpy.ma.MaskedArray brings
    its mask), or a sequence of 1 to HJ_KEY_MAX_COLS of them, all of one length; two rows have the same key when every
    column is equal as in join_on_columns (fixed elements bytewise, variable-length ones in length and bytes).
    nulls="group" sets HJ_KEY_NULLS_EQUAL on every column: a NULL equals a NULL, so the NULLs form groups (SQL's GROUP BY).
    nulls="drop" leaves a row with a NULL in any key column out of every group (pandas' default) -- except in a column
    built with nulls_equal=True, which keeps its flag.
    Returns {"rep": uint32 per row, the lowest row with the same key; "group": uint32 per row, a dense group id in order of
    first occurrence; "first_rows": the rows with rep[i] == i, ascending, one per group; "n_groups"; "null_rows": the rows
    left out, whose rep and group are NO_ROW}. key_mask (0: none) keeps only those bits of the hashed word: more collisions,
    the same result -- for tests. An empty table is answered without a device."""
    fn = "key_groups"
    cols, flags = _group_key_columns(fn, keys, nulls, key_mask)
    n = cols[0].rows
    if n == 0:
        e = np.empty(0, dtype=np.uint32)
        return _groups_result(e, e.copy(), e.copy(), 0, 0)
    with HashJoinContext(device) as ctx:
        held = _Held(ctx)
        try:
            g = _GroupedKeys(ctx, held, cols, flags, key_mask)
            return _groups_result(_fetch_map(ctx, g.d_rep, n), _fetch_map(ctx, g.d_group, n), _fetch_map(ctx, g.d_first, g.n_groups),
                                  g.n_groups, g.null_rows)
        finally:
            held.close()


def distinct_on(keys, cols=None, nulls="group", key_mask=0, device=0):
    """SELECT DISTINCT ON (keys): the first row of every distinct key, in order of first occurrence. keys, nulls, key_mask:
    as in key_groups. cols: {name: values} payload columns of the table, as join_tables takes them (numpy arrays of 1, 2, 4,
    8 or 16-byte elements, or KeyColumns, which stay KeyColumns), gathered through the first rows on the device
    (hj_gather2_dev / hj_gather_dev). Returns {"first_rows", "keys": one KeyColumn per key column, "cols": {name: column},
    "n_groups", "null_rows"}, every column with n_groups rows. An empty table is answered without a device."""
    fn = "distinct_on"
    k_cols, flags = _group_key_columns(fn, keys, nulls, key_mask)
    n = k_cols[0].rows
    cols = _table_columns(fn, "the table's", cols, n)
    if n == 0:
        return {"first_rows": np.empty(0, dtype=np.uint32), "keys": _empty_keys(k_cols),
                "cols": _take_on_host(cols, np.empty(0, dtype=np.uint32))[0], "n_groups": 0, "null_rows": 0}
    with HashJoinContext(device) as ctx:
        held = _Held(ctx)
        try:
            g = _GroupedKeys(ctx, held, k_cols, flags, key_mask)
            d_cols = [(name, _put_parts(ctx, held, c.take(0, n)), c) if isinstance(c, KeyColumn) else (name, held.put(c), c.dtype)
                      for name, c in cols.items()]
            payload, _ = _gather_side(ctx, held, g.d_first, g.n_groups, 0, n, d_cols)
            return {"first_rows": _fetch_map(ctx, g.d_first, g.n_groups), "keys": g.gather_keys(ctx, held), "cols": payload,
                    "n_groups": g.n_groups, "null_rows": g.null_rows}
        finally:
            held.close()


def group_by_columns(keys, cols, aggs, nulls="group", key_mask=0, device=0):
    """SELECT keys, COUNT / SUM / MIN / MAX ... GROUP BY keys over ONE table, without a self-join: hj_key_groups_dev gives
    every row its dense group id, and hj_pairs_agg_dev reduces the rows into one accumulator per group (its group map the
    ids, its value map the identity; the NO_ROW ids of dropped rows are skipped by that call as it stands). keys, nulls,
    key_mask: as in key_groups. cols and aggs: as s_cols and aggs of aggregate_on -- {name: int32 / uint32 / int64 / uint64
    values, a numpy array or a KeyColumn with a validity} and {output name: (op, column name or None)}, op "count" | "sum" |
    "min" | "max"; integers only (floating-point sums depend on their order).
    Returns a dict, one entry per group in order of first occurrence: "keys" (one KeyColumn per key column), "first_rows",
    "count" (uint64, the rows of the group), per COUNT a uint64 array, per SUM / MIN / MAX a KeyColumn as in
    radix_join_aggregate (NULL where the group saw no valid value; SUM wraps modulo 2^64), and "n_groups", "null_rows". An
    empty table is answered without a device."""
    fn = "group_by_columns"
    k_cols, flags = _group_key_columns(fn, keys, nulls, key_mask)
    n = k_cols[0].rows
    plan = _AggPlan(fn, cols, aggs, n)
    for out, _, _, _ in plan.outputs:
        if out in ("keys", "first_rows", "n_groups", "null_rows"):
            raise ValueError(f"{fn}: the output name {out!r} is taken")
    if n == 0:
        res = plan.without_device(0)
        res.update(keys=_empty_keys(k_cols), first_rows=np.empty(0, dtype=np.uint32), n_groups=0, null_rows=0)
        return res
    with HashJoinContext(device) as ctx:
        held = _Held(ctx)
        try:
            g = _GroupedKeys(ctx, held, k_cols, flags, key_mask)
            m = g.n_groups
            sources = _AggSources(held, plan, n)
            sources.put(ctx, 0, n)
            d_rows = held.put(np.arange(n, dtype=np.uint32))              # the value map: row i reads value i
            d_count = held.put(np.zeros(m, dtype=np.uint64))
            d_acc = [held.put(np.full(m, plan.identity(i), dtype=np.uint64)) for i in range(len(plan.cols))]
            for k, part in enumerate(plan.rounds() if m else []):
                ctx.pairs_agg(g.d_group, d_rows, n, 0, m, 0, n,
                              [sources.pointers(i) + (d_acc[i], plan.cols[i]["op"], plan.cols[i]["width"], plan.cols[i]["flags"]) for i in part],
                              d_count if k == 0 else 0)
            res = plan.result(_fetch_plane(ctx, d_count, m), [_fetch_plane(ctx, d, m) for d in d_acc])
            res.update(keys=g.gather_keys(ctx, held), first_rows=_fetch_map(ctx, g.d_first, m), n_groups=m, null_rows=g.null_rows)
            return res
        finally:
            held.close()


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
