"""Columns of the relational layer, on the host and on the device: KeyColumn (the Arrow layout), the checks of key and
payload column arguments, the host forms of the key hash, and what a wrapper call holds on the device -- its context and
allocations (_session, _Held) and a column's parts there (_DevColumn)."""
import contextlib

import numpy as np

from . import _lib
from ._lib import lib
from .engine import HashJoinContext, HashJoinError, NO_ROW, _key_cols, _key_cols2

_GATHER_WIDTHS = (1, 2, 4, 8, 16)


def _mark_words(n):
    """the 32-bit words of a plane of one bit per row"""
    return (n + 31) // 32


def _ptr(a):
    """the host address of an array for a descriptor of the C ABI; None is 0"""
    return a.ctypes.data if a is not None else 0


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


@contextlib.contextmanager
def _session(device):
    """the context of one wrapper call and its device allocations: (ctx, held); both are gone on leaving"""
    with HashJoinContext(device) as ctx:
        held = _Held(ctx)
        try:
            yield ctx, held
        finally:
            held.close()


def _fetch_map(ctx, d_map, n):
    idx = np.empty(n, dtype=np.uint32)
    if n:
        ctx.copy_d2h(idx, d_map)
    return idx


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
            words = np.zeros(_mark_words(n) or 1, dtype=np.uint32)
            words.view(np.uint8)[:bits.size] = bits
        if self.offsets is None:
            return self.values[lo:lo + n], None, words
        off = self.offsets[lo:lo + n + 1]
        return self.values[int(off[0]):int(off[-1])], off - off[0], words

    def _whole(self):
        """every row, as take gives a slice"""
        return self.take(0, self.rows)


class _DevColumn:
    """One column on the device, the only place its parts are allocated and uploaded. col: a KeyColumn, or a plain 1-D
    array, which has values alone. parts: three device pointers -- values or bytes, offsets, validity words -- 0 where the
    column has no such part. There is room for the largest slice of `step` rows (None: for the whole column), and put()
    uploads one slice into it."""

    def __init__(self, held, col, step=None):
        self.col, self.lo = col, None
        step = len(col) if step is None else step
        if not isinstance(col, KeyColumn):
            room, offsets, valid = step * col.dtype.itemsize, False, False
        elif col.offsets is None:
            room, offsets, valid = step * col.width, False, col.valid is not None
        else:
            los = np.arange(0, col.rows, step) if step else np.empty(0, dtype=np.int64)
            room = int((col.offsets[np.minimum(los + step, col.rows)].astype(np.int64) - col.offsets[los]).max()) if los.size else 0
            offsets, valid = True, col.valid is not None
        # a bytes buffer goes up in whole 32-bit words: the kernels read the aligned words of an element
        self.parts = (held.alloc(room + 3 & ~3), held.alloc(4 * (step + 1)) if offsets else 0, held.alloc(4 * _mark_words(step)) if valid else 0)

    @classmethod
    def whole(cls, ctx, held, col):
        """the whole column, uploaded"""
        dev = cls(held, col)
        dev.put(ctx, 0, len(col))
        return dev

    def put(self, ctx, lo, n):
        """rows [lo, lo + n) of the column go up; no upload when that is the slice already there"""
        if self.lo == lo:
            return
        parts = self.col.take(lo, n) if isinstance(self.col, KeyColumn) else (self.col[lo:lo + n], None, None)
        for d, a in zip(self.parts, parts):
            if a is not None and a.nbytes:
                ctx.copy_h2d(d, a)
        self.lo = lo


# ---- the checks of column arguments ------------------------------------------------------------------------------------------
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


def _as_key_columns(fn, side, keys):
    """the key columns of one side as a list of KeyColumn of one length; ValueError for what cannot be joined on"""
    cols = [keys] if isinstance(keys, (KeyColumn, np.ndarray)) else list(keys)
    if not 1 <= len(cols) <= _lib.HJ_KEY_MAX_COLS:
        raise ValueError(f"{fn}: {side} has {len(cols)} key columns; 1 to {_lib.HJ_KEY_MAX_COLS} can be joined on")
    cols = [c if isinstance(c, KeyColumn) else KeyColumn(c) for c in cols]
    if any(c.rows != cols[0].rows for c in cols):
        raise ValueError(f"{fn}: the key columns of {side} have {[c.rows for c in cols]} rows")
    return cols


def _key_mask(fn, key_mask, integral=False):
    """ValueError for a key_mask that is no 32-bit word. integral: a bool, or what int() would have to round, is none either
    -- the rule of the calls on one table; the joins take whatever int() takes, as they always have"""
    if (integral and (isinstance(key_mask, bool) or not isinstance(key_mask, (int, np.integer)))) or not 0 <= int(key_mask) <= 0xFFFFFFFF:
        raise ValueError(f"{fn}: key_mask must fit 32 bits, not {key_mask!r}")


def _join_key_args(fn, r_keys, s_keys, key_mask, widths_differ):
    """The checks the joins on key columns share, in their order: column c of both sides of one width -- widths_differ is
    the caller's text for the two lists of widths --, key_mask, the rows of a relation. r_keys / s_keys: lists of KeyColumn.
    Returns (rows of R, rows of S)."""
    widths = [[c.width for c in keys] for keys in (r_keys, s_keys)]
    if widths[0] != widths[1]:
        raise ValueError(f"{fn}: " + widths_differ.format(*widths))
    _key_mask(fn, key_mask)
    n_r, n_s = r_keys[0].rows, s_keys[0].rows
    if max(n_r, n_s) > 0xFFFFFFFF:
        raise ValueError(f"{fn}: a relation of more than 2^32 - 1 rows")
    return n_r, n_s


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


# ---- rows of columns taken and put together on the host ---------------------------------------------------------------------
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


def _empty_keys(cols):
    return [_take_key_column(c, np.empty(0, dtype=np.uint32)) for c in cols]


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


# ---- the key hash on the host ------------------------------------------------------------------------------------------------
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


def _host_key_cols2(cols, flags):
    """(what the descriptors point to -- to be kept alive --, the hj_key_col2 array, its length) for host pointers, side S"""
    held = [c._whole() for c in cols]
    arr, k = _key_cols2([(_ptr(v), 0, c.width, _ptr(off), 0, _ptr(words), 0, f) for c, (v, off, words), f in zip(cols, held, flags)])
    return held, arr, k


def key_hash2_host(cols, key_mask=0):
    """hj_key_hash2_host: key_hash_host on key columns in the Arrow layout -- cols is one KeyColumn (or plain / masked 1-D
    numpy array) or a sequence of 1 to HJ_KEY_MAX_COLS of them. Returns the join words as a numpy uint64 array, the tuples
    HashJoinContext.key_hash2 writes for the same columns on the device. A row with a NULL in a column that is not
    nulls_equal is NULL-keyed: its word is a hash of its position, not of its columns (include/htm_hashjoin.h). Needs no
    device."""
    cols = _as_key_columns("key_hash2_host", "cols", cols)
    _key_mask("key_hash2_host", key_mask)
    out = np.empty(cols[0].rows, dtype=np.uint64)
    held, arr, k = _host_key_cols2(cols, [_lib.HJ_KEY_NULLS_EQUAL if c.nulls_equal else 0 for c in cols])
    rc = lib.hj_key_hash2_host(arr, k, _lib.HJ_KEY_SIDE_S, out.size, int(key_mask), out.ctypes.data)
    del held
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, "hj_key_hash2_host")
    return out
