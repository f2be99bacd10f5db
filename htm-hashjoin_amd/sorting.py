"""The rows of one table in the order of their key columns: ORDER BY (sort_rows, sort_rows_host, sort_by_columns) and the
canonical order of a join's two gather maps (sort_pairs)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib
from .columns import KeyColumn, _DevColumn, _fetch_map, _ptr, _session, _table_columns, _take_key_column, _take_on_host
from .engine import HashJoinError, _sort_cols
from .joins import _gather_key_columns, _gather_side

_NULLS = ("last", "first")


def _val_type(fn, dtype):
    """the hj_val_type a dtype's elements are read as; ValueError for what cannot be ordered"""
    dtype = np.dtype(dtype)
    if dtype.kind in "ub" and dtype.itemsize in (1, 2, 4, 8):
        return _lib.HJ_VAL_UINT
    if dtype.kind == "i" and dtype.itemsize in (1, 2, 4, 8):
        return _lib.HJ_VAL_INT
    if dtype.kind == "f" and dtype.itemsize in (4, 8):
        return _lib.HJ_VAL_FLOAT
    raise ValueError(f"{fn}: {dtype} elements cannot be ordered; integers of 1, 2, 4 or 8 bytes and float32 / float64 can "
                     "(no strings, no 16-byte elements, no 16-bit floats)")


def _is_column(x):
    return isinstance(x, (KeyColumn, np.ndarray))


def _is_typed_column(x):
    """(KeyColumn, dtype): a fixed-width column whose elements are to be read as dtype"""
    return isinstance(x, tuple) and len(x) == 2 and isinstance(x[0], KeyColumn) and not _is_column(x[1])


def _per_column(fn, name, value, k, ok):
    """one value or one per column -> a list of k checked values"""
    vals = list(value) if isinstance(value, (list, tuple, np.ndarray)) else [value] * k
    if len(vals) != k or not all(ok(v) for v in vals):
        raise ValueError(f"{fn}: {name} must be one value or one per key column ({k}), not {value!r}")
    return vals


def _sort_columns(fn, keys, descending, nulls):
    """the key columns of sort_rows / sort_by_columns, checked -> [(KeyColumn, hj_val_type, flags)], most significant first"""
    items = [keys] if _is_column(keys) or _is_typed_column(keys) else list(keys)
    if not 1 <= len(items) <= _lib.HJ_SORT_MAX_COLS:
        raise ValueError(f"{fn}: {len(items)} key columns; 1 to {_lib.HJ_SORT_MAX_COLS} can be sorted by in a call")
    desc = _per_column(fn, "descending", descending, len(items), lambda v: isinstance(v, (bool, np.bool_)))
    where = _per_column(fn, "nulls", nulls, len(items), lambda v: isinstance(v, str) and v in _NULLS)
    out = []
    for item, d, w in zip(items, desc, where):
        col, dtype = item if _is_typed_column(item) else (item, None)
        col = col if isinstance(col, KeyColumn) else KeyColumn(col)
        if col.offsets is not None:
            raise ValueError(f"{fn}: a variable-length key column; strings cannot be sorted by (fixed elements of 1, 2, 4 or 8 bytes can)")
        dtype = col.values.dtype if dtype is None else np.dtype(dtype)
        if dtype.itemsize != col.width:
            raise ValueError(f"{fn}: a column of {col.width}-byte elements cannot be read as {dtype}")
        out.append((col, _val_type(fn, dtype), (_lib.HJ_SORT_DESC if d else 0) | (_lib.HJ_SORT_NULLS_FIRST if w == "first" else 0)))
    if any(c.rows != out[0][0].rows for c, _, _ in out):
        raise ValueError(f"{fn}: the key columns have {[c.rows for c, _, _ in out]} rows")
    if out[0][0].rows > 0xFFFFFFFE:
        raise ValueError(f"{fn}: a table of more than 2^32 - 2 rows")
    return out


def sort_rows_host(keys, descending=False, nulls="last"):
    """hj_sort_rows_host: sort_rows on the host, by the kernels' order key around a stable sort; needs no device. Arguments
    and result as in sort_rows."""
    fn = "sort_rows_host"
    cols = _sort_columns(fn, keys, descending, nulls)
    n = cols[0][0].rows
    perm = np.empty(n, dtype=np.uint32)
    held = [c._whole() for c, _, _ in cols]
    arr, k = _sort_cols([(_ptr(v), _ptr(words), c.width, t, f) for (c, t, f), (v, _, words) in zip(cols, held)])
    rc = lib.hj_sort_rows_host(arr, k, n, perm.ctypes.data if n else None, (C.c_uint64 * 8)())
    del held
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, "hj_sort_rows_host")
    return perm


class _SortedRows:
    """What sort_rows and sort_by_columns share: the key columns on the device, one hj_sort_rows_dev over them, and the
    permutation it left in d_perm. dev: the _DevColumn of every key column, for a gather behind it. lead: descriptors of
    columns that lie on the device already (window_rows' partition ids), more significant than cols; n: the rows, where
    cols may be empty."""

    def __init__(self, ctx, held, cols, lead=(), n=None):
        self.n = cols[0][0].rows if n is None else n
        self.dev = [_DevColumn.whole(ctx, held, c) for c, _, _ in cols]
        self.d_perm = held.alloc(4 * self.n)
        ctx.sort_rows(list(lead) + [(d.parts[0], d.parts[2], c.width, t, f) for d, (c, t, f) in zip(self.dev, cols)], self.n, self.d_perm)


def sort_rows(keys, descending=False, nulls="last", device=0):
    """The rows of ONE table in the order of its key columns (hj_sort_rows_dev): ORDER BY, as a uint32 permutation -- row k
    of the sorted table is row perm[k] of the input. keys: one 1-D numpy array of an integer dtype or float32 / float64 (a
    numpy.ma.MaskedArray brings its mask), a fixed-width KeyColumn (its values' dtype says how the elements are read; a
    tuple (KeyColumn, dtype) says it apart), or a sequence of 1 to HJ_SORT_MAX_COLS of them, all of one length, the most
    significant first. descending (bool) and nulls ("last" | "first"): one value, or one per column. Integers order by
    width and signedness; floats as IEEE values with -0.0 == 0.0 and every NaN one value above +inf (numpy's order);
    NULLs stand last, or first with nulls="first", whatever the direction (pandas' na_position). Rows that tie in every
    column keep their input order: the sort is stable, the result unique. ValueError for a variable-length (string)
    column, 16-byte elements and 16-bit floats. An empty table is answered without a device."""
    cols = _sort_columns("sort_rows", keys, descending, nulls)
    n = cols[0][0].rows
    if n == 0:
        return np.empty(0, dtype=np.uint32)
    with _session(device) as (ctx, held):
        return _fetch_map(ctx, _SortedRows(ctx, held, cols).d_perm, n)


def sort_by_columns(keys, cols=None, descending=False, nulls="last", limit=None, device=0):
    """SELECT ... ORDER BY keys [LIMIT limit]: keys, descending, nulls as in sort_rows. cols: {name: values} payload columns
    of the table as distinct_on takes them (numpy arrays of 1, 2, 4, 8 or 16-byte elements, or KeyColumns -- strings
    included --, which stay KeyColumns), gathered through the permutation on the device (hj_gather2_dev / hj_gather_dev):
    the permutation goes from the sort into the gather where it lies. limit=k keeps the first k rows (the sort is still
    complete). Returns {"rows": the permutation (its first k entries), "keys": one KeyColumn per key column in sorted
    order, "cols": {name: column}}. An empty table is answered without a device."""
    fn = "sort_by_columns"
    k_cols = _sort_columns(fn, keys, descending, nulls)
    n = k_cols[0][0].rows
    cols = _table_columns(fn, "the table's", cols, n)
    if limit is not None and (isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or limit < 0):
        raise ValueError(f"{fn}: limit must be None or a count, not {limit!r}")
    m = n if limit is None else min(int(limit), n)
    if n == 0:
        e = np.empty(0, dtype=np.uint32)
        return {"rows": e, "keys": [_take_key_column(c, e) for c, _, _ in k_cols], "cols": _take_on_host(cols, e)[0]}
    with _session(device) as (ctx, held):
        s = _SortedRows(ctx, held, k_cols)
        got = _gather_key_columns(ctx, held, s.d_perm, m, 0, n, list(enumerate(s.dev)))
        d_cols = [(name, _DevColumn.whole(ctx, held, c)) for name, c in cols.items()]
        payload, _ = _gather_side(ctx, held, s.d_perm, m, 0, n, d_cols)
        return {"rows": _fetch_map(ctx, s.d_perm, m), "keys": [got[k] for k in range(len(s.dev))], "cols": payload}


def sort_pairs(s_idx, r_idx, device=0):
    """The canonical order of a join's two gather maps: (s_idx, r_idx) as the pairs wrappers return them -> the same pairs
    sorted by S row, then R row. NO_ROW is 0xFFFFFFFF and therefore sorts last, which is where an outer join's tail
    belongs. It is sort_rows on two uint32 columns and one gather of both maps through the permutation on the device: two
    results of one join compare equal element for element after it, without a sort on the host."""
    fn = "sort_pairs"
    s_idx, r_idx = np.asarray(s_idx), np.asarray(r_idx)
    if s_idx.dtype != np.uint32 or r_idx.dtype != np.uint32 or s_idx.ndim != 1 or s_idx.shape != r_idx.shape:
        raise ValueError(f"{fn}: s_idx and r_idx must be 1-D uint32 arrays of one length")
    cols = _sort_columns(fn, [s_idx, r_idx], False, "last")
    n = s_idx.size
    if n == 0:
        return s_idx.copy(), r_idx.copy()
    with _session(device) as (ctx, held):
        s = _SortedRows(ctx, held, cols)
        out, _ = _gather_side(ctx, held, s.d_perm, n, 0, n, [("s", s.dev[0]), ("r", s.dev[1])])
        return out["s"].values, out["r"].values
