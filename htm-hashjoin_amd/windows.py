"""Window functions over one table: f(...) OVER (PARTITION BY keys ORDER BY cols) (window_rows, window_rows_host) -- the
groups' dense ids, the sort over (id, order columns), one segmented scan along the permutation, and a gather through the
row maps it leaves; sliding frames (ROWS BETWEEN lo AND hi) go along the same permutation through hj_window_frames_dev."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib
from .aggregates import _AGG_DTYPES
from .columns import KeyColumn, _DevColumn, _fetch_map, _host_key_cols2, _ptr, _session, _table_columns, _take_key_column
from .engine import HashJoinError, NO_ROW, _frame_funcs, _sort_cols, _win_funcs
from .groups import _GroupedKeys, _group_key_columns
from .joins import _gather_key_columns
from .sorting import _SortedRows, _sort_columns

_NUMBERS = {"row_number": _lib.HJ_WIN_ROW_NUMBER, "rank": _lib.HJ_WIN_RANK, "dense_rank": _lib.HJ_WIN_DENSE_RANK, "count": _lib.HJ_WIN_PART_ROWS}
_MAPS = {"lag": _lib.HJ_WIN_LAG, "lead": _lib.HJ_WIN_LEAD, "first": _lib.HJ_WIN_FIRST_ROW, "last": _lib.HJ_WIN_LAST_ROW}
_RUNS = {"cumsum": _lib.HJ_WIN_RUN_SUM, "cummin": _lib.HJ_WIN_RUN_MIN, "cummax": _lib.HJ_WIN_RUN_MAX}
_FRAMES = {"sum": _lib.HJ_AGG_SUM, "min": _lib.HJ_AGG_MIN, "max": _lib.HJ_AGG_MAX, "mean": _lib.HJ_AGG_SUM}
_FRAME_FAR = 0xFFFFFFFF
_TAKEN = ("perm", "n_partitions", "null_rows")


class _WindowPlan:
    """The functions of window_rows / window_rows_host, checked. funcs: the device functions, one dict each (op, src: a
    column's name or None, width, flags, offset, dtype and fill of its plane; frame: None for a function of hj_window_rows_dev,
    (lo, hi) for one of hj_window_frames_dev, whose op is an hj_agg_op), the wrapper's own RUN_COUNT of every source of a
    cumsum / cummin / cummax, and COUNT over the same frame of every framed sum / min / max / mean, behind the caller's;
    outputs: how the result dict is put together from their planes.
    ValueError for what cannot be computed."""

    def __init__(self, fn, funcs, cols, n):
        self.fn, self.n, self.funcs, self.outputs, self.counts = fn, n, [], [], {}           # counts: (source, frame) -> its count's function
        self.cols = _table_columns(fn, "the table's", cols, n)
        if not funcs:
            raise ValueError(f"{fn}: no functions")
        for out, spec in dict(funcs).items():
            if out in _TAKEN:
                raise ValueError(f"{fn}: the output name {out!r} is taken")
            name, args = (spec, ()) if isinstance(spec, str) else (spec[0], tuple(spec[1:])) if isinstance(spec, (tuple, list)) and spec else (None, ())
            name = name.lower() if isinstance(name, str) else name
            if name in _NUMBERS and not args:
                self.outputs.append((out, "number", self._func(_NUMBERS[name], np.uint32, 0)))
            elif name in _MAPS and len(args) == (2 if name in ("lag", "lead") else 1):
                k = args[1] if len(args) == 2 else 0
                if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) <= 0xFFFFFFFF:
                    raise ValueError(f"{fn}: function {out!r}: the offset must be 0 .. 2^32 - 1, not {k!r}")
                src = self._column(out, args[0])
                if not isinstance(self.cols[src], KeyColumn):
                    self.cols[src] = KeyColumn(self.cols[src])          # the result has NULLs: it comes back as a KeyColumn
                self.outputs.append((out, "map", self._func(_MAPS[name], np.uint32, NO_ROW, offset=int(k)), src))
            elif name == "cumcount" and len(args) == 1:
                src = None if args[0] is None else self._column(out, args[0])
                self.outputs.append((out, "cumcount", self._count(src)))
            elif name in _RUNS and len(args) == 1:
                src = self._column(out, args[0])
                width, flags = self._agg_type(out, src)
                self.outputs.append((out, "run", self._func(_RUNS[name], np.uint64, 0, src, width, flags), src))
            elif name == "count" and len(args) == 3:
                src = None if args[0] is None else self._column(out, args[0])
                self.outputs.append((out, "cumcount", self._count(src, self._frame(out, args[1], args[2]))))
            elif name in _FRAMES and len(args) == 3:
                src, frame = self._column(out, args[0]), self._frame(out, args[1], args[2])
                width, flags = self._agg_type(out, src)
                self.outputs.append((out, "mean" if name == "mean" else "run", self._func(_FRAMES[name], np.uint64, 0, src, width, flags, frame=frame), src, frame))
            else:
                raise ValueError(f"{fn}: function {out!r} is {spec!r}; 'row_number', 'rank', 'dense_rank', 'count', ('lag' | 'lead', column, k), "
                                 "('first' | 'last', column), ('cumcount', column or None), ('cumsum' | 'cummin' | 'cummax', column) and, over the "
                                 "frame of rows lo .. hi around the current one (None: unbounded), ('sum' | 'min' | 'max' | 'mean', column, lo, hi) "
                                 "and ('count', column or None, lo, hi) exist")
        for _, kind, _, *src in list(self.outputs):
            if kind in ("run", "mean"):
                self._count(*src)               # whether the frame held a value: the column's own count over the same frame

    def _column(self, out, name):
        if not isinstance(name, str) or name not in self.cols:
            raise ValueError(f"{self.fn}: function {out!r} names column {name!r}, which cols does not hold")
        return name

    def _agg_type(self, out, src):
        col = self.cols[src]
        dtype = None if isinstance(col, KeyColumn) and col.offsets is not None else np.asarray(col.values if isinstance(col, KeyColumn) else col).dtype
        if dtype not in _AGG_DTYPES:
            raise ValueError(f"{self.fn}: function {out!r}: column {src!r} is {dtype or 'variable-length'}; int32, uint32, int64 and uint64 "
                             "have running sums, minima and maxima (floating-point sums depend on their order)")
        return _AGG_DTYPES[dtype]

    def _frame(self, out, lo, hi):
        for x in (lo, hi):
            if x is not None and (isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not -_FRAME_FAR <= int(x) <= _FRAME_FAR):
                raise ValueError(f"{self.fn}: function {out!r}: the ends of a frame are integers in -(2^32 - 1) .. 2^32 - 1 or None, not {x!r}")
        if lo is not None and hi is not None and int(lo) > int(hi):
            raise ValueError(f"{self.fn}: function {out!r}: the frame starts at {lo} and ends at {hi}, in front of its start")
        return (None if lo is None else int(lo), None if hi is None else int(hi))

    def _func(self, op, dtype, fill, src=None, width=0, flags=0, offset=0, frame=None):
        self.funcs.append({"op": op, "dtype": np.dtype(dtype), "fill": fill, "src": src, "width": width, "flags": flags, "offset": offset, "frame": frame})
        return len(self.funcs) - 1

    def _count(self, src, frame=None):
        if (src, frame) not in self.counts:
            self.counts[src, frame] = self._func(_lib.HJ_WIN_RUN_COUNT if frame is None else _lib.HJ_AGG_COUNT, np.uint64, 0, src, frame=frame)
        return self.counts[src, frame]

    def reads(self, i):
        """function i reads its source's values, not only its validity"""
        f = self.funcs[i]
        return f["op"] in _RUNS.values() if f["frame"] is None else f["op"] != _lib.HJ_AGG_COUNT

    def rounds(self):
        """the device functions call by call: (framed, their indices) -- those of hj_window_rows_dev in runs of at most
        HJ_WIN_MAX_FUNCS, then those of hj_window_frames_dev in runs of at most HJ_FRAME_MAX_FUNCS"""
        res = []
        for framed, most in ((False, _lib.HJ_WIN_MAX_FUNCS), (True, _lib.HJ_FRAME_MAX_FUNCS)):
            idx = [i for i, f in enumerate(self.funcs) if (f["frame"] is not None) == framed]
            res += [(framed, idx[i:i + most]) for i in range(0, len(idx), most)]
        return res

    def result(self, planes, take, perm, n_partitions, null_rows):
        """planes: one array per device function, indexed by row; take(column name, row map) -> the column's rows there"""
        res = {}
        for out, kind, i, *src in self.outputs:
            if kind in ("number", "cumcount"):
                res[out] = planes[i]
            elif kind == "map":
                res[out] = take(src[0], planes[i])
            else:
                valid = planes[self.counts[tuple(src) if len(src) == 2 else (src[0], None)]] > 0
                values = np.where(valid, planes[i], np.uint64(0))
                values = values.view(np.int64) if self.funcs[i]["flags"] else values
                if kind == "mean":                # of the sum as it stands in 64 bits, wrapped if it wrapped
                    values = np.where(valid, values.astype(np.float64) / np.maximum(planes[self.counts[tuple(src)]], 1).astype(np.float64), 0.0)
                res[out] = KeyColumn(values, valid)
        res.update(perm=perm, n_partitions=int(n_partitions), null_rows=int(null_rows))
        return res


def _window_args(fn, funcs, partition_by, order_by, cols, descending, nulls, null_keys, key_mask):
    """the arguments of window_rows / window_rows_host, checked -> (plan, partition columns and flags or None, order columns
    as _sort_columns gives them, rows)"""
    p_cols = p_flags = None
    o_cols = []
    if partition_by is not None:
        p_cols, p_flags = _group_key_columns(fn, partition_by, null_keys, key_mask)
    else:
        _group_key_columns(fn, np.empty(0, dtype=np.uint32), null_keys, key_mask)      # null_keys and key_mask are checked all the same
    if order_by is not None:
        o_cols = _sort_columns(fn, order_by, descending, nulls)
        if p_cols is not None and len(o_cols) > _lib.HJ_SORT_MAX_COLS - 1:
            raise ValueError(f"{fn}: {len(o_cols)} order columns behind a partition; the sort takes the partition's id and "
                             f"{_lib.HJ_SORT_MAX_COLS - 1} more in a call")
    sizes = ([p_cols[0].rows] if p_cols else []) + ([o_cols[0][0].rows] if o_cols else [])
    if not sizes:
        sizes = [len(c) for c in dict(cols or {}).values()][:1]
        if not sizes:
            raise ValueError(f"{fn}: neither partition_by, order_by nor a column says how many rows the table has")
    if len(set(sizes)) != 1:
        raise ValueError(f"{fn}: partition_by has {sizes[0]} rows, order_by {sizes[1]}")
    if sizes[0] > 0xFFFFFFFE:
        raise ValueError(f"{fn}: a table of more than 2^32 - 2 rows")
    return _WindowPlan(fn, funcs, cols, sizes[0]), p_cols, p_flags, o_cols, sizes[0]


def _empty_result(plan):
    e = np.empty(0, dtype=np.uint32)
    return plan.result([np.empty(0, dtype=f["dtype"]) for f in plan.funcs], lambda name, idx: _take_key_column(plan.cols[name], idx), e, 0, 0)


def window_rows_host(funcs, partition_by=None, order_by=None, cols=None, descending=False, nulls="last", null_keys="group", key_mask=0):
    """window_rows on the host: hj_key_groups_host, hj_sort_rows_host and hj_window_rows_host, then the row maps taken on the
    host; needs no device. Arguments and result as in window_rows."""
    fn = "window_rows_host"
    plan, p_cols, p_flags, o_cols, n = _window_args(fn, funcs, partition_by, order_by, cols, descending, nulls, null_keys, key_mask)
    if n == 0:
        return _empty_result(plan)
    ids, null_rows, out = None, 0, (C.c_uint64 * 8)()
    if p_cols is not None:
        ids, rep = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
        held, arr, k = _host_key_cols2(p_cols, p_flags)
        rc = lib.hj_key_groups_host(arr, k, _lib.HJ_KEY_SIDE_S, n, int(key_mask), rep.ctypes.data, ids.ctypes.data, None, 0, out)
        del held
        if rc != _lib.HJ_OK:
            raise HashJoinError(rc, "hj_key_groups_host")
        null_rows = int(out[3])
    o_held = [c._whole() for c, _, _ in o_cols]
    o_desc = [(_ptr(v), _ptr(words), c.width, t, f) for (c, t, f), (v, _, words) in zip(o_cols, o_held)]
    perm = None
    if ids is not None or o_desc:
        perm = np.empty(n, dtype=np.uint32)
        arr, k = _sort_cols(([(ids.ctypes.data, 0, 4, _lib.HJ_VAL_UINT, 0)] if ids is not None else []) + o_desc)
        rc = lib.hj_sort_rows_host(arr, k, n, perm.ctypes.data, None)
        if rc != _lib.HJ_OK:
            raise HashJoinError(rc, "hj_sort_rows_host")
    n_pos = n - null_rows
    # (values, validity words) of every column a function may read
    srcs = {name: (c._whole()[0], c._whole()[2]) if isinstance(c, KeyColumn) else (c, None) for name, c in plan.cols.items()}
    planes = [np.full(n, f["fill"], dtype=f["dtype"]) for f in plan.funcs]
    o_arr, n_order = _sort_cols(o_desc)
    for framed, part in plan.rounds():
        desc = []
        for i in part:
            f = plan.funcs[i]
            v, words = srcs[f["src"]] if f["src"] is not None else (None, None)
            ptrs = (_ptr(v) if plan.reads(i) else 0, _ptr(words), f["width"], f["flags"])
            desc.append((f["op"], planes[i].ctypes.data) + (f["frame"] + ptrs if framed else ptrs + (f["offset"],)))
        if framed:
            f_arr, n_funcs = _frame_funcs(desc)
            rc = lib.hj_window_frames_host(_ptr(perm), n_pos, n, _ptr(ids), f_arr, n_funcs, out)
        else:
            f_arr, n_funcs = _win_funcs(desc)
            rc = lib.hj_window_rows_host(_ptr(perm), n_pos, n, _ptr(ids), o_arr, n_order, f_arr, n_funcs, out)
        if rc != _lib.HJ_OK:
            raise HashJoinError(rc, "hj_window_frames_host" if framed else "hj_window_rows_host")
    del o_held, srcs
    rows = perm[:n_pos] if perm is not None else np.arange(n, dtype=np.uint32)
    return plan.result(planes, lambda name, idx: _take_key_column(plan.cols[name], idx), rows, out[1], null_rows)


def window_rows(funcs, partition_by=None, order_by=None, cols=None, descending=False, nulls="last", null_keys="group", key_mask=0, device=0):
    """f(...) OVER (PARTITION BY partition_by ORDER BY order_by) over ONE table, every result in ROW order (pandas'
    groupby().cumcount() / .rank() / .shift() / .cumsum()). partition_by: what key_groups takes (64-bit, composite,
    NULL-aware, string keys), with null_keys ("group" | "drop") and key_mask as its nulls and key_mask; None: one partition.
    order_by, descending, nulls: what sort_rows takes; behind a partition at most HJ_SORT_MAX_COLS - 1 columns; None: the
    rows of a partition stay in row order and are all peers. cols: {name: column} as sort_by_columns takes them.
    funcs: {output name: spec}, a spec one of
      "row_number" | "rank" | "dense_rank" | "count"    uint32 per row: the position in the partition from 1, the rank with
                                                        gaps and without, the rows of the partition
      ("lag" | "lead", column, k), ("first" | "last", column)
                                                        the column's value k rows before / behind in the partition, of its
                                                        first / last row: a KeyColumn (strings included), NULL where there
                                                        is no such row or the source is NULL
      ("cumcount", column or None)                      uint64 per row: the valid values so far, None: the rows so far
      ("cumsum" | "cummin" | "cummax", column)          over int32 / uint32 / int64 / uint64 values so far, the current row
                                                        included: a KeyColumn as group_by_columns returns SUM / MIN / MAX,
                                                        NULL where no valid value came yet; SUM wraps modulo 2^64
      ("sum" | "min" | "max", column, lo, hi)           over the FRAME of rows lo .. hi around the current one in its partition
                                                        (ROWS BETWEEN; integers relative to the row, negative: preceding,
                                                        None: unbounded): ("sum", "v", -6, 0) is pandas' rolling(7,
                                                        min_periods=1).sum(), ("max", "v", None, None) transform("max"),
                                                        (-3, -1) leaves the row itself out. A KeyColumn as cumsum returns, NULL
                                                        where the frame held no valid value
      ("count", column or None, lo, hi)                 uint64 per row: the valid values in the frame, None: its rows
      ("mean", column, lo, hi)                          float64 KeyColumn: the frame's sum over its count, NULL where the
                                                        count is 0. The mean of the WRAPPED sum: a sum that left 64 bits
                                                        gives the mean of what is left
    On the device: hj_key_groups_dev gives the ids, hj_sort_rows_dev sorts by (id, order columns) -- with neither there is
    no sort --, one hj_window_rows_dev per HJ_WIN_MAX_FUNCS functions scans along the permutation, one hj_window_frames_dev
    per HJ_FRAME_MAX_FUNCS framed functions goes along the same ids and permutation, hj_gather2_dev goes through the row
    maps; the ids, the permutation and the maps never leave the device on the way. null_keys="drop": the
    rows with a NULL in a partition key stand at no position -- their numbers are 0, everything else is NULL.
    Returns the outputs and "perm" (the rows in partition and order, dropped rows left out), "n_partitions", "null_rows".
    An empty table is answered without a device."""
    fn = "window_rows"
    plan, p_cols, p_flags, o_cols, n = _window_args(fn, funcs, partition_by, order_by, cols, descending, nulls, null_keys, key_mask)
    if n == 0:
        return _empty_result(plan)
    with _session(device) as (ctx, held):
        d_ids, d_perm, null_rows, lead = 0, 0, 0, []
        if p_cols is not None:
            g = _GroupedKeys(ctx, held, p_cols, p_flags, key_mask)
            d_ids, null_rows, lead = g.d_group, g.null_rows, [(g.d_group, 0, 4, _lib.HJ_VAL_UINT, 0)]
        o_dev = []
        if lead or o_cols:
            s = _SortedRows(ctx, held, o_cols, lead=lead, n=n)
            d_perm, o_dev = s.d_perm, s.dev
        order = [(d.parts[0], d.parts[2], c.width, t, f) for d, (c, t, f) in zip(o_dev, o_cols)]
        n_pos = n - null_rows
        dev = {}

        def column(name):
            if name not in dev:
                dev[name] = _DevColumn.whole(ctx, held, plan.cols[name])
            return dev[name]

        d_out = [held.put(np.full(n, f["fill"], dtype=f["dtype"])) if n_pos < n else held.alloc(n * f["dtype"].itemsize) for f in plan.funcs]
        n_partitions = 0
        for k, (framed, part) in enumerate(plan.rounds()):
            desc = []
            for i in part:
                f = plan.funcs[i]
                d_v, _, d_valid = column(f["src"]).parts if f["src"] is not None else (0, 0, 0)
                ptrs = (d_v if plan.reads(i) else 0, d_valid, f["width"], f["flags"])
                desc.append((f["op"], d_out[i]) + (f["frame"] + ptrs if framed else ptrs + (f["offset"],)))
            if framed:
                ctx.window_frames(d_perm, n_pos, n, d_ids, desc)
            else:
                ctx.window_rows(d_perm, n_pos, n, d_ids, order, desc)
            if k == 0:
                n_partitions = (ctx.window_frames_info() if framed else ctx.window_rows_info())["partitions"]
        planes = [None] * len(plan.funcs)
        maps = {i for _, kind, i, *_ in plan.outputs if kind == "map"}
        for i, f in enumerate(plan.funcs):
            if i not in maps:
                planes[i] = np.empty(n, dtype=f["dtype"])
                ctx.copy_d2h(planes[i], d_out[i])
            else:
                planes[i] = d_out[i]

        def take(name, d_map):
            return _gather_key_columns(ctx, held, d_map, n, 0, n, [(name, column(name))])[name]

        rows = _fetch_map(ctx, d_perm, n_pos) if d_perm else np.arange(n, dtype=np.uint32)
        return plan.result(planes, take, rows, n_partitions, null_rows)
