"""The rows of one table grouped by their key columns: DISTINCT, GROUP BY key, a dense group id (key_groups, key_groups_host,
distinct_on, group_by_columns)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib
from .aggregates import _AggPlan, _AggSources, _PairsReduction
from .columns import (_DevColumn, _as_key_columns, _empty_keys, _fetch_map, _host_key_cols2, _key_mask, _session, _table_columns,
                      _take_on_host)
from .engine import HashJoinError
from .joins import _gather_key_columns, _gather_side

_GROUP_NULLS = ("group", "drop")


def _group_key_columns(fn, keys, nulls, key_mask):
    """the key columns of key_groups / distinct_on / group_by_columns, checked -> (list of KeyColumn, their flags)"""
    if not isinstance(nulls, str) or nulls not in _GROUP_NULLS:
        raise ValueError(f"{fn}: nulls must be 'group' or 'drop', not {nulls!r}")
    _key_mask(fn, key_mask, integral=True)
    cols = _as_key_columns(fn, "keys", keys)
    if cols[0].rows > 0xFFFFFFFE:
        raise ValueError(f"{fn}: a table of more than 2^32 - 2 rows")
    return cols, [_lib.HJ_KEY_NULLS_EQUAL if nulls == "group" or c.nulls_equal else 0 for c in cols]


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
    n_groups, null_rows. dev: the _DevColumn of every key column, for a gather behind it."""

    def __init__(self, ctx, held, cols, flags, key_mask):
        n = cols[0].rows
        self.n = n
        self.dev = [_DevColumn.whole(ctx, held, c) for c in cols]
        desc = [(d.parts[0], 0, d.col.width, d.parts[1], 0, d.parts[2], 0, f) for d, f in zip(self.dev, flags)]
        self.d_rep, self.d_group, self.d_first = held.alloc(4 * n), held.alloc(4 * n), held.alloc(4 * n)
        ctx.key_groups(desc, _lib.HJ_KEY_SIDE_S, n, self.d_rep, self.d_group, self.d_first, n, int(key_mask))
        info = ctx.key_groups_info()
        if info["failure"]:
            raise HashJoinError(_lib.HJ_ERR_STATE, f"hj_key_groups_dev: the device reported failure word {info['failure']}")
        self.n_groups, self.null_rows = info["groups"], info["null_rows"]

    def gather_keys(self, ctx, held):
        """the key columns of the first rows, one KeyColumn per key column"""
        got = _gather_key_columns(ctx, held, self.d_first, self.n_groups, 0, self.n, list(enumerate(self.dev)))
        return [got[k] for k in range(len(self.dev))]


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
    with _session(device) as (ctx, held):
        g = _GroupedKeys(ctx, held, cols, flags, key_mask)
        return _groups_result(_fetch_map(ctx, g.d_rep, n), _fetch_map(ctx, g.d_group, n), _fetch_map(ctx, g.d_first, g.n_groups),
                              g.n_groups, g.null_rows)


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
    with _session(device) as (ctx, held):
        g = _GroupedKeys(ctx, held, k_cols, flags, key_mask)
        d_cols = [(name, _DevColumn.whole(ctx, held, c)) for name, c in cols.items()]
        payload, _ = _gather_side(ctx, held, g.d_first, g.n_groups, 0, n, d_cols)
        return {"first_rows": _fetch_map(ctx, g.d_first, g.n_groups), "keys": g.gather_keys(ctx, held), "cols": payload,
                "n_groups": g.n_groups, "null_rows": g.null_rows}


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
    with _session(device) as (ctx, held):
        g = _GroupedKeys(ctx, held, k_cols, flags, key_mask)
        m = g.n_groups
        sources = _AggSources(held, plan, n)
        sources.put(ctx, 0, n)
        d_rows = held.put(np.arange(n, dtype=np.uint32))              # the value map: row i reads value i
        acc = _PairsReduction(held, plan, sources, m)
        if m:
            acc.reduce(ctx, g.d_group, d_rows, n, 0, n)
        res = plan.result(*acc.fetch(ctx))
        res.update(keys=g.gather_keys(ctx, held), first_rows=_fetch_map(ctx, g.d_first, m), n_groups=m, null_rows=g.null_rows)
        return res
