"""Aggregating joins: COUNT / SUM / MIN / MAX of S values per R row, without the pairs (radix_join_aggregate, aggregate_on)."""
import numpy as np

from . import _lib
from .columns import KeyColumn, _DevColumn, _as_key_columns, _join_key_args, _session
from .conditions import _PairChain
from .joins import _drive_join, _slice_step
from .key_joins import _COLUMN_WIDTHS_DIFFER, _ColumnKeys

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
        self.dev = {name: _DevColumn(held, c, step) for name, c in plan.sources.items() if any(col["src"] == name for col in plan.cols)}

    def put(self, ctx, lo, n, names=None):
        for name, dev in self.dev.items():
            if names is None or name in names:
                dev.put(ctx, lo, n)

    def pointers(self, i):
        """(src, valid) of device column i; a COUNT reads no value"""
        col = self.plan.cols[i]
        if col["src"] is None:
            return 0, 0
        d_v, _, d_valid = self.dev[col["src"]].parts
        return (0 if col["op"] == _lib.HJ_AGG_COUNT else d_v), d_valid


class _PairsReduction:
    """The accumulators of a reduction over pair lists (HashJoinContext.pairs_agg), one per device column of the plan and
    the counts, g_rows entries each, on the device from the start; reduce() adds a pair list, fetch() reads them back as
    (count, planes)."""

    def __init__(self, held, plan, sources, g_rows):
        self.plan, self.sources, self.g_rows = plan, sources, g_rows
        self.d_count = held.put(np.zeros(g_rows, dtype=np.uint64))
        self.d_acc = [held.put(np.full(g_rows, plan.identity(i), dtype=np.uint64)) for i in range(len(plan.cols))]

    def reduce(self, ctx, d_map_g, d_map_v, n_pairs, v_base, v_rows):
        plan = self.plan
        for k, cols in enumerate(plan.rounds()):
            ctx.pairs_agg(d_map_g, d_map_v, n_pairs, 0, self.g_rows, v_base, v_rows,
                          [self.sources.pointers(i) + (self.d_acc[i], plan.cols[i]["op"], plan.cols[i]["width"], plan.cols[i]["flags"])
                           for i in cols], self.d_count if k == 0 else 0)

    def fetch(self, ctx):
        return _fetch_plane(ctx, self.d_count, self.g_rows), [_fetch_plane(ctx, d, self.g_rows) for d in self.d_acc]


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
    with _session(device) as (ctx, held):
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
    return plan.result(count, planes)


class _ReduceChain(_PairChain):
    """aggregate_on's chain: the verify step alone, and as its tail the reduction of the slice's kept pairs, grouped by the R
    plane; after() -- _drive_join's `after` -- reads the accumulators back into .out = (count, planes)"""

    def __init__(self, keys, plan, n_r, step):
        super().__init__([keys], n_r, step, True)
        self.plan, self.acc = plan, None

    def tail(self, ctx, held, lo, n, d_ks, d_kr, kept):
        if self.acc is None:
            self.acc = _PairsReduction(held, self.plan, _AggSources(held, self.plan, self.step), self.n_r)
        self.acc.sources.put(ctx, lo, n)
        self.acc.reduce(ctx, d_kr, d_ks, kept, lo, n)

    def after(self, ctx, held):
        self.out = self.acc.fetch(ctx)


def aggregate_on(r_keys, s_keys, s_cols, aggs, nulls_equal=False, radixBits=0, slice_tuples=None, device=0, key_mask=0):
    """radix_join_aggregate for joins on real key columns: GROUP BY <R row> over the inner join of join_on_columns(r_keys,
    s_keys, nulls_equal=...), by its method -- key_hash2, the candidate join on the hashed word, pairs_verify2 -- with
    hj_pairs_agg_dev over the KEPT pairs of each slice in place of the gather (a reduction over the candidates would
    count what the verify step rejects). r_keys / s_keys, nulls_equal, radixBits, slice_tuples, key_mask: as in
    join_on_columns; s_cols, aggs and the result dict: as in radix_join_aggregate, one entry per row of R."""
    fn = "aggregate_on"
    r_keys, s_keys = _as_key_columns(fn, "R", r_keys), _as_key_columns(fn, "S", s_keys)
    n_r, n_s = _join_key_args(fn, r_keys, s_keys, key_mask, _COLUMN_WIDTHS_DIFFER)
    plan = _AggPlan(fn, s_cols, aggs, n_s)
    if n_r == 0 or n_s == 0:
        return plan.without_device(n_r)
    step = _slice_step(fn, n_s, slice_tuples)
    keys = _ColumnKeys(r_keys, s_keys, nulls_equal, key_mask, step)
    chain = _ReduceChain(keys, plan, n_r, step)
    _drive_join(np.empty(n_r, dtype=np.uint8), np.empty(n_s, dtype=np.uint8), "radix", _lib.HJ_JOIN_INNER, None, step, chain.slice, device,
                radixBits=radixBits, fill=keys.hash_keys, after=chain.after)
    return plan.result(*chain.out)
