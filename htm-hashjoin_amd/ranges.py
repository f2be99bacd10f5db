"""Range joins without an equality key: R.y BETWEEN S.lo AND S.hi (range_join), the same join with the sides swapped
(interval_join), and the host form of both (range_join_host). R's column is indexed once -- sorted, with the plane of its
order keys -- and S goes through in slices, every slice one HashJoinContext.range_pairs call; that call is the source of
pairs of a _RowChain, so where= and all eight kinds are the relational layer's own."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib
from .columns import _DevColumn, _mark_words, _ptr, _session, _table_columns, _take_on_host
from .conditions import _RowChain, _WhereStep, _where_side, _where_terms, _WHERE_TYPES, pairs_where_host
from .engine import HashJoinError, NO_ROW, _sort_cols
from .joins import _TableRows, _slice_step, _table_how

_MIRROR_HOW = {"inner": "inner", "full": "full", "left": "right", "right": "left", "semi": "right_semi", "right_semi": "semi",
               "anti": "right_anti", "right_anti": "anti"}
_MIRROR_OP = {"==": "==", "!=": "!=", "<": ">", "<=": ">=", ">": "<", ">=": "<="}


def range_layout_info(n_rows, s_rows=0):
    """hj_range_layout_info: how range_pairs cuts an index of n_rows rows probed by s_rows S rows -- pivots (searched in LDS),
    their stride, the pair tile of the expansion, workspace bytes, chunk rows, chunks, the LDS bytes the pivots may take.
    Host-only; no device."""
    out = (C.c_uint64 * 8)()
    rc = lib.hj_range_layout_info(int(n_rows), int(s_rows), out)
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, "hj_range_layout_info")
    return {"pivots": int(out[0]), "stride": int(out[1]), "tile": int(out[2]), "workspace_bytes": int(out[3]), "chunk_rows": int(out[4]),
            "chunks": int(out[5]), "lds_bytes": int(out[6])}


def _range_args(fn, r_values, s_lo, s_hi, lo_open, hi_open, pick):
    """the three columns as KeyColumns of one dtype (a missing bound: None), then hj_val_type, width, flags, hj_range_pick"""
    if s_lo is None and s_hi is None:
        raise ValueError(f"{fn}: a range has a bound: s_lo, s_hi or both")
    if not isinstance(pick, str) or pick not in _lib.RANGE_PICKS:
        raise ValueError(f"{fn}: pick must be one of {', '.join(_lib.RANGE_PICKS)}, not {pick!r}")
    r = _where_side(fn, "R", r_values, None, "the range")
    lo = None if s_lo is None else _where_side(fn, "S", s_lo, None, "the range")
    hi = None if s_hi is None else _where_side(fn, "S", s_hi, lo.rows if lo is not None else None, "the range")
    for b in (lo, hi):
        if b is not None and b.values.dtype != r.values.dtype:
            raise ValueError(f"{fn}: the range compares {b.values.dtype} (S) with {r.values.dtype} (R); there is no implicit cast")
    if max(r.rows, (lo if lo is not None else hi).rows) > 0xFFFFFFFE:
        raise ValueError(f"{fn}: a relation of more than 2^32 - 2 rows")
    flags = (_lib.HJ_RANGE_LO_OPEN if lo_open else 0) | (_lib.HJ_RANGE_HI_OPEN if hi_open else 0)
    return r, lo, hi, _WHERE_TYPES[r.values.dtype.kind], r.width, flags, _lib.RANGE_PICKS[pick]


class _RangeChain(_RowChain):
    """The chain of a range join: its source of pairs is the range call, source(ctx, lo, n, d_s, d_r, capacity, d_s_marks,
    d_r_marks) -> the pairs of the slice. With steps (where=) the source runs twice -- the sizing pass, then the pairs -- and
    the steps own the mark planes; without, the range call owns them, and a kind that returns no pair never expands one."""

    def __init__(self, steps, rows, n_r, step, source):
        super().__init__(steps, rows, n_r, step)
        self.source = source

    def _pairs(self, ctx, held, lo, n, total):
        if total > 0xFFFFFFFF:
            raise HashJoinError(_lib.HJ_ERR_INVALID, f"the slice of {n} S rows from {lo} has {total} pairs, above 2^32 - 1: use a smaller slice_rows")
        d_s, d_r = held.alloc(4 * total), held.alloc(4 * total)
        if total:
            self.source(ctx, lo, n, d_s, d_r, total, 0, 0)
        return d_s, d_r

    def range_slice(self, ctx, held, lo, n):
        if self.steps:
            total = self.source(ctx, lo, n, 0, 0, 0, 0, 0)
            d_s, d_r = self._pairs(ctx, held, lo, n, total)
            self.slice(ctx, held, lo, n, d_s, d_r, total)
            held.free(d_s, d_r)
            return
        if self.marks is None:
            self.marks = held.alloc(4 * _mark_words(self.step)), held.put(np.zeros(_mark_words(self.n_r), dtype=np.uint32))
        ctx.copy_h2d(self.marks[0], np.zeros(_mark_words(n), dtype=np.uint32))
        total = self.source(ctx, lo, n, 0, 0, 0, *self.marks)
        d_s, d_r = self._pairs(ctx, held, lo, n, total) if self.keep else (0, 0)
        self.tail(ctx, held, lo, n, d_s, d_r, total if self.keep else 0)
        if self.keep:
            held.free(d_s, d_r)


def _range_join(fn, r_values, s_lo, s_hi, lo_open, hi_open, pick, r_cols, s_cols, how, where, slice_rows, device):
    _table_how(fn, how)
    r, lo, hi, type_, width, flags, pick_id = _range_args(fn, r_values, s_lo, s_hi, lo_open, hi_open, pick)
    n_r, n_s = r.rows, (lo if lo is not None else hi).rows
    r_cols, s_cols = _table_columns(fn, "R", r_cols, n_r), _table_columns(fn, "S", s_cols, n_s)
    step = _slice_step(fn, n_s, slice_rows) if n_s else 0
    terms = _where_terms(fn, where, n_s, n_r)
    rows = _TableRows(how, r_cols, s_cols, n_r, step)
    trivial = rows.without_device(n_s)
    if trivial is not None:
        return trivial
    with _session(device) as (ctx, held):
        r_dev = _DevColumn.whole(ctx, held, r)
        d_perm, d_keys, d_head = held.alloc(4 * n_r), held.alloc((8 if width == 8 else 4) * n_r), held.alloc(16)
        ctx.range_index((r_dev.parts[0], r_dev.parts[2], width, type_), n_r, d_perm, d_keys, d_head)
        lo_dev, hi_dev = (None if b is None else _DevColumn(held, b, step) for b in (lo, hi))

        def source(ctx, at, n, d_s, d_r, capacity, d_s_marks, d_r_marks):
            for dev in (lo_dev, hi_dev):
                if dev is not None:
                    dev.put(ctx, at, n)
            term = (lo_dev.parts[0] if lo_dev is not None else 0, hi_dev.parts[0] if hi_dev is not None else 0, width, type_, flags, pick_id,
                    lo_dev.parts[2] if lo_dev is not None else 0, hi_dev.parts[2] if hi_dev is not None else 0)
            ctx.range_pairs(d_keys, d_perm, d_head, n_r, term, n, at, d_s, d_r, capacity, d_s_marks, d_r_marks)
            return ctx.range_pairs_info()[0]

        chain = _RangeChain([_WhereStep(terms, step)] if terms is not None else [], rows, n_r, step, source)
        for at in range(0, n_s, step):
            chain.range_slice(ctx, held, at, min(step, n_s - at))
        if chain.marks is not None:
            chain.after(ctx, held)
    return rows.joined()


def range_join(r_values, s_lo=None, s_hi=None, lo_open=False, hi_open=False, pick="all", r_cols=None, s_cols=None, how="inner", where=None,
               slice_rows=None, device=0):
    """The join on an order condition alone: S row s matches R row r when s_lo[s] <= r_values[r] <= s_hi[s] (lo_open / hi_open:
    < on that side; a bound that is None: no bound on that side, not both). r_values, s_lo, s_hi: 1-D numpy arrays (a
    numpy.ma.MaskedArray or a fixed-width KeyColumn brings NULLs) of ONE dtype out of uint8..uint64, int8..int64, float32,
    float64; no implicit cast. Integers compare by width and sign, floats as IEEE-754 with -0.0 == 0.0; a NULL or a NaN, in
    R or as a bound, matches nothing. pick: "all" -- every pair; "first" / "last" -- per S row the one pair with the smallest /
    largest R value in the range, ties to the lowest R row ("last" with s_lo None is the backward as-of join without a key,
    pandas.merge_asof without by=). Returns what join_tables returns, for all eight kinds of `how`, r_cols / s_cols the
    payload columns gathered through the maps. where: conditions on the matched pair as join_tables takes them, applied
    behind the pick. R is indexed once on the device; S goes through in slices of slice_rows rows (default: all at once; a
    slice's pairs must number below 2^32). The R marks of semi / anti / right_semi / right_anti cost O(|S| + |R|): no pair
    is expanded. An empty side is answered without a device. The order of the rows is unspecified."""
    return _range_join("range_join", r_values, s_lo, s_hi, lo_open, hi_open, pick, r_cols, s_cols, how, where, slice_rows, device)


def _swapped(res):
    return {"s_idx": res["r_idx"], "r_idx": res["s_idx"], "s": res["r"], "r": res["s"], "s_valid": res["r_valid"], "r_valid": res["s_valid"]}


def _mirror_where(fn, where):
    if where is None:
        return None
    out = []
    for t in where:
        if not isinstance(t, (tuple, list)) or len(t) != 3 or t[1] not in _MIRROR_OP:
            raise ValueError(f"{fn}: a where term is (s_values, op, r_values), not {t!r}")
        out.append((t[2], _MIRROR_OP[t[1]], t[0]))
    return out


def interval_join(r_lo, r_hi, s_values, lo_open=False, hi_open=False, r_cols=None, s_cols=None, how="inner", where=None, slice_rows=None,
                  device=0, host=False):
    """range_join with the sides swapped: S row s matches R row r when r_lo[r] <= s_values[s] <= r_hi[r] (events against
    sessions, S.x BETWEEN R.valid_from AND R.valid_to). S's points are indexed, R's intervals probe them in slices of
    slice_rows intervals, the two maps are swapped back and `how` keeps its meaning (S is the left side). There is no pick.
    host=True: over the host twins, as range_join_host. Everything else as range_join."""
    fn = "interval_join"
    _table_how(fn, how)
    join = range_join_host if host else range_join
    kw = {} if host else {"slice_rows": slice_rows, "device": device}
    return _swapped(join(s_values, r_lo, r_hi, lo_open, hi_open, "all", s_cols, r_cols, _MIRROR_HOW[how], _mirror_where(fn, where), **kw))


def _marked(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def range_pairs_host(r_values, s_lo=None, s_hi=None, lo_open=False, hi_open=False, pick="all", capacity=None, s_row_base=0):
    """hj_range_index_host + hj_range_pairs_host: the pairs of range_join on numpy arrays, computed by the same code on the
    host. Returns {"s_idx", "r_idx"} (the pairs written, S rows ascending), "s_marks" / "r_marks" (the planes as uint32 words),
    "info" (pairs, written, 0, S rows with a pair, S rows with a NULL or NaN bound, rows indexed, 0, 0) and the index as
    "perm", "keys", "head". capacity (None: every pair) cuts what is written, not what is counted or marked."""
    fn = "range_pairs_host"
    r, lo, hi, type_, width, flags, pick_id = _range_args(fn, r_values, s_lo, s_hi, lo_open, hi_open, pick)
    n_r, n_s = r.rows, (lo if lo is not None else hi).rows
    r_parts = r._whole()
    perm, keys = np.zeros(n_r, dtype=np.uint32), np.zeros(n_r, dtype=np.uint64 if width == 8 else np.uint32)
    head = np.zeros(4, dtype=np.uint32)
    arr, _ = _sort_cols([(_ptr(r_parts[0]), _ptr(r_parts[2]), width, type_, 0)])
    rc = lib.hj_range_index_host(arr, n_r, perm.ctypes.data, keys.ctypes.data, head.ctypes.data)
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, "hj_range_index_host")
    lo_parts, hi_parts = (None if b is None else b._whole() for b in (lo, hi))
    term = _lib.hj_range_term()
    term.lo, term.hi = (_ptr(p[0]) or None if p else None for p in (lo_parts, hi_parts))
    term.loValid, term.hiValid = (_ptr(p[2]) or None if p else None for p in (lo_parts, hi_parts))
    term.width, term.type, term.flags, term.pick = width, type_, flags, pick_id
    s_marks, r_marks = np.zeros(_mark_words(n_s), dtype=np.uint32), np.zeros(_mark_words(n_r), dtype=np.uint32)
    info = (C.c_uint64 * 8)()

    def call(out_s, out_r, cap, sm, rm):
        rc = lib.hj_range_pairs_host(keys.ctypes.data, perm.ctypes.data, head.ctypes.data, n_r, C.byref(term), n_s, int(s_row_base),
                                     _ptr(out_s) or None, _ptr(out_r) or None, cap, _ptr(sm) or None, _ptr(rm) or None, info)
        if rc != _lib.HJ_OK:
            raise HashJoinError(rc, "hj_range_pairs_host")

    call(None, None, 0, s_marks, r_marks)
    total = int(info[0])
    cap = min(total if capacity is None else int(capacity), 0xFFFFFFFF)
    out_s, out_r = np.empty(min(cap, total), dtype=np.uint32), np.empty(min(cap, total), dtype=np.uint32)
    if out_s.size:
        call(out_s, out_r, out_s.size, None, None)
    return {"s_idx": out_s, "r_idx": out_r, "s_marks": s_marks, "r_marks": r_marks, "info": tuple(int(x) for x in info), "perm": perm, "keys": keys,
            "head": head}


def range_join_host(r_values, s_lo=None, s_hi=None, lo_open=False, hi_open=False, pick="all", r_cols=None, s_cols=None, how="inner", where=None):
    """range_join over the host twins of its device calls (hj_range_index_host, hj_range_pairs_host, hj_pairs_where_host), for
    machines without a device: the same arguments without slices, the same result. The rows: the pairs, then the unmatched S
    rows, then the R-only rows."""
    fn = "range_join_host"
    _table_how(fn, how)
    r, lo, hi, *_ = _range_args(fn, r_values, s_lo, s_hi, lo_open, hi_open, pick)
    n_r, n_s = r.rows, (lo if lo is not None else hi).rows
    r_cols, s_cols = _table_columns(fn, "R", r_cols, n_r), _table_columns(fn, "S", s_cols, n_s)
    terms = _where_terms(fn, where, n_s, n_r)
    rows = _TableRows(how, r_cols, s_cols, n_r, n_s)
    trivial = rows.without_device(n_s)
    if trivial is not None:
        return trivial
    got = range_pairs_host(r, lo, hi, lo_open, hi_open, pick)
    if got["info"][0] > 0xFFFFFFFF:
        raise HashJoinError(_lib.HJ_ERR_INVALID, f"{got['info'][0]} pairs, above 2^32 - 1")
    if terms is not None:
        got = pairs_where_host(got["s_idx"], got["r_idx"], 0, where, marks=True)
    s_hit, r_hit = _marked(got["s_marks"], n_s), _marked(got["r_marks"], n_r)
    none = np.empty(0, dtype=np.uint32)
    keep = rows.kind is not None and rows.kind <= _lib.HJ_JOIN_LEFT
    s_idx, r_idx = (got["s_idx"], got["r_idx"]) if keep else (none, none)
    if rows.kind in (_lib.HJ_JOIN_LEFT, _lib.HJ_JOIN_SEMI, _lib.HJ_JOIN_ANTI):
        extra = np.flatnonzero(s_hit if rows.kind == _lib.HJ_JOIN_SEMI else ~s_hit).astype(np.uint32)
        s_idx, r_idx = np.concatenate([s_idx, extra]), np.concatenate([r_idx, np.full(extra.size, NO_ROW, dtype=np.uint32)])
    if rows.which is not None:
        extra = np.flatnonzero(r_hit if rows.which == _lib.HJ_R_MATCHED else ~r_hit).astype(np.uint32)
        s_idx, r_idx = np.concatenate([s_idx, np.full(extra.size, NO_ROW, dtype=np.uint32)]), np.concatenate([r_idx, extra])
    return rows.result(s_idx if rows.plane_s else None, r_idx if rows.plane_r else None, _take_on_host(s_cols, s_idx) if rows.plane_s else None,
                       _take_on_host(r_cols, r_idx) if rows.plane_r else None)
