"""What stands between a probe's pairs and the rows of a join: the terms of where= and asof= (parsed, on the host, on the
device) and the chain of pair steps -- verify, where, asof -- with the one tail behind it."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import lib
from .columns import KeyColumn, _DevColumn, _mark_words, _ptr
from .engine import HashJoinError, _terms_arr

# ---- join conditions beyond equality: where= and asof= ----------------------------------------------------------------------
_WHERE_TYPES = {"u": _lib.HJ_VAL_UINT, "i": _lib.HJ_VAL_INT, "f": _lib.HJ_VAL_FLOAT}


def _where_side(fn, side, values, n, what):
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


def _term(fn, term, ops, what, is_, n_s, n_r):
    """(s_values, op, r_values) as (S KeyColumn, hj_cmp_op, R KeyColumn, hj_val_type, width). ops: the permitted ops by name;
    what / is_: the keyword's wording ("a where term" / "a where term is")"""
    if not isinstance(term, (tuple, list)) or len(term) != 3:
        raise ValueError(f"{fn}: {is_} (s_values, op, r_values), not {term!r}")
    s_values, op, r_values = term
    if not isinstance(op, str) or op not in ops:
        raise ValueError(f"{fn}: the op of {what} must be one of {', '.join(ops)}, not {op!r}")
    s, r = _where_side(fn, "S", s_values, n_s, what), _where_side(fn, "R", r_values, n_r, what)
    if s.values.dtype != r.values.dtype:
        raise ValueError(f"{fn}: {what} compares {s.values.dtype} (S) with {r.values.dtype} (R); there is no implicit cast")
    return (s, ops[op], r, _WHERE_TYPES[s.values.dtype.kind], s.width)


def _where_terms(fn, where, n_s=None, n_r=None):
    """where= as a list of terms as _term gives them; None for None or an empty sequence"""
    if where is None:
        return None
    where = list(where)
    if len(where) > _lib.HJ_WHERE_MAX_TERMS:
        raise ValueError(f"{fn}: where has {len(where)} terms; 1 to {_lib.HJ_WHERE_MAX_TERMS} can be evaluated")
    return [_term(fn, t, _lib.CMP_OPS, "a where term", "a where term is", n_s, n_r) for t in where] or None


def _asof_term(fn, asof, n_s=None, n_r=None):
    """asof= as one term as _term gives it; None for None"""
    return None if asof is None else _term(fn, asof, _lib.ASOF_OPS, "the asof term", "asof is one term", n_s, n_r)


def _term_desc(term, s_parts, r_parts):
    """a term and the parts of its two columns -- host or device addresses -- as _terms_arr takes it"""
    _, op, _, type_, width = term
    return (s_parts[0], r_parts[0], width, type_, op, s_parts[2], r_parts[2])


def _host_maps(fn, map_s, map_r):
    map_s, map_r = np.ascontiguousarray(map_s, dtype=np.uint32), np.ascontiguousarray(map_r, dtype=np.uint32)
    if map_s.ndim != 1 or map_s.shape != map_r.shape:
        raise ValueError(f"{fn}: the maps must be 1-D and of one length, not shapes {map_s.shape} and {map_r.shape}")
    return map_s, map_r


def _host_filter(name, map_s, capacity, marks, terms, call, **more):
    """What the host forms of the pair filters share behind their checks: the output planes of `capacity` pairs (None: every
    pair fits), the mark planes, call(n_s, n_r, descriptors of the terms, out_s, out_r, s_marks, r_marks, info) -> status,
    and the result dict, `more` being the filter's own planes in it."""
    n_s, n_r = terms[0][0].rows, terms[0][2].rows
    capacity = map_s.size if capacity is None else int(capacity)
    held = [(s._whole(), r._whole()) for s, _, r, _, _ in terms]
    descs = [_term_desc(t, [_ptr(a) for a in sp], [_ptr(a) for a in rp]) for t, (sp, rp) in zip(terms, held)]
    out_s, out_r = np.empty(min(capacity, map_s.size), dtype=np.uint32), np.empty(min(capacity, map_s.size), dtype=np.uint32)
    s_marks = np.zeros(_mark_words(n_s), dtype=np.uint32) if marks else None
    r_marks = np.zeros(_mark_words(n_r), dtype=np.uint32) if marks else None
    info = (C.c_uint64 * 4)()
    rc = call(n_s, n_r, descs, out_s, out_r, _ptr(s_marks) or None, _ptr(r_marks) or None, info)
    del held
    if rc != _lib.HJ_OK:
        raise HashJoinError(rc, name)
    info = tuple(int(x) for x in info)
    out = {"s_idx": out_s[:info[1]], "r_idx": out_r[:info[1]], **{k: v[:n_s] for k, v in more.items()}, "info": info}
    if marks:
        out["s_marks"], out["r_marks"] = s_marks, r_marks
    return out


def pairs_where_host(map_s, map_r, s_row_base, terms, capacity=None, marks=False):
    """hj_pairs_where_host: HashJoinContext.pairs_where on numpy arrays, computed by the same code on the host. map_s / map_r:
    the pairs as two uint32 arrays of one length; terms: 1 to HJ_WHERE_MAX_TERMS tuples (s_values, op, r_values) as the
    where= of the joins takes them, op out of CMP_OPS; the S side has len(s_values) rows from s_row_base, the R side
    len(r_values). capacity (None: every pair fits) cuts what is written, not what is counted or marked.
    Returns {"s_idx", "r_idx"} (the kept pairs written, in input order), "info" (kept, written, 0, dropped) and, with
    marks=True, "s_marks" / "r_marks": the two planes as uint32 words, zero before the call. Needs no device."""
    fn = "pairs_where_host"
    map_s, map_r = _host_maps(fn, map_s, map_r)
    cols = _where_terms(fn, terms)
    if cols is None:
        raise ValueError(f"{fn}: 1 to {_lib.HJ_WHERE_MAX_TERMS} terms, not none")
    if any(s.rows != cols[0][0].rows or r.rows != cols[0][2].rows for s, _, r, _, _ in cols):
        raise ValueError(f"{fn}: the values of every term must have one length per side")

    def call(n_s, n_r, descs, out_s, out_r, s_marks, r_marks, info):
        arr, k = _terms_arr(descs)
        return lib.hj_pairs_where_host(map_s.ctypes.data, map_r.ctypes.data, map_s.size, int(s_row_base), n_s, n_r, arr, k,
                                       out_s.ctypes.data, out_r.ctypes.data, out_s.size, s_marks, r_marks, info)

    return _host_filter("hj_pairs_where_host", map_s, capacity, marks, cols, call)


def pairs_asof_host(map_s, map_r, s_row_base, term, capacity=None, marks=False):
    """hj_pairs_asof_host: HashJoinContext.pairs_asof on numpy arrays, computed by the same code on the host. map_s / map_r:
    the pairs as two uint32 arrays of one length; term: (s_values, op, r_values) as the asof= of the joins takes it; the S
    side has len(s_values) rows from s_row_base, the R side len(r_values). capacity (None: every pair fits) cuts what is
    written, not what is counted or marked.
    Returns {"s_idx", "r_idx"} (the kept pairs written, in input order), "best_row" (per S row the R row kept, or NO_ROW: the
    left-outer as-of map), "info" (kept, written, 0, dropped) and, with marks=True, "s_marks" / "r_marks": the two planes as
    uint32 words, zero before the call. Needs no device."""
    fn = "pairs_asof_host"
    map_s, map_r = _host_maps(fn, map_s, map_r)
    col = _asof_term(fn, term)
    if col is None:
        raise ValueError(f"{fn}: one term (s_values, op, r_values), not None")
    best_val, best_row = np.empty(max(col[0].rows, 1), dtype=np.uint64), np.empty(max(col[0].rows, 1), dtype=np.uint32)

    def call(n_s, n_r, descs, out_s, out_r, s_marks, r_marks, info):
        return lib.hj_pairs_asof_host(map_s.ctypes.data, map_r.ctypes.data, map_s.size, int(s_row_base), n_s, n_r,
                                      _terms_arr(descs, _lib.hj_asof_term)[0], best_val.ctypes.data, best_row.ctypes.data,
                                      out_s.ctypes.data, out_r.ctypes.data, out_s.size, s_marks, r_marks, info)

    return _host_filter("hj_pairs_asof_host", map_s, capacity, marks, [col], call, best_row=best_row)


# ---- the chain of pair steps: verify, where, asof ---------------------------------------------------------------------------
# which rows of the slice's S plane a kind adds to the kept pairs (left, full) or returns (semi, anti)
_ON_S_SWEEP = {_lib.HJ_JOIN_LEFT: _lib.HJ_R_UNMATCHED, _lib.HJ_JOIN_SEMI: _lib.HJ_R_MATCHED, _lib.HJ_JOIN_ANTI: _lib.HJ_R_UNMATCHED}


class _PairStep:
    """One filter over a slice's pair list, as _PairChain runs it: put() has the step's columns of the slice [lo, lo + n)
    on the device, filter() is the device call -- the pairs in, the kept pairs out, into planes of `capacity` entries and
    the two mark planes, either of which may be 0 --, info() its *_info read, capacity() the entries its kept pairs need."""

    def put(self, ctx, held, lo, n):
        pass

    def capacity(self, n_pairs, n):
        return n_pairs


class _TermStep(_PairStep):
    """a step over terms: their R columns whole on the device, room for one slice of the S columns; descs: the terms as
    HashJoinContext.pairs_where / pairs_asof take them"""

    def __init__(self, terms, step):
        self.terms, self.step, self.descs = terms, step, None

    def put(self, ctx, held, lo, n):
        if self.descs is None:      # the first slice: R's columns whole, room for a slice of S's
            r_dev = [_DevColumn.whole(ctx, held, r) for _, _, r, _, _ in self.terms]
            self.s_dev = [_DevColumn(held, s, self.step) for s, _, _, _, _ in self.terms]
            self.descs = [_term_desc(t, sd.parts, rd.parts) for t, sd, rd in zip(self.terms, self.s_dev, r_dev)]
        for sd in self.s_dev:
            sd.put(ctx, lo, n)


class _WhereStep(_TermStep):
    """where=: the pairs for which every term holds (HashJoinContext.pairs_where)"""

    def filter(self, ctx, lo, n, n_r, d_s, d_r, n_pairs, d_ks, d_kr, capacity, d_s_marks, d_r_marks):
        ctx.pairs_where(d_s, d_r, n_pairs, lo, n, n_r, self.descs, d_ks, d_kr, capacity, d_s_marks, d_r_marks)

    def info(self, ctx):
        return ctx.where_info()


class _AsofBestStep(_TermStep):
    """asof=: per S row the one eligible pair whose R value is nearest (HashJoinContext.pairs_asof). The two best planes are
    sized for one slice; a slice's pair list is complete when it arrives here (_drive_join probes a slice again whose rows
    exceeded the planes), so every S row has all its pairs in one call."""

    def put(self, ctx, held, lo, n):
        if self.descs is None:
            self.best = held.alloc(8 * self.step), held.alloc(4 * self.step)
        super().put(ctx, held, lo, n)

    def capacity(self, n_pairs, n):
        return min(n_pairs, n)      # one pair per S row at most

    def filter(self, ctx, lo, n, n_r, d_s, d_r, n_pairs, d_ks, d_kr, capacity, d_s_marks, d_r_marks):
        ctx.pairs_asof(d_s, d_r, n_pairs, lo, n, n_r, self.descs[0], *self.best, d_ks, d_kr, capacity, d_s_marks, d_r_marks)

    def info(self, ctx):
        return ctx.asof_info()


def _condition_steps(terms, best, step):
    """the steps of where= (terms, or None) and asof= (best, or None) for slices of `step` rows, in the chain's order"""
    return ([_WhereStep(terms, step)] if terms is not None else []) + ([_AsofBestStep([best], step)] if best is not None else [])


class _PairChain:
    """The steps behind a probe's pairs, in order: verify (a join on key columns), where, asof. Every step but the last
    keeps all its pairs -- its capacity is what comes in -- and touches no mark plane. The last one owns the only pair of
    mark planes (R's for the whole join, S's for one slice, cleared per slice) and writes its kept pairs only where the
    tail reads them (keep; False: a mark-only pass, capacity 0 and no planes). slice() has the signature of _drive_join's
    on_maps and ends in tail(ctx, held, lo, n, d_ks, d_kr, kept), the subclass's."""

    def __init__(self, steps, n_r, step, keep):
        self.steps, self.n_r, self.step, self.keep, self.marks = steps, n_r, step, keep, None

    def _run(self, st, ctx, held, lo, n, d_s, d_r, n_pairs, keep, marks=(0, 0)):
        st.put(ctx, held, lo, n)
        capacity = st.capacity(n_pairs, n) if keep else 0
        d_ks, d_kr = (held.alloc(4 * capacity), held.alloc(4 * capacity)) if keep else (0, 0)
        st.filter(ctx, lo, n, self.n_r, d_s, d_r, n_pairs, d_ks, d_kr, capacity, *marks)
        return d_ks, d_kr, (st.info(ctx)[1] if keep else 0)

    def slice(self, ctx, held, lo, n, d_s, d_r, n_pairs):
        """the n_pairs pairs of the slice [lo, lo + n) that the probe found -> the tail"""
        if self.marks is None:
            self.marks = held.alloc(4 * _mark_words(self.step)), held.put(np.zeros(_mark_words(self.n_r), dtype=np.uint32))
        mine = []
        for st in self.steps[:-1]:
            d_s, d_r, n_pairs = self._run(st, ctx, held, lo, n, d_s, d_r, n_pairs, True)
            mine += [d_s, d_r]
        ctx.copy_h2d(self.marks[0], np.zeros(_mark_words(n), dtype=np.uint32))
        d_ks, d_kr, kept = self._run(self.steps[-1], ctx, held, lo, n, d_s, d_r, n_pairs, self.keep, self.marks)
        self.tail(ctx, held, lo, n, d_ks, d_kr, kept)
        held.free(*mine, *(p for p in (d_ks, d_kr) if p))


class _RowChain(_PairChain):
    """The chain of a join that returns rows. rows: the _TableRows the result grows in. The tail: the kept pairs, where they
    are rows of the kind, then the rows the kind takes from the sweep of the slice's S plane; after() -- _drive_join's
    `after` -- adds the R-only rows from the sweep of the R plane."""

    def __init__(self, steps, rows, n_r, step):
        super().__init__(steps, n_r, step, rows.kind is not None and rows.kind <= _lib.HJ_JOIN_LEFT)     # the kept pairs are rows of the result
        self.rows, self.s_sweep = rows, _ON_S_SWEEP.get(rows.kind)

    def tail(self, ctx, held, lo, n, d_ks, d_kr, kept):
        if self.keep:           # right_semi / right_anti, semi / anti ran a mark-only pass
            self.rows.add(ctx, held, lo, n, d_ks, d_kr, kept)
        if self.s_sweep is not None:
            d_rows = held.alloc(4 * n)
            ctx.mark_rows(self.marks[0], n, lo, self.s_sweep, d_rows, n)
            self.rows.add(ctx, held, lo, n, d_rows, 0, ctx.mark_rows_info()[1])
            held.free(d_rows)

    def after(self, ctx, held):
        if self.rows.which is not None:
            d_rows = held.alloc(4 * self.n_r)
            ctx.mark_rows(self.marks[1], self.n_r, 0, self.rows.which, d_rows, self.n_r)
            self.rows.add(ctx, held, None, 0, 0, d_rows, ctx.mark_rows_info()[1])
