"""Joins on the key word of a tuple: the host sequence of every materialising join (_drive_join), the joins as gather maps
(the four pairs wrappers), and the joined rows themselves -- payload columns through the maps, on the device (join_tables)."""
import functools

import numpy as np

from . import _lib
from .columns import KeyColumn, _DevColumn, _concat_key_columns, _fetch_map, _mark_words, _session, _table_columns, _take_key_column, _take_on_host
from .conditions import _RowChain, _asof_term, _condition_steps, _where_terms
from .engine import HashJoinError, NO_ROW


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
    with _session(device) as (ctx, held):
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


def _pairs(fn, relR, relS, path, how, outer, device, slice_tuples=None, **kw):
    """The body of the four pairs wrappers, behind their own checks. outer: `how` is one of the R-preserving kinds, whose
    result ends in the sweep's rows. path "radix" probes relS in slices of slice_tuples; **kw goes to _drive_join."""
    kind, which = _outer_kind(fn, how) if outer else (_join_kind(fn, how), None)
    relR = np.ascontiguousarray(relR, dtype=np.uint64)
    relS = np.ascontiguousarray(relS, dtype=np.uint64)
    trivial = _outer_without_device(kind, which, relR.size, relS.size) if outer else _join_without_device(kind, relR.size, relS.size)
    if trivial is not None:
        return trivial
    step = _slice_step(fn, relS.size, slice_tuples) if path == "radix" else relS.size
    s_parts, r_parts = _join_maps(relR, relS, path, kind, which, step, device, **kw)
    if outer:
        return _outer_result(kind, s_parts, r_parts[:-1], r_parts[-1])
    return np.concatenate(s_parts), (np.concatenate(r_parts) if r_parts else None)


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
    return _pairs("join_pairs", relR, relS, algo, how, False, device, probeLength=probeLength)


def radix_join_pairs(relR, relS, radixBits=0, slice_tuples=None, device=0, how="inner"):
    """The complete equi-join on the key word (the low 32 bits of a tuple) through the resident radix join, as two gather
    maps like join_pairs: (s_idx, r_idx), numpy uint32 arrays, row k of the result being (relS[s_idx[k]], relR[r_idx[k]]),
    in no particular order. The path for a scattered or skewed relS. R is partitioned once with its row ids; relS is
    probed in slices of slice_tuples (default: all of it at once).
    Sizing, per slice, as in join_pairs: the outputs start with one entry per S tuple of the slice; if the probe reports
    more pairs than that, they are enlarged to the reported count and the slice is probed once more.
    how: as in join_pairs (r_idx is None for "semi" and "anti", and carries NO_ROW in the unmatched rows of "left")."""
    return _pairs("radix_join_pairs", relR, relS, "radix", how, False, device, slice_tuples, radixBits=radixBits)


def outer_join_pairs(relR, relS, algo="htm", probeLength=4, device=0, how="right"):
    """The joins that preserve relR, the build side, as gather maps like join_pairs (same algo, same meaning of a match).
    how = "right": (s_idx, r_idx), the inner rows first, then one row (NO_ROW, r) for every R row no inner row names, r
    ascending. "full": the same with the left-outer rows in front (an S tuple without a match is (s, NO_ROW)).
    "right_semi" / "right_anti": (None, r_idx), the R rows some / no inner row names, ascending. With "atomic" / "nocc"
    an R tuple that ran out of probeLength is not in the table and therefore unmatched."""
    if algo not in ("htm", "atomic", "nocc"):
        raise ValueError(f"outer_join_pairs: algo must be htm, atomic or nocc, not {algo!r}")
    return _pairs("outer_join_pairs", relR, relS, algo, how, True, device, probeLength=probeLength)


def radix_outer_join_pairs(relR, relS, radixBits=0, slice_tuples=None, device=0, how="right"):
    """outer_join_pairs through the resident radix join (the complete equi-join on the key word, as radix_join_pairs): R is
    partitioned once with its row ids, relS is probed in slices of slice_tuples, and the marks the slices leave on R's
    rows become the R-only rows at the end. how and the result as in outer_join_pairs."""
    return _pairs("radix_outer_join_pairs", relR, relS, "radix", how, True, device, slice_tuples, radixBits=radixBits)


# ---- the joined rows themselves: payload columns through the maps, on the device --------------------------------------
_TABLE_HOWS = tuple(_lib.JOIN_KINDS) + tuple(_OUTER_KINDS)


def _table_how(fn, how):
    if not isinstance(how, str) or how not in _TABLE_HOWS:
        raise ValueError(f"{fn}: how must be one of {', '.join(_TABLE_HOWS)}, not {how!r}")


def _fetch_valid(ctx, d_words, n_rows):
    """a device plane of one bit per row as one bool per row"""
    words = np.zeros(_mark_words(n_rows), dtype=np.uint32)
    ctx.copy_d2h(words, d_words)
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n_rows].astype(bool)


def _gather_key_columns(ctx, held, d_map, n_rows, row_base, src_rows, k_cols):
    """The KeyColumn columns of one side through HashJoinContext.gather2: k_cols = [(name, the column's _DevColumn)] ->
    {name: KeyColumn of n_rows rows}. Variable-length columns are gathered as a sizing call (dst_capacity 0) followed by
    the copy call."""
    out = {}
    if not n_rows:
        return {name: _take_key_column(dev.col, np.empty(0, dtype=np.uint32)) for name, dev in k_cols}
    for i in range(0, len(k_cols), _lib.HJ_GATHER_MAX_COLS):
        part, descs = k_cols[i:i + _lib.HJ_GATHER_MAX_COLS], []
        for name, dev in part:
            d_values, d_offsets, d_valid = dev.parts
            d = {"src": d_values, "width": dev.col.width, "src_valid": d_valid, "dst_valid": held.alloc(4 * _mark_words(n_rows)), "dst": 0}
            if dev.col.width:
                d["dst"] = held.alloc(n_rows * dev.col.width)
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
        for (name, dev), d in zip(part, descs):
            col = dev.col
            valid = _fetch_valid(ctx, d["dst_valid"], n_rows)
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
    """One side of n_rows result rows out of the device map d_map: d_cols = [(name, the column's _DevColumn)] -> ({name:
    column}, valid). A plain array goes through HashJoinContext.gather and comes back as an array: one call per
    HJ_GATHER_MAX_COLS columns, the validity plane with the first (alone when the side has no column). The library's own
    maps have no out-of-range entry: one is an error. A KeyColumn goes through _gather_key_columns behind the plain ones."""
    k_cols = [c for c in d_cols if isinstance(c[1].col, KeyColumn)]
    d_cols = [(name, dev.parts[0], dev.col.dtype) for name, dev in d_cols if not isinstance(dev.col, KeyColumn)]
    out = {name: np.empty(n_rows, dtype=dt) for name, _, dt in d_cols}
    valid = np.empty(0, dtype=bool)
    if n_rows:
        d_valid = held.alloc(4 * _mark_words(n_rows))
        dsts = [held.alloc(n_rows * dt.itemsize) for _, _, dt in d_cols]
        calls = [(d_cols[i:i + _lib.HJ_GATHER_MAX_COLS], dsts[i:i + _lib.HJ_GATHER_MAX_COLS])
                 for i in range(0, len(d_cols), _lib.HJ_GATHER_MAX_COLS)] or [([], [])]
        for k, (part, part_dst) in enumerate(calls):
            ctx.gather(d_map, n_rows, src_rows, [(src, dst, dt.itemsize, 0) for (_, src, dt), dst in zip(part, part_dst)],
                       d_valid=0 if k else d_valid, row_base=row_base)
            stray = ctx.gather_info()[3]
            if stray:
                raise HashJoinError(_lib.HJ_ERR_STATE, f"{stray} map entries outside the {src_rows} source rows from {row_base}")
        valid = _fetch_valid(ctx, d_valid, n_rows)
        for (name, _, _), dst in zip(d_cols, dsts):
            ctx.copy_d2h(out[name], dst)
        held.free(d_valid, *dsts)
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

    def __init__(self, how, r_cols, s_cols, n_r, step):
        self.outer = how in _OUTER_KINDS
        self.kind, self.which = _OUTER_KINDS[how] if self.outer else (_lib.JOIN_KINDS[how], None)
        self.plane_s = self.kind is not None                                # right_semi / right_anti: R rows alone
        self.plane_r = self.outer or self.kind <= _lib.HJ_JOIN_LEFT         # semi / anti: S rows alone
        self.r_cols, self.s_cols, self.n_r, self.step = r_cols, s_cols, n_r, step
        self.s_maps, self.r_maps, self.s_parts, self.r_parts, self.dev = [], [], [], [], {}

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
            self.dev["r"] = [(name, _DevColumn.whole(ctx, held, col)) for name, col in self.r_cols.items()] if self.plane_r else []
            self.dev["s"] = [(name, _DevColumn(held, col, self.step)) for name, col in self.s_cols.items()] if self.plane_s else []
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
            for _, dev in self.dev["s"]:        # the slice's columns go up once, however many calls name rows of it
                dev.put(ctx, lo, n_s)
            parts.append(_gather_side(ctx, held, d_map, rows, lo, n_s, self.dev["s"]))

    def joined(self):
        return self.result(np.concatenate(self.s_maps) if self.plane_s else None, np.concatenate(self.r_maps) if self.plane_r else None,
                           _concat_side(self.s_parts, self.s_cols), _concat_side(self.r_parts, self.r_cols))


def _where_keyword(impl):
    """The keywords where= and asof= on a join: the decorated function keeps its parameters and, called with neither, runs as
    it is; a call with either goes to `impl`, the function that takes the same arguments and the two."""
    def deco(fn):
        @functools.wraps(fn)
        def join(*args, where=None, asof=None, **kw):
            return fn(*args, **kw) if where is None and asof is None else impl(*args, where=where, asof=asof, **kw)
        return join
    return deco


def _join_tables(relR, relS, r_cols=None, s_cols=None, how="inner", path="htm", probeLength=4, radixBits=0, slice_tuples=None,
                 device=0, where=None, asof=None):
    """join_tables, and join_tables with a condition or an as-of term (_where_keyword)"""
    fn = "join_tables"
    _table_how(fn, how)
    if not isinstance(path, str) or path not in ("htm", "atomic", "nocc", "radix"):
        raise ValueError(f"{fn}: path must be htm, atomic, nocc or radix, not {path!r}")
    relR = np.ascontiguousarray(relR, dtype=np.uint64)
    relS = np.ascontiguousarray(relS, dtype=np.uint64)
    r_cols = _table_columns(fn, "R", r_cols, relR.size)
    s_cols = _table_columns(fn, "S", s_cols, relS.size)
    step = _slice_step(fn, relS.size, slice_tuples) if path == "radix" and relS.size else relS.size
    steps = _condition_steps(_where_terms(fn, where, relS.size, relR.size), _asof_term(fn, asof, relS.size, relR.size), step)
    rows = _TableRows(how, r_cols, s_cols, relR.size, step)
    trivial = rows.without_device(relS.size)
    if trivial is not None:
        return trivial
    if steps:
        # as in join_on: the probe is INNER whatever the kind, and the context's own R marks stay out of it -- a pair that
        # the condition rejects would have set them
        chain = _RowChain(steps, rows, relR.size, step)
        _drive_join(relR, relS, path, _lib.HJ_JOIN_INNER, None, step, chain.slice, device, probeLength=probeLength, radixBits=radixBits,
                    after=chain.after)
    else:
        _drive_join(relR, relS, path, rows.kind, rows.which, step, rows.add, device, probeLength=probeLength, radixBits=radixBits)
    return rows.joined()


@_where_keyword(_join_tables)
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
