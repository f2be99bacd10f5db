"""What the tests of hj_window_frames_dev / hj_window_frames_host share: the model, the case builder, the library on host
pointers, the comparison, and the framed specs of window_rows against a per-partition Python loop. No test in here.

The model restates the header's definitions in numpy and never calls the library: positions, partitions and skipped
entries are window_common.model_runs' (the window's own), start / end by running maxima and minima, the frame of p is
[max(start, p + lo), min(end, p + hi)] in Python-sized integers, COUNT and SUM are differences of ONE cumulative sum in
uint64 (modulo 2^64, as the header says), MIN and MAX the extreme of a per-position slice of the values (int64 or uint64
by the source's sign, a NULL holding the op's identity). It knows no blocks, no scans, no running window and no deque."""
import ctypes as C

import numpy as np

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

import sort_common as sc
import window_common as wc

U32, U64 = np.uint32, np.uint64
NO_ROW, SENT64, M64 = wc.NO_ROW, wc.SENT64, wc.M64
A = _lib
OPS = (A.HJ_AGG_COUNT, A.HJ_AGG_SUM, A.HJ_AGG_MIN, A.HJ_AGG_MAX)
FAR = (1 << 32) - 1                                  # the largest offset


def layout(n_pos):
    """hj_frames_layout_info -> (tile positions, chunk positions, chunks, workspace bytes)"""
    out = (C.c_uint64 * 4)()
    assert lib.hj_frames_layout_info(n_pos, out) == _lib.HJ_OK
    return tuple(int(x) for x in out)


class Func:
    """one function of a call: the op (an hj_agg_op), the frame (lo, hi; None: unbounded on that side), the source (values
    per ROW, any bytes under a NULL)"""

    def __init__(self, op, lo, hi, src=None, valid=None, width=None):
        self.op, self.lo, self.hi = op, lo, hi
        self.src = None if src is None else np.ascontiguousarray(src)
        self.valid = None if valid is None else np.ascontiguousarray(valid, dtype=bool)
        self.width = (0 if self.src is None else self.src.dtype.itemsize) if width is None else width
        self.signed = self.src is not None and self.src.dtype.kind == "i"
        self.flags = ((_lib.HJ_AGG_SIGNED if self.signed else 0) | (_lib.HJ_FRAME_UNBOUNDED_LO if lo is None else 0)
                      | (_lib.HJ_FRAME_UNBOUNDED_HI if hi is None else 0))
        self.dtype, self.sentinel = U64, SENT64

    def plane(self, n_rows, garbage=None):
        return None if self.valid is None else sc.Col(np.zeros(n_rows, dtype=np.uint8), self.valid).plane(garbage)

    def identity(self):
        if self.op == A.HJ_AGG_MIN:
            return (1 << 63) - 1 if self.signed else M64
        if self.op == A.HJ_AGG_MAX:
            return -(1 << 63) if self.signed else 0
        return 0


class Case:
    """perm: uint32 per position or None (the identity); part: uint32 per ROW or None; funcs: at most HJ_FRAME_MAX_FUNCS Func"""

    def __init__(self, n_pos, n_rows, perm, part, funcs):
        self.n_pos, self.n_rows, self.perm, self.part, self.order, self.funcs = n_pos, n_rows, perm, part, [], list(funcs)
        assert perm is None or (perm.dtype == U32 and perm.size >= n_pos)
        assert part is None or (part.dtype == U32 and part.size == n_rows)


# ---- the model -------------------------------------------------------------------------------------------------------------------
def frame_ends(case, f):
    """(rows, in-range mask, L, R) per position: the clamped frame by the header's definition, in int64 (no wrap: |offset| < 2^32)"""
    n = case.n_pos
    rows, inr, head, _ = wc.model_runs(case)
    pos = np.arange(n, dtype=np.int64)
    start = np.maximum.accumulate(np.where(head, pos, 0))
    tail = np.append(head[1:], True)
    end = np.minimum.accumulate(np.where(tail, pos, n)[::-1])[::-1]
    left = start if f.lo is None else np.maximum(start, pos + int(f.lo))
    right = end if f.hi is None else np.minimum(end, pos + int(f.hi))
    return rows, inr, head, left, right


def model(case):
    """-> ([one uint64 array per function, indexed by row, the sentinel where nothing is written], info: partitions, skipped)"""
    n = case.n_pos
    outs = [np.full(case.n_rows, SENT64, dtype=U64) for _ in case.funcs]
    if n == 0:
        return outs, (0, 0)
    info = None
    for f, out in zip(case.funcs, outs):
        rows, inr, head, left, right = frame_ends(case, f)
        info = (int((head & inr).sum()), int((~inr).sum()))
        live = np.flatnonzero(inr)
        r = rows[live]
        ok = np.ones(r.size, dtype=bool) if f.valid is None else f.valid[r]
        empty = left > right
        lo_i, hi_i = np.clip(left, 0, n - 1), np.clip(right, 0, n - 1)
        if f.op in (A.HJ_AGG_COUNT, A.HJ_AGG_SUM):
            x = np.zeros(n, dtype=U64)
            v = np.ones(r.size, dtype=U64) if f.op == A.HJ_AGG_COUNT else f.src[r].astype(np.int64).view(U64) if f.signed else f.src[r].astype(U64)
            x[live] = np.where(ok, v, U64(0))
            total = np.concatenate([np.zeros(1, dtype=U64), np.cumsum(x, dtype=U64)])       # total[q] = the sum below q
            val = np.where(empty, U64(0), total[hi_i + 1] - total[lo_i])
        else:
            dt = np.int64 if f.signed else U64
            x = np.full(n, f.identity(), dtype=dt)
            x[live] = np.where(ok, f.src[r].astype(dt), dt(f.identity()))
            pick = np.min if f.op == A.HJ_AGG_MIN else np.max
            val = np.full(n, f.identity(), dtype=dt)
            for p in live:
                if not empty[p]:
                    val[p] = pick(x[lo_i[p]:hi_i[p] + 1])
            val = val.view(U64)
        out[rows[live]] = val[live]
    return outs, info


# ---- the library on host pointers ------------------------------------------------------------------------------------------------
def func_array(funcs, pointers):
    """pointers: [(out_ptr, src_ptr or 0, valid_ptr or 0)] -> (hj_frame_func array, its length)"""
    arr = (_lib.hj_frame_func * max(len(funcs), 1))()
    for a, f, (out, src, valid) in zip(arr, funcs, pointers):
        a.src, a.srcValid, a.out = src or None, valid or None, out or None
        a.lo, a.hi = 0 if f.lo is None else f.lo, 0 if f.hi is None else f.hi
        a.op, a.width, a.flags, a.reserved = f.op, f.width, f.flags, 0
    return arr, len(funcs)


def host_call(case, garbage=None):
    """hj_window_frames_host over sentinel-filled outputs -> ([one array per function], out[8])"""
    outs = [np.full(case.n_rows, SENT64, dtype=U64) for _ in case.funcs]
    planes = [f.plane(case.n_rows, garbage) for f in case.funcs]
    f_arr, n_funcs = func_array(case.funcs, [(o.ctypes.data, f.src.ctypes.data if f.src is not None else 0, p.ctypes.data if p is not None else 0)
                                             for f, o, p in zip(case.funcs, outs, planes)])
    info = (C.c_uint64 * 8)()
    rc = lib.hj_window_frames_host(case.perm.ctypes.data if case.perm is not None else None, case.n_pos, case.n_rows,
                                   case.part.ctypes.data if case.part is not None else None, f_arr, n_funcs, info)
    assert rc == _lib.HJ_OK, rc
    return outs, [int(x) for x in info]


same = wc.same


def check_info(info, case, want, tag=None):
    """out[8] of hj_window_frames_info / hj_window_frames_host against the model's counts and the layout"""
    if case.n_pos == 0:
        assert info[:3] == [0, 0, 0] and info[4:] == [0, 0, 0, 0], (tag, info)
        return
    _, _, chunks, nbytes = layout(case.n_pos)
    assert (info[0], info[1], info[2], info[4]) == (case.n_pos, want[0], 0, want[1]), (tag, info, want)
    assert (info[5], info[6], info[7]) == (chunks, nbytes, 0), (tag, info)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
def placements(w):
    """a width placed four ways: trailing, leading, centred, and clear of the current row on either side"""
    return [(-(w - 1), 0), (0, w - 1), (-(w // 2), w - 1 - w // 2), (-(w + 2), -3), (3, w + 2)]


def build(n_pos, frames, shape="geometric", perm="random", extra_rows=0, holes=0, seed=0, null_pct=10):
    """window_common.build's shapes, permutations, holes and extra rows, and run_funcs' data (sums that wrap, signed extremes,
    NULLs): its eight sources in turn, one per frame of `frames` ((lo, hi), None: unbounded; at most eight)."""
    assert 1 <= len(frames) <= A.HJ_FRAME_MAX_FUNCS
    base = wc.build(n_pos, shape, "none", perm=perm, extra_rows=extra_rows, holes=holes, seed=seed, funcs="run", null_pct=null_pct)
    funcs = []
    for i, (lo, hi) in enumerate(frames):
        r = base.funcs[i % len(base.funcs)]
        funcs.append(Func(r.op - _lib.HJ_WIN_RUN_COUNT, lo, hi, r.src, r.valid, r.width))
    return Case(base.n_pos, base.n_rows, base.perm, base.part, funcs)


def rotate(frames, k):
    """eight frames from a list, starting at k: every frame meets every source type as k runs"""
    return [frames[(k + i) % len(frames)] for i in range(min(8, len(frames)))]


# ---- the block rule against brute force (no library): what hj_frames.hip's combine step relies on ---------------------------------
def block_rule_check(rng, cases=3000):
    """random partitions, frames on either side of p, empty frames, unbounded sides: G / H by their definitions, combined by
    the rule of the header comment of hj_frames.hip, against the minimum / sum of the frame itself. -> mismatches"""
    bad = 0
    for _ in range(cases):
        n = int(rng.integers(1, 40))
        vals = [int(v) for v in rng.integers(-50, 50, n)]
        heads = [True] + [bool(rng.random() < 0.25) for _ in range(n - 1)]
        start = [0] * n
        for q in range(n):
            start[q] = q if heads[q] else start[q - 1]
        end = [0] * n
        for q in range(n - 1, -1, -1):
            end[q] = q if q == n - 1 or heads[q + 1] else end[q + 1]
        lo = None if rng.random() < 0.15 else int(rng.integers(-12, 12))
        hi = None if rng.random() < 0.15 else int(rng.integers(-12, 12))
        if lo is not None and hi is not None and lo > hi:
            lo, hi = hi, lo
        op, ident = ((min, 1 << 60), (lambda a, b: a + b, 0))[int(rng.integers(0, 2))]
        w = hi - lo + 1 if lo is not None and hi is not None else None

        def fold(a, b):
            r = ident
            for q in range(a, b + 1):
                r = op(r, vals[q])
            return r

        G = [fold(max(start[q], q // w * w) if w else start[q], q) for q in range(n)]
        H = [fold(q, min(end[q], q // w * w + w - 1) if w else end[q]) for q in range(n)]
        for p in range(n):
            left = start[p] if lo is None else max(start[p], p + lo)
            right = end[p] if hi is None else min(end[p], p + hi)
            if left > right:
                got = ident
            elif lo is None:
                got = G[right]
            elif hi is None:
                got = H[left]
            elif left // w == right // w:
                got = G[right] if left == start[p] or left % w == 0 else H[left]
            else:
                got = op(H[left], G[right])
            bad += got != (fold(left, right) if left <= right else ident)
    return bad


# ---- the wrapper against a per-partition loop --------------------------------------------------------------------------------------------
FRAMED = {"s7": ("sum", "v", -6, 0), "lead_u": ("sum", "u", 0, 2), "mn": ("min", "v", -3, -1), "mx": ("max", "u", -1, 1), "tot": ("sum", "v", None, None),
          "top": ("max", "v", None, None), "rest": ("min", "u", 1, None), "sofar": ("count", "v", None, 0), "rows3": ("count", None, -1, 1),
          "words": ("count", "w", -2, 2), "avg": ("mean", "v", -2, 2), "avg_all": ("mean", "v", None, None)}
BESIDE = {"rn": "row_number", "c": "count", "sum_v": ("cumsum", "v"), "seen_v": ("cumcount", "v"), "prev_w": ("lag", "w", 1)}


def framed_call(fn, t, null_keys, keys="both", funcs=None, **kw):
    by = {"both": [hj.KeyColumn.from_list(t["names"]), hj.KeyColumn(t["num"], t["num_valid"])], "string": hj.KeyColumn.from_list(t["names"]),
          "integer": hj.KeyColumn(t["num"], t["num_valid"])}[keys]
    return fn(dict(FRAMED, **BESIDE) if funcs is None else funcs, partition_by=by, order_by=[hj.KeyColumn(t["o1"], t["o1_valid"]), t["o2"]],
              descending=[True, False], nulls=["first", "last"],
              cols={"w": hj.KeyColumn.from_list(t["words"]), "v": hj.KeyColumn(t["v"], t["v_valid"]), "u": t["u"]}, null_keys=null_keys, **kw)


def framed_check(got, t, null_keys, keys="both"):
    """every framed output against a loop over each partition's rows in got["perm"]'s order (the order itself is the old
    specs' business: row_number beside them is checked against it)"""
    n = len(t["names"])
    key = {"both": lambda i: (t["names"][i], int(t["num"][i]) if t["num_valid"][i] else None), "string": lambda i: (t["names"][i],),
           "integer": lambda i: (int(t["num"][i]) if t["num_valid"][i] else None,)}[keys]
    cols = {"w": [None if w is None else w for w in t["words"]], "v": [int(x) if ok else None for x, ok in zip(t["v"], t["v_valid"])],
            "u": [int(x) for x in t["u"]], None: [1] * n}
    parts = {}
    for i in got["perm"].tolist():
        parts.setdefault(key(i), []).append(i)
    dropped = [i for i in range(n) if null_keys == "drop" and any(k is None for k in key(i))]
    assert got["null_rows"] == len(dropped) and got["n_partitions"] == len(parts) and sorted(sum(parts.values(), []) + dropped) == list(range(n))
    for rows in parts.values():
        assert [int(got["rn"][i]) for i in rows] == list(range(1, len(rows) + 1))
    for name, (op, col, lo, hi) in FRAMED.items():
        want = [None] * n
        for rows in parts.values():
            for j, i in enumerate(rows):
                a, b = 0 if lo is None else max(0, j + lo), len(rows) - 1 if hi is None else min(len(rows) - 1, j + hi)
                vals = [cols[col][q] for q in rows[a:b + 1] if cols[col][q] is not None] if a <= b else []
                if op == "count":
                    want[i] = len(vals)
                elif vals:
                    want[i] = {"sum": sum, "min": min, "max": max, "mean": lambda x: sum(x) / len(x)}[op](vals)
        g = got[name]
        if op == "count":
            assert g.dtype == U64 and g.tolist() == [0 if w is None else w for w in want], name
            continue
        assert isinstance(g, hj.KeyColumn) and g.values.dtype == (np.float64 if op == "mean" else np.int64 if col == "v" else U64), (name, g.values.dtype)
        ok = g.valid if g.valid is not None else np.ones(n, dtype=bool)
        assert ok.tolist() == [w is not None for w in want], name
        if op == "mean":
            # v's sums stay below 2^53: both sides divide two exact floats, correctly rounded
            assert g.values[ok].tolist() == [w for w in want if w is not None], name
        else:
            assert [int(x) % (1 << 64) for x in g.values[ok]] == [w % (1 << 64) for w in want if w is not None], name
