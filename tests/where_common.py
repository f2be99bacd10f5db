"""What the tests of the join conditions share (test_where_abi.py, test_gpu_where.py, test_gpu_join_where.py,
test_gpu_where_stream_order.py): a numpy model of one hj_pairs_where call, a nested-loop model of a whole join with terms
for all eight kinds, a value ladder per dtype, and the ctypes plumbing of a term. Everything is written from the contract
in include/htm_hashjoin.h; nothing in here asks the library what a result should be.

A model term is (s_values, op, r_values, s_valid, r_valid): two numpy arrays of one dtype, op out of OPS, and per side
one bool per row (False: NULL) or None."""
import ctypes as C
import operator

import numpy as np

from htm_hashjoin_amd import _lib

from gpu_harness import packed, plane_words, row_bits

NO_ROW = 0xFFFFFFFF
U32, U64 = np.uint32, np.uint64
OPS = {"==": operator.eq, "!=": operator.ne, "<": operator.lt, "<=": operator.le, ">": operator.gt, ">=": operator.ge}
DTYPES = [np.dtype(t) for t in (np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64)]
TYPE_OF = {"u": _lib.HJ_VAL_UINT, "i": _lib.HJ_VAL_INT, "f": _lib.HJ_VAL_FLOAT}
HOWS = ("inner", "left", "semi", "anti", "right", "full", "right_semi", "right_anti")


def ladder(dtype):
    """the values of `dtype` a comparison can get wrong: 0, 1, the ends of the range, -1, both sides of the sign bit (uint64:
    of 2^63, where a signed compare turns the order round); floats: both zeros, both infinities, NaN, the smallest
    subnormal, adjacent values, and negative values, whose bit patterns order the other way round"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        one = dtype.type(1)
        sub = np.nextafter(dtype.type(0), one)
        return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, sub, -sub, 1.0, np.nextafter(one, dtype.type(2)), -1.0, -2.0,
                         np.finfo(dtype).max, np.finfo(dtype).tiny, 16777216.0, 16777218.0], dtype=dtype)
    info, bits = np.iinfo(dtype), 8 * dtype.itemsize
    vals = [0, 1, 2, info.min, info.min + 1, info.max, info.max - 1]
    vals += [(1 << (bits - 1)) - 1, 1 << (bits - 1), (1 << (bits - 1)) + 1] if dtype.kind == "u" else [-1, -2, 100, -100]
    return np.array(list(dict.fromkeys(vals)), dtype=dtype)


def term_of(s, op, r, s_valid=None, r_valid=None):
    assert s.dtype == r.dtype and op in OPS
    return (s, op, r, s_valid, r_valid)


def holds(term, si, ri):
    """whether the term holds for the pairs (si[k], ri[k]): numpy's own comparison of two arrays of one dtype -- integers
    by value, floats by IEEE-754 -- and False where either side is NULL"""
    s, op, r, s_valid, r_valid = term
    with np.errstate(invalid="ignore"):
        ok = OPS[op](s[si], r[ri])
    if s_valid is not None:
        ok &= s_valid[si]
    if r_valid is not None:
        ok &= r_valid[ri]
    return ok


def model_call(map_s, map_r, base, s_rows, r_rows, terms, capacity=None):
    """one call: -> {"keep": one bool per pair, "kept": the kept multiset (packed, sorted), "s_marks" / "r_marks": the planes
    a call on cleared planes leaves, "info": (kept, written, 0, dropped)}"""
    s = (map_s.astype(np.int64) - base) % (1 << 32)
    r = map_r.astype(np.int64)
    ok = (map_s != NO_ROW) & (map_r != NO_ROW) & (s < s_rows) & (r < r_rows)
    keep = ok.copy()
    for term in terms:
        keep[ok] &= holds(term, s[ok], r[ok])
    kept = int(keep.sum())
    cap = map_s.size if capacity is None else capacity
    return {"keep": keep, "kept": packed(map_s[keep], map_r[keep]), "s_marks": plane_words(row_bits(s[keep], s_rows)),
            "r_marks": plane_words(row_bits(r[keep], r_rows)), "info": (kept, min(kept, cap), 0, int((~ok).sum()))}


def model_join(how, r_keys, s_keys, terms):
    """The whole join by nested loops: r_keys / s_keys one hashable key per row (None: a NULL key, which matches nothing).
    A pair is a match iff the keys are equal and every term holds. -> the rows of the kind as a sorted list of (s, r), NO_ROW
    on the side a row does not have; semi / anti: (s, NO_ROW) per S row, right_semi / right_anti: (NO_ROW, r) per R row"""
    n_r, n_s = len(r_keys), len(s_keys)
    by_key = {}
    for r, k in enumerate(r_keys):
        if k is not None:
            by_key.setdefault(k, []).append(r)
    cand = [(s, r) for s, k in enumerate(s_keys) if k is not None for r in by_key.get(k, ())]
    si, ri = np.array([c[0] for c in cand], dtype=np.int64), np.array([c[1] for c in cand], dtype=np.int64)
    keep = np.ones(len(cand), dtype=bool)
    for term in terms:
        keep &= holds(term, si, ri)
    inner = [c for c, k in zip(cand, keep) if k]
    s_hit, r_hit = {s for s, _ in inner}, {r for _, r in inner}
    s_un = [(s, NO_ROW) for s in range(n_s) if s not in s_hit]
    r_un = [(NO_ROW, r) for r in range(n_r) if r not in r_hit]
    rows = {"inner": inner, "left": inner + s_un, "semi": [(s, NO_ROW) for s in sorted(s_hit)], "anti": s_un,
            "right": inner + r_un, "full": inner + s_un + r_un, "right_semi": [(NO_ROW, r) for r in sorted(r_hit)], "right_anti": r_un}[how]
    return sorted(rows), {"cand": cand, "keep": keep, "inner": inner, "s_hit": s_hit, "r_hit": r_hit}


def rows_of(result):
    """the (s, r) rows of a join_tables / join_on result dict, in model_join's form"""
    s_idx, r_idx = result["s_idx"], result["r_idx"]
    n = s_idx.size if s_idx is not None else r_idx.size
    s = s_idx if s_idx is not None else np.full(n, NO_ROW, dtype=U32)
    r = r_idx if r_idx is not None else np.full(n, NO_ROW, dtype=U32)
    return sorted(zip(s.tolist(), r.tolist()))


def c_terms(terms, ptr=None):
    """model terms -> (hj_where_term array, count, what must stay alive). ptr(array) gives the address the library is to
    read (default: the numpy array's own, aligned by numpy's allocator for these sizes); a validity goes through
    plane_words first"""
    keep = []

    def at(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        keep.append(a)
        return (ptr(a) if ptr else a.ctypes.data) or None

    arr = (_lib.hj_where_term * max(len(terms), 1))()
    for c, (s, op, r, s_valid, r_valid) in zip(arr, terms):
        c.s, c.r = at(s), at(r)
        c.sValid = at(plane_words(s_valid)) if s_valid is not None else None
        c.rValid = at(plane_words(r_valid)) if r_valid is not None else None
        c.width, c.type, c.op, c.reserved = s.dtype.itemsize, TYPE_OF[s.dtype.kind], _lib.CMP_OPS[op], 0
    return arr, len(terms), keep
