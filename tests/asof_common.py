"""What the tests of the as-of joins share (test_asof_abi.py, test_gpu_asof.py, test_gpu_join_asof.py,
test_gpu_asof_stream_order.py): a model of one hj_pairs_asof call in numpy and Python loops, a nested-loop model of a whole
join with where terms and an as-of term for all eight kinds, and the ctypes plumbing of a term. Everything is written from
the contract in include/htm_hashjoin.h; nothing in here asks the library what a result should be. The values come from
where_common.ladder.

A model term is where_common's: (s_values, op, r_values, s_valid, r_valid), op out of ASOF_OPS."""
import numpy as np

from htm_hashjoin_amd import _lib

import where_common as wc
from gpu_harness import packed, plane_words, row_bits

NO_ROW, U32, U64 = wc.NO_ROW, np.uint32, np.uint64
ASOF_OPS = (">=", ">", "<=", "<")
BACKWARD = (">=", ">")


def better(op, v, cur):
    """whether the R value v beats the R value cur: the larger one backward, the smaller one forward (numpy's own compare)"""
    return bool(v > cur) if op in BACKWARD else bool(v < cur)


def pick(term, pairs):
    """{s: r}: per S row, of the (s, r) in `pairs` (all eligible), the one with the best R value, ties to the lowest R row"""
    _s, op, r_values, _sv, _rv = term
    best = {}
    for s, r in pairs:
        cur = best.get(s)
        if cur is None or better(op, r_values[r], r_values[cur]) or (r_values[r] == r_values[cur] and r < cur):
            best[s] = r
    return best


def model_call(map_s, map_r, base, s_rows, r_rows, term, capacity=None):
    """one call: -> {"keep": one bool per pair, "kept": the kept multiset (packed, sorted), "s_marks" / "r_marks": the planes
    a call on cleared planes leaves, "best_row": the plane the call leaves, "info": (kept, written, 0, dropped)}"""
    assert term[1] in ASOF_OPS
    s = (map_s.astype(np.int64) - base) % (1 << 32)
    r = map_r.astype(np.int64)
    ok = (map_s != NO_ROW) & (map_r != NO_ROW) & (s < s_rows) & (r < r_rows)
    elig = ok.copy()
    elig[ok] &= wc.holds(term, s[ok], r[ok])
    best = pick(term, zip(s[elig].tolist(), r[elig].tolist()))
    best_row = np.full(s_rows, NO_ROW, dtype=U32)
    for si, ri in best.items():
        best_row[si] = ri
    keep = ok.copy()
    keep[ok] = best_row[s[ok]] == r[ok]         # every copy of the winning pair; an entry of NO_ROW equals no live r
    kept = int(keep.sum())
    cap = map_s.size if capacity is None else capacity
    return {"keep": keep, "kept": packed(map_s[keep], map_r[keep]), "s_marks": plane_words(row_bits(s[keep], s_rows)),
            "r_marks": plane_words(row_bits(r[keep], r_rows)), "best_row": best_row, "info": (kept, min(kept, cap), 0, int((~ok).sum()))}


def model_join_asof(how, r_keys, s_keys, where_terms, asof_term):
    """The whole join by nested loops: r_keys / s_keys one hashable key per row (None: a NULL key, which matches nothing).
    A pair is a match iff the keys are equal, every where term holds, and it is the as-of pair of its S row among such
    pairs. -> the rows of the kind as a sorted list of (s, r) in where_common.model_join's form, and the parts"""
    n_r, n_s = len(r_keys), len(s_keys)
    by_key = {}
    for r, k in enumerate(r_keys):
        if k is not None:
            by_key.setdefault(k, []).append(r)
    cand = [(s, r) for s, k in enumerate(s_keys) if k is not None for r in by_key.get(k, ())]
    si, ri = np.array([c[0] for c in cand], dtype=np.int64), np.array([c[1] for c in cand], dtype=np.int64)
    ok = np.ones(len(cand), dtype=bool)
    for term in list(where_terms or []) + [asof_term]:
        ok &= wc.holds(term, si, ri)
    inner = sorted(pick(asof_term, [c for c, k in zip(cand, ok) if k]).items())
    s_hit, r_hit = {s for s, _ in inner}, {r for _, r in inner}
    s_un = [(s, NO_ROW) for s in range(n_s) if s not in s_hit]
    r_un = [(NO_ROW, r) for r in range(n_r) if r not in r_hit]
    rows = {"inner": inner, "left": inner + s_un, "semi": [(s, NO_ROW) for s in sorted(s_hit)], "anti": s_un,
            "right": inner + r_un, "full": inner + s_un + r_un, "right_semi": [(NO_ROW, r) for r in sorted(r_hit)], "right_anti": r_un}[how]
    return sorted(rows), {"cand": cand, "eligible": ok, "inner": inner, "s_hit": s_hit, "r_hit": r_hit}


def c_term(term, ptr=None):
    """a model term -> (hj_asof_term, what must stay alive); ptr(array) gives the address the library is to read (default:
    the numpy array's own); a validity goes through plane_words first"""
    keep = []

    def at(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        keep.append(a)
        return (ptr(a) if ptr else a.ctypes.data) or None

    s, op, r, s_valid, r_valid = term
    t = _lib.hj_asof_term()
    t.s, t.r = at(s), at(r)
    t.sValid = at(plane_words(s_valid)) if s_valid is not None else None
    t.rValid = at(plane_words(r_valid)) if r_valid is not None else None
    t.width, t.type, t.op, t.reserved = s.dtype.itemsize, wc.TYPE_OF[s.dtype.kind], _lib.CMP_OPS[op], 0
    return t, keep
