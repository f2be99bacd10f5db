"""What the range-join tests share: the numpy model of hj_range_index_* / hj_range_pairs_* (np.searchsorted over an order key
built HERE, never the library's), the brute-force O(|S| |R|) join that range_join / interval_join are held against (plain
numpy comparisons on the values, no order key at all), directed inputs and the seeded fuzz. No test in here, no device, and
nothing that asks the library what a result should be."""
import numpy as np

import htm_hashjoin_amd as hj

U32, U64 = np.uint32, np.uint64
NO_ROW = 0xFFFFFFFF
DTYPES = (np.uint8, np.uint16, np.uint32, np.uint64, np.int8, np.int16, np.int32, np.int64, np.float32, np.float64)
PICKS = ("all", "first", "last")


def val_type(dtype):
    return {"u": hj.HJ_VAL_UINT, "i": hj.HJ_VAL_INT, "f": hj.HJ_VAL_FLOAT}[np.dtype(dtype).kind]


def order_key(a):
    """(key, ordered): a uint64 per element that orders as the values do and ties exactly where they are equal (-0.0 == 0.0);
    ordered is False for a NaN, whose key means nothing"""
    a = np.asarray(a)
    if a.dtype.kind == "u":
        return a.astype(U64), np.ones(a.size, dtype=bool)
    if a.dtype.kind == "i":
        return a.astype(np.int64).view(U64) ^ U64(1 << 63), np.ones(a.size, dtype=bool)
    x = a.astype(np.float64) + 0.0                      # binary32 widens exactly; -0.0 + 0.0 is +0.0
    bits = x.view(U64)
    return np.where(bits >> U64(63) != 0, ~bits, bits | U64(1 << 63)), ~np.isnan(x)


def plane_words(bits):
    bits = np.asarray(bits, dtype=bool)
    padded = np.zeros(-(-bits.size // 32) * 32, dtype=bool)
    padded[:bits.size] = bits
    return np.packbits(padded, bitorder="little").view(U32).copy()


def packed(s, r):
    return np.sort((np.asarray(s).astype(U64) << U64(32)) | np.asarray(r).astype(U64))


def model_index(r, r_valid=None):
    """the index of a column: perm (indexed rows by value, stable; then the NaN rows, then the NULL rows, each by row), the
    order keys of the indexed prefix, head = (indexed, NULLs, NaNs)"""
    key, ordered = order_key(r)
    valid = np.ones(key.size, dtype=bool) if r_valid is None else np.asarray(r_valid, dtype=bool)
    idx = np.flatnonzero(valid & ordered)
    idx = idx[np.argsort(key[idx], kind="stable")]
    nans, nulls = np.flatnonzero(valid & ~ordered), np.flatnonzero(~valid)
    return {"perm": np.concatenate([idx, nans, nulls]).astype(U32), "keys": key[idx], "head": (idx.size, nulls.size, nans.size)}


def model_bounds(index, lo, hi, lo_valid=None, hi_valid=None, lo_open=False, hi_open=False, pick="all"):
    """per S row the half-open run [a, b) of index positions it pairs with (a == b: none), and whether a bound is NULL or NaN"""
    keys = index["keys"]
    n_s = (lo if lo is not None else hi).size
    a, b, ok = np.zeros(n_s, dtype=np.int64), np.full(n_s, keys.size, dtype=np.int64), np.ones(n_s, dtype=bool)
    if lo is not None:
        k, ordered = order_key(lo)
        ok &= ordered & (np.ones(n_s, dtype=bool) if lo_valid is None else np.asarray(lo_valid, dtype=bool))
        a = np.searchsorted(keys, k, side="right" if lo_open else "left").astype(np.int64)
    if hi is not None:
        k, ordered = order_key(hi)
        ok &= ordered & (np.ones(n_s, dtype=bool) if hi_valid is None else np.asarray(hi_valid, dtype=bool))
        b = np.searchsorted(keys, k, side="left" if hi_open else "right").astype(np.int64)
    hit = ok & (b > a)
    a, b = np.where(hit, a, 0), np.where(hit, b, 0)
    if pick == "first":
        b = np.where(hit, a + 1, 0)
    elif pick == "last":
        a = np.where(hit, np.searchsorted(keys, keys[np.maximum(b - 1, 0)] if keys.size else np.zeros(n_s, dtype=U64), side="left"), 0)
        b = np.where(hit, a + 1, 0)
    return a, b, ~ok


def model_call(r, lo, hi, r_valid=None, lo_valid=None, hi_valid=None, lo_open=False, hi_open=False, pick="all", s_row_base=0, capacity=None,
               expand=True):
    """what one range call leaves: "kept" (the pairs, packed and sorted; None with expand=False), "info" (pairs, written, 0, S
    rows with a pair, S rows with a NULL or NaN bound, rows indexed, 0, 0), the two mark planes of a call on cleared planes"""
    index = model_index(r, r_valid)
    a, b, bad = model_bounds(index, lo, hi, lo_valid, hi_valid, lo_open, hi_open, pick)
    cnt = b - a
    total = int(cnt.sum())
    covered = np.zeros(index["keys"].size + 1, dtype=np.int64)
    np.add.at(covered, a[cnt > 0], 1)
    np.add.at(covered, b[cnt > 0], -1)
    covered = np.cumsum(covered)[:-1] > 0
    r_bits = np.zeros(np.asarray(r).size, dtype=bool)
    r_bits[index["perm"][:covered.size][covered]] = True
    kept = None
    if expand:
        s = np.repeat(np.arange(cnt.size, dtype=np.int64), cnt)
        pos = np.repeat(a, cnt) + (np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt))
        kept = packed(s + s_row_base, index["perm"][pos])
    written = total if capacity is None else min(total, capacity)
    return {"kept": kept, "info": (total, written, 0, int((cnt > 0).sum()), int(bad.sum()), index["head"][0], 0, 0),
            "s_marks": plane_words(cnt > 0), "r_marks": plane_words(r_bits), "index": index, "a": a, "b": b}


# ---- the brute-force join: every (S row, R row) compared as values -------------------------------------------------------------
_OPS = {"==": np.equal, "!=": np.not_equal, "<": np.less, "<=": np.less_equal, ">": np.greater, ">=": np.greater_equal}


def _values(a):
    """(the values, one bool per row: valid)"""
    if isinstance(a, hj.KeyColumn):
        return a.values, (np.ones(a.rows, dtype=bool) if a.valid is None else a.valid)
    if isinstance(a, np.ma.MaskedArray):
        return np.ma.getdata(a), ~np.ma.getmaskarray(a)
    a = np.asarray(a)
    return a, np.ones(a.size, dtype=bool)


def brute_matches(r_values, s_lo, s_hi, lo_open=False, hi_open=False, pick="all", where=None):
    """match[s, r] of range_join: the range as plain comparisons (a NaN compares False, -0.0 == 0.0 by itself), then the
    pick, then the where terms"""
    r, r_ok = _values(r_values)
    n_r = r.size
    n_s = _values(s_lo if s_lo is not None else s_hi)[0].size
    nan = np.isnan(r) if r.dtype.kind == "f" else np.zeros(n_r, dtype=bool)
    m = np.broadcast_to((r_ok & ~nan)[None, :], (n_s, n_r)).copy()
    with np.errstate(invalid="ignore"):
        if s_lo is not None:
            lo, ok = _values(s_lo)
            m &= ok[:, None] & (np.less if lo_open else np.less_equal)(lo[:, None], r[None, :])
        if s_hi is not None:
            hi, ok = _values(s_hi)
            m &= ok[:, None] & (np.less if hi_open else np.less_equal)(r[None, :], hi[:, None])
    if pick != "all":
        out = np.zeros_like(m)
        for s in range(n_s):
            rows = np.flatnonzero(m[s])
            if rows.size:
                vals = r[rows]
                best = vals.min() if pick == "first" else vals.max()
                out[s, rows[vals == best][0]] = True        # ties to the lowest R row
        m = out
    for sv, op, rv in (where or ()):
        (a, a_ok), (b, b_ok) = _values(sv), _values(rv)
        with np.errstate(invalid="ignore"):
            m &= a_ok[:, None] & b_ok[None, :] & _OPS[op](a[:, None], b[None, :])
    return m


def brute_rows(m, how):
    """(s_idx, r_idx) of the join kind over the match matrix m[s, r], packed with NO_ROW where a side is absent; None for a
    plane the kind does not have"""
    s, r = np.nonzero(m)
    s_hit, r_hit = m.any(axis=1), m.any(axis=0)
    no = lambda n: np.full(n, NO_ROW, dtype=np.int64)      # noqa: E731
    s_un, r_un = np.flatnonzero(~s_hit), np.flatnonzero(~r_hit)
    if how == "inner":
        return s, r
    if how == "left":
        return np.concatenate([s, s_un]), np.concatenate([r, no(s_un.size)])
    if how == "semi":
        return np.flatnonzero(s_hit), None
    if how == "anti":
        return s_un, None
    if how == "right":
        return np.concatenate([s, no(r_un.size)]), np.concatenate([r, r_un])
    if how == "full":
        return np.concatenate([s, s_un, no(r_un.size)]), np.concatenate([r, no(s_un.size), r_un])
    if how == "right_semi":
        return None, np.flatnonzero(r_hit)
    return None, r_un                                       # right_anti


def assert_join(res, m, how, r_cols=None, s_cols=None, tag=None):
    """a result of range_join / interval_join / range_join_host against the brute-force rows of `how`, payload columns included"""
    s, r = brute_rows(m, how)
    assert (res["s_idx"] is None) == (s is None) and (res["r_idx"] is None) == (r is None), (tag, how, "planes")
    got_s = res["s_idx"] if s is not None else np.zeros(res["r_idx"].size, dtype=U32)
    got_r = res["r_idx"] if r is not None else np.zeros(res["s_idx"].size, dtype=U32)
    want = packed(s if s is not None else np.zeros(r.size, dtype=np.int64), r if r is not None else np.zeros(s.size, dtype=np.int64))
    assert np.array_equal(packed(got_s, got_r), want), (tag, how, "rows", got_s.size, want.size)
    for side, cols, idx in (("s", s_cols, res["s_idx"]), ("r", r_cols, res["r_idx"])):
        if idx is None:
            assert res[side] is None and res[side + "_valid"] is None, (tag, how, side)
            continue
        there = idx != NO_ROW
        assert np.array_equal(res[side + "_valid"], there), (tag, how, side, "valid")
        for name, col in (cols or {}).items():
            got = res[side][name]
            if isinstance(col, hj.KeyColumn):
                src_ok = np.ones(col.rows, dtype=bool) if col.valid is None else col.valid
                got_ok = np.ones(got.rows, dtype=bool) if got.valid is None else got.valid
                want_ok = there.copy()
                want_ok[there] = src_ok[idx[there]]
                assert np.array_equal(got_ok, want_ok), (tag, how, side, name, "NULLs")
                assert np.array_equal(got.values[want_ok], col.values[idx[want_ok]]), (tag, how, side, name)
            else:
                assert np.array_equal(got[there], col[idx[there]]), (tag, how, side, name)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def extremes(dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return np.array([-np.inf, np.finfo(dtype).min, -1.5, -0.0, 0.0, np.finfo(dtype).tiny, 1.5, np.finfo(dtype).max, np.inf], dtype=dtype)
    i = np.iinfo(dtype)
    return np.array(sorted({i.min, i.min + 1, 0, 1, i.max - 1, i.max} | ({-1} if dtype.kind == "i" else set())), dtype=dtype)


def directed(dtype):
    """R with runs of equal values and the type's extremes; bounds that hit a key, fall between two, lie below the first and
    above the last, are reversed, equal, extreme"""
    dtype = np.dtype(dtype)
    ext = extremes(dtype)
    r = np.concatenate([ext, np.array([3, 3, 3, 5, 9, 9, 20], dtype=dtype), ext[:2]])
    pts = np.concatenate([ext, np.array([2, 3, 4, 5, 9, 10, 20, 21], dtype=dtype)])
    lo, hi = np.repeat(pts, pts.size), np.tile(pts, pts.size)
    return r, lo, hi


def fuzz_case(seed, dtype, n_r, n_s, nulls=True):
    """a seeded case: R with duplicates, the type's extremes, NaNs and NULLs; bounds drawn from R's values, from between them and
    from the extremes, NULL and NaN bounds among them. -> (r, r_valid, lo, hi, lo_valid, hi_valid)"""
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    ext = extremes(dtype)

    def draw(n, spread):
        if dtype.kind == "f":
            a = (rng.integers(-spread, spread, n) / 4.0).astype(dtype)
        else:
            lo, hi = (0, min(2 * spread, int(np.iinfo(dtype).max))) if dtype.kind == "u" else (max(-spread, int(np.iinfo(dtype).min)), min(spread, int(np.iinfo(dtype).max)))
            a = rng.integers(lo, hi, n, endpoint=True).astype(dtype)
        at = rng.random(n) < 0.08
        a[at] = rng.choice(ext, int(at.sum()))
        if dtype.kind == "f":
            a[rng.random(n) < 0.04] = np.nan
        return a

    spread = max(4, n_r // 3)
    r, lo = draw(n_r, spread), draw(n_s, spread)
    width = draw(n_s, max(2, spread // 16))
    with np.errstate(all="ignore"):
        hi = np.where(rng.random(n_s) < 0.5, lo, (lo + np.abs(width)).astype(dtype) if dtype.kind == "f" else np.maximum(lo, lo + (np.abs(width.astype(np.int64)) % 7).astype(dtype)))
    hi = hi.astype(dtype)
    valid = lambda n: rng.random(n) > 0.05 if nulls else None     # noqa: E731
    return r, valid(n_r), lo, hi, valid(n_s), valid(n_s)
