"""hj_pairs_where_host and the argument checks of hj_pairs_where_dev / hj_where_info through ctypes -> C ABI, without a GPU:
the host form runs the body the kernel runs for a term (hj_where.hip: where_holds), so the comparison semantics of
include/htm_hashjoin.h -- integers by width and signedness, floats by IEEE-754, NULL as unknown -- are checked here, against
the numpy model of where_common.py. The device form is held against the same model in test_gpu_where.py."""
import ctypes as C
import itertools

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

import where_common as wc
from gpu_harness import packed

U32, NO_ROW = np.uint32, wc.NO_ROW
SENT = 0xA5A5A5A5
INVALID, OK = _lib.HJ_ERR_INVALID, _lib.HJ_OK


def vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def host_call(map_s, map_r, base, s_rows, r_rows, terms, capacity=None, marks=True, s_marks=None, r_marks=None):
    """one hj_pairs_where_host -> (status, out_s, out_r with 8 sentinel words behind the capacity, the planes, info)"""
    n = map_s.size
    cap = n if capacity is None else capacity
    out_s, out_r = np.full(cap + 8, SENT, dtype=U32), np.full(cap + 8, SENT, dtype=U32)
    if marks and s_marks is None:
        s_marks, r_marks = np.zeros(-(-s_rows // 32), dtype=U32), np.zeros(-(-r_rows // 32), dtype=U32)
    arr, k, _alive = wc.c_terms(terms)
    info = (C.c_uint64 * 4)(7, 7, 7, 7)
    rc = lib.hj_pairs_where_host(vp(map_s), vp(map_r), n, base, s_rows, r_rows, arr, k, vp(out_s) if cap else None, vp(out_r) if cap else None,
                                 cap, vp(s_marks), vp(r_marks), info)
    return rc, out_s, out_r, s_marks, r_marks, tuple(int(x) for x in info)


def check(map_s, map_r, base, s_rows, r_rows, terms, capacity=None, tag=None):
    want = wc.model_call(map_s, map_r, base, s_rows, r_rows, terms, capacity)
    rc, out_s, out_r, s_marks, r_marks, info = host_call(map_s, map_r, base, s_rows, r_rows, terms, capacity)
    assert rc == OK, tag
    assert info == want["info"], (tag, info, want["info"])
    written = info[1]
    assert (out_s[written:] == SENT).all() and (out_r[written:] == SENT).all(), (tag, "a word behind the run was written")
    # the host form keeps the input order
    keep = want["keep"]
    assert np.array_equal(out_s[:written], map_s[keep][:written]) and np.array_equal(out_r[:written], map_r[keep][:written]), tag
    assert np.array_equal(s_marks, want["s_marks"]) and np.array_equal(r_marks, want["r_marks"]), (tag, "marks")
    return want


def cross(n_s, n_r):
    """every pair of n_s x n_r rows"""
    s, r = np.divmod(np.arange(n_s * n_r, dtype=np.int64), n_r)
    return s.astype(U32), r.astype(U32)


def test_the_term_is_48_bytes():
    assert C.sizeof(_lib.hj_where_term) == 48
    assert _lib.CMP_OPS == {"==": 0, "!=": 1, "<": 2, "<=": 3, ">": 4, ">=": 5}
    assert _lib.HJ_WHERE_MAX_TERMS == 4


@pytest.mark.parametrize("dtype", wc.DTYPES, ids=str)
@pytest.mark.parametrize("op", list(wc.OPS))
def test_every_op_on_every_type_and_width(dtype, op):
    """the ladder against itself: every pair of its values under the op"""
    v = wc.ladder(dtype)
    map_s, map_r = cross(v.size, v.size)
    want = check(map_s, map_r, 0, v.size, v.size, [wc.term_of(v, op, v.copy())], tag=(str(dtype), op))
    assert 0 < want["info"][0] < map_s.size                  # the ladder has pairs on both sides of every op


def test_the_values_the_ladders_must_hold():
    u64, i8, f32 = wc.ladder(np.uint64), wc.ladder(np.int8), wc.ladder(np.float32)
    assert {(1 << 63) - 1, 1 << 63, (1 << 63) + 1, 0, 1, (1 << 64) - 1} <= set(u64.tolist())
    assert {-128, 127, -1, 0, 1} <= set(i8.tolist())
    assert np.isnan(f32).any() and np.isinf(f32).sum() == 2 and (np.signbit(f32) & (f32 == 0)).any()
    assert (f32 == np.nextafter(np.float32(0), np.float32(1))).any() and (f32 == np.nextafter(np.float32(1), np.float32(2))).any()
    # the spelled-out cases of the contract, straight through the host form
    one = lambda a, op, b, dt: host_call(np.zeros(1, U32), np.zeros(1, U32), 0, 1, 1, [wc.term_of(np.array([a], dt), op, np.array([b], dt))])[5][0]    # noqa: E731
    assert one(1 << 63, ">", (1 << 63) - 1, np.uint64) == 1 and one(1 << 63, "<", (1 << 63) - 1, np.uint64) == 0
    assert one(-128, "<", 127, np.int8) == 1 and one(-1, "<", 0, np.int64) == 1 and one(0xFF, ">", 0, np.uint8) == 1
    assert one(-0.0, "==", 0.0, np.float64) == 1 and one(-0.0, "<", 0.0, np.float32) == 0 and one(-0.0, "!=", 0.0, np.float32) == 0
    for dt in (np.float32, np.float64):
        for a, b in ((np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan)):
            assert [one(a, op, b, dt) for op in ("==", "!=", "<", "<=", ">", ">=")] == [0, 1, 0, 0, 0, 0], (dt, a, b)
    assert one(16777216.0, "<", 16777218.0, np.float32) == 1 and one(-2.0, "<", -1.0, np.float32) == 1


@pytest.mark.parametrize("op", list(wc.OPS))
@pytest.mark.parametrize("dtype", [np.dtype(np.int32), np.dtype(np.float64), np.dtype(np.uint8)], ids=str)
def test_a_null_on_either_side_does_not_hold(dtype, op):
    v = wc.ladder(dtype)
    n = v.size
    map_s, map_r = cross(n, n)
    s_valid, r_valid = np.arange(n) % 3 != 0, np.arange(n) % 2 != 1
    for sv, rv in ((s_valid, None), (None, r_valid), (s_valid, r_valid)):
        want = check(map_s, map_r, 0, n, n, [wc.term_of(v, op, v.copy(), sv, rv)], tag=(str(dtype), op))
        si, ri = np.divmod(np.flatnonzero(want["keep"]), n)
        assert (sv is None or sv[si].all()) and (rv is None or rv[ri].all())
    # all NULL on one side: nothing holds, "!=" included
    want = check(map_s, map_r, 0, n, n, [wc.term_of(v, op, v.copy(), np.zeros(n, dtype=bool), None)])
    assert want["info"][0] == 0


def four_terms(rng, n_s, n_r):
    """four terms of the four widths and the three types, two of them with NULLs"""
    return [wc.term_of(rng.integers(0, 4, n_s).astype(np.uint8), "<=", rng.integers(0, 4, n_r).astype(np.uint8)),
            wc.term_of(rng.integers(-3, 3, n_s).astype(np.int16), ">=", rng.integers(-3, 3, n_r).astype(np.int16), rng.random(n_s) < 0.9, None),
            wc.term_of(rng.integers(0, 3, n_s).astype(np.float32), "!=", rng.integers(0, 3, n_r).astype(np.float32)),
            wc.term_of(rng.integers(-5, 5, n_s).astype(np.int64), "<", rng.integers(-5, 5, n_r).astype(np.int64), None, rng.random(n_r) < 0.9)]


def test_four_terms_of_different_widths():
    rng = np.random.default_rng(4)
    n_s, n_r, n = 300, 200, 5000
    terms = four_terms(rng, n_s, n_r)
    map_s, map_r = rng.integers(0, n_s, n).astype(U32), rng.integers(0, n_r, n).astype(U32)
    want = check(map_s, map_r, 0, n_s, n_r, terms)
    assert 0 < want["info"][0] < n // 4
    for k in range(1, 4):       # every prefix keeps no less
        assert check(map_s, map_r, 0, n_s, n_r, terms[:k])["info"][0] >= want["info"][0]


def test_dropped_entries_and_a_row_base():
    rng = np.random.default_rng(5)
    n_s, n_r, n, base = 100, 70, 3000, 1000
    s, r = rng.integers(0, 1 << 20, n_s).astype(np.uint32), rng.integers(0, 1 << 20, n_r).astype(np.uint32)
    map_s, map_r = (base + rng.integers(0, n_s, n)).astype(U32), rng.integers(0, n_r, n).astype(U32)
    map_s[::7] = NO_ROW
    map_r[3::11] = NO_ROW
    map_s[5::13] = base + n_s            # the first row behind S
    map_s[6::17] = base - 1              # below the base: wraps to a huge row
    map_r[8::19] = n_r
    want = check(map_s, map_r, base, n_s, n_r, [wc.term_of(s, "!=", r)], tag="dropped")
    assert want["info"][3] > n // 4 and want["info"][0] > 0
    assert want["info"][0] + want["info"][3] == n        # "!=" on random values keeps everything that is not dropped
    # a relation without rows: everything is dropped, and its column may be NULL
    none = np.zeros(0, dtype=np.uint32)
    for s_rows, r_rows, a, b in ((0, n_r, none, r), (n_s, 0, s, none), (0, 0, none, none)):
        arr, k, _alive = wc.c_terms([wc.term_of(a, "==", b)])
        if not s_rows:
            arr[0].s = None
        if not r_rows:
            arr[0].r = None
        info = (C.c_uint64 * 4)()
        out, out2 = np.full(n, SENT, dtype=U32), np.full(n, SENT, dtype=U32)
        assert lib.hj_pairs_where_host(vp(map_s), vp(map_r), n, base, s_rows, r_rows, arr, k, vp(out), vp(out2), n, None, None, info) == OK
        assert tuple(info) == (0, 0, 0, n) and (out == SENT).all() and (out2 == SENT).all()


def test_capacity_and_the_mark_only_pass():
    rng = np.random.default_rng(6)
    n_s, n_r, n = 500, 400, 4000
    s, r = rng.integers(0, 10, n_s).astype(np.int32), rng.integers(0, 10, n_r).astype(np.int32)
    map_s, map_r = rng.integers(0, n_s, n).astype(U32), rng.integers(0, n_r, n).astype(U32)
    terms = [wc.term_of(s, "<=", r)]
    full = check(map_s, map_r, 0, n_s, n_r, terms)
    kept = full["info"][0]
    assert kept > 1000
    cut = check(map_s, map_r, 0, n_s, n_r, terms, capacity=kept // 3, tag="cut")        # exact count, nothing behind, marks of cut pairs
    assert cut["info"][:2] == (kept, kept // 3) and np.array_equal(cut["s_marks"], full["s_marks"])
    rc, _s, _r, s_marks, r_marks, info = host_call(map_s, map_r, 0, n_s, n_r, terms, capacity=0)         # NULL outputs
    assert rc == OK and info == (kept, 0, 0, 0)
    assert np.array_equal(s_marks, full["s_marks"]) and np.array_equal(r_marks, full["r_marks"])
    # no planes at all, no info: the pairs alone
    arr, k, _alive = wc.c_terms(terms)
    out_s, out_r = np.empty(n, dtype=U32), np.empty(n, dtype=U32)
    assert lib.hj_pairs_where_host(vp(map_s), vp(map_r), n, 0, n_s, n_r, arr, k, vp(out_s), vp(out_r), n, None, None, None) == OK
    assert np.array_equal(packed(out_s[:kept], out_r[:kept]), full["kept"])
    # nPairs 0 keeps nothing, maps and outputs NULL
    info = (C.c_uint64 * 4)(9, 9, 9, 9)
    assert lib.hj_pairs_where_host(None, None, 0, 0, n_s, n_r, arr, k, None, None, 5, None, None, info) == OK and tuple(info) == (0, 0, 0, 0)


def test_preset_mark_bits_survive():
    rng = np.random.default_rng(7)
    n_s, n_r, n = 200, 300, 500
    s, r = rng.integers(0, 4, n_s).astype(np.uint16), rng.integers(0, 4, n_r).astype(np.uint16)
    map_s, map_r = rng.integers(0, n_s, n).astype(U32), rng.integers(0, n_r, n).astype(U32)
    terms = [wc.term_of(s, "==", r)]
    want = wc.model_call(map_s, map_r, 0, n_s, n_r, terms)
    pre_s, pre_r = rng.integers(0, 1 << 32, -(-n_s // 32)).astype(U32), rng.integers(0, 1 << 32, -(-n_r // 32)).astype(U32)
    rc, _s, _r, s_marks, r_marks, _info = host_call(map_s, map_r, 0, n_s, n_r, terms, s_marks=pre_s.copy(), r_marks=pre_r.copy())
    assert rc == OK
    assert np.array_equal(s_marks, pre_s | want["s_marks"]) and np.array_equal(r_marks, pre_r | want["r_marks"])
    assert not np.array_equal(s_marks, pre_s)


def test_the_python_form():
    rng = np.random.default_rng(8)
    n_s, n_r, n = 90, 80, 700
    terms = four_terms(rng, n_s, n_r)
    map_s, map_r = (10 + rng.integers(0, n_s + 5, n)).astype(U32), rng.integers(0, n_r, n).astype(U32)
    want = wc.model_call(map_s, map_r, 10, n_s, n_r, terms)
    py_terms = [(np.ma.MaskedArray(s, mask=~sv) if sv is not None else s, op, hj.KeyColumn(r, rv)) for s, op, r, sv, rv in terms]
    got = hj.pairs_where_host(map_s, map_r, 10, py_terms, marks=True)
    assert got["info"] == want["info"] and np.array_equal(packed(got["s_idx"], got["r_idx"]), want["kept"])
    assert np.array_equal(got["s_marks"], want["s_marks"]) and np.array_equal(got["r_marks"], want["r_marks"])
    cut = hj.pairs_where_host(map_s, map_r, 10, py_terms, capacity=3)
    assert cut["info"][:2] == (want["info"][0], 3) and cut["s_idx"].size == 3 and "s_marks" not in cut
    a32, a64 = np.zeros(n_s, np.int32), np.zeros(n_r, np.int64)
    for bad in ([], [(a32, "=", a32[:n_r])], [(a32, "<", a64)], [(a32, "<", a32[:n_r])] * 5, [(a32.astype(np.float16), "<", a32[:n_r].astype(np.float16))],
                [(hj.KeyColumn.from_list([b"a"] * n_s), "<", hj.KeyColumn.from_list([b"a"] * n_r))], [(a32.reshape(2, -1), "<", a32[:n_r])],
                [(a32, "<", a32[:n_r]), (a32[:-1], "<", a32[:n_r])]):
        with pytest.raises(ValueError):
            hj.pairs_where_host(map_s, map_r, 10, bad)


def test_what_is_refused_writes_nothing():
    """every HJ_ERR_INVALID of the header, on the host form (outputs, planes and info keep their sentinels) and, for a NULL
    context, on the device form"""
    n_s, n_r, n = 40, 30, 64
    s, r = np.arange(n_s, dtype=np.uint64), np.arange(n_r, dtype=np.uint64)
    map_s, map_r = (np.arange(n) % n_s).astype(U32), (np.arange(n) % n_r).astype(U32)
    good = dict(mapS=map_s, mapR=map_r, nPairs=n, sRows=n_s, rRows=n_r, nTerms=1, outS=True, outR=True, capacity=n, terms=True)

    def call(edit=None, **kw):
        a = dict(good, **kw)
        arr, _k, _alive = wc.c_terms([wc.term_of(s, "<", r, np.ones(n_s, dtype=bool), np.ones(n_r, dtype=bool))] * 4)
        if edit:
            edit(arr[0])
        out_s, out_r = np.full(n, SENT, dtype=U32), np.full(n, SENT, dtype=U32)
        s_marks, r_marks = np.full(2, SENT, dtype=U32), np.full(1, SENT, dtype=U32)
        info = (C.c_uint64 * 4)(7, 7, 7, 7)
        rc = lib.hj_pairs_where_host(vp(a["mapS"]), vp(a["mapR"]), a["nPairs"], 0, a["sRows"], a["rRows"], arr if a["terms"] else None, a["nTerms"],
                                     vp(out_s) if a["outS"] else None, vp(out_r) if a["outR"] else None, a["capacity"], vp(s_marks), vp(r_marks), info)
        untouched = (out_s == SENT).all() and (out_r == SENT).all() and (s_marks == SENT).all() and (r_marks == SENT).all() and tuple(info) == (7, 7, 7, 7)
        return rc, untouched

    assert call()[0] == OK and not call()[1]

    def field(name, value):
        return lambda t: setattr(t, name, value)

    def shifted(name, by):
        return lambda t: setattr(t, name, getattr(t, name) + by)

    refused = {
        "no term": dict(nTerms=0), "five terms": dict(nTerms=5), "terms NULL": dict(terms=False),
        "type": dict(edit=field("type", 3)), "op": dict(edit=field("op", 6)), "width 3": dict(edit=field("width", 3)),
        "width 16": dict(edit=field("width", 16)), "width 0": dict(edit=field("width", 0)),
        "float of 2 bytes": dict(edit=lambda t: (setattr(t, "type", _lib.HJ_VAL_FLOAT), setattr(t, "width", 2))),
        "float of 1 byte": dict(edit=lambda t: (setattr(t, "type", _lib.HJ_VAL_FLOAT), setattr(t, "width", 1))),
        "reserved": dict(edit=field("reserved", 1)),
        "s NULL": dict(edit=field("s", None)), "r NULL": dict(edit=field("r", None)),
        "s misaligned": dict(edit=shifted("s", 4)), "r misaligned": dict(edit=shifted("r", 2)),
        "sValid misaligned": dict(edit=shifted("sValid", 2)), "rValid misaligned": dict(edit=shifted("rValid", 1)),
        "mapS NULL": dict(mapS=None), "mapR NULL": dict(mapR=None), "outS NULL": dict(outS=False), "outR NULL": dict(outR=False),
        "nPairs 2^32": dict(nPairs=1 << 32), "sRows 2^32": dict(sRows=1 << 32), "rRows 2^32": dict(rRows=1 << 32),
    }
    for name, kw in refused.items():
        rc, untouched = call(**kw)
        assert rc == INVALID and untouched, name
    # what is NOT refused: a NULL column of a side without rows, NULL maps without pairs, NULL outputs without a capacity
    assert call(edit=field("s", None), sRows=0)[0] == OK and call(edit=field("r", None), rRows=0)[0] == OK
    assert call(mapS=None, mapR=None, nPairs=0)[0] == OK and call(outS=False, outR=False, capacity=0)[0] == OK
    # the device form and its info: a NULL context is refused before anything else
    arr, k, _alive = wc.c_terms([wc.term_of(s, "<", r)])
    assert lib.hj_pairs_where_dev(None, vp(map_s), vp(map_r), n, 0, n_s, n_r, arr, k, None, None, 0, None, None) == INVALID
    assert lib.hj_where_info(None, (C.c_uint64 * 4)()) == INVALID


def test_where_is_checked_before_any_device_work():
    """the wrappers' ValueErrors need no device; None and [] are no condition (and then need one, which this box lacks)"""
    R, S = np.arange(1, 9, dtype=np.uint64), np.arange(1, 6, dtype=np.uint64)
    a_r, a_s = np.zeros(8, np.int32), np.zeros(5, np.int32)
    for join in (lambda **kw: hj.join_tables(R, S, **kw), lambda **kw: hj.join_on(R, S, **kw), lambda **kw: hj.join_on_columns(R, S, **kw)):
        for bad in ([(a_s, "~", a_r)], [(a_s, "<", a_r.astype(np.int64))], [(a_s, "<", a_r)] * 5, [(a_s[:-1], "<", a_r)], [(a_s, "<", a_r[:-1])],
                    [(a_s, "<")], [(hj.KeyColumn.from_list([b"x"] * 5), "<", hj.KeyColumn.from_list([b"x"] * 8))],
                    [(a_s.astype(np.float16), "<", a_r.astype(np.float16))], [(a_s.astype(bool), "<", a_r.astype(bool))]):
            with pytest.raises(ValueError):
                join(where=bad)
    # one side empty: the result needs no device, with a condition as without
    none = np.zeros(0, dtype=np.uint64)
    for how in wc.HOWS:
        got = hj.join_tables(R, none, how=how, where=[(np.zeros(0, np.int32), "<", a_r)])
        want = hj.join_tables(R, none, how=how)
        assert got.keys() == want.keys() and all(np.array_equal(got[k], want[k]) for k in ("s_idx", "r_idx")), how
