"""hj_pairs_asof_host and the argument checks of hj_pairs_asof_dev / hj_asof_info through ctypes -> C ABI, without a GPU: the
host form runs the bodies the kernels run (hj_columns.h: where_holds for eligibility, asof_key for the order), so which pair
an S row keeps -- by type, width and signedness, with NULLs, NaNs, both zeros and ties -- is checked here, against the model
of asof_common.py. The device form is held against the same model in test_gpu_asof.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

import asof_common as ac
import stream_order as so
import where_common as wc
from gpu_harness import packed, plane_words, row_bits

U32, U64, NO_ROW = np.uint32, np.uint64, wc.NO_ROW
SENT = 0xA5A5A5A5
INVALID, OK = _lib.HJ_ERR_INVALID, _lib.HJ_OK
HEADER = os.path.join(os.path.dirname(__file__), "..", "include", "htm_hashjoin.h")


def vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def host_call(map_s, map_r, base, s_rows, r_rows, term, capacity=None, marks=True):
    """one hj_pairs_asof_host -> (status, out_s, out_r with 8 sentinel words behind the capacity, the two mark planes, the
    bestRow plane with 8 sentinel words behind it, info)"""
    n = map_s.size
    cap = n if capacity is None else capacity
    out_s, out_r = np.full(cap + 8, SENT, dtype=U32), np.full(cap + 8, SENT, dtype=U32)
    s_marks, r_marks = (np.zeros(-(-s_rows // 32), dtype=U32), np.zeros(-(-r_rows // 32), dtype=U32)) if marks else (None, None)
    best_val, best_row = np.full(s_rows + 8, 0x5A5A5A5A5A5A5A5A, dtype=U64), np.full(s_rows + 8, SENT, dtype=U32)
    t, _alive = ac.c_term(term)
    info = (C.c_uint64 * 4)(7, 7, 7, 7)
    rc = lib.hj_pairs_asof_host(vp(map_s), vp(map_r), n, base, s_rows, r_rows, C.byref(t), vp(best_val), vp(best_row),
                                vp(out_s) if cap else None, vp(out_r) if cap else None, cap, vp(s_marks), vp(r_marks), info)
    assert (best_val[s_rows:] == 0x5A5A5A5A5A5A5A5A).all() and (best_row[s_rows:] == SENT).all(), "a word behind a best plane was written"
    return rc, out_s, out_r, s_marks, r_marks, best_row[:s_rows], tuple(int(x) for x in info)


def check(map_s, map_r, base, s_rows, r_rows, term, capacity=None, tag=None):
    want = ac.model_call(map_s, map_r, base, s_rows, r_rows, term, capacity)
    rc, out_s, out_r, s_marks, r_marks, best_row, info = host_call(map_s, map_r, base, s_rows, r_rows, term, capacity)
    assert rc == OK, tag
    assert info == want["info"], (tag, info, want["info"])
    written = info[1]
    assert (out_s[written:] == SENT).all() and (out_r[written:] == SENT).all(), (tag, "a word behind the run was written")
    keep = want["keep"]         # the host form keeps the input order
    assert np.array_equal(out_s[:written], map_s[keep][:written]) and np.array_equal(out_r[:written], map_r[keep][:written]), tag
    assert np.array_equal(s_marks, want["s_marks"]) and np.array_equal(r_marks, want["r_marks"]), (tag, "marks")
    assert np.array_equal(best_row, want["best_row"]), (tag, "bestRow")
    return want


def cross(n_s, n_r):
    s, r = np.divmod(np.arange(n_s * n_r, dtype=np.int64), n_r)
    return s.astype(U32), r.astype(U32)


def _declared_args(symbol):
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % symbol, code)
    assert decl, f"{symbol} is not declared in include/htm_hashjoin.h"
    return [a.strip() for a in decl.group(1).split(",")]


def test_header_lib_and_contract_table_agree():
    code = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"#define\s+HJ_ABI_VERSION\s+4\b", code) and lib.hj_abi_version() == 4        # additive
    assert re.search(r"\}\s*hj_asof_term\s*;", code)
    assert C.sizeof(_lib.hj_asof_term) == 48 and [f[0] for f in _lib.hj_asof_term._fields_] == ["s", "r", "sValid", "rValid", "width", "type", "op", "reserved"]
    assert _lib.ASOF_OPS == {">=": 5, ">": 4, "<=": 3, "<": 2}
    vpt, u64, u32, P = C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER
    sig = lib._hj_signatures
    assert sig["hj_pairs_asof_dev"] == ([vpt, vpt, vpt, u64, u32, u64, u64, P(_lib.hj_asof_term), vpt, vpt, vpt, vpt, u64, vpt, vpt], C.c_int)
    assert sig["hj_asof_info"] == ([vpt, P(u64)], C.c_int)
    assert sig["hj_pairs_asof_host"] == (sig["hj_pairs_asof_dev"][0][1:] + [P(u64)], C.c_int)
    dev, host = _declared_args("hj_pairs_asof_dev"), _declared_args("hj_pairs_asof_host")
    assert len(dev) == 15 and re.fullmatch(r"hj_ctx\s*\*\s*ctx", dev[0]) and len(host) == 15
    kinds = ["const uint32_t *", "const uint32_t *", "uint64_t", "uint32_t", "uint64_t", "uint64_t", "const hj_asof_term *", "uint64_t *",
             "uint32_t *", "uint32_t *", "uint32_t *", "uint64_t", "uint32_t *", "uint32_t *"]
    for arg, hostarg, kind in zip(dev[1:], host, kinds):
        assert arg.replace(" ", "").startswith(kind.replace(" ", "")) and hostarg.replace(" ", "").startswith(kind.replace(" ", "")), (arg, hostarg)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("hj_pairs_asof_dev", "hj_asof_info", "hj_pairs_asof_host"):
        assert hasattr(raw, name), f"{name} is not exported"
    table = so.contract()
    assert table["hj_pairs_asof_dev"][0] == "asynchronous" and table["hj_asof_info"][0] == "waits"
    assert table["hj_pairs_asof_host"][0] == table["hj_pairs_where_host"][0]


@pytest.mark.parametrize("dtype", wc.DTYPES, ids=str)
@pytest.mark.parametrize("op", ac.ASOF_OPS)
def test_every_op_on_every_type_and_width(dtype, op):
    """the ladder against itself: every S value has every R value as a candidate, NaN and both zeros included"""
    v = wc.ladder(dtype)
    map_s, map_r = cross(v.size, v.size)
    want = check(map_s, map_r, 0, v.size, v.size, wc.term_of(v, op, v.copy()), tag=(str(dtype), op))
    assert 0 < want["info"][0] <= v.size
    nan = np.flatnonzero(v != v)
    assert (want["best_row"][nan] == NO_ROW).all() and not np.isin(want["best_row"], nan).any()       # a NaN wins and is won by nothing
    if op in (">=", "<="):          # every value that is no NaN has itself at least
        assert (want["best_row"][np.flatnonzero(v == v)] != NO_ROW).all()


def test_the_spelled_out_cases():
    one = lambda s, op, r, dt: host_call(*cross(1, len(r)), 0, 1, len(r), wc.term_of(np.array([s], dt), op, np.array(r, dt)))[5][0]    # noqa: E731
    assert one(10, ">=", [3, 10, 11], np.int64) == 1 and one(10, ">", [3, 10, 11], np.int64) == 0
    assert one(10, "<=", [3, 10, 11], np.int64) == 1 and one(10, "<", [3, 10, 11, 12], np.int64) == 2
    assert one(2, ">=", [3, 4], np.uint8) == NO_ROW and one(5, "<", [3, 4, 5], np.uint8) == NO_ROW
    # the order is the type's: signed values below zero, unsigned values above 2^63, a key of 0 as the true maximum
    assert one(0, ">=", [-128, -1, 127], np.int8) == 1 and one(-1, "<=", [-128, 0, 127], np.int8) == 1
    assert one((1 << 64) - 1, ">=", [1, (1 << 63) + 1, (1 << 63) - 1], np.uint64) == 1
    assert one(0, ">=", [0], np.uint64) == 0 and one(0, ">=", [5, 0, 7], np.uint32) == 1 and one((1 << 64) - 1, "<=", [(1 << 64) - 1], np.uint64) == 0
    # floats: negatives below positives, both zeros one value (the tie goes to the lowest row), NaN unordered
    for dt in (np.float32, np.float64):
        assert one(0.5, ">=", [-2.0, -1.0, -np.inf], dt) == 1 and one(-1.5, "<=", [-1.0, 2.0, -2.0], dt) == 0
        assert one(1.0, ">=", [-0.0, 0.0], dt) == 0 and one(1.0, ">=", [0.0, -0.0], dt) == 0 and one(-1.0, "<", [0.0, -0.0, 1.0], dt) == 0
        assert one(0.0, ">=", [-0.0], dt) == 0 and one(-0.0, ">", [0.0], dt) == NO_ROW
        assert one(1.0, ">=", [np.nan, 0.5, np.nan], dt) == 1 and one(np.nan, ">=", [0.5], dt) == NO_ROW and one(1.0, "<", [np.nan], dt) == NO_ROW
        assert one(np.inf, ">=", [np.inf, 1.0], dt) == 0 and one(-np.inf, "<=", [1.0, -np.inf], dt) == 1
    assert one(16777218.0, ">", [16777216.0, 16777218.0], np.float32) == 0


@pytest.mark.parametrize("op", ac.ASOF_OPS)
@pytest.mark.parametrize("dtype", [np.dtype(np.int32), np.dtype(np.float64), np.dtype(np.uint8)], ids=str)
def test_a_null_on_either_side_is_not_eligible(dtype, op):
    v = wc.ladder(dtype)
    n = v.size
    map_s, map_r = cross(n, n)
    s_valid, r_valid = np.arange(n) % 3 != 0, np.arange(n) % 2 != 1
    for sv, rv in ((s_valid, None), (None, r_valid), (s_valid, r_valid)):
        want = check(map_s, map_r, 0, n, n, wc.term_of(v, op, v.copy(), sv, rv), tag=(str(dtype), op))
        best = want["best_row"]
        assert sv is None or (best[~sv] == NO_ROW).all()                 # a NULL S value keeps nothing
        assert rv is None or rv[best[best != NO_ROW]].all()              # a NULL R value is kept by nothing
    assert check(map_s, map_r, 0, n, n, wc.term_of(v, op, v.copy(), None, np.zeros(n, dtype=bool)))["info"][0] == 0


def test_ties_go_to_the_lowest_r_row_wherever_it_stands_in_the_list():
    rng = np.random.default_rng(3)
    n_s, n_r = 40, 64
    r = rng.integers(0, 4, n_r).astype(np.int16)                # four values: every S row meets ties
    s = rng.integers(0, 5, n_s).astype(np.int16)
    map_s, map_r = cross(n_s, n_r)
    for op in ac.ASOF_OPS:
        asc = check(map_s, map_r, 0, n_s, n_r, wc.term_of(s, op, r), tag=("ascending", op))
        desc = check(map_s[::-1].copy(), map_r[::-1].copy(), 0, n_s, n_r, wc.term_of(s, op, r), tag=("the lowest row last", op))
        assert np.array_equal(asc["best_row"], desc["best_row"]) and np.array_equal(asc["kept"], desc["kept"])
        won = asc["best_row"][asc["best_row"] != NO_ROW]
        assert won.size and all((r[:w] != r[w]).all() for w in won)     # no lower row holds the same value
    # all pairs tied on the value: row 0 wins everything, and marks alone of R
    flat = np.full(n_r, 7, dtype=np.int16)
    tied = check(map_s, map_r, 0, n_s, n_r, wc.term_of(np.full(n_s, 7, np.int16), ">=", flat), tag="all tied")
    assert (tied["best_row"] == 0).all() and tied["r_marks"].tolist() == [1, 0]


def test_a_shuffled_list_gives_the_sorted_lists_result():
    rng = np.random.default_rng(4)
    n_s, n_r, n = 300, 200, 5000
    s, r = rng.integers(-20, 20, n_s).astype(np.int64), rng.integers(-20, 20, n_r).astype(np.int64)
    pairs = np.unique(rng.integers(0, n_s * n_r, n))            # each (s, r) once, sorted by S row
    map_s, map_r = (pairs // n_r).astype(U32), (pairs % n_r).astype(U32)
    for op in ac.ASOF_OPS:
        term = wc.term_of(s, op, r, rng.random(n_s) < 0.9, rng.random(n_r) < 0.9)
        a = check(map_s, map_r, 0, n_s, n_r, term, tag=("sorted", op))
        p = rng.permutation(pairs.size)
        b = check(map_s[p], map_r[p], 0, n_s, n_r, term, tag=("shuffled", op))
        assert np.array_equal(a["kept"], b["kept"]) and np.array_equal(a["best_row"], b["best_row"])
        assert np.array_equal(a["s_marks"], b["s_marks"]) and np.array_equal(a["r_marks"], b["r_marks"])
        assert 0 < a["info"][0] < n_s and a["info"][0] == (a["best_row"] != NO_ROW).sum()
        # an R row is marked only when it wins some S row
        assert a["r_marks"].tolist() == plane_words(row_bits(np.unique(a["best_row"][a["best_row"] != NO_ROW]), n_r)).tolist()


def test_dropped_entries_a_row_base_and_a_repeated_pair():
    rng = np.random.default_rng(5)
    n_s, n_r, n, base = 100, 70, 3000, 1000
    s, r = rng.integers(0, 1 << 20, n_s).astype(np.uint32), rng.integers(0, 1 << 20, n_r).astype(np.uint32)
    map_s, map_r = (base + rng.integers(0, n_s, n)).astype(U32), rng.integers(0, n_r, n).astype(U32)
    map_s[::7] = NO_ROW
    map_r[3::11] = NO_ROW
    map_s[5::13] = base + n_s            # the first row behind S
    map_s[6::17] = base - 1              # below the base: wraps to a huge row
    map_r[8::19] = n_r
    want = check(map_s, map_r, base, n_s, n_r, wc.term_of(s, ">=", r), tag="dropped")
    assert want["info"][3] > n // 4 and want["info"][0] > 0
    # random pairs repeat: each copy of a winning pair is kept and counted
    assert want["info"][0] > (want["best_row"] != NO_ROW).sum()
    none = np.zeros(0, dtype=np.uint32)
    for s_rows, r_rows, a, b in ((0, n_r, none, r), (n_s, 0, s, none), (0, 0, none, none)):
        rc, out_s, out_r, _sm, _rm, best_row, info = host_call(map_s, map_r, base, s_rows, r_rows, wc.term_of(a, "<", b))
        assert rc == OK and info == (0, 0, 0, n) and (out_s == SENT).all() and (out_r == SENT).all() and (best_row == NO_ROW).all()


def test_capacity_cuts_the_output_not_the_counts_or_the_marks():
    rng = np.random.default_rng(6)
    n_s, n_r = 500, 400
    s, r = rng.integers(0, 50, n_s).astype(np.int32), rng.integers(0, 50, n_r).astype(np.int32)
    pairs = rng.permutation(np.unique(rng.integers(0, n_s * n_r, 6000)))
    map_s, map_r = (pairs // n_r).astype(U32), (pairs % n_r).astype(U32)
    term = wc.term_of(s, "<=", r)
    full = check(map_s, map_r, 0, n_s, n_r, term)
    kept = full["info"][0]
    assert kept > 300
    cut = check(map_s, map_r, 0, n_s, n_r, term, capacity=kept // 3, tag="cut")
    assert cut["info"][:2] == (kept, kept // 3) and np.array_equal(cut["s_marks"], full["s_marks"]) and np.array_equal(cut["r_marks"], full["r_marks"])
    rc, _s, _r, s_marks, r_marks, best_row, info = host_call(map_s, map_r, 0, n_s, n_r, term, capacity=0)        # NULL outputs: marks only
    assert rc == OK and info == (kept, 0, 0, 0) and np.array_equal(best_row, full["best_row"])
    assert np.array_equal(s_marks, full["s_marks"]) and np.array_equal(r_marks, full["r_marks"])
    rc, out_s, out_r, s_marks, r_marks, _b, info = host_call(map_s, map_r, 0, n_s, n_r, term, marks=False)       # no planes
    assert rc == OK and s_marks is None and np.array_equal(packed(out_s[:kept], out_r[:kept]), full["kept"])
    rc, _s, _r, _sm, _rm, best_row, info = host_call(map_s[:0], map_r[:0], 0, n_s, n_r, term)                    # no pairs: the planes are initialised
    assert rc == OK and info == (0, 0, 0, 0) and (best_row == NO_ROW).all()


def test_the_python_form():
    rng = np.random.default_rng(8)
    n_s, n_r, n = 90, 80, 700
    s, r = rng.integers(-5, 5, n_s).astype(np.float32), rng.integers(-5, 5, n_r).astype(np.float32)
    sv, rv = rng.random(n_s) < 0.9, rng.random(n_r) < 0.9
    map_s, map_r = (10 + rng.integers(0, n_s + 5, n)).astype(U32), rng.integers(0, n_r, n).astype(U32)
    want = ac.model_call(map_s, map_r, 10, n_s, n_r, wc.term_of(s, ">", r, sv, rv))
    got = hj.pairs_asof_host(map_s, map_r, 10, (np.ma.MaskedArray(s, mask=~sv), ">", hj.KeyColumn(r, rv)), marks=True)
    assert got["info"] == want["info"] and np.array_equal(packed(got["s_idx"], got["r_idx"]), want["kept"])
    assert np.array_equal(got["s_marks"], want["s_marks"]) and np.array_equal(got["r_marks"], want["r_marks"])
    assert np.array_equal(got["best_row"], want["best_row"])
    cut = hj.pairs_asof_host(map_s, map_r, 10, (s, ">", r), capacity=3)
    assert cut["info"][1] == 3 and cut["s_idx"].size == 3 and "s_marks" not in cut
    a32, a64 = np.zeros(n_s, np.int32), np.zeros(n_r, np.int64)
    for bad in (None, [], (a32, "==", a32[:n_r]), (a32, "!=", a32[:n_r]), (a32, "<", a64), (a32, "<"), [(a32, "<", a32[:n_r])],
                (a32.astype(np.float16), "<", a32[:n_r].astype(np.float16)), (a32.reshape(2, -1), "<", a32[:n_r]),
                (hj.KeyColumn.from_list([b"a"] * n_s), "<", hj.KeyColumn.from_list([b"a"] * n_r))):
        with pytest.raises(ValueError):
            hj.pairs_asof_host(map_s, map_r, 10, bad)


def test_what_is_refused_writes_nothing():
    """every HJ_ERR_INVALID of the header, on the host form (outputs, planes and info keep their sentinels) and, for a NULL
    context, on the device form"""
    n_s, n_r, n = 40, 30, 64
    s, r = np.arange(n_s, dtype=np.uint64), np.arange(n_r, dtype=np.uint64)
    map_s, map_r = (np.arange(n) % n_s).astype(U32), (np.arange(n) % n_r).astype(U32)
    good = dict(mapS=map_s, mapR=map_r, nPairs=n, sRows=n_s, rRows=n_r, outS=True, outR=True, capacity=n, term=True, bestVal=0, bestRow=0)

    def call(edit=None, **kw):
        a = dict(good, **kw)
        t, _alive = ac.c_term(wc.term_of(s, "<", r, np.ones(n_s, dtype=bool), np.ones(n_r, dtype=bool)))
        if edit:
            edit(t)
        out_s, out_r = np.full(n, SENT, dtype=U32), np.full(n, SENT, dtype=U32)
        s_marks, r_marks = np.full(2, SENT, dtype=U32), np.full(1, SENT, dtype=U32)
        best_val, best_row = np.full(n_s + 1, SENT, dtype=U64), np.full(n_s + 1, SENT, dtype=U32)
        info = (C.c_uint64 * 4)(7, 7, 7, 7)
        at = lambda arr, by: None if by is None else C.c_void_p(arr.ctypes.data + by)      # noqa: E731
        rc = lib.hj_pairs_asof_host(vp(a["mapS"]), vp(a["mapR"]), a["nPairs"], 0, a["sRows"], a["rRows"], C.byref(t) if a["term"] else None,
                                    at(best_val, a["bestVal"]), at(best_row, a["bestRow"]), vp(out_s) if a["outS"] else None,
                                    vp(out_r) if a["outR"] else None, a["capacity"], vp(s_marks), vp(r_marks), info)
        untouched = all((x == SENT).all() for x in (out_s, out_r, s_marks, r_marks, best_val, best_row)) and tuple(info) == (7, 7, 7, 7)
        return rc, untouched

    assert call()[0] == OK and not call()[1]

    def field(name, value):
        return lambda t: setattr(t, name, value)

    def shifted(name, by):
        return lambda t: setattr(t, name, getattr(t, name) + by)

    refused = {
        "term NULL": dict(term=False), "type": dict(edit=field("type", 3)), "op 6": dict(edit=field("op", 6)),
        "op ==": dict(edit=field("op", _lib.HJ_CMP_EQ)), "op !=": dict(edit=field("op", _lib.HJ_CMP_NE)),
        "width 3": dict(edit=field("width", 3)), "width 16": dict(edit=field("width", 16)), "width 0": dict(edit=field("width", 0)),
        "float of 2 bytes": dict(edit=lambda t: (setattr(t, "type", _lib.HJ_VAL_FLOAT), setattr(t, "width", 2))),
        "reserved": dict(edit=field("reserved", 1)),
        "s NULL": dict(edit=field("s", None)), "r NULL": dict(edit=field("r", None)),
        "s misaligned": dict(edit=shifted("s", 4)), "r misaligned": dict(edit=shifted("r", 2)),
        "sValid misaligned": dict(edit=shifted("sValid", 2)), "rValid misaligned": dict(edit=shifted("rValid", 1)),
        "bestVal NULL": dict(bestVal=None), "bestRow NULL": dict(bestRow=None), "bestVal misaligned": dict(bestVal=4), "bestRow misaligned": dict(bestRow=2),
        "mapS NULL": dict(mapS=None), "mapR NULL": dict(mapR=None), "outS NULL": dict(outS=False), "outR NULL": dict(outR=False),
        "nPairs 2^32": dict(nPairs=1 << 32), "sRows 2^32": dict(sRows=1 << 32), "rRows 2^32": dict(rRows=1 << 32),
    }
    for name, kw in refused.items():
        rc, untouched = call(**kw)
        assert rc == INVALID and untouched, name
    for op in (_lib.HJ_CMP_GE, _lib.HJ_CMP_GT, _lib.HJ_CMP_LE, _lib.HJ_CMP_LT):
        assert call(edit=field("op", op))[0] == OK
    assert call(edit=field("s", None), sRows=0)[0] == OK and call(edit=field("r", None), rRows=0)[0] == OK
    assert call(mapS=None, mapR=None, nPairs=0)[0] == OK and call(outS=False, outR=False, capacity=0)[0] == OK
    t, _alive = ac.c_term(wc.term_of(s, "<", r))
    assert lib.hj_pairs_asof_dev(None, vp(map_s), vp(map_r), n, 0, n_s, n_r, C.byref(t), vp(s), vp(map_s), None, None, 0, None, None) == INVALID
    assert lib.hj_asof_info(None, (C.c_uint64 * 4)()) == INVALID


def test_asof_is_checked_before_any_device_work():
    """the wrappers' ValueErrors need no device"""
    R, S = np.arange(1, 9, dtype=np.uint64), np.arange(1, 6, dtype=np.uint64)
    a_r, a_s = np.zeros(8, np.int32), np.zeros(5, np.int32)
    for join in (lambda **kw: hj.join_tables(R, S, **kw), lambda **kw: hj.join_on(R, S, **kw), lambda **kw: hj.join_on_columns(R, S, **kw)):
        for bad in ((a_s, "==", a_r), (a_s, "!=", a_r), (a_s, "~", a_r), (a_s, 5, a_r), (a_s, "<", a_r.astype(np.int64)), (a_s[:-1], "<", a_r),
                    (a_s, "<", a_r[:-1]), (a_s, "<"), [(a_s, "<", a_r)], (hj.KeyColumn.from_list([b"x"] * 5), "<", hj.KeyColumn.from_list([b"x"] * 8)),
                    (a_s.astype(np.float16), "<", a_r.astype(np.float16)), (a_s.astype(bool), "<", a_r.astype(bool))):
            with pytest.raises(ValueError):
                join(asof=bad)
            with pytest.raises(ValueError):
                join(where=[(a_s, "<", a_r)], asof=bad)
        with pytest.raises(ValueError):
            join(where=[(a_s, "~", a_r)], asof=(a_s, "<", a_r))
    # one side empty: the result needs no device, with an as-of term as without
    none = np.zeros(0, dtype=np.uint64)
    for how in wc.HOWS:
        got = hj.join_tables(R, none, how=how, asof=(np.zeros(0, np.int32), ">=", a_r))
        want = hj.join_tables(R, none, how=how)
        assert got.keys() == want.keys() and all(np.array_equal(got[k], want[k]) for k in ("s_idx", "r_idx")), how
