"""hj_range_index_* / hj_range_pairs_* without a GPU: the symbols, structs and constants against the header, the invariants of
hj_range_layout_info, every refusal, the host twins bit for bit against the numpy model of range_common (directed cases and a
seeded fuzz over every type and width, both open flags and the three picks), and range_join_host / interval_join over the
host path against the brute-force join for all eight kinds."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

import range_common as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "htm_hashjoin.h")).read()
NAMES = ("hj_range_index_dev", "hj_range_index_info", "hj_range_index_host", "hj_range_layout_info", "hj_range_pairs_dev",
         "hj_range_pairs_info", "hj_range_pairs_host")
HOWS = ("inner", "left", "semi", "anti", "right", "full", "right_semi", "right_anti")


def test_symbols_are_declared_exported_and_bound():
    raw = C.CDLL(_lib.LIB_PATH)
    code = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert hasattr(raw, name) and name in hj.lib._hj_signatures, name
    assert hj.lib.hj_abi_version() == 4


def test_structs_and_constants_match_the_header():
    assert C.sizeof(_lib.hj_range_term) == 48 and "} hj_range_term;                        /* 48 bytes */" in HEADER
    assert [f for f, _ in _lib.hj_range_term._fields_] == ["lo", "hi", "loValid", "hiValid", "width", "type", "flags", "pick"]
    for name in ("HJ_RANGE_LO_OPEN", "HJ_RANGE_HI_OPEN"):
        assert int(re.search(r"#define %s\s+(0x[0-9a-f]+)u" % name, HEADER).group(1), 16) == getattr(_lib, name)
    enum = re.search(r"typedef enum \{([^}]*)\} hj_range_pick;", HEADER).group(1)
    assert {k.strip(): int(v) for k, v in (e.split("=") for e in enum.split(","))} == {
        "HJ_RANGE_ALL": _lib.HJ_RANGE_ALL, "HJ_RANGE_FIRST": _lib.HJ_RANGE_FIRST, "HJ_RANGE_LAST": _lib.HJ_RANGE_LAST}
    assert _lib.RANGE_PICKS == {"all": 0, "first": 1, "last": 2}


def test_layout_invariants():
    sizes = [0, 1, 2, 15, 16, 17, 4095, 4096, 4097, 65535, 65536, 65537, 1 << 20, (1 << 20) + 1, 3_000_001, 1 << 27, (1 << 27) + 5, 1 << 31,
             (1 << 32) - 2]
    last = 0
    for n in sizes:
        l = hj.range_layout_info(n, n)
        assert l["stride"] >= 16 and l["stride"] & (l["stride"] - 1) == 0
        assert l["pivots"] == -(-n // l["stride"]) and 8 * l["pivots"] <= l["lds_bytes"] <= 64 * 1024
        assert l["stride"] == 16 or -(-n // (l["stride"] // 2)) * 8 > l["lds_bytes"]       # the smallest stride that fits
        assert l["chunks"] == -(-n // l["chunk_rows"]) and l["chunk_rows"] % 64 == 0 and l["tile"] % 256 == 0
        assert l["workspace_bytes"] >= last
        last = l["workspace_bytes"]
        assert hj.range_layout_info(n, 0)["workspace_bytes"] <= l["workspace_bytes"] and hj.range_layout_info(0, n)["workspace_bytes"] <= l["workspace_bytes"]
        assert l["workspace_bytes"] >= 8 * n + 4 * (n + 1)                                  # two bound planes and the difference plane
    out = (C.c_uint64 * 8)()
    assert hj.lib.hj_range_layout_info(1 << 32, 0, out) == _lib.HJ_ERR_INVALID and hj.lib.hj_range_layout_info(0, (1 << 32) - 1, out) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_range_layout_info(1, 1, None) == _lib.HJ_ERR_INVALID


def test_the_order_key_of_the_model_agrees_with_numpy():
    rng = np.random.default_rng(5)
    for dtype in rc.DTYPES:
        a = np.concatenate([rc.extremes(dtype), rc.fuzz_case(1, dtype, 400, 4, nulls=False)[0]])
        key, ordered = rc.order_key(a)
        a, key = a[ordered], key[ordered]
        by_key = a[np.argsort(key, kind="stable")]
        assert np.array_equal(by_key, np.sort(a)), dtype           # -0.0 == 0.0 under array_equal, as under the sort
        i, j = rng.integers(0, a.size, 500), rng.integers(0, a.size, 500)
        assert np.array_equal(key[i] < key[j], a[i] < a[j]) and np.array_equal(key[i] == key[j], a[i] == a[j]), dtype


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_the_index_writes_nothing():
    r = np.arange(40, dtype=np.int32)
    perm, keys, head = np.full(40, 7, dtype=np.uint32), np.full(44, 7, dtype=np.uint32), np.full(4, 7, dtype=np.uint32)

    def call(values=r.ctypes.data, width=4, type_=1, flags=0, n=40, p=perm.ctypes.data, k=keys.ctypes.data, h=head.ctypes.data, valid=0, reserved=0, col=True):
        arr = (_lib.hj_sort_col * 1)()
        arr[0].values, arr[0].valid, arr[0].width, arr[0].type, arr[0].flags, arr[0].reserved = values or None, valid or None, width, type_, flags, reserved
        return hj.lib.hj_range_index_host(arr if col else None, n, p or None, k or None, h or None)

    bad = [dict(col=False), dict(n=(1 << 32) - 1), dict(flags=_lib.HJ_SORT_DESC), dict(flags=_lib.HJ_SORT_NULLS_FIRST), dict(flags=4), dict(type_=3),
           dict(width=3), dict(width=16), dict(type_=2, width=2), dict(reserved=1), dict(values=0), dict(values=r.ctypes.data + 2), dict(valid=r.ctypes.data + 2),
           dict(p=0), dict(p=perm.ctypes.data + 2), dict(k=0), dict(k=keys.ctypes.data + 2), dict(width=8, k=keys.ctypes.data + 4), dict(h=0),
           dict(h=head.ctypes.data + 1)]
    for kw in bad:
        assert call(**kw) == _lib.HJ_ERR_INVALID, kw
    assert (perm == 7).all() and (keys == 7).all() and (head == 7).all()
    assert call() == _lib.HJ_OK and tuple(head) == (40, 0, 0, 4) and np.array_equal(perm, np.arange(40))
    assert call(n=0, values=0, p=0, k=0) == _lib.HJ_OK and tuple(head) == (0, 0, 0, 4)


def test_every_refusal_of_the_range_step_writes_nothing():
    r = np.arange(64, dtype=np.int64)
    idx = hj.range_pairs_host(r, s_lo=np.zeros(0, dtype=np.int64))
    keys, perm, head = idx["keys"], idx["perm"], idx["head"]
    lo, hi = np.zeros(8, dtype=np.int64), np.full(8, 70, dtype=np.int64)
    out_s, out_r = np.full(600, 7, dtype=np.uint32), np.full(600, 7, dtype=np.uint32)
    sm, rm, info = np.full(4, 7, dtype=np.uint32), np.full(4, 7, dtype=np.uint32), (C.c_uint64 * 8)(*[7] * 8)
    head4 = head.copy()
    head4[3] = 4

    def call(term=True, lo_p=lo.ctypes.data, hi_p=hi.ctypes.data, width=8, type_=1, flags=0, pick=0, lv=0, hv=0, k=keys.ctypes.data, p=perm.ctypes.data,
             h=head.ctypes.data, n_r=64, n_s=8, os_=out_s.ctypes.data, or_=out_r.ctypes.data, cap=600, sm_=sm.ctypes.data, rm_=rm.ctypes.data):
        t = _lib.hj_range_term()
        t.lo, t.hi, t.loValid, t.hiValid, t.width, t.type, t.flags, t.pick = lo_p or None, hi_p or None, lv or None, hv or None, width, type_, flags, pick
        return hj.lib.hj_range_pairs_host(k or None, p or None, h or None, n_r, C.byref(t) if term else None, n_s, 0, os_ or None, or_ or None, cap,
                                          sm_ or None, rm_ or None, info)

    bad = [dict(term=False), dict(lo_p=0, hi_p=0), dict(type_=3), dict(width=3), dict(width=16), dict(type_=2, width=2), dict(width=4), dict(h=head4.ctypes.data),
           dict(flags=4), dict(flags=0x80000000), dict(pick=3), dict(lo_p=lo.ctypes.data + 4), dict(hi_p=hi.ctypes.data + 2), dict(lv=lo.ctypes.data + 2),
           dict(hv=lo.ctypes.data + 1), dict(k=0), dict(k=keys.ctypes.data + 4), dict(p=0), dict(p=perm.ctypes.data + 2), dict(h=0), dict(h=head.ctypes.data + 2),
           dict(n_s=(1 << 32) - 1), dict(n_r=(1 << 32) - 1), dict(cap=1 << 32), dict(os_=0), dict(or_=0), dict(os_=out_s.ctypes.data + 2),
           dict(sm_=sm.ctypes.data + 1), dict(rm_=rm.ctypes.data + 3)]
    for kw in bad:
        assert call(**kw) == _lib.HJ_ERR_INVALID, kw
    assert (out_s == 7).all() and (out_r == 7).all() and (sm == 7).all() and (rm == 7).all() and list(info) == [7] * 8
    sm[:], rm[:] = 0, 0
    assert call() == _lib.HJ_OK and tuple(info)[:6] == (512, 512, 0, 8, 0, 64) and (out_s[512:] == 7).all()
    assert call(os_=0, or_=0, cap=0) == _lib.HJ_OK and call(lo_p=0) == _lib.HJ_OK and call(hi_p=0) == _lib.HJ_OK


# ---- the host twins against the model ------------------------------------------------------------------------------------------
def check_host(r, lo, hi, r_valid=None, lo_valid=None, hi_valid=None, lo_open=False, hi_open=False, pick="all", base=0, capacity=None, tag=None):
    want = rc.model_call(r, lo, hi, r_valid, lo_valid, hi_valid, lo_open, hi_open, pick, base, capacity)
    col = lambda a, v: None if a is None else hj.KeyColumn(a, v)      # noqa: E731
    got = hj.range_pairs_host(col(r, r_valid), col(lo, lo_valid), col(hi, hi_valid), lo_open, hi_open, pick, capacity, base)
    assert got["info"] == want["info"], (tag, got["info"], want["info"])
    assert np.array_equal(got["perm"], want["index"]["perm"]) and tuple(got["head"][:3]) == want["index"]["head"], (tag, "index")
    n = want["index"]["head"][0]
    assert np.array_equal(np.unique(got["keys"][:n], return_inverse=True)[1], np.unique(want["index"]["keys"], return_inverse=True)[1]), (tag, "keys")
    assert (np.diff(got["keys"][:n].astype(np.float64)) >= 0).all(), (tag, "the key plane ascends")
    assert np.array_equal(got["s_marks"], want["s_marks"]) and np.array_equal(got["r_marks"], want["r_marks"]), (tag, "marks")
    mine = rc.packed(got["s_idx"], got["r_idx"])
    if capacity is None or capacity >= want["info"][0]:
        assert np.array_equal(mine, want["kept"]), (tag, "pairs")
    else:
        assert mine.size == capacity and np.isin(mine, want["kept"]).all() and np.unique(mine).size == mine.size, (tag, "cut")
    return got, want


@pytest.mark.parametrize("dtype", rc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_host_twins_equal_the_model_on_directed_cases(dtype):
    r, lo, hi = rc.directed(dtype)
    for lo_open in (False, True):
        for hi_open in (False, True):
            for pick in rc.PICKS:
                check_host(r, lo, hi, lo_open=lo_open, hi_open=hi_open, pick=pick, tag=(lo_open, hi_open, pick))
    check_host(r, lo, None, lo_open=True, tag="hi unbounded")
    check_host(r, None, hi, pick="last", base=1000, tag="lo unbounded: the keyless as-of")
    if np.dtype(dtype).kind == "f":
        rn = np.concatenate([r, np.array([np.nan, -np.nan], dtype=dtype)])
        ln = lo.copy()
        ln[::7] = np.nan
        got, want = check_host(rn, ln, hi, tag="NaN in R and as a bound")
        assert want["info"][4] == np.isnan(ln).sum() and want["index"]["head"][2] == 2
        z = np.array([-0.0, 0.0], dtype=dtype)
        got, _ = check_host(z, z, z, tag="-0.0 against 0.0")
        assert got["info"][0] == 4
        got, _ = check_host(z, z, z, lo_open=True, tag="-0.0 < 0.0 is false")
        assert got["info"][0] == 0
    for cap in (0, 1, 5):
        check_host(r, lo, hi, capacity=cap, tag=("capacity", cap))


def test_open_bounds_at_the_ends_of_the_type():
    for dtype, lo_v, hi_v in ((np.int64, np.iinfo(np.int64).min, np.iinfo(np.int64).max), (np.uint64, 0, np.iinfo(np.uint64).max)):
        r = np.array([lo_v, lo_v, hi_v, 5, hi_v], dtype=dtype)
        full = lambda v: np.array([v], dtype=dtype)        # noqa: E731
        assert check_host(r, None, full(hi_v), hi_open=True)[0]["info"][0] == 3        # x < MAX
        assert check_host(r, None, full(hi_v))[0]["info"][0] == 5
        assert check_host(r, full(lo_v), None, lo_open=True)[0]["info"][0] == 3        # x > MIN
        assert check_host(r, full(lo_v), None)[0]["info"][0] == 5
    r = np.array([-np.inf, 1.0, np.inf, np.nan], dtype=np.float64)
    inf = np.array([np.inf]), np.array([-np.inf])
    assert check_host(r, inf[1], inf[0])[0]["info"][0] == 3 and check_host(r, inf[1], inf[0], lo_open=True, hi_open=True)[0]["info"][0] == 1


@pytest.mark.parametrize("dtype", rc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_host_twins_equal_the_model_on_a_seeded_fuzz(dtype):
    for seed, (lo_open, hi_open), pick in zip(range(12), [(a, b) for a in (False, True) for b in (False, True)] * 3, rc.PICKS * 4):
        r, rv, lo, hi, lv, hv = rc.fuzz_case(100 + seed, dtype, 700, 500)
        check_host(r, lo, hi, rv, lv, hv, lo_open, hi_open, pick, base=seed * 11, tag=(seed, lo_open, hi_open, pick))
    r, rv, lo, hi, lv, hv = rc.fuzz_case(7, dtype, 300, 200)
    check_host(r, lo, None, rv, lv, None, pick="first", tag="one bound")
    check_host(r, None, hi, rv, None, hv, hi_open=True, pick="last", tag="as-of")


def test_nulls_and_nans_of_r_are_never_paired_or_marked():
    r = np.array([1.0, np.nan, 2.0, 3.0, np.nan, 4.0], dtype=np.float32)
    valid = np.array([True, True, False, True, False, True])
    got, want = check_host(r, np.array([-np.inf], dtype=np.float32), np.array([np.inf], dtype=np.float32), r_valid=valid)
    assert got["info"][0] == 3 and tuple(got["head"]) == (3, 2, 1, 4) and set(got["r_idx"]) == {0, 3, 5}
    assert rc.plane_words([True, False, False, True, False, True])[0] == got["r_marks"][0]


# ---- range_join_host / interval_join against the brute-force join ----------------------------------------------------------------
def _tables(seed, dtype, n_r=200, n_s=300):
    rng = np.random.default_rng(seed)
    r, rv, lo, hi, lv, hv = rc.fuzz_case(seed, dtype, n_r, n_s)
    r_cols = {"a": rng.integers(0, 1 << 40, n_r).astype(np.uint64), "n": hj.KeyColumn(rng.integers(0, 99, n_r).astype(np.int32), rng.random(n_r) > 0.2)}
    s_cols = {"b": rng.integers(0, 1 << 15, n_s).astype(np.uint16)}
    wr, ws = rng.integers(0, 9, n_r).astype(np.int16), rng.integers(0, 9, n_s).astype(np.int16)
    return hj.KeyColumn(r, rv), hj.KeyColumn(lo, lv), hj.KeyColumn(hi, hv), r_cols, s_cols, [(ws, "<=", wr)]


@pytest.mark.parametrize("how", HOWS)
def test_range_join_host_equals_the_brute_force_join(how):
    for seed, dtype in ((1, np.int32), (2, np.float64), (3, np.uint8)):
        r, lo, hi, r_cols, s_cols, where = _tables(seed, dtype)
        for w in (None, where):
            for pick, lo_open in (("all", False), ("last", True)):
                res = hj.range_join_host(r, lo, hi, lo_open=lo_open, pick=pick, r_cols=r_cols, s_cols=s_cols, how=how, where=w)
                rc.assert_join(res, rc.brute_matches(r, lo, hi, lo_open, False, pick, w), how, r_cols, s_cols, (seed, w is not None, pick))
        res = hj.range_join_host(r, None, hi, hi_open=True, pick="last", how=how)
        rc.assert_join(res, rc.brute_matches(r, None, hi, False, True, "last"), how, tag="as-of")


@pytest.mark.parametrize("how", HOWS)
def test_interval_join_over_the_host_path_equals_the_brute_force_join(how):
    for seed, dtype in ((4, np.int64), (5, np.float32)):
        pts, lo, hi, p_cols, i_cols, where = _tables(seed, dtype)          # the points are S's, the intervals R's
        for w in (None, [(where[0][2], ">=", where[0][0])]):
            res = hj.interval_join(lo, hi, pts, hi_open=True, r_cols=i_cols, s_cols=p_cols, how=how, where=w, host=True)
            m = rc.brute_matches(pts, lo, hi, False, True, "all", None if w is None else where)      # m[interval, point]
            rc.assert_join(res, m.T, how, i_cols, p_cols, (seed, w is not None))


def test_wrapper_argument_checks():
    r, lo = np.arange(5, dtype=np.int32), np.arange(3, dtype=np.int32)
    for fn in (hj.range_join, hj.range_join_host):
        with pytest.raises(ValueError, match="a range has a bound"):
            fn(r)
        with pytest.raises(ValueError, match="pick"):
            fn(r, lo, pick="nearest")
        with pytest.raises(ValueError, match="no implicit cast"):
            fn(r, lo.astype(np.int64))
        with pytest.raises(ValueError, match="no implicit cast"):
            fn(r, lo, lo.astype(np.uint32))
        with pytest.raises(ValueError, match="must have 3 elements"):
            fn(r, lo, np.arange(4, dtype=np.int32))
        with pytest.raises(ValueError, match="how must be"):
            fn(r, lo, how="cross")
        with pytest.raises(ValueError, match="float16"):
            fn(r.astype(np.float16), lo.astype(np.float16))
        with pytest.raises(ValueError, match="variable-length"):
            fn(hj.KeyColumn.from_list(["a"]), lo)
        with pytest.raises(ValueError, match="R column 'x' must be 1-D with 5 elements"):
            fn(r, lo, r_cols={"x": np.arange(4)})
        with pytest.raises(ValueError, match="must have 5 elements"):
            fn(r, lo, where=[(lo, "<", lo)])
    with pytest.raises(ValueError, match="slice_tuples must be positive"):
        hj.range_join(r, lo, slice_rows=-1)
    with pytest.raises(ValueError, match="how must be"):
        hj.interval_join(lo, lo, r, how="outer")
    with pytest.raises(ValueError, match="a where term is"):
        hj.interval_join(lo, lo, r, where=[(lo, "~", r)], host=True)


@pytest.mark.parametrize("how", HOWS)
def test_an_empty_side_is_answered_without_a_device(how):
    r, none = np.arange(4, dtype=np.float32), np.zeros(0, dtype=np.float32)
    cols = {"p": np.arange(4, dtype=np.uint8)}
    for fn in (hj.range_join, hj.range_join_host):            # no context is created: this passes on a machine without a GPU
        res = fn(none, r, r, s_cols=cols, how=how)
        rc.assert_join(res, np.zeros((4, 0), dtype=bool), how, None, cols)
        res = fn(r, none, none, r_cols=cols, how=how)
        rc.assert_join(res, np.zeros((0, 4), dtype=bool), how, cols, None)
    res = hj.interval_join(none, none, r, s_cols=cols, how=how)
    rc.assert_join(res, np.zeros((4, 0), dtype=bool), how, None, cols)
