"""Rows grouped by key columns at the ABI boundary: hj_key_groups_dev, hj_key_groups_info and hj_key_groups_host are declared,
exported and bound, nothing of the ABI around them moved; hj_key_groups_host equals the model of groups_common (a dict on the
key's bytes) in rep, group, firstRows, the counts and the cut at the capacity, whatever the keyMask; it refuses what the
header says it refuses and then writes nothing; the Python wrappers validate their arguments and answer empty tables
without a device. No GPU needed."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

import groups_common as gc
import keys2_common as k2
from keys_common import _declared_args, _header
from keys2_common import _bad_columns, _col2

COL2 = "const hj_key_col2 *"
DEV_ARGS = [COL2, "uint32_t", "uint32_t", "uint64_t", "uint32_t", "uint32_t *", "uint32_t *", "uint32_t *", "uint64_t"]
HOST_ARGS = DEV_ARGS + ["uint64_t"]


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    dev, info, host = _declared_args("hj_key_groups_dev"), _declared_args("hj_key_groups_info"), _declared_args("hj_key_groups_host")
    assert re.fullmatch(r"hj_ctx\s*\*\s*ctx", dev[0]) and len(dev) == 1 + len(DEV_ARGS)
    assert re.fullmatch(r"hj_ctx\s*\*\s*ctx", info[0]) and info[1].replace(" ", "") == "uint64_tout[8]" and len(info) == 2
    assert len(host) == len(HOST_ARGS) and host[-1].replace(" ", "") == "uint64_tout[8]"
    for args, kinds in ((dev[1:], DEV_ARGS), (host, HOST_ARGS)):
        for arg, kind in zip(args, kinds):
            assert arg.replace(" ", "").startswith(kind.replace(" ", "")), arg
    for symbol in ("hj_key_groups_dev", "hj_key_groups_info", "hj_key_groups_host"):
        assert hasattr(raw, symbol), f"{symbol} is not exported"
    sig = hj.lib._hj_signatures
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    cols = ctypes.POINTER(_lib.hj_key_col2)
    assert sig["hj_key_groups_dev"] == ([vp, cols, u32, u32, u64, u32, vp, vp, vp, u64], ctypes.c_int)
    assert sig["hj_key_groups_info"] == ([vp, ctypes.POINTER(u64)], ctypes.c_int)
    assert sig["hj_key_groups_host"] == ([cols, u32, u32, u64, u32, vp, vp, vp, u64, ctypes.POINTER(u64)], ctypes.c_int)


def test_abi_version_and_the_structs_around_are_unchanged():
    assert hj.lib.hj_abi_version() == 4
    assert re.search(r"#define\s+HJ_ABI_VERSION\s+4\b", _header())
    assert ctypes.sizeof(_lib.hj_key_col) == 24 and ctypes.sizeof(_lib.hj_key_col2) == 56
    assert ctypes.sizeof(_lib.hj_params) == 48 and ctypes.sizeof(_lib.hj_result) == 232
    assert ctypes.sizeof(_lib.hj_gather_col) == 40
    assert _lib.HJ_NO_ROW == gc.NO_ROW


# ---- the host twin against the model ---------------------------------------------------------------------------------------
def check_host(cols, nulls, tag):
    """key_groups_host over the KeyColumns of the model columns `cols`: the model's answer under every mask, the cut at a
    capacity below the group count, and the counts"""
    want = gc.model_groups(gc.model_keys(cols, nulls))
    keys = gc.key_columns(cols)
    for key_mask in gc.MASKS:
        gc.same(hj.key_groups_host(keys, nulls=nulls, key_mask=key_mask), want, (tag, nulls, key_mask))
    for capacity in (0, 1, want["n_groups"] // 2, want["n_groups"], want["n_groups"] + 5):
        cut = gc.model_groups(gc.model_keys(cols, nulls), capacity)
        gc.same(hj.key_groups_host(keys, nulls=nulls, key_mask=0xF, capacity=capacity), cut, (tag, nulls, "capacity", capacity))
    return want


@pytest.mark.parametrize("width", [1, 2, 4, 8, 16])
def test_host_groups_one_fixed_column(width):
    rng = np.random.default_rng(width)
    for n, distinct in ((1, 1), (65, 7), (700, 90)):
        want = check_host(gc.fixed_table(rng, [width], n, distinct), "group", (width, n))
        assert want["null_rows"] == 0 and 1 <= want["n_groups"] <= min(n, distinct, 256 ** width)


@pytest.mark.parametrize("widths", [(8, 2), (1, 16, 4), (4, 8, 2, 1), (16, 16)])
def test_host_groups_mixed_columns(widths):
    rng = np.random.default_rng(sum(widths))
    want = check_host(gc.fixed_table(rng, list(widths), 600, 60), "group", widths)
    assert 10 < want["n_groups"] < 600


@pytest.mark.parametrize("nulls", ["group", "drop"])
def test_host_groups_strings_and_nulls(nulls):
    """strings of 0 to 40 bytes at unaligned offsets; 10 % NULLs with the flag set (group) and clear (drop); a string next
    to fixed columns"""
    rng = np.random.default_rng(40)
    strings = gc.string_col(rng, 900, 70)
    assert len({len(e) for e in strings.items}) > 20 and max(len(e) for e in strings.items) <= 40
    check_host([strings], nulls, "strings")
    nullable = gc.string_col(rng, 900, 70, nulls=0.1)
    want = check_host([nullable], nulls, "nullable strings")
    assert (want["null_rows"] > 50) == (nulls == "drop")
    for widths in ([4], [8, 1]):
        want = check_host(gc.fixed_table(rng, widths, 800, 50, nulls=0.1), nulls, ("nullable", widths))
        assert (want["null_rows"] > 40) == (nulls == "drop")
    mixed = [gc.string_col(rng, 500, 12, nulls=0.1), k2.fixed_col(rng, 2, 500, nulls=0.1, distinct=5), k2.fixed_col(rng, 16, 500, distinct=3)]
    check_host(mixed, nulls, "mixed")


def test_host_groups_a_flag_per_column():
    """the flag is the column's: NULLs group in the column that has it and drop the row in the one that has not"""
    rng = np.random.default_rng(6)
    cols = [k2.fixed_col(rng, 4, 400, nulls=0.2, nulls_equal=True, distinct=6), gc.string_col(rng, 400, 8, nulls=0.2)]
    want = gc.model_groups(k2.row_keys(cols))
    assert 40 < want["null_rows"] < 200
    keys = [k2.key_column(c, lead=3) for c in cols]
    for key_mask in gc.MASKS:
        gc.same(hj.key_groups_host(keys, nulls="drop", key_mask=key_mask), want, key_mask)


def test_host_groups_what_is_equal():
    """a prefix is another key, an empty string is no NULL, a NULL equals a NULL under "group" alone, and the bytes under a
    NULL are not compared"""
    items = [b"ab", b"abc", b"", None, b"ab", None, b"", b"ab\0"]
    got = hj.key_groups_host(hj.KeyColumn.from_list(items))
    assert got["rep"].tolist() == [0, 1, 2, 3, 0, 3, 2, 7] and got["group"].tolist() == [0, 1, 2, 3, 0, 3, 2, 4]
    got = hj.key_groups_host(hj.KeyColumn.from_list(items), nulls="drop")
    assert got["rep"].tolist() == [0, 1, 2, gc.NO_ROW, 0, gc.NO_ROW, 2, 7] and got["null_rows"] == 2 and got["first_rows"].tolist() == [0, 1, 2, 7]
    a = hj.KeyColumn(np.array([7, 1, 2, 7], dtype=np.uint32), valid=np.array([True, False, False, True]))
    assert hj.key_groups_host(a)["rep"].tolist() == [0, 1, 1, 0]


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_host_refusals_write_nothing():
    n = 32
    held, good_fixed, good_var, bad = _bad_columns(n)
    rep, group, first = (np.full(n, 0xABCD, dtype=np.uint32) for _ in range(3))
    out = (ctypes.c_uint64 * 8)(*[77] * 8)
    ptrs = dict(rep=rep.ctypes.data, group=group.ctypes.data, first=first.ctypes.data)

    def call(col, n_cols=1, side=0, n_rows=n, cols_null=False, capacity=n, out_null=False, **kw):
        p = dict(ptrs, **kw)
        cols = _col2(n_cols, side == 0, side == 1, **col)
        return hj.lib.hj_key_groups_host(None if cols_null else cols, n_cols, side, n_rows, 0, p["rep"] or None, p["group"] or None,
                                         p["first"] or None, capacity, None if out_null else out)

    def untouched():
        return all((a == 0xABCD).all() for a in (rep, group, first)) and list(out) == [77] * 8

    for col in bad:
        assert call(col) == _lib.HJ_ERR_INVALID and call(col, side=1) == _lib.HJ_ERR_INVALID, col
    for kw in (dict(n_cols=0), dict(n_cols=5), dict(cols_null=True), dict(side=2), dict(n_rows=(1 << 32) - 1), dict(n_rows=1 << 32),
               dict(rep=0), dict(first=0), dict(out_null=True), dict(rep=ptrs["rep"] + 2), dict(group=ptrs["group"] + 1),
               dict(first=ptrs["first"] + 2)):
        assert call(good_fixed, **kw) == _lib.HJ_ERR_INVALID, kw
        assert call(good_var, **kw) == _lib.HJ_ERR_INVALID, kw
    assert untouched(), "a refused call wrote something"
    # what is allowed: no group plane; no first rows with capacity 0; no rows at all, with no pointers
    for good in (good_fixed, good_var):
        rep[:], group[:], first[:] = 0xABCD, 0xABCD, 0xABCD
        assert call(good, group=0) == _lib.HJ_OK and (group == 0xABCD).all() and first[0] == 0 and rep[0] == 0
        first[:] = 0xABCD
        assert call(good, first=0, capacity=0) == _lib.HJ_OK and (first == 0xABCD).all() and out[1] == 0 and out[0] >= 1
        assert call(good, side=1) == _lib.HJ_OK
    none = dict(ptr=0, off=0, valid=0, flags=0)
    assert call(dict(none, width=8), n_rows=0, rep=0, group=0, first=0) == _lib.HJ_OK and list(out) == [0] * 8
    assert call(dict(none, width=3), n_rows=0, rep=0, group=0, first=0) == _lib.HJ_ERR_INVALID


def test_device_entry_points_refuse_a_null_context():
    n = 16
    _, good_fixed, _, _ = _bad_columns(n)
    rep = np.zeros(n, dtype=np.uint32)
    out = (ctypes.c_uint64 * 8)()
    cols = _col2(1, True, True, **good_fixed)
    assert hj.lib.hj_key_groups_dev(None, None, 0, 0, 0, 0, None, None, None, 0) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_key_groups_dev(None, cols, 1, 0, n, 0, rep.ctypes.data, None, None, 0) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_key_groups_info(None, out) == _lib.HJ_ERR_INVALID and hj.lib.hj_key_groups_info(None, None) == _lib.HJ_ERR_INVALID


# ---- the Python wrappers -------------------------------------------------------------------------------------------------------
K8 = np.array([5, 3, 5, 7, 3, 3, 9], dtype=np.uint64)


def test_python_surface():
    C = hj.HashJoinContext
    assert list(inspect.signature(C.key_groups).parameters) == ["self", "cols", "side", "n_rows", "d_rep", "d_group", "d_first_rows",
                                                                 "capacity", "key_mask"]
    assert list(inspect.signature(C.key_groups_info).parameters) == ["self"]
    params = inspect.signature(hj.key_groups).parameters
    assert list(params) == ["keys", "nulls", "key_mask", "device"] and [p.default for p in list(params.values())[1:]] == ["group", 0, 0]
    assert list(inspect.signature(hj.key_groups_host).parameters)[:3] == ["keys", "nulls", "key_mask"]
    assert list(inspect.signature(hj.distinct_on).parameters)[:2] == ["keys", "cols"]
    assert list(inspect.signature(hj.group_by_columns).parameters)[:4] == ["keys", "cols", "aggs", "nulls"]
    for f in (C.key_groups, C.key_groups_info, hj.key_groups, hj.key_groups_host, hj.distinct_on, hj.group_by_columns):
        assert f.__doc__


def test_wrappers_validate_before_any_device_call():
    s = hj.KeyColumn.from_list([b"k%d" % (i % 3) for i in range(7)])
    vals = {"v": np.arange(7, dtype=np.int64)}
    for fn, more in ((hj.key_groups, ()), (hj.key_groups_host, ()), (hj.distinct_on, ()), (hj.group_by_columns, (vals, {"n": ("count", None)}))):
        def call(keys, **kw):
            return fn(keys, *more, **kw)
        for keys in ([], [K8] * 5, [K8, s.values[:3]], K8.reshape(7, 1), np.zeros(4, dtype="S3"), [K8, hj.KeyColumn.from_list([b"x"])]):
            with pytest.raises(ValueError):
                call(keys)
        for kw in (dict(nulls="keep"), dict(nulls=None), dict(nulls=True), dict(key_mask=-1), dict(key_mask=1 << 32), dict(key_mask=0.5)):
            with pytest.raises(ValueError):
                call([K8, s], **kw)
    for capacity in (-1, 1.5, True):
        with pytest.raises(ValueError):
            hj.key_groups_host(K8, capacity=capacity)
    with pytest.raises(ValueError):
        hj.distinct_on(K8, {"x": np.zeros(6)})                                   # a payload column of another length
    with pytest.raises(ValueError):
        hj.distinct_on(K8, {"x": np.zeros(7, dtype="S3")})
    bad_aggs = [({"v": np.arange(7.0)}, {"s": ("sum", "v")}),                    # floats are not aggregated
                (vals, {}), (vals, {"s": ("avg", "v")}), (vals, {"s": ("sum", None)}), (vals, {"s": ("sum", "w")}),
                (vals, {"count": ("count", None)}), (vals, {"keys": ("count", None)}), (vals, {"first_rows": ("sum", "v")}),
                ({"v": np.arange(6, dtype=np.int64)}, {"s": ("sum", "v")})]
    for cols, aggs in bad_aggs:
        with pytest.raises(ValueError):
            hj.group_by_columns(K8, cols, aggs)


@pytest.mark.parametrize("nulls", ["group", "drop"])
def test_empty_tables_need_no_device(nulls):
    e8, es = K8[:0], hj.KeyColumn.from_list([])
    for keys in (e8, es, [e8, es]):
        got = hj.key_groups(keys, nulls=nulls)
        assert [got[k].tolist() for k in ("rep", "group", "first_rows")] == [[], [], []] and (got["n_groups"], got["null_rows"]) == (0, 0)
        assert all(got[k].dtype == np.uint32 for k in ("rep", "group", "first_rows"))
        gc.same(hj.key_groups_host(keys, nulls=nulls), got)
        d = hj.distinct_on(keys, {"x": np.zeros(0, dtype=np.int16), "s": hj.KeyColumn.from_list([])}, nulls=nulls)
        assert d["first_rows"].size == 0 and d["n_groups"] == 0 and d["null_rows"] == 0
        assert [k.rows for k in d["keys"]] == [0] * len(d["keys"]) and all(isinstance(k, hj.KeyColumn) for k in d["keys"])
        assert d["cols"]["x"].dtype == np.int16 and d["cols"]["x"].size == 0 and isinstance(d["cols"]["s"], hj.KeyColumn)
        g = hj.group_by_columns(keys, {"v": np.zeros(0, dtype=np.uint32)}, {"n": ("count", None), "s": ("sum", "v")}, nulls=nulls)
        assert g["count"].size == 0 and g["n"].size == 0 and isinstance(g["s"], hj.KeyColumn) and g["s"].rows == 0
        assert g["n_groups"] == 0 and g["first_rows"].size == 0 and len(g["keys"]) == len(d["keys"])


def test_host_wrapper_on_plain_arrays():
    """numpy columns, composite, through the wrapper: the model on the rows' bytes"""
    rng = np.random.default_rng(12)
    a, b = rng.integers(0, 9, 3000).astype(np.uint64) << np.uint64(40), rng.integers(-3, 3, 3000).astype(np.int16)
    want = gc.model_groups(gc.array_keys([a, b]))
    assert 20 < want["n_groups"] <= 54
    for key_mask in gc.MASKS:
        gc.same(hj.key_groups_host([a, b], key_mask=key_mask), want, key_mask)
    masked = np.ma.masked_array(a, mask=rng.random(3000) < 0.1)
    got = hj.key_groups_host(masked, nulls="drop")
    assert got["null_rows"] == int(np.ma.getmaskarray(masked).sum()) and (got["rep"][np.ma.getmaskarray(masked)] == gc.NO_ROW).all()
