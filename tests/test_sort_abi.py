"""hj_sort_rows_dev and its family without a GPU: the declarations, the layout function, the host twin against the model
of sort_common on every case family, every refusal of the header's list, and the wrappers' own checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

import sort_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "htm_hashjoin.h")).read()
U32, U64 = np.uint32, np.uint64
SENT = 0xA5A5A5A5
SYMBOLS = ("hj_sort_rows_dev", "hj_sort_rows_info", "hj_sort_rows_host", "hj_sort_layout_info")


# ---- declarations ----------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_and_bound():
    raw = C.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(rf"^int {s}\(", HEADER, re.M), f"{s} is not declared in the header"
        assert hasattr(raw, s), f"{s} is not exported"
        assert s in lib._hj_signatures, f"{s} has no ctypes signature"
    for fn in (hj.sort_rows, hj.sort_rows_host, hj.sort_by_columns, hj.sort_pairs, hj.HashJoinContext.sort_rows, hj.HashJoinContext.sort_rows_info):
        assert callable(fn)


def test_struct_and_constants_match_the_header():
    assert C.sizeof(_lib.hj_sort_col) == 32
    assert [f for f, _ in _lib.hj_sort_col._fields_] == ["values", "valid", "width", "type", "flags", "reserved"]
    for name, value in (("HJ_SORT_MAX_COLS", 4), ("HJ_SORT_DESC", 1), ("HJ_SORT_NULLS_FIRST", 2)):
        m = re.search(rf"#define {name}\s+(0x[0-9a-fA-F]+|\d+)u?", HEADER)
        assert m and int(m.group(1), 0) == value == getattr(_lib, name) == getattr(hj, name), name
    # the ABI around it has not moved
    assert lib.hj_abi_version() == 4 and re.search(r"#define HJ_ABI_VERSION\s+4\b", HEADER)
    assert C.sizeof(_lib.hj_where_term) == 48 and C.sizeof(_lib.hj_asof_term) == 48 and C.sizeof(_lib.hj_key_col2) == 56
    assert C.sizeof(_lib.hj_key_col) == 24 and C.sizeof(_lib.hj_gather_col) == 40 and C.sizeof(_lib.hj_agg_col) == 40
    assert C.sizeof(_lib.hj_params) == 48


def test_header_states_the_order_and_the_limits():
    text = HEADER[HEADER.index("ORDER BY ----"):HEADER.index("int hj_sort_layout_info")]
    for phrase in ("ASCENDING LEXICOGRAPHIC", "-0.0 == 0.0", "greater than +inf", "na_position", "PostgreSQL", "stable",
                   "does NOT do", "16-byte", "collations", "top-k", "2^32 - 2", "look-back"):
        assert phrase in text, phrase


# ---- the layout --------------------------------------------------------------------------------------------------------------------
def test_layout_invariants():
    sizes = [0, 1, 2, 63, 2047, 2048, 2049, 4096, 4097, 1 << 16, (1 << 16) + 1, 1 << 20, 3_000_001, 1 << 24, (1 << 24) + 5, 1 << 27,
             (1 << 27) + 12345, 1 << 30, (1 << 31) + 7, (1 << 32) - 2]
    tile0, last = sc.layout(1)[0], -1
    for n in sizes:
        tile, chunk, chunks, work = sc.layout(n)
        assert tile == tile0 and tile >= 64 and tile % 64 == 0
        assert chunk % tile == 0 and chunk >= tile and chunk < 1 << 32
        assert chunks * chunk >= n and (chunks == 0 or (chunks - 1) * chunk < n), n
        assert chunks <= 4096, "the histogram of a pass (256 words per chunk) stays bounded"
        assert work >= 2 * n * 8 + 2 * n * 4 + 4 * 256 * chunks
        assert work >= last, "the workspace is monotone in nRows"
        last = work
    assert sc.layout(1 << 16)[2] >= 3
    out = (C.c_uint64 * 4)(*[SENT] * 4)
    assert lib.hj_sort_layout_info((1 << 32) - 1, out) == _lib.HJ_ERR_INVALID and lib.hj_sort_layout_info(5, None) == _lib.HJ_ERR_INVALID
    assert list(out) == [SENT] * 4


def test_workspace_is_monotone_across_the_chunk_steps():
    """where the chunk grows by a tile the chunk count drops: the workspace must not"""
    tile = sc.layout(1)[0]
    for tiles in (8191, 8192, 8193, 12288, 12289, 16384, 16385):
        a, b = sc.layout(tiles * tile)[3], sc.layout(tiles * tile + 1)[3]
        assert b >= a, tiles


# ---- the host twin against the model -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.FAMILIES)
def test_host_twin_equals_the_model(name):
    tile, chunk, _, _ = sc.layout(1)
    for n in (1, 2, 65, tile + 1, 2 * chunk + tile + 17):
        cols, want = sc.case(name, n)
        got, out = sc.host_perm(cols, garbage=np.random.default_rng(n))
        sc.same(got, want, (name, n))
        _, chunk_n, chunks_n, _ = sc.layout(n)
        assert out[0] == n and out[1] == sum(c.passes() for c in cols) and out[2] == 0 and out[3] == 0, (name, n, out)
        assert out[4] == chunks_n and out[5] == chunk_n and out[6] > 0 and out[7] == 0, (name, n, out)


def test_host_twin_fuzz():
    for seed in range(40):
        cols = sc.fuzz_case(seed, max_rows=3000)
        sc.same(sc.host_perm(cols, garbage=np.random.default_rng(seed))[0], sc.model_perm(cols), ("fuzz", seed))


def test_the_model_is_numpys_order_where_numpy_has_one():
    """a plain column ascending is np.argsort(kind='stable') -- NaNs last, -0.0 with 0.0 -- so the model is anchored outside itself"""
    for name in ("type_int64", "type_uint8", "type_float32", "type_float64", "ties_f32", "ties_f64"):
        cols = sc.make(name, 5000, seed=1)
        cols[0].desc = False
        assert np.array_equal(sc.model_perm(cols), np.argsort(cols[0].values, kind="stable").astype(U32)), name


def test_no_rows_on_the_host():
    arr, k = sc.sort_col_array([sc.Col(np.empty(0, dtype=np.int32))], [(0, 0)])
    out = (C.c_uint64 * 8)(*[SENT] * 8)
    assert lib.hj_sort_rows_host(arr, k, 0, None, out) == _lib.HJ_OK and list(out) == [0] * 8
    assert lib.hj_sort_rows_host(arr, k, 0, None, None) == _lib.HJ_OK


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _refusals():
    """(tag, change to a good call) for every refusal of the header's list"""
    def field(i, name, value):
        return lambda a: setattr(a["arr"][i], name, value)
    def arg(name, value):
        return lambda a: a.__setitem__(name, value)
    yield "nCols 0", arg("k", 0)
    yield "nCols above the maximum", arg("k", 5)
    yield "cols NULL", arg("arr", None)
    yield "type above FLOAT", field(0, "type", 3)
    for t, w in ((_lib.HJ_VAL_UINT, 3), (_lib.HJ_VAL_INT, 16), (_lib.HJ_VAL_INT, 0), (_lib.HJ_VAL_FLOAT, 2), (_lib.HJ_VAL_FLOAT, 1)):
        yield f"type {t} width {w}", lambda a, t=t, w=w: (setattr(a["arr"][1], "type", t), setattr(a["arr"][1], "width", w))
    yield "unknown flag bit", field(1, "flags", 4)
    yield "reserved set", field(0, "reserved", 1)
    yield "values NULL", field(1, "values", None)
    yield "values misaligned", lambda a: setattr(a["arr"][0], "values", a["arr"][0].values + 4)          # an 8-byte column
    yield "validity misaligned", lambda a: setattr(a["arr"][1], "valid", a["arr"][1].valid + 2)
    yield "perm NULL", arg("perm", None)
    yield "perm misaligned", lambda a: a.__setitem__("perm", a["perm"] + 2)
    yield "nRows above 2^32 - 2", arg("n", (1 << 32) - 1)


@pytest.mark.parametrize("tag,change", list(_refusals()), ids=[t for t, _ in _refusals()])
def test_refusals(tag, change):
    n = 100
    cols = [sc.Col(np.arange(n, dtype=np.int64)), sc.Col(np.arange(n, dtype=U32), np.arange(n) % 3 > 0)]
    planes = [c.plane() for c in cols]
    arr, k = sc.sort_col_array(cols, [(c.values.ctypes.data, p.ctypes.data if p is not None else 0) for c, p in zip(cols, planes)])
    perm, out = np.full(n + 1, SENT, dtype=U32), (C.c_uint64 * 8)(*[SENT] * 8)
    a = {"arr": arr, "k": k, "n": n, "perm": perm.ctypes.data}
    assert lib.hj_sort_rows_host(a["arr"], a["k"], a["n"], a["perm"], out) == _lib.HJ_OK               # the good call is good
    perm[:] = SENT
    out[:] = [SENT] * 8
    change(a)
    assert lib.hj_sort_rows_host(a["arr"], a["k"], a["n"], a["perm"], out) == _lib.HJ_ERR_INVALID, tag
    assert (perm == SENT).all() and list(out) == [SENT] * 8, (tag, "a refused call wrote something")
    # a NULL context is refused before anything else, and the info call likewise
    assert lib.hj_sort_rows_dev(None, a["arr"], a["k"], a["n"], a["perm"]) == _lib.HJ_ERR_INVALID
    assert lib.hj_sort_rows_info(None, out) == _lib.HJ_ERR_INVALID and list(out) == [SENT] * 8


def test_pointers_are_not_needed_without_rows():
    arr = (_lib.hj_sort_col * 1)()
    arr[0].width, arr[0].type = 8, _lib.HJ_VAL_FLOAT
    assert lib.hj_sort_rows_host(arr, 1, 0, None, None) == _lib.HJ_OK
    arr[0].width = 2
    assert lib.hj_sort_rows_host(arr, 1, 0, None, None) == _lib.HJ_ERR_INVALID


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------------
def test_wrappers_validate_their_arguments():
    a = np.arange(10, dtype=np.int32)
    for bad in ([], [a] * 5, hj.KeyColumn.from_list(["x", "y"]), np.zeros(4, dtype=np.float16), np.zeros(4, dtype=np.complex128),
                np.zeros(4, dtype=[("a", "u8"), ("b", "u8")]), [a, a[:5]], (hj.KeyColumn(a), np.int64)):
        for fn in (hj.sort_rows, hj.sort_rows_host, hj.sort_by_columns):
            with pytest.raises(ValueError):
                fn(bad)
    for kw in ({"descending": [True]}, {"descending": "yes"}, {"descending": 1}, {"nulls": "middle"}, {"nulls": ["last"]}, {"nulls": None}):
        for fn in (hj.sort_rows, hj.sort_rows_host, hj.sort_by_columns):
            with pytest.raises(ValueError):
                fn([a, a], **kw)
    with pytest.raises(ValueError, match="16-byte"):
        hj.sort_rows(np.zeros(4, dtype=[("a", "u8"), ("b", "u8")]))
    with pytest.raises(ValueError, match="strings"):
        hj.sort_rows_host([a[:2], hj.KeyColumn.from_list(["x", None])])
    for limit in (-1, 1.5, True):
        with pytest.raises(ValueError):
            hj.sort_by_columns(a, limit=limit)
    with pytest.raises(ValueError):
        hj.sort_by_columns(a, {"p": np.arange(9)})
    for s, r in ((a, a), (a.astype(U32), a.astype(U32)[:5]), (a.astype(U32).reshape(2, 5), a.astype(U32).reshape(2, 5))):
        with pytest.raises(ValueError):
            hj.sort_pairs(s, r)


def test_wrappers_answer_empty_tables_without_a_device():
    e = np.empty(0, dtype=np.float64)
    assert hj.sort_rows(e).dtype == U32 and hj.sort_rows(e).size == 0 and hj.sort_rows_host([e, e], descending=[True, False]).size == 0
    got = hj.sort_by_columns(hj.KeyColumn(e), {"p": np.empty(0, dtype=np.int16), "s": hj.KeyColumn.from_list([])}, limit=3)
    assert got["rows"].size == 0 and got["keys"][0].rows == 0 and got["cols"]["p"].dtype == np.int16 and got["cols"]["s"].rows == 0
    s, r = hj.sort_pairs(np.empty(0, dtype=U32), np.empty(0, dtype=U32))
    assert s.size == 0 and r.size == 0 and s.dtype == U32


def test_host_wrapper_equals_the_model():
    """the wrapper's own plumbing: masked arrays, KeyColumns, a dtype given apart, flags per column"""
    cols, want = sc.case("multi4", 3000)
    keys = [np.ma.MaskedArray(c.values, mask=~c.valid) if c.valid is not None and i == 1 else c.key() for i, c in enumerate(cols)]
    got = hj.sort_rows_host(keys, descending=[c.desc for c in cols], nulls=[c.nulls for c in cols])
    sc.same(got, want, "multi4 through the wrapper")
    cols, want = sc.case("type_int32", 3000)
    raw = hj.KeyColumn(cols[0].values.view(U32))
    sc.same(hj.sort_rows_host((raw, np.int32)), want, "bytes read as int32")
    assert not np.array_equal(hj.sort_rows_host(raw), want)
