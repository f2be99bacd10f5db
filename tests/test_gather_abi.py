"""The gather through the row maps at the ABI boundary: hj_gather_dev and hj_gather_info are declared, exported and bound
with the argument types of the header, hj_gather_col is 40 bytes, nothing of the ABI around them moved, and join_tables
refuses what it cannot take and answers empty inputs without a device. No GPU needed."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# symbol -> its arguments behind the context, as the header spells their types
SYMBOLS = {"hj_gather_dev": ["const uint32_t *", "uint64_t", "uint32_t", "uint64_t", "const hj_gather_col *", "uint32_t", "uint32_t *"],
           "hj_gather_info": ["uint64_t"]}
HOWS = ("inner", "left", "semi", "anti", "right", "full", "right_semi", "right_anti")
S_PLANE = ("inner", "left", "semi", "anti", "right", "full")
R_PLANE = ("inner", "left", "right", "full", "right_semi", "right_anti")
PAIR = np.dtype([("a", np.uint64), ("b", np.float64)])         # a 16-byte structured element


def _header():
    return open(os.path.join(ROOT, "include", "htm_hashjoin.h")).read()


def _code():
    return re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)


@pytest.mark.parametrize("symbol", sorted(SYMBOLS))
def test_symbol_is_declared_exported_and_bound(symbol):
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % symbol, _code())
    assert decl, f"{symbol} is not declared in include/htm_hashjoin.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert re.fullmatch(r"hj_ctx\s*\*\s*ctx", args[0]) and len(args) == 1 + len(SYMBOLS[symbol])
    for arg, kind in zip(args[1:], SYMBOLS[symbol]):
        assert arg.replace(" ", "").startswith(kind.replace(" ", "")), (symbol, arg)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), symbol), f"{symbol} is not exported"
    assert symbol in hj.lib._hj_signatures, f"{symbol} has no ctypes signature in _lib.py"
    bound, res = hj.lib._hj_signatures[symbol]
    assert len(bound) == len(args) and res is ctypes.c_int and bound[0] is ctypes.c_void_p


def test_bound_argument_types():
    sig = hj.lib._hj_signatures
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    assert sig["hj_gather_dev"][0] == [vp, vp, u64, u32, u64, ctypes.POINTER(_lib.hj_gather_col), u32, vp]
    assert sig["hj_gather_info"][0] == [vp, ctypes.POINTER(u64)]


def test_column_descriptor_layout():
    col = _lib.hj_gather_col
    assert ctypes.sizeof(col) == 40
    assert [(n, getattr(col, n).offset, getattr(col, n).size) for n, _ in col._fields_] == [
        ("src", 0, 8), ("dst", 8, 8), ("width", 16, 4), ("reserved", 20, 4), ("fill", 24, 16)]
    struct = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*hj_gather_col\s*;", _code())
    assert struct, "hj_gather_col is not declared in include/htm_hashjoin.h"
    fields = [re.sub(r"\s+", " ", f.strip()) for f in struct.group(1).split(";") if f.strip()]
    assert fields == ["const void *src", "void *dst", "uint32_t width", "uint32_t reserved", "uint64_t fill[2]"]
    assert hj.hj_gather_col is col


def test_max_cols():
    assert re.search(r"#define\s+HJ_GATHER_MAX_COLS\s+8\b", _code())
    assert (_lib.HJ_GATHER_MAX_COLS, hj.HJ_GATHER_MAX_COLS) == (8, 8)


def test_abi_version_and_struct_sizes_are_unchanged():
    assert hj.lib.hj_abi_version() == 4
    assert re.search(r"#define\s+HJ_ABI_VERSION\s+4\b", _header())
    assert ctypes.sizeof(_lib.hj_params) == 48
    assert ctypes.sizeof(_lib.hj_result) == 232


def test_null_context_is_invalid():
    out = (ctypes.c_uint64 * 4)()
    cols = (_lib.hj_gather_col * 1)()
    assert hj.lib.hj_gather_dev(None, None, 0, 0, 0, None, 0, None) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_gather_dev(None, None, 16, 0, 16, cols, 1, None) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_gather_info(None, out) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_gather_info(None, None) == _lib.HJ_ERR_INVALID


def test_python_surface():
    params = inspect.signature(hj.HashJoinContext.gather).parameters
    assert list(params) == ["self", "d_map", "n_rows", "src_rows", "cols", "d_valid", "row_base"]
    assert (params["d_valid"].default, params["row_base"].default) == (0, 0)
    assert list(inspect.signature(hj.HashJoinContext.gather_info).parameters) == ["self"]
    params = inspect.signature(hj.join_tables).parameters
    assert list(params) == ["relR", "relS", "r_cols", "s_cols", "how", "path", "probeLength", "radixBits", "slice_tuples", "device"]
    assert [params[k].default for k in list(params)[2:]] == [None, None, "inner", "htm", 4, 0, None, 0]
    # the pairs wrappers keep their signatures
    assert list(inspect.signature(hj.join_pairs).parameters) == ["relR", "relS", "algo", "probeLength", "device", "how"]
    assert list(inspect.signature(hj.outer_join_pairs).parameters) == ["relR", "relS", "algo", "probeLength", "device", "how"]
    assert list(inspect.signature(hj.radix_join_pairs).parameters) == ["relR", "relS", "radixBits", "slice_tuples", "device", "how"]


# no device here: anything but ValueError would be a device call's error
R8 = np.arange(1, 9, dtype=np.uint64)
S5 = np.arange(3, 8, dtype=np.uint64)


@pytest.mark.parametrize("how", ["outer", "right_outer", "cross", "", None, 1, ["inner"]])
def test_an_unknown_how_is_refused_before_any_device_call(how):
    for R in (R8, R8[:0]):
        with pytest.raises(ValueError):
            hj.join_tables(R, S5, how=how)


@pytest.mark.parametrize("path", ["prj", "auto", "hash", "", None, 3, ["htm"]])
def test_an_unknown_path_is_refused_before_any_device_call(path):
    for how in ("inner", "full"):
        with pytest.raises(ValueError):
            hj.join_tables(R8, S5, how=how, path=path)


@pytest.mark.parametrize("side", ["r_cols", "s_cols"])
@pytest.mark.parametrize("how", ["inner", "right_anti"])
def test_a_bad_column_is_refused_before_any_device_call(side, how):
    n = R8.size if side == "r_cols" else S5.size
    bad = [np.zeros(n + 1, dtype=np.uint32),                    # too long
           np.zeros(n - 1, dtype=np.uint32),                    # too short
           np.zeros((n, 2), dtype=np.uint32),                   # not 1-D
           np.zeros(n, dtype="S3"),                             # 3-byte elements
           np.zeros(n, dtype=np.dtype([("a", np.uint64), ("b", np.uint64), ("c", np.uint64)])),      # 24-byte elements
           np.zeros(n, dtype=np.complex256 if hasattr(np, "complex256") else "S32")]                # 32-byte elements
    for col in bad:
        with pytest.raises(ValueError):
            hj.join_tables(R8, S5, how=how, **{side: {"ok": np.zeros(n, dtype=np.uint8), "bad": col}})


@pytest.mark.parametrize("path", ["htm", "atomic", "radix"])
@pytest.mark.parametrize("how", HOWS)
def test_empty_inputs_need_no_device(how, path):
    """no S: no probe row, every R row unmatched. No R: every S tuple unmatched, no R-only row. The columns come back with
    their dtypes, the rows without a partner as all-zero bytes with validity False."""
    r_cols = {"w1": np.arange(10, 18, dtype=np.uint8), "pair": np.zeros(8, dtype=PAIR)}
    r_cols["pair"]["a"] = np.arange(100, 108)
    r_cols["pair"]["b"] = np.arange(8) + 0.5
    s_cols = {"w2": np.arange(20, 25, dtype=np.int16), "w8": np.arange(5, dtype=np.float64) - 2.5}
    keeps_s = how in ("left", "anti", "full")                   # with no R: the S tuples, all unmatched
    keeps_r = how in ("right", "full", "right_anti")            # with no S: the R rows, all unmatched

    def check(out, rows_s, rows_r):
        """rows_s / rows_r: the source row of every result row per side, -1 = NULL"""
        assert set(out) == {"s_idx", "r_idx", "s", "r", "s_valid", "r_valid"}
        for side, plane, rows, cols in (("s", how in S_PLANE, rows_s, s_cols), ("r", how in R_PLANE, rows_r, r_cols)):
            idx, got, valid = out[side + "_idx"], out[side], out[side + "_valid"]
            if not plane:
                assert idx is None and got is None and valid is None, (how, side)
                continue
            rows = np.asarray(rows, dtype=np.int64)
            assert idx.dtype == np.uint32 and np.array_equal(idx, np.where(rows < 0, hj.NO_ROW, rows).astype(np.uint32)), (how, side)
            assert valid.dtype == np.bool_ and np.array_equal(valid, rows >= 0), (how, side)
            assert set(got) == set(cols)
            for name, col in cols.items():
                want = np.zeros(rows.size, dtype=col.dtype)
                want[rows >= 0] = col[rows[rows >= 0]]
                assert got[name].dtype == col.dtype and got[name].shape == (rows.size,), (how, side, name)
                assert got[name].tobytes() == want.tobytes(), (how, side, name)

    kw = dict(r_cols=r_cols, s_cols=s_cols, how=how, path=path, slice_tuples=2 if path == "radix" else None)
    all_r, all_s = list(range(8)), list(range(5))
    check(hj.join_tables(R8, S5[:0], **{**kw, "s_cols": {k: v[:0] for k, v in s_cols.items()}}),
          [-1] * 8 if keeps_r else [], all_r if keeps_r else [])
    check(hj.join_tables(R8[:0], S5, **{**kw, "r_cols": {k: v[:0] for k, v in r_cols.items()}}),
          all_s if keeps_s else [], [-1] * 5 if keeps_s else [])
    check(hj.join_tables(R8[:0], S5[:0], r_cols={k: v[:0] for k, v in r_cols.items()},
                         s_cols={k: v[:0] for k, v in s_cols.items()}, how=how, path=path), [], [])
    # no columns at all: the maps and the validity alone
    out = hj.join_tables(R8, S5[:0], how=how, path=path)
    assert (out["s"] == {} if how in S_PLANE else out["s"] is None) and (out["r"] == {} if how in R_PLANE else out["r"] is None)
