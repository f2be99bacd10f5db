"""hj_gather2_dev / hj_gather2_info and the KeyColumn payload columns of the join wrappers, as far as no device is needed:
the declarations, the descriptor's layout, the Python surface, the refusals that come before any device call, and the
joins with an empty side, whose answers are made on the host. Expected values come from plain Python."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

from keys2_common import HOWS, ModelCol, fixed_col, key_column, varlen_col
from keys_common import _code, _declared_args, _header

COL2 = "const hj_gather_col2 *"
S_PLANE = ("inner", "left", "semi", "anti", "right", "full")
R_PLANE = ("inner", "left", "right", "full", "right_semi", "right_anti")


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_gather2_dev_is_declared_exported_and_bound():
    args = _declared_args("hj_gather2_dev")
    kinds = ["const uint32_t *", "uint64_t", "uint32_t", "uint64_t", COL2, "uint32_t", "uint32_t *"]
    assert re.fullmatch(r"hj_ctx\s*\*\s*ctx", args[0]) and len(args) == 1 + len(kinds)
    for arg, kind in zip(args[1:], kinds):
        assert arg.replace(" ", "").startswith(kind.replace(" ", "")), arg
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "hj_gather2_dev"), "hj_gather2_dev is not exported"
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    assert hj.lib._hj_signatures["hj_gather2_dev"] == ([vp, vp, u64, u32, u64, ctypes.POINTER(_lib.hj_gather_col2), u32, vp], ctypes.c_int)
    # word for word the arguments of hj_gather_dev, but for the descriptor
    assert [a.replace("hj_gather_col2", "hj_gather_col") for a in args] == _declared_args("hj_gather_dev")


def test_gather2_info_is_declared_exported_and_bound():
    args = _declared_args("hj_gather2_info")
    assert len(args) == 2 and re.fullmatch(r"hj_ctx\s*\*\s*ctx", args[0])
    assert re.fullmatch(r"uint64_t\s+out\[\s*4\s*\+\s*HJ_GATHER_MAX_COLS\s*\]", args[1]), args[1]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "hj_gather2_info"), "hj_gather2_info is not exported"
    assert hj.lib._hj_signatures["hj_gather2_info"] == ([ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int)


def test_column_descriptor_layout():
    col = _lib.hj_gather_col2
    assert ctypes.sizeof(col) == 80
    assert re.search(r"\}\s*hj_gather_col2\s*;\s*/\*\s*80 bytes\s*\*/", _header()), "the header states the size"
    assert [(n, getattr(col, n).offset, getattr(col, n).size) for n, _ in col._fields_] == [
        ("src", 0, 8), ("dst", 8, 8), ("srcOffsets", 16, 8), ("dstOffsets", 24, 8), ("srcValid", 32, 8), ("dstValid", 40, 8),
        ("dstCapacity", 48, 8), ("width", 56, 4), ("flags", 60, 4), ("fill", 64, 16)]
    struct = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*hj_gather_col2\s*;", _code())
    assert struct, "hj_gather_col2 is not declared in include/htm_hashjoin.h"
    fields = [re.sub(r"\s+", " ", f.strip()) for f in struct.group(1).split(";") if f.strip()]
    assert fields == ["const void *src", "void *dst", "const uint32_t *srcOffsets", "uint32_t *dstOffsets", "const uint32_t *srcValid",
                      "uint32_t *dstValid", "uint64_t dstCapacity", "uint32_t width", "uint32_t flags", "uint64_t fill[2]"]
    assert hj.hj_gather_col2 is col


def test_abi_version_and_the_structs_around_are_unchanged():
    assert hj.lib.hj_abi_version() == 4
    assert re.search(r"#define\s+HJ_ABI_VERSION\s+4\b", _header())
    assert ctypes.sizeof(_lib.hj_params) == 48
    assert ctypes.sizeof(_lib.hj_result) == 232
    assert ctypes.sizeof(_lib.hj_gather_col) == 40
    assert ctypes.sizeof(_lib.hj_key_col2) == 56
    assert _lib.HJ_GATHER_MAX_COLS == 8 and re.search(r"#define\s+HJ_GATHER_MAX_COLS\s+8\b", _header())


def test_a_null_context_is_refused():
    arr = (_lib.hj_gather_col2 * 1)()
    out = (ctypes.c_uint64 * 12)()
    assert hj.lib.hj_gather2_dev(None, None, 0, 0, 0, arr, 1, None) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_gather2_dev(None, None, 0, 0, 0, None, 0, None) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_gather2_info(None, out) == _lib.HJ_ERR_INVALID


# ---- Python ----------------------------------------------------------------------------------------------------------------
def test_python_surface():
    args = list(inspect.signature(hj.HashJoinContext.gather2).parameters)
    assert args == ["self", "d_map", "n_rows", "src_rows", "cols", "d_valid", "row_base"]
    assert args == list(inspect.signature(hj.HashJoinContext.gather).parameters)
    assert list(inspect.signature(hj.HashJoinContext.gather2_info).parameters) == ["self"]
    assert callable(hj.KeyColumn.to_list)
    for fn in (hj.join_tables, hj.join_on, hj.join_on_columns):
        assert {"r_cols", "s_cols"} <= set(inspect.signature(fn).parameters)


ITEMS = [[], [None], [b""], [b"", None, b"a", "été", b"\x00" * 40, None, b"", b"xyz" * 100]]


@pytest.mark.parametrize("items", ITEMS)
def test_to_list_is_the_inverse_of_from_list(items):
    want = [x.encode("utf-8") if isinstance(x, str) else x for x in items]
    col = hj.KeyColumn.from_list(items)
    assert col.to_list() == want
    assert hj.KeyColumn.from_list(col.to_list()).to_list() == want
    assert (col.valid is None) == all(x is not None for x in items)


def test_to_list_of_a_fixed_column_gives_the_elements_bytes():
    values = np.array([1, 0x0203, 0xFFFF], dtype=np.uint16)
    assert hj.KeyColumn(values).to_list() == [b"\x01\x00", b"\x03\x02", b"\xff\xff"]
    assert hj.KeyColumn(values, np.array([True, False, True])).to_list() == [b"\x01\x00", None, b"\xff\xff"]
    wide = np.arange(32, dtype=np.uint8).view("V16")
    assert hj.KeyColumn(wide).to_list() == [bytes(range(16)), bytes(range(16, 32))]
    rng = np.random.default_rng(1)
    for width in (1, 2, 4, 8, 16):
        model = fixed_col(rng, width, 37, nulls=0.3)
        assert key_column(model).to_list() == model.items
    model = varlen_col(rng, [0, 1, 5, 0, 33, 2], nulls=0.4)
    assert key_column(model, lead=3).to_list() == model.items      # offsets[0] need not be 0


def _joins(n_r, n_s, r_cols, s_cols, how):
    """every wrapper on relations of n_r and n_s rows (one of them 0)"""
    tuples = lambda n: np.arange(1, n + 1, dtype=np.uint64)     # noqa: E731
    yield "join_tables", lambda: hj.join_tables(tuples(n_r), tuples(n_s), r_cols=r_cols, s_cols=s_cols, how=how)
    yield "join_on", lambda: hj.join_on(tuples(n_r), tuples(n_s), r_cols=r_cols, s_cols=s_cols, how=how)
    keys = lambda n: hj.KeyColumn.from_list([b"k%d" % i for i in range(n)])     # noqa: E731
    yield "join_on_columns", lambda: hj.join_on_columns(keys(n_r), keys(n_s), r_cols=r_cols, s_cols=s_cols, how=how)


@pytest.mark.parametrize("how", HOWS)
def test_a_bad_key_column_payload_is_refused_before_any_device_call(how):
    good = hj.KeyColumn.from_list([b"a", None, b"ccc"])
    for bad in (hj.KeyColumn.from_list([b"a", b"b"]), hj.KeyColumn(np.arange(4, dtype=np.uint32)), object(), {"x": 1}):
        for side in ("r_cols", "s_cols"):
            cols = {"r_cols": {"p": good}, "s_cols": {"p": good}}
            cols[side] = {"p": bad}
            for name, call in _joins(3, 3, cols["r_cols"], cols["s_cols"], how):
                with pytest.raises(ValueError):
                    call()


@pytest.mark.parametrize("how", HOWS)
@pytest.mark.parametrize("empty", ["R", "S"])
def test_empty_side_joins_return_key_columns_without_a_device(how, empty):
    rng = np.random.default_rng(5)
    n = 9
    n_r, n_s = (0, n) if empty == "R" else (n, 0)
    model = {side: {"text": varlen_col(rng, [0, 3, 17, 1, 0, 64, 2, 5, 9][:rows], nulls=0.3), "num": fixed_col(rng, 8, rows, nulls=0.3)}
             for side, rows in (("r", n_r), ("s", n_s))}
    cols = {side: {name: key_column(c) for name, c in m.items()} for side, m in model.items()}
    plain = np.arange(n, dtype=np.uint32) * 3
    cols["s" if n_s else "r"]["plain"] = plain                      # a numpy column next to them behaves as it did
    for name, call in _joins(n_r, n_s, cols["r"], cols["s"], how):
        res = call()
        for side, plane, idx_name in (("s", how in S_PLANE, "s_idx"), ("r", how in R_PLANE, "r_idx")):
            if not plane:
                assert res[side] is None
                continue
            idx = res[idx_name]
            for col_name, m in model[side].items():
                got = res[side][col_name]
                assert isinstance(got, hj.KeyColumn) and got.rows == idx.size, (name, how, side, col_name)
                want = [None if i == hj.NO_ROW else m.items[i] for i in idx]
                assert got.to_list() == want, (name, how, side, col_name)
                assert (got.valid is None) == all(w is not None for w in want)
                assert got.width == m.width
            if "plain" in cols[side]:
                ok = idx != hj.NO_ROW
                assert np.array_equal(res[side]["plain"][ok], plain[idx[ok]]) and (res[side]["plain"][~ok] == 0).all()
        # the preserved side is there in full
        if (empty == "R" and how in ("left", "anti", "full")) or (empty == "S" and how in ("right", "full", "right_anti")):
            assert res["s_idx" if empty == "R" else "r_idx"].size == n
