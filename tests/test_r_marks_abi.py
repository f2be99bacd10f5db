"""The R-side match marks at the ABI boundary: hj_r_marks_clear, hj_r_rows_dev and hj_r_rows_info are declared, exported
and bound, HJ_FLAG_TRACK_R_MATCHES is 0x2, nothing of the ABI around them moved, and outer_join_pairs /
radix_outer_join_pairs refuse an unknown `how` and answer empty inputs without a device. No GPU needed."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# symbol -> its arguments behind the context, as the header spells their types
SYMBOLS = {"hj_r_marks_clear": [], "hj_r_rows_dev": ["uint32_t", "uint32_t *", "uint64_t"], "hj_r_rows_info": ["uint64_t"]}
HOWS = ("right", "full", "right_semi", "right_anti")
JOINS = ("outer_join_pairs", "radix_outer_join_pairs")


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
    assert sig["hj_r_rows_dev"][0] == [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64]
    assert sig["hj_r_rows_info"][0] == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)]
    assert sig["hj_r_marks_clear"][0] == [ctypes.c_void_p]


def test_flag_and_which_values():
    code = _code()
    assert re.search(r"#define\s+HJ_FLAG_TRACK_R_MATCHES\s+0x2u\b", code)
    assert re.search(r"#define\s+HJ_FLAG_KEEP_ROW_IDS\s+0x1u\b", code)
    assert re.search(r"#define\s+HJ_R_UNMATCHED\s+0u\b", code) and re.search(r"#define\s+HJ_R_MATCHED\s+1u\b", code)
    assert (_lib.HJ_FLAG_TRACK_R_MATCHES, hj.HJ_FLAG_TRACK_R_MATCHES) == (2, 2)
    assert (hj.HJ_R_UNMATCHED, hj.HJ_R_MATCHED) == (0, 1)


def test_this_is_no_fifth_join_kind():
    enum = re.search(r"typedef\s+enum\s*\{([^}]*)\}\s*hj_join_kind\s*;", _code())
    assert len(re.findall(r"HJ_JOIN_[A-Z]+", enum.group(1))) == 4
    assert set(_lib.JOIN_KINDS) == {"inner", "left", "semi", "anti"}


def test_abi_version_and_struct_sizes_are_unchanged():
    assert hj.lib.hj_abi_version() == 4
    assert re.search(r"#define\s+HJ_ABI_VERSION\s+4\b", _header())
    assert ctypes.sizeof(_lib.hj_params) == 48
    assert ctypes.sizeof(_lib.hj_result) == 232


def test_params_carry_the_flag():
    assert engine._params("atomic", trackRMatches=True, keepRowIds=True).flags == 3
    assert engine._params("htm", trackRMatches=True).flags == 2
    assert engine._params("atomic", keepRowIds=True).flags == 1
    assert engine._params("atomic").flags == 0


def test_null_context_is_invalid():
    out = (ctypes.c_uint64 * 4)()
    assert hj.lib.hj_r_marks_clear(None) == _lib.HJ_ERR_INVALID
    for which in (0, 1, 2):
        assert hj.lib.hj_r_rows_dev(None, which, None, 0) == _lib.HJ_ERR_INVALID
        assert hj.lib.hj_r_rows_dev(None, which, None, 16) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_r_rows_info(None, out) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_r_rows_info(None, None) == _lib.HJ_ERR_INVALID


def test_python_surface():
    params = inspect.signature(hj.outer_join_pairs).parameters
    assert list(params) == ["relR", "relS", "algo", "probeLength", "device", "how"]
    assert (params["algo"].default, params["probeLength"].default, params["device"].default, params["how"].default) == ("htm", 4, 0, "right")
    params = inspect.signature(hj.radix_outer_join_pairs).parameters
    assert list(params) == ["relR", "relS", "radixBits", "slice_tuples", "device", "how"]
    assert (params["radixBits"].default, params["slice_tuples"].default, params["device"].default, params["how"].default) == (0, None, 0, "right")
    assert list(inspect.signature(hj.HashJoinContext.r_rows).parameters) == ["self", "which", "d_out_r", "capacity"]
    assert list(inspect.signature(hj.HashJoinContext.r_rows_info).parameters) == ["self"]
    assert list(inspect.signature(hj.HashJoinContext.r_marks_clear).parameters) == ["self"]
    # join_pairs and radix_join_pairs keep their four kinds
    assert inspect.signature(hj.join_pairs).parameters["how"].default == "inner"
    assert inspect.signature(hj.radix_join_pairs).parameters["how"].default == "inner"


@pytest.mark.parametrize("join", JOINS)
def test_an_unknown_how_is_refused_before_any_device_call(join):
    fn = getattr(hj, join)
    R = np.arange(1, 9, dtype=np.uint64)
    for how in ("inner", "left", "semi", "anti", "outer", "right_outer", "", None, 1, ["right"]):
        with pytest.raises(ValueError):
            fn(R, R, how=how)               # no device here: anything but ValueError would be a device call's error
        with pytest.raises(ValueError):
            fn(R[:0], R, how=how)


@pytest.mark.parametrize("join", JOINS)
@pytest.mark.parametrize("how", HOWS)
def test_empty_inputs_need_no_device(join, how):
    fn = getattr(hj, join)
    R = np.arange(1, 9, dtype=np.uint64)
    S = np.arange(3, 8, dtype=np.uint64)
    all_r = np.arange(R.size, dtype=np.uint32)
    pairs = how in ("right", "full")

    def check(got, want_s, want_r):
        s_idx, r_idx = got
        assert r_idx.dtype == np.uint32 and np.array_equal(r_idx, want_r), (how, r_idx)
        if pairs:
            assert s_idx.dtype == np.uint32 and np.array_equal(s_idx, want_s), (how, s_idx)
        else:
            assert s_idx is None

    no_row = np.full(R.size, hj.NO_ROW, dtype=np.uint32)
    # empty S: no R row is matched -- right anti is all of R ascending, and so is the tail of right / full
    check(fn(R, S[:0], how=how), no_row, all_r[:0] if how == "right_semi" else all_r)
    # empty R: no R-only rows; full keeps every S tuple as an unmatched left row
    if how == "full":
        check(fn(R[:0], S, how=how), np.arange(S.size, dtype=np.uint32), np.full(S.size, hj.NO_ROW, dtype=np.uint32))
    else:
        check(fn(R[:0], S, how=how), all_r[:0], all_r[:0])
    check(fn(R[:0], S[:0], how=how), all_r[:0], all_r[:0])
