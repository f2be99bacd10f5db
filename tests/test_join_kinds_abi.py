"""The join kinds at the ABI boundary: hj_probe_join_dev and hj_prj_probe_join_dev are declared, exported and bound, the
enum and HJ_NO_ROW are in the header, nothing of the ABI they join moved, and the host-buffer conveniences take `how`.
No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hj_probe_join_dev", "hj_prj_probe_join_dev")
KINDS = ("inner", "left", "semi", "anti")


def _header():
    return open(os.path.join(ROOT, "include", "htm_hashjoin.h")).read()


def _code():
    return re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_symbol_is_declared_exported_and_bound_with_8_arguments(symbol):
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % symbol, _code())
    assert decl, f"{symbol} is not declared in include/htm_hashjoin.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 8 and re.fullmatch(r"uint32_t\s+kind", args[1])
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), symbol), f"{symbol} is not exported"
    assert symbol in hj.lib._hj_signatures, f"{symbol} has no ctypes signature in _lib.py"
    bound, res = hj.lib._hj_signatures[symbol]
    assert len(bound) == 8 and res is ctypes.c_int and bound[1] is ctypes.c_uint32


def test_the_two_entry_points_share_one_signature():
    a, b = (hj.lib._hj_signatures[s] for s in SYMBOLS)
    assert a == b
    # the kind in front of the seven arguments of the pairs probes
    assert a[0][:1] + a[0][2:] == hj.lib._hj_signatures["hj_probe_pairs_dev"][0] == hj.lib._hj_signatures["hj_prj_probe_pairs_dev"][0]


def test_enum_and_no_row_are_in_the_header():
    code = _code()
    enum = re.search(r"typedef\s+enum\s*\{([^}]*)\}\s*hj_join_kind\s*;", code)
    assert enum, "hj_join_kind is not declared"
    values = dict(re.findall(r"(HJ_JOIN_[A-Z]+)\s*=\s*(\d+)", enum.group(1)))
    assert values == {"HJ_JOIN_INNER": "0", "HJ_JOIN_LEFT": "1", "HJ_JOIN_SEMI": "2", "HJ_JOIN_ANTI": "3"}
    assert re.search(r"#define\s+HJ_NO_ROW\s+0xFFFFFFFFu\b", code)
    assert (_lib.HJ_JOIN_INNER, _lib.HJ_JOIN_LEFT, _lib.HJ_JOIN_SEMI, _lib.HJ_JOIN_ANTI) == (0, 1, 2, 3)
    assert hj.NO_ROW == _lib.HJ_NO_ROW == 0xFFFFFFFF


def test_abi_version_and_struct_sizes_are_unchanged():
    assert hj.lib.hj_abi_version() == 4
    assert re.search(r"#define\s+HJ_ABI_VERSION\s+4\b", _header())
    assert ctypes.sizeof(_lib.hj_params) == 48
    assert ctypes.sizeof(_lib.hj_result) == 232


@pytest.mark.parametrize("symbol", SYMBOLS)
def test_null_context_is_invalid(symbol):
    fn = getattr(hj.lib, symbol)
    for kind in (0, 1, 2, 3, 4):
        assert fn(None, kind, None, 0, 0, None, None, 0) == _lib.HJ_ERR_INVALID
        assert fn(None, kind, None, 16, 0, None, None, 16) == _lib.HJ_ERR_INVALID


def test_python_surface():
    import inspect
    for fn in (hj.HashJoinContext.probe_pairs, hj.HashJoinContext.prj_probe_pairs):
        assert inspect.signature(fn).parameters["kind"].default == 0
    for fn in (hj.join_pairs, hj.radix_join_pairs):
        assert inspect.signature(fn).parameters["how"].default == "inner"


@pytest.mark.parametrize("join", ["join_pairs", "radix_join_pairs"])
def test_an_unknown_kind_is_refused_before_any_device_call(join):
    fn = getattr(hj, join)
    R = np.arange(1, 9, dtype=np.uint64)
    for how in ("outer", "right", "", None, 1):
        with pytest.raises(ValueError):
            fn(R, R, how=how)               # no device here: anything but ValueError would be a device call's error
        with pytest.raises(ValueError):
            fn(R[:0], R, how=how)


@pytest.mark.parametrize("join", ["join_pairs", "radix_join_pairs"])
@pytest.mark.parametrize("how", KINDS)
def test_empty_inputs_need_no_device(join, how):
    fn = getattr(hj, join)
    R = np.arange(1, 9, dtype=np.uint64)
    S = np.arange(3, 8, dtype=np.uint64)
    with_r = how in ("inner", "left")
    # empty S: no rows, whatever the kind
    for r_in in (R, R[:0]):
        s_idx, r_idx = fn(r_in, S[:0], how=how)
        assert s_idx.dtype == np.uint32 and s_idx.size == 0
        assert (r_idx is not None and r_idx.dtype == np.uint32 and r_idx.size == 0) if with_r else r_idx is None
    # empty R: every S tuple is unmatched
    s_idx, r_idx = fn(R[:0], S, how=how)
    assert s_idx.dtype == np.uint32
    if how in ("left", "anti"):
        assert np.array_equal(s_idx, np.arange(S.size, dtype=np.uint32))
    else:
        assert s_idx.size == 0
    if how == "left":
        assert r_idx.dtype == np.uint32 and np.array_equal(r_idx, np.full(S.size, hj.NO_ROW, dtype=np.uint32))
    elif how == "inner":
        assert r_idx.dtype == np.uint32 and r_idx.size == 0
    else:
        assert r_idx is None
