"""The materialising radix join at the ABI boundary: hj_prj_probe_pairs_dev is declared, exported and bound, nothing of
the ABI it joins moved, and the Python surface carries it. No GPU needed."""
import ctypes
import os
import re

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd.engine import _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "hj_prj_probe_pairs_dev"


def _header():
    return open(os.path.join(ROOT, "include", "htm_hashjoin.h")).read()


def test_symbol_is_declared_exported_and_bound_with_7_arguments():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % SYMBOL, code)
    assert decl, f"{SYMBOL} is not declared in include/htm_hashjoin.h"
    assert len(decl.group(1).split(",")) == 7
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), SYMBOL), f"{SYMBOL} is not exported"
    assert SYMBOL in hj.lib._hj_signatures, f"{SYMBOL} has no ctypes signature in _lib.py"
    args, res = hj.lib._hj_signatures[SYMBOL]
    assert len(args) == 7 and res is ctypes.c_int
    # the same shape as the table probe's entry point: the two share one output contract
    assert args == hj.lib._hj_signatures["hj_probe_pairs_dev"][0]


def test_null_context_is_invalid():
    fn = getattr(hj.lib, SYMBOL)
    assert fn(None, None, 0, 0, None, None, 0) == _lib.HJ_ERR_INVALID
    assert fn(None, None, 16, 0, None, None, 16) == _lib.HJ_ERR_INVALID


def test_abi_version_and_struct_sizes_are_unchanged():
    assert hj.lib.hj_abi_version() == 4
    assert re.search(r"#define\s+HJ_ABI_VERSION\s+4\b", _header())
    assert ctypes.sizeof(_lib.hj_params) == 48
    assert ctypes.sizeof(_lib.hj_result) == 232
    assert _lib.hj_params.flags.offset == 32
    assert re.search(r"#define\s+HJ_FLAG_KEEP_ROW_IDS\s+0x1u", _header())


def test_the_flag_comment_covers_the_radix_join():
    head = _header()
    at = head.index("#define HJ_FLAG_KEEP_ROW_IDS")
    comment = head[head.rindex("/*", 0, at):at]
    assert "hj_prj_probe_pairs_dev" in comment and "and on HJ_ALGO_PRJ" not in comment


def test_python_surface():
    assert callable(hj.radix_join_pairs)
    assert callable(hj.HashJoinContext.prj_probe_pairs)
    assert _params("prj", keepRowIds=True).flags == 1 and _params("auto", keepRowIds=True).flags == 1
    # the host-buffer convenience needs no device for empty inputs
    import numpy as np
    R = np.arange(1, 9, dtype=np.uint64)
    for a, b in ((R, R[:0]), (R[:0], R)):
        s_idx, r_idx = hj.radix_join_pairs(a, b)
        assert s_idx.size == r_idx.size == 0 and s_idx.dtype == r_idx.dtype == np.uint32
