"""The materialising probe at the ABI boundary: hj_probe_pairs_dev / hj_pairs_info are declared, exported and bound,
hj_params.flags took the place of the first reserved word without moving anything. No GPU needed."""
import ctypes
import os
import re

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd.engine import _params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hj_probe_pairs_dev", "hj_pairs_info")


def _header():
    return open(os.path.join(ROOT, "include", "htm_hashjoin.h")).read()


def test_symbols_are_declared_exported_and_bound():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), f"{s} is not declared in include/htm_hashjoin.h"
        assert hasattr(raw, s), f"{s} is not exported"
        assert s in hj.lib._hj_signatures, f"{s} has no ctypes signature in _lib.py"
    assert len(hj.lib._hj_signatures["hj_probe_pairs_dev"][0]) == 7
    assert re.search(r"#define\s+HJ_FLAG_KEEP_ROW_IDS\s+0x1u", code)
    assert hj.HJ_FLAG_KEEP_ROW_IDS == _lib.HJ_FLAG_KEEP_ROW_IDS == 1


def test_abi_version_and_params_layout_are_unchanged():
    assert hj.lib.hj_abi_version() == 4
    assert re.search(r"#define\s+HJ_ABI_VERSION\s+4\b", _header())
    assert ctypes.sizeof(_lib.hj_params) == 48
    assert _lib.hj_params.flags.offset == 32 and _lib.hj_params.flags.size == 4
    assert _lib.hj_params.prjMode.offset == 28
    assert _lib.hj_params.reserved.offset == 36 and _lib.hj_params.reserved.size == 12
    # the header says the same: flags follows prjMode, three reserved words follow it
    body = re.search(r"typedef struct \{(.*?)\} hj_params;", re.sub(r"/\*.*?\*/", "", _header(), flags=re.S), flags=re.S).group(1)
    fields = re.findall(r"uint32_t\s+(\w+)(?:\[(\d+)\])?;", body)
    assert [f[0] for f in fields][-3:] == ["prjMode", "flags", "reserved"] and fields[-1][1] == "3"
    assert sum(int(f[1] or 1) for f in fields) == 12


def test_null_context_is_invalid():
    out = (ctypes.c_uint64 * 4)()
    assert hj.lib.hj_probe_pairs_dev(None, None, 0, 0, None, None, 0) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_probe_pairs_dev(None, None, 16, 0, None, None, 16) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_pairs_info(None, out) == _lib.HJ_ERR_INVALID


def test_params_carry_the_flag():
    assert _params("atomic", keepRowIds=True).flags == 1
    assert _params("atomic").flags == 0
    assert _params("htm", keepRowIds=True).flags == 1
    p = _params("atomic", probeLength=2, buildVariant=3, prjMode=1, keepRowIds=True)
    assert (p.probeLength, p.buildVariant, p.prjMode, list(p.reserved)) == (2, 3, 1, [0, 0, 0])


def test_python_surface():
    assert callable(hj.join_pairs)
    assert callable(hj.HashJoinContext.probe_pairs) and callable(hj.HashJoinContext.pairs_info)
