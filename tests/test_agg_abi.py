"""The aggregating joins at the ABI boundary: the seven calls are declared, exported and bound with the header's argument
types, hj_agg_spec / hj_agg_src / hj_agg_col are 16, 16 and 40 bytes, the ABI version stays 4; hj_prj_agg_layout_info's
arithmetic fits the LDS; every device call refuses a NULL context; the wrappers refuse what they cannot take and answer an
empty side without a device. No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# symbol -> its arguments behind the context, as the header spells their types
DEVICE_SYMBOLS = {
    "hj_prj_agg_begin": ["const hj_agg_spec *", "uint32_t"],
    "hj_prj_probe_agg_dev": ["const uint64_t *", "uint64_t", "const hj_agg_src *", "uint32_t"],
    "hj_prj_agg_rows_dev": ["void *const *", "uint64_t *"],
    "hj_prj_agg_info": ["uint64_t"],
    "hj_pairs_agg_dev": ["const uint32_t *", "const uint32_t *", "uint64_t", "uint32_t", "uint64_t", "uint32_t", "uint64_t",
                         "const hj_agg_col *", "uint32_t", "uint64_t *"],
    "hj_pairs_agg_info": ["uint64_t"]}


def _code():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "htm_hashjoin.h")).read(), flags=re.S)


def _declared_args(symbol):
    decl = re.search(r"\bint\s+%s\s*\(([^)]*)\)" % symbol, _code())
    assert decl, f"{symbol} is not declared in include/htm_hashjoin.h"
    return [a.strip() for a in decl.group(1).split(",")]


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_device_symbol_is_declared_exported_and_bound(symbol):
    args = _declared_args(symbol)
    assert re.fullmatch(r"hj_ctx\s*\*\s*ctx", args[0]) and len(args) == 1 + len(DEVICE_SYMBOLS[symbol])
    for arg, kind in zip(args[1:], DEVICE_SYMBOLS[symbol]):
        assert arg.replace(" ", "").startswith(kind.replace(" ", "")), (symbol, arg)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), symbol), f"{symbol} is not exported"
    bound, res = hj.lib._hj_signatures[symbol]
    assert len(bound) == len(args) and res is ctypes.c_int and bound[0] is ctypes.c_void_p


def test_layout_info_is_declared_exported_and_bound():
    args = _declared_args("hj_prj_agg_layout_info")
    assert [a.replace(" ", "")[:8] for a in args] == ["uint32_t", "uint64_t"]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "hj_prj_agg_layout_info")
    assert hj.lib._hj_signatures["hj_prj_agg_layout_info"] == ([ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)], ctypes.c_int)


def test_bound_argument_types():
    sig = hj.lib._hj_signatures
    vp, u64, u32, P = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER
    assert sig["hj_prj_agg_begin"][0] == [vp, P(_lib.hj_agg_spec), u32]
    assert sig["hj_prj_probe_agg_dev"][0] == [vp, vp, u64, P(_lib.hj_agg_src), u32]
    assert sig["hj_prj_agg_rows_dev"][0] == [vp, P(vp), vp]
    assert sig["hj_prj_agg_info"][0] == [vp, P(u64)]
    assert sig["hj_pairs_agg_dev"][0] == [vp, vp, vp, u64, u32, u64, u32, u64, P(_lib.hj_agg_col), u32, vp]
    assert sig["hj_pairs_agg_info"][0] == [vp, P(u64)]


def _fields(name):
    struct = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, _code())
    assert struct, f"{name} is not declared in include/htm_hashjoin.h"
    return [re.sub(r"\s+", " ", f.strip()) for f in struct.group(1).split(";") if f.strip()]


def test_descriptor_layouts():
    layout = lambda s: [(n, getattr(s, n).offset, getattr(s, n).size) for n, _ in s._fields_]      # noqa: E731
    assert ctypes.sizeof(_lib.hj_agg_spec) == 16 and ctypes.sizeof(_lib.hj_agg_src) == 16 and ctypes.sizeof(_lib.hj_agg_col) == 40
    assert layout(_lib.hj_agg_spec) == [("op", 0, 4), ("width", 4, 4), ("flags", 8, 4), ("reserved", 12, 4)]
    assert layout(_lib.hj_agg_src) == [("src", 0, 8), ("srcValid", 8, 8)]
    assert layout(_lib.hj_agg_col) == [("src", 0, 8), ("srcValid", 8, 8), ("acc", 16, 8), ("op", 24, 4), ("width", 28, 4),
                                       ("flags", 32, 4), ("reserved", 36, 4)]
    assert _fields("hj_agg_spec") == ["uint32_t op", "uint32_t width", "uint32_t flags", "uint32_t reserved"]
    assert _fields("hj_agg_src") == ["const void *src", "const uint32_t *srcValid"]
    assert _fields("hj_agg_col") == ["const void *src", "const uint32_t *srcValid", "void *acc", "uint32_t op", "uint32_t width",
                                     "uint32_t flags", "uint32_t reserved"]
    assert hj.hj_agg_spec is _lib.hj_agg_spec and hj.hj_agg_src is _lib.hj_agg_src and hj.hj_agg_col is _lib.hj_agg_col


def test_constants_and_version():
    code = _code()
    assert re.search(r"#define\s+HJ_ABI_VERSION\s+4\b", code) and hj.lib.hj_abi_version() == 4
    assert re.search(r"#define\s+HJ_AGG_MAX_COLS\s+4\b", code) and re.search(r"#define\s+HJ_AGG_SIGNED\s+0x1u\b", code)
    assert re.search(r"HJ_AGG_COUNT\s*=\s*0\s*,\s*HJ_AGG_SUM\s*=\s*1\s*,\s*HJ_AGG_MIN\s*=\s*2\s*,\s*HJ_AGG_MAX\s*=\s*3\s*\}\s*hj_agg_op", code)
    assert (hj.HJ_AGG_MAX_COLS, hj.HJ_AGG_COUNT, hj.HJ_AGG_SUM, hj.HJ_AGG_MIN, hj.HJ_AGG_MAX, hj.HJ_AGG_SIGNED) == (4, 0, 1, 2, 3, 1)


def test_layout_info_fits_the_lds():
    infos = [hj.prj_agg_layout_info(n) for n in (1, 2, 3, 4)]
    for n, i in zip((1, 2, 3, 4), infos):
        assert i["slots"] * 3 >= i["blockTuples"] * 4, i                             # load at most 0.75
        assert i["blockTuples"] <= 1 << 16                                           # the 16-bit position plane
        lds = i["blockTuples"] * (4 + 8 * n) + i["slots"] * (4 + 2)                  # counts, accumulators; keys, positions
        assert lds <= 160 * 1024, (n, lds)
        assert i["roundS"] == 2048 and i["itemS"] == 1 << 16
    blocks = [i["blockTuples"] for i in infos]
    assert blocks == sorted(blocks, reverse=True) and len(set(blocks)) == 4          # B falls as nCols rises
    out = (ctypes.c_uint64 * 4)()
    assert hj.lib.hj_prj_agg_layout_info(0, out) == hj.HJ_ERR_INVALID and hj.lib.hj_prj_agg_layout_info(5, out) == hj.HJ_ERR_INVALID
    assert hj.lib.hj_prj_agg_layout_info(1, None) == hj.HJ_ERR_INVALID
    for n in (0, 5):
        with pytest.raises(hj.HashJoinError):
            hj.prj_agg_layout_info(n)


def test_null_context_is_invalid_on_every_device_call():
    out8, out4 = (ctypes.c_uint64 * 8)(), (ctypes.c_uint64 * 4)()
    spec, src, col, planes = (_lib.hj_agg_spec * 1)(), (_lib.hj_agg_src * 1)(), (_lib.hj_agg_col * 1)(), (ctypes.c_void_p * 1)()
    lib = hj.lib
    assert lib.hj_prj_agg_begin(None, spec, 1) == hj.HJ_ERR_INVALID
    assert lib.hj_prj_probe_agg_dev(None, None, 0, src, 1) == hj.HJ_ERR_INVALID
    assert lib.hj_prj_agg_rows_dev(None, planes, None) == hj.HJ_ERR_INVALID
    assert lib.hj_prj_agg_info(None, out8) == hj.HJ_ERR_INVALID
    assert lib.hj_pairs_agg_dev(None, None, None, 0, 0, 0, 0, 0, col, 1, None) == hj.HJ_ERR_INVALID
    assert lib.hj_pairs_agg_info(None, out4) == hj.HJ_ERR_INVALID


R = np.arange(1, 9, dtype=np.uint64)
S = np.arange(1, 17, dtype=np.uint64)
COLS = {"a": np.arange(16, dtype=np.int64), "f": np.arange(16, dtype=np.float64)}


def _both(s_cols, aggs, r=R, s=S):
    """the two wrappers on the same request (aggregate_on joins on the tuples as one 8-byte key column)"""
    yield lambda: hj.radix_join_aggregate(r, s, s_cols, aggs)
    yield lambda: hj.aggregate_on(r, s, s_cols, aggs)


@pytest.mark.parametrize("s_cols, aggs", [
    ({"a": COLS["a"]}, {"x": ("median", "a")}),                  # an unknown op
    (COLS, {"x": ("sum", "f")}),                                 # a float column
    ({"a": COLS["a"]}, {"x": ("sum", "b")}),                     # a missing column name
    ({"a": COLS["a"]}, {"x": ("sum", None)}),                    # SUM needs a column
    ({"a": COLS["a"][:15]}, {"x": ("sum", "a")}),                # length mismatch
    ({"a": COLS["a"].astype(np.int16)}, {"x": ("sum", "a")}),    # widths 1 and 2 are widened by the caller
    ({"a": COLS["a"]}, {}),
    ({"a": COLS["a"]}, {"count": ("count", None)}),              # the name of the match counts
    ({"a": COLS["a"]}, {"x": "sum"}),
])
def test_wrappers_raise_value_error(s_cols, aggs):
    for call in _both(s_cols, aggs):
        with pytest.raises(ValueError):
            call()


def test_key_length_mismatch_raises():
    with pytest.raises(ValueError):
        hj.aggregate_on([R, R[:4]], [S, S], {"a": COLS["a"]}, {"x": ("sum", "a")})
    with pytest.raises(ValueError):
        hj.aggregate_on(R, S.astype(np.uint32), {"a": COLS["a"]}, {"x": ("sum", "a")})


@pytest.mark.parametrize("n_r, n_s", [(0, 16), (8, 0), (0, 0)])
def test_an_empty_side_needs_no_device(n_r, n_s):
    valid = np.arange(n_s) % 3 != 0
    s_cols = {"a": np.arange(n_s, dtype=np.int32), "b": hj.KeyColumn(np.arange(n_s, dtype=np.uint64), valid)}
    aggs = {"n": ("count", None), "nb": ("count", "b"), "sa": ("sum", "a"), "lo": ("min", "b"), "hi": ("max", "a")}
    for call in _both(s_cols, aggs, R[:n_r], S[:n_s]):
        res = call()
        assert sorted(res) == sorted(["count", *aggs])
        for name in ("count", "n", "nb"):
            assert res[name].dtype == np.uint64 and res[name].shape == (n_r,) and not res[name].any()
        for name, dtype in (("sa", np.int64), ("lo", np.uint64), ("hi", np.int64)):
            col = res[name]
            assert isinstance(col, hj.KeyColumn) and len(col) == n_r and col.values.dtype == dtype
            assert col.valid is not None and not col.valid.any()                     # SQL: an empty group is NULL
