"""Joins on real key columns at the ABI boundary: hj_key_hash_dev, hj_key_hash_host, hj_pairs_verify_dev, hj_verify_info,
hj_mark_rows_dev and hj_mark_rows_info are declared, exported and bound with the argument types of the header, hj_key_col
is 24 bytes, nothing of the ABI around them moved; hj_key_hash_host computes the header's hash (restated in keys_common.py in numpy)
and refuses what the header says it refuses; join_on refuses what it cannot take and answers empty inputs without a
device. No GPU needed."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

from keys_common import MIXES, PAIR, _code, _declared_args, _header, key_words, murmur3_words, random_column

# symbol -> its arguments behind the context, as the header spells their types
DEVICE_SYMBOLS = {
    "hj_key_hash_dev": ["const hj_key_col *", "uint32_t", "uint32_t", "uint64_t", "uint32_t", "uint64_t *"],
    "hj_pairs_verify_dev": ["const uint32_t *", "const uint32_t *", "uint64_t", "uint32_t", "uint64_t", "uint64_t",
                            "const hj_key_col *", "uint32_t", "uint32_t *", "uint32_t *", "uint64_t", "uint32_t *", "uint32_t *"],
    "hj_verify_info": ["uint64_t"],
    "hj_mark_rows_dev": ["const uint32_t *", "uint64_t", "uint32_t", "uint32_t", "uint32_t *", "uint64_t"],
    "hj_mark_rows_info": ["uint64_t"]}
HOST_ARGS = ["const hj_key_col *", "uint32_t", "uint32_t", "uint64_t", "uint32_t", "uint64_t *"]
HOWS = ("inner", "left", "semi", "anti", "right", "full", "right_semi", "right_anti")
S_PLANE = ("inner", "left", "semi", "anti", "right", "full")
R_PLANE = ("inner", "left", "right", "full", "right_semi", "right_anti")


@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_device_symbol_is_declared_exported_and_bound(symbol):
    args = _declared_args(symbol)
    assert re.fullmatch(r"hj_ctx\s*\*\s*ctx", args[0]) and len(args) == 1 + len(DEVICE_SYMBOLS[symbol])
    for arg, kind in zip(args[1:], DEVICE_SYMBOLS[symbol]):
        assert arg.replace(" ", "").startswith(kind.replace(" ", "")), (symbol, arg)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), symbol), f"{symbol} is not exported"
    assert symbol in hj.lib._hj_signatures, f"{symbol} has no ctypes signature in _lib.py"
    bound, res = hj.lib._hj_signatures[symbol]
    assert len(bound) == len(args) and res is ctypes.c_int and bound[0] is ctypes.c_void_p


def test_host_hash_is_declared_exported_and_bound():
    args = _declared_args("hj_key_hash_host")
    assert len(args) == len(HOST_ARGS)
    for arg, kind in zip(args, HOST_ARGS):
        assert arg.replace(" ", "").startswith(kind.replace(" ", "")), arg
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "hj_key_hash_host")
    bound, res = hj.lib._hj_signatures["hj_key_hash_host"]
    assert len(bound) == len(args) and res is ctypes.c_int


def test_bound_argument_types():
    sig = hj.lib._hj_signatures
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    cols = ctypes.POINTER(_lib.hj_key_col)
    assert sig["hj_key_hash_dev"][0] == [vp, cols, u32, u32, u64, u32, vp]
    assert sig["hj_key_hash_host"][0] == [cols, u32, u32, u64, u32, vp]
    assert sig["hj_pairs_verify_dev"][0] == [vp, vp, vp, u64, u32, u64, u64, cols, u32, vp, vp, u64, vp, vp]
    assert sig["hj_verify_info"][0] == [vp, ctypes.POINTER(u64)]
    assert sig["hj_mark_rows_dev"][0] == [vp, vp, u64, u32, u32, vp, u64]
    assert sig["hj_mark_rows_info"][0] == [vp, ctypes.POINTER(u64)]


def test_key_column_descriptor_layout():
    col = _lib.hj_key_col
    assert ctypes.sizeof(col) == 24
    assert [(n, getattr(col, n).offset, getattr(col, n).size) for n, _ in col._fields_] == [
        ("s", 0, 8), ("r", 8, 8), ("width", 16, 4), ("reserved", 20, 4)]
    struct = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*hj_key_col\s*;", _code())
    assert struct, "hj_key_col is not declared in include/htm_hashjoin.h"
    fields = [re.sub(r"\s+", " ", f.strip()) for f in struct.group(1).split(";") if f.strip()]
    assert fields == ["const void *s", "const void *r", "uint32_t width", "uint32_t reserved"]
    assert hj.hj_key_col is col


def test_constants():
    assert re.search(r"#define\s+HJ_KEY_MAX_COLS\s+4\b", _code())
    assert re.search(r"#define\s+HJ_KEY_SIDE_S\s+0u\b", _code()) and re.search(r"#define\s+HJ_KEY_SIDE_R\s+1u\b", _code())
    assert (_lib.HJ_KEY_MAX_COLS, hj.HJ_KEY_MAX_COLS) == (4, 4)
    assert (hj.HJ_KEY_SIDE_S, hj.HJ_KEY_SIDE_R) == (0, 1)


def test_abi_version_and_struct_sizes_are_unchanged():
    assert hj.lib.hj_abi_version() == 4
    assert re.search(r"#define\s+HJ_ABI_VERSION\s+4\b", _header())
    assert ctypes.sizeof(_lib.hj_params) == 48
    assert ctypes.sizeof(_lib.hj_result) == 232
    assert ctypes.sizeof(_lib.hj_gather_col) == 40


def test_null_context_is_invalid():
    out = (ctypes.c_uint64 * 4)()
    keys = np.arange(16, dtype=np.uint64)
    tuples = np.zeros(16, dtype=np.uint64)
    maps = np.zeros(16, dtype=np.uint32)
    cols = (_lib.hj_key_col * 1)()
    cols[0].s = cols[0].r = keys.ctypes.data
    cols[0].width = 8
    assert hj.lib.hj_key_hash_dev(None, None, 0, 0, 0, 0, None) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_key_hash_dev(None, cols, 1, 0, 16, 0, tuples.ctypes.data) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_pairs_verify_dev(None, None, None, 0, 0, 0, 0, None, 0, None, None, 0, None, None) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_pairs_verify_dev(None, maps.ctypes.data, maps.ctypes.data, 16, 0, 16, 16, cols, 1, None, None, 0,
                                      None, None) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_verify_info(None, out) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_verify_info(None, None) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_mark_rows_dev(None, None, 0, 0, 0, None, 0) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_mark_rows_dev(None, maps.ctypes.data, 16, 0, 1, None, 0) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_mark_rows_info(None, out) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_mark_rows_info(None, None) == _lib.HJ_ERR_INVALID


# ---- the hash: the header's wording, restated ----------------------------------------------------------------------------
def test_the_published_vector():
    """4 zero bytes, seed 0 -> 0x2362F9DE"""
    assert int(murmur3_words(np.zeros((1, 1), dtype=np.uint32))[0]) == 0x2362F9DE
    assert int(hj.key_hash_host(np.zeros(1, dtype=np.uint32))[0]) == 0x2362F9DE
    # a 1- or 2-byte zero is the same one word
    assert int(hj.key_hash_host(np.zeros(1, dtype=np.uint8))[0]) == 0x2362F9DE
    assert int(hj.key_hash_host([np.zeros(1, dtype=np.uint16)])[0]) == 0x2362F9DE


@pytest.mark.parametrize("key_mask", [0, 0x3F, 0xFFFF0000])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_host_hash_equals_the_headers_wording(n, key_mask):
    rng = np.random.default_rng(1000 * n + (key_mask & 0xFF))
    for widths in MIXES:
        cols = [random_column(rng, w, n) for w in widths]
        got = hj.key_hash_host(cols if len(cols) > 1 else cols[0], key_mask=key_mask)
        assert got.dtype == np.uint64 and got.shape == (n,)
        assert np.array_equal(got, murmur3_words(key_words(cols), key_mask)), (widths, n, key_mask)


def test_host_hash_reads_the_side_it_is_given():
    s, r = np.arange(100, dtype=np.uint64), np.arange(100, dtype=np.uint64)[::-1].copy()
    cols = (_lib.hj_key_col * 1)()
    cols[0].s, cols[0].r, cols[0].width = s.ctypes.data, r.ctypes.data, 8
    out = np.zeros(100, dtype=np.uint64)
    assert hj.lib.hj_key_hash_host(cols, 1, hj.HJ_KEY_SIDE_S, 100, 0, out.ctypes.data) == _lib.HJ_OK
    assert np.array_equal(out, murmur3_words(key_words([s])))
    assert hj.lib.hj_key_hash_host(cols, 1, hj.HJ_KEY_SIDE_R, 100, 0, out.ctypes.data) == _lib.HJ_OK
    assert np.array_equal(out, murmur3_words(key_words([r])))
    # the other side's pointer is not needed
    cols[0].r = None
    assert hj.lib.hj_key_hash_host(cols, 1, hj.HJ_KEY_SIDE_S, 100, 0, out.ctypes.data) == _lib.HJ_OK
    assert hj.lib.hj_key_hash_host(cols, 1, hj.HJ_KEY_SIDE_R, 100, 0, out.ctypes.data) == _lib.HJ_ERR_INVALID


def test_host_hash_argument_errors():
    n = 32
    keys = np.arange(2 * n, dtype=np.uint64)
    out = np.full(n, 0xABCD, dtype=np.uint64)

    def call(n_cols=1, side=0, n_rows=n, width=8, reserved=0, ptr=keys.ctypes.data, cols_null=False, out_ptr=out.ctypes.data):
        cols = (_lib.hj_key_col * 5)()
        for c in cols:
            c.s, c.r, c.width, c.reserved = ptr, ptr, width, reserved
        return hj.lib.hj_key_hash_host(None if cols_null else cols, n_cols, side, n_rows, 0, out_ptr)

    assert call() == _lib.HJ_OK
    out[:] = 0xABCD
    bad = [dict(n_cols=0), dict(n_cols=5), dict(cols_null=True), dict(side=2), dict(reserved=1), dict(ptr=None),
           dict(out_ptr=None), dict(n_rows=1 << 32)]
    bad += [dict(width=w) for w in (0, 3, 5, 12, 32)]
    bad += [dict(width=w, ptr=keys.ctypes.data + w // 2) for w in (2, 4, 8, 16)]      # misaligned for its width
    for kw in bad:
        assert call(**kw) == _lib.HJ_ERR_INVALID, kw
    assert np.all(out == 0xABCD), "a refused call wrote something"
    # nRows 0 is a no-op that needs no pointers; the descriptors are still checked
    assert call(n_rows=0, ptr=None, out_ptr=None) == _lib.HJ_OK
    assert call(n_rows=0, ptr=None, out_ptr=None, width=3) == _lib.HJ_ERR_INVALID


def test_python_surface():
    C = hj.HashJoinContext
    assert list(inspect.signature(C.key_hash).parameters) == ["self", "cols", "side", "n_rows", "d_out", "key_mask"]
    assert list(inspect.signature(C.pairs_verify).parameters) == [
        "self", "d_map_s", "d_map_r", "n_pairs", "s_row_base", "s_rows", "r_rows", "cols", "d_out_s", "d_out_r", "capacity",
        "d_s_marks", "d_r_marks"]
    assert list(inspect.signature(C.mark_rows).parameters) == ["self", "d_marks", "rows", "row_base", "which", "d_out", "capacity"]
    assert list(inspect.signature(C.verify_info).parameters) == ["self"]
    assert list(inspect.signature(C.mark_rows_info).parameters) == ["self"]
    for f in (C.key_hash, C.pairs_verify, C.verify_info, C.mark_rows, C.mark_rows_info, hj.key_hash_host, hj.join_on):
        assert f.__doc__
    params = inspect.signature(hj.key_hash_host).parameters
    assert list(params) == ["cols", "key_mask"] and params["key_mask"].default == 0
    params = inspect.signature(hj.join_on).parameters
    assert list(params) == ["r_keys", "s_keys", "r_cols", "s_cols", "how", "radixBits", "slice_tuples", "device", "key_mask"]
    assert [params[k].default for k in list(params)[2:]] == [None, None, "inner", 0, None, 0, 0]
    assert "join_on" in hj.join_tables.__doc__


def test_the_other_wrappers_keep_their_signatures():
    params = inspect.signature(hj.join_tables).parameters
    assert list(params) == ["relR", "relS", "r_cols", "s_cols", "how", "path", "probeLength", "radixBits", "slice_tuples", "device"]
    assert [params[k].default for k in list(params)[2:]] == [None, None, "inner", "htm", 4, 0, None, 0]
    assert list(inspect.signature(hj.join_pairs).parameters) == ["relR", "relS", "algo", "probeLength", "device", "how"]
    assert list(inspect.signature(hj.outer_join_pairs).parameters) == ["relR", "relS", "algo", "probeLength", "device", "how"]
    assert list(inspect.signature(hj.radix_join_pairs).parameters) == ["relR", "relS", "radixBits", "slice_tuples", "device", "how"]


# no device here: anything but ValueError would be a device call's error
R8 = np.arange(1, 9, dtype=np.uint64) << np.uint64(33)
S5 = np.arange(3, 8, dtype=np.uint64) << np.uint64(33)


@pytest.mark.parametrize("how", ["outer", "right_outer", "cross", "", None, 1, ["inner"]])
def test_an_unknown_how_is_refused_before_any_device_call(how):
    for R in (R8, R8[:0]):
        with pytest.raises(ValueError):
            hj.join_on(R, S5, how=how)


@pytest.mark.parametrize("how", ["inner", "right_anti"])
def test_bad_keys_are_refused_before_any_device_call(how):
    r32, s32 = np.arange(8, dtype=np.uint32), np.arange(5, dtype=np.uint32)
    bad = [(R8, s32),                                                          # mismatched itemsizes
           ([R8, r32], [S5, S5]),                                              # ... in the second column
           ([R8, r32], S5),                                                    # two columns against one
           (np.zeros(8, dtype="S3"), np.zeros(5, dtype="S3")),                 # a 3-byte key
           (np.zeros(8, dtype="S32"), np.zeros(5, dtype="S32")),               # a 32-byte key
           ([R8] * 5, [S5] * 5),                                               # five key columns
           ([], []),                                                           # none
           ([R8, r32[:7]], [S5, s32]),                                         # ragged lengths on R
           ([R8, r32], [S5, s32[:4]]),                                         # ... on S
           (R8.reshape(4, 2), S5),                                             # a 2-D key
           ([R8.reshape(4, 2)], [S5])]
    for r_keys, s_keys in bad:
        with pytest.raises(ValueError):
            hj.join_on(r_keys, s_keys, how=how)
    for kw in (dict(key_mask=-1), dict(key_mask=1 << 32), dict(slice_tuples=-3),
               dict(r_cols={"x": np.zeros(7)}), dict(s_cols={"x": np.zeros(5, dtype="S3")})):
        with pytest.raises(ValueError):
            hj.join_on(R8, S5, how=how, **kw)


@pytest.mark.parametrize("composite", [False, True])
@pytest.mark.parametrize("how", HOWS)
def test_empty_inputs_need_no_device(how, composite):
    """no S: no probe row, every R row unmatched. No R: every S tuple unmatched, no R-only row. The columns come back with
    their dtypes, the rows without a partner as all-zero bytes with validity False."""
    r_cols = {"w1": np.arange(10, 18, dtype=np.uint8), "pair": np.zeros(8, dtype=PAIR)}
    r_cols["pair"]["a"] = np.arange(100, 108)
    r_cols["pair"]["b"] = np.arange(8) + 0.5
    s_cols = {"w2": np.arange(20, 25, dtype=np.int16), "w8": np.arange(5, dtype=np.float64) - 2.5}
    keeps_s = how in ("left", "anti", "full")                   # with no R: the S tuples, all unmatched
    keeps_r = how in ("right", "full", "right_anti")            # with no S: the R rows, all unmatched

    def keys(k, n):
        k = k[:n]
        return [k, np.zeros(k.size, dtype=np.int16), np.zeros(k.size, dtype=PAIR)] if composite else k

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

    kw = dict(how=how, slice_tuples=2)
    all_r, all_s = list(range(8)), list(range(5))
    check(hj.join_on(keys(R8, 8), keys(S5, 0), r_cols=r_cols, s_cols={k: v[:0] for k, v in s_cols.items()}, **kw),
          [-1] * 8 if keeps_r else [], all_r if keeps_r else [])
    check(hj.join_on(keys(R8, 0), keys(S5, 5), r_cols={k: v[:0] for k, v in r_cols.items()}, s_cols=s_cols, **kw),
          all_s if keeps_s else [], [-1] * 5 if keeps_s else [])
    check(hj.join_on(keys(R8, 0), keys(S5, 0), r_cols={k: v[:0] for k, v in r_cols.items()},
                     s_cols={k: v[:0] for k, v in s_cols.items()}, how=how), [], [])
    # no columns at all: the maps and the validity alone
    out = hj.join_on(keys(R8, 8), keys(S5, 0), how=how)
    assert (out["s"] == {} if how in S_PLANE else out["s"] is None) and (out["r"] == {} if how in R_PLANE else out["r"] is None)
