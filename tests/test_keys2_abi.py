"""Key columns in the Arrow layout at the ABI boundary: hj_key_hash2_dev, hj_key_hash2_host and hj_pairs_verify2_dev are
declared, exported and bound, hj_key_col2 is 56 bytes, nothing of the ABI around them moved; hj_key_hash2_host computes the
header's hash with its NULL and variable-length rules (restated in keys2_common) and refuses what the header says it
refuses; KeyColumn validates what it is given, join_on_columns refuses what it cannot take and answers empty inputs
without a device. No GPU needed."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

from keys2_common import (HOWS, LENGTHS, MASKS, M32, ROWS, ModelCol, _bad_columns, _col2, fixed_col, hash_matrix, key_column, mm3_final,
                          mm3_mix, model_words, varlen_col)
from keys_common import MIXES, PAIR, _code, _declared_args, _header, key_words, murmur3_words, random_column

COL2 = "const hj_key_col2 *"
DEVICE_SYMBOLS = {
    "hj_key_hash2_dev": [COL2, "uint32_t", "uint32_t", "uint64_t", "uint32_t", "uint64_t *"],
    "hj_pairs_verify2_dev": ["const uint32_t *", "const uint32_t *", "uint64_t", "uint32_t", "uint64_t", "uint64_t", COL2, "uint32_t",
                             "uint32_t *", "uint32_t *", "uint64_t", "uint32_t *", "uint32_t *"]}
HOST_ARGS = [COL2, "uint32_t", "uint32_t", "uint64_t", "uint32_t", "uint64_t *"]
S_PLANE = ("inner", "left", "semi", "anti", "right", "full")
R_PLANE = ("inner", "left", "right", "full", "right_semi", "right_anti")


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("symbol", sorted(DEVICE_SYMBOLS))
def test_device_symbol_is_declared_exported_and_bound(symbol):
    args = _declared_args(symbol)
    assert re.fullmatch(r"hj_ctx\s*\*\s*ctx", args[0]) and len(args) == 1 + len(DEVICE_SYMBOLS[symbol])
    for arg, kind in zip(args[1:], DEVICE_SYMBOLS[symbol]):
        assert arg.replace(" ", "").startswith(kind.replace(" ", "")), (symbol, arg)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), symbol), f"{symbol} is not exported"
    bound, res = hj.lib._hj_signatures[symbol]
    assert len(bound) == len(args) and res is ctypes.c_int and bound[0] is ctypes.c_void_p


def test_host_hash_is_declared_exported_and_bound():
    args = _declared_args("hj_key_hash2_host")
    assert len(args) == len(HOST_ARGS)
    for arg, kind in zip(args, HOST_ARGS):
        assert arg.replace(" ", "").startswith(kind.replace(" ", "")), arg
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "hj_key_hash2_host")


def test_bound_argument_types():
    sig = hj.lib._hj_signatures
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    cols = ctypes.POINTER(_lib.hj_key_col2)
    assert sig["hj_key_hash2_dev"] == ([vp, cols, u32, u32, u64, u32, vp], ctypes.c_int)
    assert sig["hj_key_hash2_host"] == ([cols, u32, u32, u64, u32, vp], ctypes.c_int)
    assert sig["hj_pairs_verify2_dev"] == ([vp, vp, vp, u64, u32, u64, u64, cols, u32, vp, vp, u64, vp, vp], ctypes.c_int)


def test_column_descriptor_layout():
    col = _lib.hj_key_col2
    assert ctypes.sizeof(col) == 56
    assert [(n, getattr(col, n).offset, getattr(col, n).size) for n, _ in col._fields_] == [
        ("s", 0, 8), ("r", 8, 8), ("sOffsets", 16, 8), ("rOffsets", 24, 8), ("sValid", 32, 8), ("rValid", 40, 8),
        ("width", 48, 4), ("flags", 52, 4)]
    struct = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*hj_key_col2\s*;", _code())
    assert struct, "hj_key_col2 is not declared in include/htm_hashjoin.h"
    fields = [re.sub(r"\s+", " ", f.strip()) for f in struct.group(1).split(";") if f.strip()]
    assert fields == ["const void *s, *r", "const uint32_t *sOffsets, *rOffsets", "const uint32_t *sValid, *rValid",
                      "uint32_t width", "uint32_t flags"]
    assert hj.hj_key_col2 is col
    assert re.search(r"#define\s+HJ_KEY_NULLS_EQUAL\s+0x1u\b", _code()) and (_lib.HJ_KEY_NULLS_EQUAL, hj.HJ_KEY_NULLS_EQUAL) == (1, 1)


def test_abi_version_and_the_structs_around_are_unchanged():
    assert hj.lib.hj_abi_version() == 4
    assert re.search(r"#define\s+HJ_ABI_VERSION\s+4\b", _header())
    assert ctypes.sizeof(_lib.hj_key_col) == 24
    assert ctypes.sizeof(_lib.hj_params) == 48
    assert ctypes.sizeof(_lib.hj_result) == 232
    assert ctypes.sizeof(_lib.hj_gather_col) == 40


# ---- the hash --------------------------------------------------------------------------------------------------------------
def test_the_model_is_the_old_restatement_on_plain_columns():
    """keys2_common's scalar hash against keys_common's numpy one, neither of them the library"""
    rng = np.random.default_rng(5)
    for widths in MIXES:
        cols = [random_column(rng, w, 40) for w in widths]
        model = [ModelCol(w, [c[i].tobytes() for i in range(40)], False) for w, c in zip(widths, cols)]
        assert np.array_equal(model_words(model, 0x3F0F), murmur3_words(key_words(cols), 0x3F0F)), widths


@pytest.mark.parametrize("n", ROWS)
def test_host_hash_equals_the_headers_wording(n):
    """fixed mixes plain and nullable, every length of LENGTHS, composites; validity words that end mid-word"""
    rng = np.random.default_rng(77 + n)
    for model in hash_matrix(rng, n):
        want = model_words(model)
        cols = [key_column(c, lead=k % 4) for k, c in enumerate(model)]
        for key_mask in MASKS:
            got = hj.key_hash2_host(cols, key_mask=key_mask)
            assert got.dtype == np.uint64 and got.shape == (n,)
            assert np.array_equal(got, want & np.uint64(key_mask or M32)), ([(c.width, c.nulls_equal) for c in model], n, key_mask)


@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_every_length_at_every_alignment(lead):
    """one element per length, off[0] = lead != 0 for three of the four; over the four leads every element starts at every
    byte alignment. The bytes in front of the first element and behind the last are not part of any element."""
    rng = np.random.default_rng(lead)
    model = [varlen_col(rng, LENGTHS)]
    col = key_column(model[0], lead=lead)
    assert int(col.offsets[0]) == lead and {int(o) % 4 for o in col.offsets[:-1]} == {0, 1, 2, 3}
    for key_mask in MASKS:
        assert np.array_equal(hj.key_hash2_host(col, key_mask=key_mask), model_words(model, key_mask))
    # the same elements behind another lead hash the same: only the element's bytes count
    assert np.array_equal(hj.key_hash2_host(key_column(model[0], lead=(lead + 1) % 4)), hj.key_hash2_host(col))


def test_a_variable_length_element_is_its_length_then_its_padded_words():
    """"ab" and "ab\\0" differ (the length is mixed), and so do "" and a NULL that equals NULLs"""
    words = hj.key_hash2_host(hj.KeyColumn.from_list([b"ab", b"ab\0", b"", "ab", "é"]))
    h = mm3_mix(mm3_mix(0, 2), 0x6261)
    assert int(words[0]) == mm3_final(h, 8) == int(words[3])
    assert int(words[1]) == mm3_final(mm3_mix(mm3_mix(0, 3), 0x6261), 8) != int(words[0])
    assert int(words[2]) == mm3_final(mm3_mix(0, 0), 4)
    assert int(words[4]) == mm3_final(mm3_mix(mm3_mix(0, 2), 0xA9C3), 8)          # UTF-8
    null = hj.key_hash2_host(hj.KeyColumn.from_list([None, b""], nulls_equal=True))
    assert int(null[0]) == mm3_final(mm3_mix(0, M32), 4) != int(null[1]) == int(words[2])


def test_null_keyed_rows_hash_their_position():
    """a NULL in a column without HJ_KEY_NULLS_EQUAL: the word is the row number's, whatever the columns hold and whatever
    the other columns' flags; with the flag everywhere no row is NULL-keyed"""
    n = 200
    rng = np.random.default_rng(3)
    model = [fixed_col(rng, 8, n, nulls=0.5), varlen_col(rng, [5] * n, nulls=0.0, nulls_equal=True)]
    for key_mask in MASKS:
        got = hj.key_hash2_host([key_column(c) for c in model], key_mask=key_mask)
        for i in range(n):
            by_position = mm3_final(mm3_mix(0x4E554C4C, i), 4) & (key_mask or M32)
            if model[0].items[i] is None:
                assert int(got[i]) == by_position, i
    nulls = np.flatnonzero([e is None for e in model[0].items])
    full = hj.key_hash2_host([key_column(c) for c in model])
    assert np.unique(full[nulls]).size == nulls.size, "NULL-keyed rows spread like unique keys"
    # the filler under a NULL is not hashed
    assert np.array_equal(hj.key_hash2_host([key_column(model[0], filler=0x11), key_column(model[1])]), full)
    equal = [c._replace(nulls_equal=True) for c in model]
    got = hj.key_hash2_host([key_column(c) for c in equal])
    assert np.array_equal(got, model_words(equal))
    first = [c.items[nulls[0]] for c in equal]
    assert first[0] is None and int(got[nulls[0]]) == mm3_final(mm3_mix(mm3_mix(mm3_mix(mm3_mix(0, M32), 5),
                                                                int.from_bytes(first[1][:4], "little")), first[1][4]), 16)


@pytest.mark.parametrize("key_mask", MASKS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025])
def test_plain_columns_hash_as_hj_key_hash_host(n, key_mask):
    """the compatibility property: no offsets, no validity, flags 0 -> the tuples of hj_key_hash_host, tuple for tuple.
    Both entry points run one body, so the tuples are also held to the header's wording, restated in keys_common.py"""
    rng = np.random.default_rng(1000 * n + (key_mask & 0xFF))
    for widths in MIXES:
        cols = [random_column(rng, w, n) for w in widths]
        old = hj.key_hash_host(cols if len(cols) > 1 else cols[0], key_mask=key_mask)
        assert np.array_equal(old, murmur3_words(key_words(cols), key_mask)), (widths, n, key_mask)
        assert np.array_equal(hj.key_hash2_host(cols if len(cols) > 1 else cols[0], key_mask=key_mask), old), (widths, n, key_mask)
        assert np.array_equal(hj.key_hash2_host([hj.KeyColumn(c) for c in cols], key_mask=key_mask), old)


def test_host_hash_reads_the_side_it_is_given():
    s = hj.KeyColumn.from_list([b"a", None, b"ccc"])
    r = hj.KeyColumn(np.ma.masked_array(np.arange(3, dtype=np.uint64), mask=[True, False, False]))
    s_vals, s_off, s_valid = s.take(0, 3)
    r_vals, _, r_valid = r.take(0, 3)
    out = np.zeros(3, dtype=np.uint64)

    def cols(width, **ptrs):
        arr = (_lib.hj_key_col2 * 1)()
        arr[0].width = width
        for k, a in ptrs.items():
            setattr(arr[0], k, a.ctypes.data)
        return arr

    # a variable-length S side and nothing on R's; a fixed R side and nothing on S's
    var = cols(0, s=s_vals, sOffsets=s_off, sValid=s_valid)
    assert hj.lib.hj_key_hash2_host(var, 1, hj.HJ_KEY_SIDE_S, 3, 0, out.ctypes.data) == _lib.HJ_OK
    assert np.array_equal(out, hj.key_hash2_host(s)) and int(out[1]) == mm3_final(mm3_mix(0x4E554C4C, 1), 4)
    assert hj.lib.hj_key_hash2_host(var, 1, hj.HJ_KEY_SIDE_R, 3, 0, out.ctypes.data) == _lib.HJ_ERR_INVALID
    fixed = cols(8, r=r_vals, rValid=r_valid)
    assert hj.lib.hj_key_hash2_host(fixed, 1, hj.HJ_KEY_SIDE_R, 3, 0, out.ctypes.data) == _lib.HJ_OK
    assert np.array_equal(out, hj.key_hash2_host(r)) and int(out[0]) == mm3_final(mm3_mix(0x4E554C4C, 0), 4)
    assert hj.lib.hj_key_hash2_host(fixed, 1, hj.HJ_KEY_SIDE_S, 3, 0, out.ctypes.data) == _lib.HJ_ERR_INVALID


# ---- argument errors -------------------------------------------------------------------------------------------------------
def test_host_hash_argument_errors():
    n = 32
    held, good_fixed, good_var, bad = _bad_columns(n)
    out = np.full(n, 0xABCD, dtype=np.uint64)

    def call(col, n_cols=1, side=0, n_rows=n, cols_null=False, out_ptr=out.ctypes.data):
        cols = _col2(n_cols, side == 0, side == 1, **col)
        return hj.lib.hj_key_hash2_host(None if cols_null else cols, n_cols, side, n_rows, 0, out_ptr)

    for good in (good_fixed, good_var):
        assert call(good) == _lib.HJ_OK and call(good, side=1) == _lib.HJ_OK and call(good, n_cols=4) == _lib.HJ_OK
    out[:] = 0xABCD
    for col in bad:
        assert call(col) == _lib.HJ_ERR_INVALID, col
        assert call(col, side=1) == _lib.HJ_ERR_INVALID, col
    for kw in (dict(n_cols=0), dict(n_cols=5), dict(cols_null=True), dict(side=2), dict(out_ptr=None), dict(n_rows=1 << 32)):
        assert call(good_fixed, **kw) == _lib.HJ_ERR_INVALID, kw
        assert call(good_var, **kw) == _lib.HJ_ERR_INVALID, kw
    assert np.all(out == 0xABCD), "a refused call wrote something"
    # offsets on the side that is not in use still make a fixed column invalid: the two sides agree in kind
    cols = _col2(1, True, False, **good_fixed)
    cols[0].rOffsets = held[1].ctypes.data
    assert hj.lib.hj_key_hash2_host(cols, 1, 0, n, 0, out.ctypes.data) == _lib.HJ_ERR_INVALID
    assert np.all(out == 0xABCD)
    # nRows 0 is a no-op that needs no pointers; the descriptors are still checked
    none = dict(ptr=0, off=0, valid=0, flags=0)
    assert call(dict(none, width=8), n_rows=0, out_ptr=None) == _lib.HJ_OK
    assert call(dict(none, width=0), n_rows=0, out_ptr=None) == _lib.HJ_OK
    assert call(dict(none, width=3), n_rows=0, out_ptr=None) == _lib.HJ_ERR_INVALID
    assert call(dict(none, width=8, flags=4), n_rows=0, out_ptr=None) == _lib.HJ_ERR_INVALID


def test_device_entry_points_refuse_a_null_context():
    """with and without arguments that would be fine: nothing is looked at before the context"""
    n = 16
    _, good_fixed, good_var, _ = _bad_columns(n)
    tuples, maps = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32)
    assert hj.lib.hj_key_hash2_dev(None, None, 0, 0, 0, 0, None) == _lib.HJ_ERR_INVALID
    assert hj.lib.hj_pairs_verify2_dev(None, None, None, 0, 0, 0, 0, None, 0, None, None, 0, None, None) == _lib.HJ_ERR_INVALID
    for good in (good_fixed, good_var):
        cols = _col2(1, True, True, **good)
        assert hj.lib.hj_key_hash2_dev(None, cols, 1, 0, n, 0, tuples.ctypes.data) == _lib.HJ_ERR_INVALID
        assert hj.lib.hj_pairs_verify2_dev(None, maps.ctypes.data, maps.ctypes.data, n, 0, n, n, cols, 1, None, None, 0,
                                           None, None) == _lib.HJ_ERR_INVALID


# ---- KeyColumn -------------------------------------------------------------------------------------------------------------
def test_key_column_constructors():
    c = hj.KeyColumn(np.arange(5, dtype=np.int32))
    assert (c.width, c.rows, len(c), c.offsets, c.valid, c.nulls_equal) == (4, 5, 5, None, None, False)
    c = hj.KeyColumn(np.arange(5, dtype=np.int64), valid=np.array([1, 0, 1, 1, 0], dtype=bool))
    assert c.width == 8 and c.valid.tolist() == [True, False, True, True, False]
    m = hj.KeyColumn(np.ma.masked_array(np.arange(5, dtype=np.int64), mask=[0, 1, 0, 0, 1]))
    assert m.valid.tolist() == c.valid.tolist() and np.array_equal(m.values, c.values)
    assert hj.KeyColumn(np.ma.masked_array(np.arange(5), mask=False)).valid.all()
    assert hj.KeyColumn(np.zeros(3, dtype=PAIR)).width == 16
    v = hj.KeyColumn.varlen([2, 2, 5, 5], b"..abc", valid=[True, True, False])
    assert (v.width, v.rows, v.offsets.dtype, v.offsets.tolist(), bytes(v.values)) == (0, 3, np.uint32, [2, 2, 5, 5], b"..abc")
    f = hj.KeyColumn.from_list([b"x", "yz", None, ""])
    assert (f.rows, f.offsets.tolist(), bytes(f.values), f.valid.tolist()) == (4, [0, 1, 3, 3, 3], b"xyz", [True, True, False, True])
    assert hj.KeyColumn.from_list([b"x"]).valid is None and hj.KeyColumn.from_list([]).rows == 0
    # a slice as the C ABI takes it: validity from bit 0, offsets from the slice's own first byte
    vals, off, words = f.take(1, 3)
    assert (bytes(vals), off.tolist(), off.dtype, words.tolist(), words.dtype) == (b"yz", [0, 2, 2, 2], np.uint32, [0b101], np.uint32)
    big = hj.KeyColumn(np.arange(100, dtype=np.uint16), valid=np.arange(100) % 3 != 0)
    vals, off, words = big.take(33, 40)
    assert off is None and vals.tolist() == list(range(33, 73)) and words.size == 2
    assert [(int(words[i >> 5]) >> (i & 31)) & 1 for i in range(40)] == [int((33 + i) % 3 != 0) for i in range(40)]
    assert int(words[1]) >> 8 == 0, "the bits behind the slice are 0"


def test_key_column_validation():
    bad = [lambda: hj.KeyColumn(np.zeros((2, 2), dtype=np.uint32)),
           lambda: hj.KeyColumn(np.zeros(4, dtype="S3")),
           lambda: hj.KeyColumn(np.zeros(4, dtype="S32")),
           lambda: hj.KeyColumn(np.array(["a", None], dtype=object)),
           lambda: hj.KeyColumn(np.zeros(4, dtype=np.uint32), valid=np.ones(3, dtype=bool)),          # lengths disagree
           lambda: hj.KeyColumn(np.zeros(4, dtype=np.uint32), valid=np.ones(4, dtype=np.uint8)),      # not bools
           lambda: hj.KeyColumn(np.ma.masked_array(np.zeros(4), mask=False), valid=np.ones(4, dtype=bool)),
           lambda: hj.KeyColumn.varlen([0, 3, 2], b"abc"),                                            # decreasing
           lambda: hj.KeyColumn.varlen([-1, 1], b"abc"),
           lambda: hj.KeyColumn.varlen([0, 2, 4], b"abc"),                                            # ends behind the data
           lambda: hj.KeyColumn.varlen([], b"abc"),
           lambda: hj.KeyColumn.varlen([[0, 1]], b"abc"),
           lambda: hj.KeyColumn.varlen([0.0, 1.0], b"abc"),
           lambda: hj.KeyColumn.varlen([0, 1], np.zeros(4, dtype=np.uint16)),
           lambda: hj.KeyColumn.varlen([0, 1, 2], b"abc", valid=[True]),                              # lengths disagree
           lambda: hj.KeyColumn.varlen([0, 1], np.lib.stride_tricks.as_strided(np.zeros(1, dtype=np.uint8), (1 << 32,), (0,))),
           lambda: hj.KeyColumn.from_list([b"a", 3])]
    for k, make in enumerate(bad):
        with pytest.raises(ValueError):
            make()
            pytest.fail(f"case {k} was accepted")
    assert hj.KeyColumn.varlen([0, 3], b"abc").rows == 1 and hj.KeyColumn.varlen([3], b"abc").rows == 0


# ---- join_on_columns without a device ----------------------------------------------------------------------------------------
R8 = np.arange(1, 9, dtype=np.uint64) << np.uint64(33)
S5 = np.arange(3, 8, dtype=np.uint64) << np.uint64(33)
STR8, STR5 = [b"k%d" % i for i in range(8)], [b"k%d" % i for i in range(3, 8)]


def test_python_surface():
    C = hj.HashJoinContext
    assert list(inspect.signature(C.key_hash2).parameters) == ["self", "cols", "side", "n_rows", "d_out", "key_mask"]
    assert list(inspect.signature(C.pairs_verify2).parameters) == list(inspect.signature(C.pairs_verify).parameters)
    params = inspect.signature(hj.key_hash2_host).parameters
    assert list(params) == ["cols", "key_mask"] and params["key_mask"].default == 0
    params = inspect.signature(hj.join_on_columns).parameters
    assert list(params) == ["r_keys", "s_keys", "r_cols", "s_cols", "how", "nulls_equal", "radixBits", "slice_tuples", "device", "key_mask"]
    assert [params[k].default for k in list(params)[2:]] == [None, None, "inner", False, 0, None, 0, 0]
    assert list(inspect.signature(hj.KeyColumn.__init__).parameters)[:3] == ["self", "values", "valid"]
    assert list(inspect.signature(hj.KeyColumn.varlen).parameters)[:3] == ["offsets", "data", "valid"]
    assert list(inspect.signature(hj.KeyColumn.from_list).parameters)[:1] == ["items"]
    for f in (C.key_hash2, C.pairs_verify2, hj.key_hash2_host, hj.join_on_columns, hj.KeyColumn):
        assert f.__doc__
    # join_on is what it was
    params = inspect.signature(hj.join_on).parameters
    assert list(params) == ["r_keys", "s_keys", "r_cols", "s_cols", "how", "radixBits", "slice_tuples", "device", "key_mask"]


@pytest.mark.parametrize("how", ["outer", "right_outer", "cross", "", None, 1, ["inner"]])
def test_an_unknown_how_is_refused_before_any_device_call(how):
    for R in (R8, R8[:0], hj.KeyColumn.from_list(STR8)):
        with pytest.raises(ValueError):
            hj.join_on_columns(R, S5 if isinstance(R, np.ndarray) else hj.KeyColumn.from_list(STR5), how=how)


@pytest.mark.parametrize("how", ["inner", "right_anti"])
def test_bad_keys_are_refused_before_any_device_call(how):
    r32, s32 = np.arange(8, dtype=np.uint32), np.arange(5, dtype=np.uint32)
    r_str, s_str = hj.KeyColumn.from_list(STR8), hj.KeyColumn.from_list(STR5)
    bad = [(R8, s32),                                                          # mismatched itemsizes
           (r_str, S5), (R8, s_str),                                           # variable-length against fixed
           ([R8, r_str], [S5, s32]),                                           # ... in the second column
           ([R8, r32], S5),                                                    # two columns against one
           (np.zeros(8, dtype="S3"), np.zeros(5, dtype="S3")),                 # a 3-byte key
           ([R8] * 5, [S5] * 5), ([r_str] * 5, [s_str] * 5),                   # five key columns
           ([], []),                                                           # none
           ([R8, hj.KeyColumn.from_list(STR8[:7])], [S5, s_str]),              # ragged lengths on R
           ([r_str, r32], [s_str, s32[:4]]),                                   # ... on S
           (R8.reshape(4, 2), S5)]                                             # a 2-D key
    for r_keys, s_keys in bad:
        with pytest.raises(ValueError):
            hj.join_on_columns(r_keys, s_keys, how=how)
    for kw in (dict(key_mask=-1), dict(key_mask=1 << 32), dict(slice_tuples=-3),
               dict(r_cols={"x": np.zeros(7)}), dict(s_cols={"x": np.zeros(5, dtype="S3")})):
        with pytest.raises(ValueError):
            hj.join_on_columns(r_str, s_str, how=how, **kw)


@pytest.mark.parametrize("kind", ["nullable", "string", "composite"])
@pytest.mark.parametrize("how", HOWS)
def test_empty_inputs_need_no_device(how, kind):
    """no S: no probe row, every R row unmatched. No R: every S tuple unmatched, no R-only row -- NULL-keyed or not"""
    r_cols = {"w1": np.arange(10, 18, dtype=np.uint8)}
    s_cols = {"w2": np.arange(20, 25, dtype=np.int16), "w8": np.arange(5, dtype=np.float64) - 2.5}
    keeps_s = how in ("left", "anti", "full")
    keeps_r = how in ("right", "full", "right_anti")

    def keys(k, strs, n):
        nullable = hj.KeyColumn(k[:n], valid=np.arange(n) % 2 == 0)
        string = hj.KeyColumn.from_list([None if i == 1 else s for i, s in enumerate(strs[:n])])
        return {"nullable": nullable, "string": string, "composite": [np.ma.masked_array(k[:n], mask=np.arange(n) == 0), string]}[kind]

    def check(out, rows_s, rows_r):
        assert set(out) == {"s_idx", "r_idx", "s", "r", "s_valid", "r_valid"}
        for side, plane, rows, cols in (("s", how in S_PLANE, rows_s, s_cols), ("r", how in R_PLANE, rows_r, r_cols)):
            idx, got, valid = out[side + "_idx"], out[side], out[side + "_valid"]
            if not plane:
                assert idx is None and got is None and valid is None, (how, side)
                continue
            rows = np.asarray(rows, dtype=np.int64)
            assert idx.dtype == np.uint32 and np.array_equal(idx, np.where(rows < 0, hj.NO_ROW, rows).astype(np.uint32)), (how, side)
            assert valid.dtype == np.bool_ and np.array_equal(valid, rows >= 0), (how, side)
            for name, col in cols.items():
                want = np.zeros(rows.size, dtype=col.dtype)
                want[rows >= 0] = col[rows[rows >= 0]]
                assert got[name].dtype == col.dtype and got[name].tobytes() == want.tobytes(), (how, side, name)

    kw = dict(how=how, slice_tuples=2)
    for nulls_equal in (False, True):
        check(hj.join_on_columns(keys(R8, STR8, 8), keys(S5, STR5, 0), r_cols=r_cols, s_cols={k: v[:0] for k, v in s_cols.items()},
                                 nulls_equal=nulls_equal, **kw), [-1] * 8 if keeps_r else [], list(range(8)) if keeps_r else [])
        check(hj.join_on_columns(keys(R8, STR8, 0), keys(S5, STR5, 5), r_cols={k: v[:0] for k, v in r_cols.items()}, s_cols=s_cols,
                                 nulls_equal=nulls_equal, **kw), list(range(5)) if keeps_s else [], [-1] * 5 if keeps_s else [])
        check(hj.join_on_columns(keys(R8, STR8, 0), keys(S5, STR5, 0), r_cols={k: v[:0] for k, v in r_cols.items()},
                                 s_cols={k: v[:0] for k, v in s_cols.items()}, how=how, nulls_equal=nulls_equal), [], [])
