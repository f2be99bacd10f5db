"""hj_window_frames_dev and its family without a GPU: the declarations, the layout function and its workspace bound, every
refusal on the host twin with its outputs untouched, the host twin (a running window and a deque) against the model of
frames_common (cumulative sums and slices) at small sizes, the block rule of hj_frames.hip against brute force, and
window_rows_host with the framed specs against a per-partition Python loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

import frames_common as fc
from frames_common import BESIDE, FRAMED, framed_call, framed_check
import window_common as wc
from window_common import wrapper_table

U32, U64 = np.uint32, np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "htm_hashjoin.h")).read()
SYMBOLS = ("hj_window_frames_dev", "hj_window_frames_info", "hj_window_frames_host", "hj_frames_layout_info")
T, L = fc.layout(1)[:2]
A = _lib
FAR = fc.FAR
# the frames every size meets: trailing, leading, centred, clear of the row, single positions, each unbounded side, the widest
FRAMES = ([(-6, 0), (0, 6), (-3, 3), (-5, -3), (3, 5), (0, 0), (-1, -1), (1, 1), (-63, 0), (0, 64), (-64, 64), (-999, 0), (-1000, 1000),
           (-(L + 1), -(L + 1)), (-FAR, FAR), (-FAR, 0), (0, FAR)]
          + [(None, 0), (None, 1), (None, -1), (None, L + 1), (0, None), (1, None), (-1, None), (-(L + 1), None), (None, None)])


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_declarations_and_struct_size():
    for name in SYMBOLS:
        assert name in lib._hj_signatures and re.search(r"\bint\s+%s\s*\(" % name, HEADER), name
    size = int(re.search(r"\}\s*hj_frame_func;\s*/\*\s*(\d+) bytes\s*\*/", HEADER).group(1))
    assert C.sizeof(_lib.hj_frame_func) == size == 56
    assert _lib.HJ_FRAME_MAX_FUNCS == 8 and re.search(r"#define\s+HJ_FRAME_MAX_FUNCS\s+8\b", HEADER)
    for name in ("HJ_FRAME_UNBOUNDED_LO", "HJ_FRAME_UNBOUNDED_HI"):
        assert re.search(r"#define\s+%s\s+0x%xu" % (name, getattr(_lib, name)), HEADER), name
    assert len({_lib.HJ_AGG_SIGNED, _lib.HJ_FRAME_UNBOUNDED_LO, _lib.HJ_FRAME_UNBOUNDED_HI}) == 3
    assert lib.hj_abi_version() == 4                         # additive
    assert C.sizeof(_lib.hj_win_func) == 40                  # the window's own struct is as it was
    for fn in (hj.window_rows, hj.window_rows_host, hj.frames_layout_info, hj.HashJoinContext.window_frames, hj.HashJoinContext.window_frames_info):
        assert fn.__doc__


def test_layout_is_a_pure_function_within_its_bound():
    out = (C.c_uint64 * 4)()
    assert lib.hj_frames_layout_info((1 << 32) - 1, out) == _lib.HJ_ERR_INVALID and lib.hj_frames_layout_info(5, None) == _lib.HJ_ERR_INVALID
    last = 0
    for n in [0, 1, T, L, L + 1, 1 << 17, 1 << 20, (1 << 23) + 1, 1 << 24, (1 << 24) + 1, 1 << 27, (1 << 30) + 12345, (1 << 32) - 2]:
        tile, chunk, chunks, nbytes = fc.layout(n)
        assert fc.layout(n) == (tile, chunk, chunks, nbytes)
        assert (tile, chunk, chunks) == wc.layout(n)[:3]                    # the window's own tiles and chunks
        assert tile == T and chunk % tile == 0 and chunk >= L and chunks <= 4096 and chunks == -(-n // chunk)
        # what the header promises: at most 32 bytes per position plus the chunk summaries (a constant), whatever nFuncs; and
        # what the method needs: the head byte, the end, two 8-byte planes
        assert last <= nbytes <= 32 * n + (1 << 20) and nbytes >= 21 * n
        last = nbytes
    assert "32 bytes" in HEADER and "per position plus 1 MiB" in HEADER
    assert hj.frames_layout_info(L + 1) == {"tile": T, "chunk": L, "chunks": 2, "workspace_bytes": fc.layout(L + 1)[3]}


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _good():
    """a small call every refusal departs from: raw ctypes, so that every field can be broken"""
    n = 40
    rng = np.random.default_rng(0)
    a = {"n_pos": n, "n_rows": n, "perm": rng.permutation(n).astype(U32), "part": rng.integers(0, 3, n).astype(U32),
         "plane": np.full(2, 0xFFFFFFFF, dtype=U32), "src": rng.integers(0, 9, n).astype(np.int64),
         "out0": np.full(n + 2, fc.SENT64, dtype=U64), "out1": np.full(n + 2, fc.SENT64, dtype=U64)}
    a["funcs"] = (_lib.hj_frame_func * 9)()
    f0, f1 = a["funcs"][0], a["funcs"][1]
    f0.out, f0.op, f0.lo, f0.hi = a["out0"].ctypes.data, A.HJ_AGG_COUNT, -2, 0
    f1.src, f1.srcValid, f1.out = a["src"].ctypes.data, a["plane"].ctypes.data, a["out1"].ctypes.data
    f1.op, f1.width, f1.flags, f1.lo, f1.hi = A.HJ_AGG_SUM, 8, _lib.HJ_AGG_SIGNED | _lib.HJ_FRAME_UNBOUNDED_LO, 0, 3
    a["n_funcs"] = 2
    return a


def _call(a, out=None):
    return lib.hj_window_frames_host(a["perm"].ctypes.data if a["perm"] is not None else None, a["n_pos"], a["n_rows"],
                                     a["part"].ctypes.data if a["part"] is not None else None, a["funcs"], a["n_funcs"], out)


def _set(path, value):
    def brk(a):
        obj = a
        for key in path[:-1]:
            obj = obj[key]
        if isinstance(obj, dict):
            obj[path[-1]] = value
        else:
            setattr(obj, path[-1], value)
    return brk


def _odd(i, field, by):
    def brk(a):
        setattr(a["funcs"][i], field, getattr(a["funcs"][i], field) + by)
    return brk


def _plane_odd(which):
    def brk(a):
        raw = np.zeros(4 * a["n_rows"] + 8, dtype=np.uint8)
        a[which] = raw[2:]                                    # ctypes.data is 2 off a word
    return brk


def _frame(i, lo, hi, flags=None):
    def brk(a):
        f = a["funcs"][i]
        f.lo, f.hi = lo, hi
        if flags is not None:
            f.flags = flags
    return brk


REFUSALS = {
    "nFuncs 0": _set(("n_funcs",), 0),
    "nFuncs above the maximum": _set(("n_funcs",), 9),
    "funcs NULL": _set(("funcs",), None),
    "op above MAX": _set(("funcs", 0, "op"), 4),
    "a window op": _set(("funcs", 0, "op"), _lib.HJ_WIN_RUN_SUM),
    "SUM of width 0": _set(("funcs", 1, "width"), 0),
    "SUM of width 2": _set(("funcs", 1, "width"), 2),
    "COUNT of width 2": _set(("funcs", 0, "width"), 2),
    "an unknown flag": _set(("funcs", 0, "flags"), 8),
    "reserved": _set(("funcs", 0, "reserved"), 1),
    "lo above hi": _frame(0, 1, 0),
    "lo above hi, both preceding": _frame(0, -2, -3),
    "lo below the range": _frame(0, -(1 << 32), 0),
    "hi above the range": _frame(0, 0, 1 << 32),
    "lo above the range": _frame(0, 1 << 32, 1 << 32),
    "an offset beside UNBOUNDED_LO": _frame(1, -1, 3),
    "an offset beside UNBOUNDED_HI": _frame(0, 0, 1, _lib.HJ_FRAME_UNBOUNDED_HI),
    "offsets beside both flags": _frame(0, -1, 1, _lib.HJ_FRAME_UNBOUNDED_LO | _lib.HJ_FRAME_UNBOUNDED_HI),
    "out NULL": _set(("funcs", 0, "out"), None),
    "out aligned to 4 only": _odd(1, "out", 4),
    "src NULL": _set(("funcs", 1, "src"), None),
    "src misaligned": _odd(1, "src", 4),
    "srcValid misaligned": _odd(1, "srcValid", 2),
    "dPerm NULL with nPos above nRows": lambda a: a.update(perm=None, n_rows=a["n_rows"] - 1),
    "dPerm misaligned": _plane_odd("perm"),
    "dPart misaligned": _plane_odd("part"),
    "nPos too large": _set(("n_pos",), (1 << 32) - 1),
    "nRows too large": _set(("n_rows",), (1 << 32) - 1),
}


def test_the_good_call_is_good():
    a = _good()
    out = (C.c_uint64 * 8)()
    assert _call(a, out) == _lib.HJ_OK and out[0] == 40 and out[2] == 0 and out[3] == 0 and out[7] == 0
    for o in (a["out0"], a["out1"]):
        assert (o[40:] == fc.SENT64).all() and (o[:40] != fc.SENT64).all()
    assert _call(a, None) == _lib.HJ_OK                      # out may be NULL
    b = _good()
    b["n_pos"] = 0                                            # no position: nothing is written
    assert _call(b, out) == _lib.HJ_OK and list(out) == [0] * 8
    assert (b["out0"] == fc.SENT64).all() and (b["out1"] == fc.SENT64).all()
    # the ends of the offsets' range, and an unbounded side with the other one on the far side of the row
    for lo, hi, flags in ((-FAR, FAR, 0), (FAR, FAR, 0), (-FAR, -FAR, 0), (0, -5, _lib.HJ_FRAME_UNBOUNDED_LO), (5, 0, _lib.HJ_FRAME_UNBOUNDED_HI),
                          (0, 0, _lib.HJ_FRAME_UNBOUNDED_LO | _lib.HJ_FRAME_UNBOUNDED_HI)):
        c = _good()
        _frame(0, lo, hi, flags)(c)
        assert _call(c) == _lib.HJ_OK, (lo, hi, flags)


def test_count_widths_and_a_src_that_is_not_read():
    a = _good()
    f = a["funcs"][1]
    f.op, f.flags = A.HJ_AGG_COUNT, 0
    for width in (0, 4, 8):
        f.width = width
        f.src = None                                         # COUNT reads no value
        assert _call(a) == _lib.HJ_OK, width
    b = _good()
    b["n_rows"], b["n_pos"] = 0, 0
    b["funcs"][1].src = None                                 # nRows 0: no src is read
    assert _call(b) == _lib.HJ_OK


@pytest.mark.parametrize("cause", sorted(REFUSALS))
def test_refusals_write_nothing(cause):
    a = _good()
    REFUSALS[cause](a)
    out = (C.c_uint64 * 8)(*([wc.SENT32] * 8))
    assert _call(a, out) == _lib.HJ_ERR_INVALID, cause
    assert list(out) == [wc.SENT32] * 8, cause
    assert (a["out0"] == fc.SENT64).all() and (a["out1"] == fc.SENT64).all(), (cause, "a refused call wrote")


def test_null_context():
    a = _good()
    out = (C.c_uint64 * 8)(*([wc.SENT32] * 8))
    assert lib.hj_window_frames_dev(None, a["perm"].ctypes.data, 40, 40, a["part"].ctypes.data, a["funcs"], 2) == _lib.HJ_ERR_INVALID
    assert lib.hj_window_frames_info(None, out) == _lib.HJ_ERR_INVALID and list(out) == [wc.SENT32] * 8


# ---- the host twin against the model ---------------------------------------------------------------------------------------------------
def check_host(case, tag):
    want, counts = fc.model(case)
    got, info = fc.host_call(case, np.random.default_rng(case.n_pos))
    fc.same(got, want, tag)
    fc.check_info(info, case, counts, tag)
    assert info[3] == 0


SHAPES = ("one", "each", "fixed2", "fixed3", "fixed6", "fixed7", "fixed8", "fixed63", "fixed64", "fixed65", "geometric", "seams")


@pytest.mark.parametrize("shape", SHAPES)
def test_host_twin_against_the_model(shape):
    """every frame of the list at n in (1, 2, 65, 1000), every frame on two source types"""
    for i, n in enumerate((1, 2, 65, 1000)):
        for k in range(0, len(FRAMES), 4):
            case = fc.build(n, fc.rotate(FRAMES, k), shape, perm=("random", "identity", None)[(i + k) % 3], seed=i + k, null_pct=(0, 10, 100)[k // 4 % 3])
            check_host(case, (shape, n, k))


def test_host_holes_extra_rows_and_unsorted_runs():
    rng = np.random.default_rng(9)
    for k in range(0, len(FRAMES), 8):
        check_host(fc.build(2000, fc.rotate(FRAMES, k), "geometric", holes=40, extra_rows=17, seed=4), ("holes", k))
        check_host(fc.build(100, fc.rotate(FRAMES, k), "one", holes=3, seed=5), ("holes in one partition", k))
        n = 3000
        perm = rng.permutation(n + 50).astype(U32)           # unsorted: many runs of one and two positions
        part = rng.integers(0, 2, n + 50).astype(U32)
        check_host(fc.Case(n, n + 50, perm, part, fc.build(n + 50, fc.rotate(FRAMES, k), "one", perm=None).funcs), ("random runs", k))
    funcs = [fc.Func(A.HJ_AGG_COUNT, -1, 1), fc.Func(A.HJ_AGG_COUNT, None, None)]
    case = fc.Case(10, 4, np.array([4, 5, fc.NO_ROW] * 3 + [9], dtype=U32), None, funcs)
    check_host(case, "all skipped")
    assert fc.host_call(case)[1][:5] == [10, 0, 0, 0, 10]


def test_host_values_by_hand():
    v = np.array([5, -2, 7, 1, 4, 9], dtype=np.int32)
    part = np.array([0, 0, 0, 1, 1, 1], dtype=U32)
    frames = [(A.HJ_AGG_SUM, -1, 0), (A.HJ_AGG_MAX, None, None), (A.HJ_AGG_MIN, -3, -1), (A.HJ_AGG_COUNT, -1, 1), (A.HJ_AGG_SUM, 1, None)]
    got, _ = fc.host_call(fc.Case(6, 6, None, part, [fc.Func(op, lo, hi, v) for op, lo, hi in frames]))
    assert got[0].view(np.int64).tolist() == [5, 3, 5, 1, 5, 13] and got[1].view(np.int64).tolist() == [7, 7, 7, 9, 9, 9]
    assert got[2].view(np.int64).tolist() == [(1 << 63) - 1, 5, -2, (1 << 63) - 1, 1, 1]
    assert got[3].tolist() == [2, 3, 2, 2, 3, 2] and got[4].view(np.int64).tolist() == [5, 7, 0, 13, 9, 0]


def test_the_block_rule_against_brute_force():
    """G, H and the combine step as hj_frames.hip's header comment states them, over 3000 random cases: partitions, frames on
    either side of p, empty frames, unbounded sides"""
    assert fc.block_rule_check(np.random.default_rng(2024), 3000) == 0


# ---- the wrapper against a per-partition loop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("null_keys", ["group", "drop"])
@pytest.mark.parametrize("keys", ["both", "string", "integer"])
def test_window_rows_host_framed_against_a_loop(keys, null_keys):
    for seed, n in enumerate((1, 7, 400)):
        t = wrapper_table(n, seed)
        t["u"] = t["u"] >> np.uint64(8)                     # sums of a few stay inside 64 bits: the loop's mean is the wrapper's
        got = framed_call(hj.window_rows_host, t, null_keys, keys)
        framed_check(got, t, null_keys, keys)
        wc_like = hj.window_rows_host(BESIDE, partition_by=[hj.KeyColumn.from_list(t["names"]), hj.KeyColumn(t["num"], t["num_valid"])],
                                      order_by=[hj.KeyColumn(t["o1"], t["o1_valid"]), t["o2"]], descending=[True, False], nulls=["first", "last"],
                                      cols={"w": hj.KeyColumn.from_list(t["words"]), "v": hj.KeyColumn(t["v"], t["v_valid"])}, null_keys=null_keys)
        if keys == "both":                                   # the old specs beside the new ones mean what they meant
            for name in BESIDE:
                a, b = got[name], wc_like[name]
                assert (a.to_list() == b.to_list()) if isinstance(a, hj.KeyColumn) else np.array_equal(a, b), name


def test_framed_specs_alone_and_the_sum_that_wraps():
    v = np.array([5, -2, 7, 1], dtype=np.int32)
    got = hj.window_rows_host({"s": ("sum", "v", -1, 0), "m": ("mean", "v", None, None), "c": ("count", None, 0, 1)}, cols={"v": v})
    assert got["s"].values.tolist() == [5, 3, 5, 8] and got["m"].values.tolist() == [2.75] * 4 and got["c"].tolist() == [2, 2, 2, 1]
    assert got["perm"].tolist() == [0, 1, 2, 3] and got["n_partitions"] == 1 and got["c"].dtype == U64
    u = np.array([(1 << 64) - 1, 3], dtype=U64)
    got = hj.window_rows_host({"s": ("sum", "u", None, None), "m": ("mean", "u", None, None)}, cols={"u": u})
    assert got["s"].values.tolist() == [2, 2] and got["m"].values.tolist() == [1.0, 1.0]      # the mean of the wrapped sum


def test_wrapper_arguments():
    a = np.arange(4, dtype=np.int32)
    for fn in (hj.window_rows, hj.window_rows_host):
        with pytest.raises(ValueError, match="exist$"):
            fn({"x": "median"}, partition_by=a)
        with pytest.raises(ValueError, match=r"'mean', column, lo, hi.*exist$"):
            fn({"x": ("sum", "v", 1)}, partition_by=a, cols={"v": a})
        with pytest.raises(ValueError, match="exist$"):
            fn({"x": ("cumsum", "v", -1, 0)}, partition_by=a, cols={"v": a})
        with pytest.raises(ValueError, match="in front of its start"):
            fn({"x": ("sum", "v", 1, 0)}, partition_by=a, cols={"v": a})
        with pytest.raises(ValueError, match="ends of a frame"):
            fn({"x": ("sum", "v", -(1 << 32), 0)}, partition_by=a, cols={"v": a})
        with pytest.raises(ValueError, match="ends of a frame"):
            fn({"x": ("max", "v", 0.5, 1)}, partition_by=a, cols={"v": a})
        with pytest.raises(ValueError, match="ends of a frame"):
            fn({"x": ("count", None, True, 1)}, partition_by=a)
        with pytest.raises(ValueError, match="does not hold"):
            fn({"x": ("sum", "w", -1, 0)}, partition_by=a, cols={"v": a})
        with pytest.raises(ValueError, match="does not hold"):
            fn({"x": ("mean", None, -1, 0)}, partition_by=a, cols={"v": a})
        with pytest.raises(ValueError, match="running sums"):
            fn({"x": ("mean", "v", -1, 0)}, partition_by=a, cols={"v": a.astype(np.float64)})
        # an empty table is answered without a device
        e = np.empty(0, dtype=np.int64)
        got = fn({"s": ("sum", "v", -1, 0), "c": ("count", None, None, None), "m": ("mean", "v", 0, 0), "rn": "row_number"}, partition_by=e, order_by=e, cols={"v": e})
        assert got["s"].rows == 0 and got["c"].size == 0 and got["c"].dtype == U64 and got["m"].rows == 0 and got["m"].values.dtype == np.float64
        assert got["perm"].size == 0 and (got["n_partitions"], got["null_rows"]) == (0, 0)
