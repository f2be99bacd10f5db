"""hj_window_rows_dev and its family without a GPU: the declarations, the layout function, every refusal on the host twin
with its outputs untouched, the host twin against the model of window_common at small sizes, and window_rows_host against a
per-partition Python loop."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

import sort_common as sc
import window_common as wc
from window_common import wrapper_call, wrapper_check, wrapper_table

U32, U64 = np.uint32, np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "htm_hashjoin.h")).read()
SYMBOLS = ("hj_window_rows_dev", "hj_window_rows_info", "hj_window_rows_host", "hj_window_layout_info")
T, L = wc.layout(1)[:2]
W = _lib


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_declarations_and_struct_size():
    for name in SYMBOLS:
        assert name in lib._hj_signatures and re.search(r"\bint\s+%s\s*\(" % name, HEADER), name
    assert C.sizeof(_lib.hj_win_func) == 40 and "/* 40 bytes */" in HEADER
    assert _lib.HJ_WIN_MAX_FUNCS == 8 and re.search(r"#define\s+HJ_WIN_MAX_FUNCS\s+8\b", HEADER)
    names = ("ROW_NUMBER", "RANK", "DENSE_RANK", "PART_ROWS", "LAG", "LEAD", "FIRST_ROW", "LAST_ROW", "RUN_COUNT", "RUN_SUM", "RUN_MIN", "RUN_MAX")
    for value, name in enumerate(names):
        assert getattr(_lib, "HJ_WIN_" + name) == value and re.search(r"HJ_WIN_%s\s*=\s*%d\b" % (name, value), HEADER), name
    assert lib.hj_abi_version() == 4                         # additive
    for fn in (hj.window_rows, hj.window_rows_host, hj.window_layout_info, hj.HashJoinContext.window_rows, hj.HashJoinContext.window_rows_info):
        assert fn.__doc__


def test_layout_is_a_pure_function():
    out = (C.c_uint64 * 4)()
    assert lib.hj_window_layout_info((1 << 32) - 1, out) == _lib.HJ_ERR_INVALID and lib.hj_window_layout_info(5, None) == _lib.HJ_ERR_INVALID
    last = 0
    for n in [0, 1, T, L, L + 1, 1 << 17, 1 << 20, (1 << 23) + 1, 1 << 24, (1 << 24) + 1, 1 << 27, (1 << 30) + 12345, (1 << 32) - 2]:
        tile, chunk, chunks, nbytes = wc.layout(n)
        assert wc.layout(n) == (tile, chunk, chunks, nbytes)
        assert tile == T and chunk % tile == 0 and chunk >= L and chunks <= 4096 and chunks == -(-n // chunk)
        assert nbytes >= last and nbytes >= 5 * n
        last = nbytes
    assert hj.window_layout_info(L + 1) == {"tile": T, "chunk": L, "chunks": 2, "workspace_bytes": wc.layout(L + 1)[3]}


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _good():
    """a small call every refusal departs from: raw ctypes, so that every field can be broken"""
    n = 40
    rng = np.random.default_rng(0)
    a = {"n_pos": n, "n_rows": n, "perm": rng.permutation(n).astype(U32), "part": rng.integers(0, 3, n).astype(U32),
         "key": rng.integers(0, 5, n).astype(np.int32), "plane": np.full(2, 0xFFFFFFFF, dtype=U32), "src": rng.integers(0, 9, n).astype(np.int64),
         "out32": np.full(n + 2, wc.SENT32, dtype=U32), "out64": np.full(n + 2, wc.SENT64, dtype=U64)}
    a["order"] = (_lib.hj_sort_col * 1)()
    o = a["order"][0]
    o.values, o.valid, o.width, o.type = a["key"].ctypes.data, a["plane"].ctypes.data, 4, _lib.HJ_VAL_INT
    a["funcs"] = (_lib.hj_win_func * 9)()
    f0, f1 = a["funcs"][0], a["funcs"][1]
    f0.out, f0.op, f0.offset = a["out32"].ctypes.data, W.HJ_WIN_LAG, 1
    f1.src, f1.srcValid, f1.out = a["src"].ctypes.data, a["plane"].ctypes.data, a["out64"].ctypes.data
    f1.op, f1.width, f1.flags = W.HJ_WIN_RUN_SUM, 8, _lib.HJ_AGG_SIGNED
    a["n_order"], a["n_funcs"] = 1, 2
    return a


def _call(a, out=None):
    return lib.hj_window_rows_host(a["perm"].ctypes.data if a["perm"] is not None else None, a["n_pos"], a["n_rows"],
                                   a["part"].ctypes.data if a["part"] is not None else None, a["order"], a["n_order"], a["funcs"], a["n_funcs"], out)


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


def _odd(name, by):
    """the pointer of a["funcs"][i].<field> / a["order"][0].<field> moved off its alignment"""
    def brk(a):
        obj = a[name[0]][name[1]]
        setattr(obj, name[2], getattr(obj, name[2]) + by)
    return brk


def _plane_odd(which):
    def brk(a):
        raw = np.zeros(4 * a["n_rows"] + 8, dtype=np.uint8)
        a[which] = raw[2:]                                    # ctypes.data is 2 off a word
    return brk


REFUSALS = {
    "nFuncs 0": _set(("n_funcs",), 0),
    "nFuncs above the maximum": _set(("n_funcs",), 9),
    "funcs NULL": _set(("funcs",), None),
    "op above RUN_MAX": _set(("funcs", 0, "op"), 12),
    "a width on a numbering op": _set(("funcs", 0, "width"), 4),
    "RUN_SUM of width 0": _set(("funcs", 1, "width"), 0),
    "RUN_SUM of width 2": _set(("funcs", 1, "width"), 2),
    "flags on a row map": _set(("funcs", 0, "flags"), _lib.HJ_AGG_SIGNED),
    "an unknown flag": _set(("funcs", 1, "flags"), 2),
    "an offset on RUN_SUM": _set(("funcs", 1, "offset"), 1),
    "out NULL": _set(("funcs", 0, "out"), None),
    "out32 misaligned": _odd(("funcs", 0, "out"), 2),
    "out64 aligned to 4 only": _odd(("funcs", 1, "out"), 4),
    "src NULL": _set(("funcs", 1, "src"), None),
    "src misaligned": _odd(("funcs", 1, "src"), 4),
    "srcValid misaligned": _odd(("funcs", 1, "srcValid"), 2),
    "nOrder above the maximum": _set(("n_order",), 5),
    "order NULL": _set(("order",), None),
    "order type": _set(("order", 0, "type"), 3),
    "order width": _set(("order", 0, "width"), 3),
    "order flags": _set(("order", 0, "flags"), 4),
    "order reserved": _set(("order", 0, "reserved"), 1),
    "order values NULL": _set(("order", 0, "values"), None),
    "order values misaligned": _odd(("order", 0, "values"), 2),
    "order valid misaligned": _odd(("order", 0, "valid"), 1),
    "dPerm NULL with nPos above nRows": lambda a: a.update(perm=None, n_rows=a["n_rows"] - 1),
    "dPerm misaligned": _plane_odd("perm"),
    "dPart misaligned": _plane_odd("part"),
    "nPos too large": _set(("n_pos",), (1 << 32) - 1),
    "nRows too large": _set(("n_rows",), (1 << 32) - 1),
}


def test_the_good_call_is_good():
    a = _good()
    out = (C.c_uint64 * 8)()
    assert _call(a, out) == _lib.HJ_OK and out[0] == 40 and out[3] == 0 and out[7] == 0
    assert (a["out32"][40:] == wc.SENT32).all() and (a["out64"][40:] == wc.SENT64).all() and (a["out64"][:40] != wc.SENT64).all()
    assert _call(a, None) == _lib.HJ_OK                      # out may be NULL
    b = _good()
    b["n_pos"] = 0                                            # no position: nothing is written
    assert _call(b, out) == _lib.HJ_OK and list(out) == [0] * 8
    assert (b["out32"] == wc.SENT32).all() and (b["out64"] == wc.SENT64).all()


def test_count_widths_and_a_src_that_is_not_read():
    a = _good()
    f = a["funcs"][1]
    f.op, f.flags = W.HJ_WIN_RUN_COUNT, 0
    for width in (0, 4, 8):
        f.width = width
        f.src = None                                         # RUN_COUNT reads no value
        assert _call(a) == _lib.HJ_OK, width
    f.width = 2
    assert _call(a) == _lib.HJ_ERR_INVALID
    b = _good()
    b["n_rows"], b["n_pos"] = 0, 0
    b["funcs"][1].src = None                                 # nRows 0: no src is read
    b["order"][0].values = None
    assert _call(b) == _lib.HJ_OK


@pytest.mark.parametrize("cause", sorted(REFUSALS))
def test_refusals_write_nothing(cause):
    a = _good()
    REFUSALS[cause](a)
    out = (C.c_uint64 * 8)(*([wc.SENT32] * 8))
    assert _call(a, out) == _lib.HJ_ERR_INVALID, cause
    assert list(out) == [wc.SENT32] * 8, cause
    assert (a["out32"] == wc.SENT32).all() and (a["out64"] == wc.SENT64).all(), (cause, "a refused call wrote")


def test_null_context():
    a = _good()
    out = (C.c_uint64 * 8)(*([wc.SENT32] * 8))
    assert lib.hj_window_rows_dev(None, a["perm"].ctypes.data, 40, 40, a["part"].ctypes.data, a["order"], 1, a["funcs"], 2) == _lib.HJ_ERR_INVALID
    assert lib.hj_window_rows_info(None, out) == _lib.HJ_ERR_INVALID and list(out) == [wc.SENT32] * 8


# ---- the host twin against the model ---------------------------------------------------------------------------------------------------
def check_host(case, tag):
    want, counts = wc.model(case)
    got, info = wc.host_call(case, np.random.default_rng(case.n_pos))
    wc.same(got, want, tag)
    wc.check_info(info, case, counts, tag)
    assert info[3] == 0


SHAPES = ("one", "each", "fixed2", "fixed3", "fixed63", "fixed64", "fixed65", "geometric", "seams")
PEERS = ("none", "const", "distinct", "runs", "f32", "f64", "nulls", "two", "four")


@pytest.mark.parametrize("shape", SHAPES)
def test_host_partition_shapes(shape):
    for i, n in enumerate((1, 2, 65, 1000)):
        for funcs in (None, "run"):
            check_host(wc.build(n, shape, "runs", perm=("random", "identity", None)[i % 3], seed=i, funcs=funcs), (shape, n, funcs))


@pytest.mark.parametrize("peers", PEERS)
def test_host_peers(peers):
    for i, n in enumerate((3, 64, 777)):
        check_host(wc.build(n, "geometric", peers, seed=i), (peers, n))
        check_host(wc.build(n, "one", peers, seed=i), (peers, n, "one partition"))


def test_host_lag_and_lead_offsets():
    for n, shape in ((300, "fixed63"), (300, "one"), (5, "fixed2")):
        for k in (0, 1, 2, 63, 64, n - 1, n, (1 << 32) - 1):
            check_host(wc.build(n, shape, "none", seed=k % 7, funcs=[wc.Func(W.HJ_WIN_LAG, k), wc.Func(W.HJ_WIN_LEAD, k)]), (n, shape, k))


def test_host_running_ops():
    for null_pct in (0, 10, 100):
        for shape in ("geometric", "one", "fixed3"):
            check_host(wc.build(500, shape, "none", seed=null_pct, funcs="run", null_pct=null_pct), (shape, null_pct))
    # a partition whose first elements are all NULL: the identity and a count of 0, then values
    n = 200
    for dtype in (np.int32, np.uint32, np.int64, np.uint64):
        valid = np.ones(n, dtype=bool)
        valid[:20] = valid[100:130] = False
        src = np.arange(n).astype(dtype) + 5
        funcs = [wc.Func(op, src=src, valid=valid) for op in wc.RUN_OPS]
        case = wc.Case(n, n, None, np.repeat(np.arange(2, dtype=U32), 100), [], funcs)
        check_host(case, dtype)
        got, _ = wc.host_call(case)
        signed = np.dtype(dtype).kind == "i"
        assert (got[0][:20] == 0).all() and (got[1][:20] == 0).all() and got[1][20] == 25
        assert (got[2][:20] == ((1 << 63) - 1 if signed else wc.M64)).all() and (got[3][100:130] == ((1 << 63) if signed else 0)).all()


def test_host_definition_by_runs():
    rng = np.random.default_rng(9)
    n = 3000
    perm = rng.permutation(n + 50).astype(U32)               # unsorted: many runs of one and two positions
    part = rng.integers(0, 2, n + 50).astype(U32)
    check_host(wc.Case(n, n + 50, perm, part, [sc.Col(rng.integers(0, 2, n + 50).astype(np.uint8))], wc.number_funcs()), "random runs")
    check_host(wc.Case(n, n + 50, perm, part, [], wc.run_funcs(n + 50)), "random runs, running ops")
    for funcs in (None, "run"):
        check_host(wc.build(2000, "geometric", "runs", holes=40, extra_rows=17, seed=4, funcs=funcs), ("holes", funcs))
        check_host(wc.build(100, "one", "const", holes=3, seed=5, funcs=funcs), ("holes in one partition", funcs))
    # every entry out of range: nothing is written, everything is skipped
    case = wc.Case(10, 4, np.array([4, 5, wc.NO_ROW] * 3 + [9], dtype=U32), None, [], wc.number_funcs())
    check_host(case, "all skipped")
    assert wc.host_call(case)[1][:5] == [10, 0, 0, 0, 10]
    # HJ_NO_ROW as a partition id is a value like any other
    part = np.array([wc.NO_ROW, wc.NO_ROW, 0, wc.NO_ROW], dtype=U32)
    got, info = wc.host_call(wc.Case(4, 4, None, part, [], [wc.Func(W.HJ_WIN_ROW_NUMBER), wc.Func(W.HJ_WIN_PART_ROWS)]))
    assert got[0].tolist() == [1, 2, 1, 1] and got[1].tolist() == [2, 2, 1, 1] and info[1] == 3


# ---- the wrapper against a per-partition loop (window_common.wrapper_check) ------------------------------------------------------------
@pytest.mark.parametrize("null_keys", ["group", "drop"])
def test_window_rows_host_against_a_loop(null_keys):
    for seed, n in enumerate((1, 7, 400)):
        t = wrapper_table(n, seed)
        wrapper_check(wrapper_call(hj.window_rows_host, t, null_keys), t, null_keys)


def test_window_rows_host_without_partition_or_order():
    v = np.array([5, -2, 7, 1], dtype=np.int32)
    got = hj.window_rows_host({"rn": "row_number", "s": ("cumsum", "v"), "p": ("lag", "v", 1), "dr": "dense_rank"}, cols={"v": v})
    assert got["rn"].tolist() == [1, 2, 3, 4] and got["s"].values.tolist() == [5, 3, 10, 11] and got["dr"].tolist() == [1] * 4
    assert got["p"].to_list() == [None] + [x.tobytes() for x in v[:3]] and got["perm"].tolist() == [0, 1, 2, 3] and got["n_partitions"] == 1
    got = hj.window_rows_host({"rk": "rank", "dr": "dense_rank"}, order_by=np.array([3.0, 1.0, 3.0, 2.0]))
    assert got["rk"].tolist() == [3, 1, 3, 2] and got["dr"].tolist() == [3, 1, 3, 2] and got["perm"].tolist() == [1, 3, 0, 2]


def test_wrapper_arguments():
    a = np.arange(4, dtype=np.int32)
    for fn in (hj.window_rows, hj.window_rows_host):
        with pytest.raises(ValueError, match="order columns behind a partition"):
            fn({"rn": "row_number"}, partition_by=a, order_by=[a, a, a, a])
        with pytest.raises(ValueError, match="exist"):
            fn({"x": "median"}, partition_by=a)
        with pytest.raises(ValueError, match="exist"):
            fn({"x": ("lag", "v")}, partition_by=a, cols={"v": a})
        with pytest.raises(ValueError, match="does not hold"):
            fn({"x": ("cumsum", "w")}, partition_by=a, cols={"v": a})
        with pytest.raises(ValueError, match="running sums"):
            fn({"x": ("cumsum", "v")}, partition_by=a, cols={"v": a.astype(np.float64)})
        with pytest.raises(ValueError, match="offset"):
            fn({"x": ("lag", "v", -1)}, partition_by=a, cols={"v": a})
        with pytest.raises(ValueError, match="taken"):
            fn({"perm": "row_number"}, partition_by=a)
        with pytest.raises(ValueError, match="no functions"):
            fn({}, partition_by=a)
        with pytest.raises(ValueError, match="how many rows"):
            fn({"rn": "row_number"})
        with pytest.raises(ValueError, match="'group' or 'drop'"):
            fn({"rn": "row_number"}, partition_by=a, null_keys="keep")
        # an empty table is answered without a device
        e = np.empty(0, dtype=np.int64)
        got = fn({"rn": "row_number", "s": ("cumsum", "v"), "p": ("lag", "v", 1), "n": ("cumcount", None)}, partition_by=e, order_by=e, cols={"v": e})
        assert got["rn"].size == 0 and got["rn"].dtype == U32 and got["s"].rows == 0 and got["p"].rows == 0 and got["n"].dtype == U64
        assert got["perm"].size == 0 and (got["n_partitions"], got["null_rows"]) == (0, 0)
