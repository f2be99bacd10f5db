"""hj_window_rows_dev / hj_window_rows_info on an MI355X, through ctypes -> C ABI. At every case the device result equals the
host twin AND the model of window_common bit for bit, every output lies between guard words that are checked, and the info
fields equal the model's partitions, peer runs and skipped entries. The sizes come from hj_window_layout_info (T = tile
positions, L = chunk positions), not from constants. Then the wrapper against its host form, and one stream-order case.
Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

from gpu_harness import Device, GuardedPlane, dev, fl  # noqa: F401
import sort_common as sc
import stream_order as so
import window_common as wc
from window_common import WRAPPER_FUNCS, wrapper_call, wrapper_check, wrapper_table

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
W = _lib
GUARD = 64                       # entries in front of and behind every output
T, L = wc.layout(1)[:2]          # at the sizes of this file the chunk is the smallest one
assert wc.layout(1 << 17)[:2] == (T, L) and L >= 2 * T
EDGES = (1, 2, 63, 64, 65, T - 1, T, T + 1, L - 1, L, L + 1, 2 * L + T + 17, 3 * L + 1, 1 << 16)
assert max(EDGES) <= 1 << 17


def on_device(dev, case, tag=None, garbage=None, funcs=None, release=True):
    """one hj_window_rows_dev -> ([one array per function], the info dict)"""
    funcs = case.funcs if funcs is None else funcs
    d_perm = dev.put(case.perm) if case.perm is not None else 0
    d_part = dev.put(case.part) if case.part is not None else 0
    order = []
    for c in case.order:
        plane = c.plane(garbage)
        order.append((dev.put(c.values), dev.put(plane) if plane is not None else 0, c.width, c.type, c.flags))
    outs, desc = [GuardedPlane(dev, case.n_rows, f.dtype, f.sentinel, front=GUARD, behind=GUARD, what="an entry outside out was written")
                  for f in funcs], []
    for f, o in zip(funcs, outs):
        plane = f.plane(case.n_rows, garbage)
        desc.append((f.op, o.ptr, dev.put(f.src) if f.src is not None else 0, dev.put(plane) if plane is not None else 0, f.width, f.flags, f.offset))
    dev.ctx.window_rows(d_perm, case.n_pos, case.n_rows, d_part, order, desc)
    info = dev.ctx.window_rows_info()
    got = [o.read(case.n_rows, tag) for o in outs]
    if release:
        dev.release()
    return got, info


def check(dev, case, tag=None):
    """device == host twin == model, and the info fields"""
    garbage = np.random.default_rng(case.n_pos + len(case.funcs))
    want, counts = wc.model(case)
    got, info = on_device(dev, case, tag, garbage)
    wc.same(got, want, (tag, "device against the model"))
    host, host_info = wc.host_call(case, garbage)
    wc.same(host, got, (tag, "host twin against the device"))
    wc.check_info(list(info.values()), case, counts, tag)
    assert list(info.values())[:3] + list(info.values())[4:] == host_info[:3] + host_info[4:], (tag, info, host_info)
    return got, info


def check_both(dev, n, tag=None, **kw):
    """the numbering ops and row maps in one call of eight, the running ops in another"""
    for funcs in (None, "run"):
        check(dev, wc.build(n, funcs=funcs, **kw), (tag, n, funcs, kw))


# ---- sizes and partition shapes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", EDGES)
def test_every_edge(dev, n):
    check_both(dev, n, "geometric", shape="geometric", peers="runs", seed=n % 5)
    check_both(dev, n, "one partition", shape="one", peers="runs", seed=n % 5 + 1)
    check_both(dev, n, "each its own", shape="each", peers="const", seed=n % 5)


@pytest.mark.parametrize("length", [2, 3, 63, 64, 65, T, L, L + 1])
def test_fixed_lengths(dev, length):
    for n in (L + 1, 3 * L + 1):
        check_both(dev, n, "fixed", shape=f"fixed{length}", peers="runs", seed=length % 3)


def test_heads_at_the_seams(dev):
    """a head exactly at the first and at the last position of every wavefront, tile and chunk"""
    for n in (L, 2 * L + T + 17):
        check_both(dev, n, "seams", shape="seams", peers="runs")


def test_a_partition_over_whole_chunks(dev):
    """a carry crosses chunks that hold no head: forward for start, the ranks and the running ops, backward for end"""
    n = 5 * L + 77
    for perm in ("random", None):
        check_both(dev, n, "long", shape="long", peers="runs", perm=perm)
    ids = wc.shape_ids("long", n)
    assert (np.bincount(ids)[1] >= 3 * L) and ids[L] == ids[4 * L] == 1


# ---- peers -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("peers", ["none", "const", "distinct", "runs", "f32", "f64", "nulls", "two", "four"])
def test_peers(dev, peers):
    """all peers, no two peers, runs across tile and chunk seams, floats whose peers differ in their bits, NULL peers with
    random bytes under them, two and four columns of mixed widths"""
    for n, shape in ((65, "one"), (L + T + 3, "one"), (2 * L + T + 17, "geometric"), (2 * L + T + 17, "fixed64")):
        check(dev, wc.build(n, shape, peers, seed=3), (peers, n, shape))


# ---- LAG / LEAD ----------------------------------------------------------------------------------------------------------------------------
def test_lag_and_lead_offsets(dev):
    for n, shape in ((2 * L + T + 17, "fixed65"), (2 * L + T + 17, "one"), (5 * L + 77, "long"), (100, "fixed3")):
        offsets = (0, 1, 63, 64, T, L + 1, n - 1, n, 2 ** 32 - 1)
        funcs = [wc.Func(W.HJ_WIN_LAG, k) for k in offsets[:4]] + [wc.Func(W.HJ_WIN_LEAD, k) for k in offsets[:4]]
        check(dev, wc.build(n, shape, "none", funcs=funcs), ("offsets", n, shape, offsets[:4]))
        funcs = [wc.Func(W.HJ_WIN_LAG, k) for k in offsets[4:]] + [wc.Func(W.HJ_WIN_LEAD, k) for k in offsets[6:]]
        check(dev, wc.build(n, shape, "none", funcs=funcs), ("offsets", n, shape, offsets[4:]))
        check(dev, wc.build(n, shape, "none", funcs=[wc.Func(W.HJ_WIN_LEAD, k) for k in offsets[4:6]]), ("lead", n, shape))


# ---- running ops ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("null_pct", [0, 10, 100])
def test_running_ops(dev, null_pct):
    """the four source types, sums that wrap 2^64, the extremes of the signed types, counts with and without a plane"""
    for n, shape in ((65, "fixed3"), (2 * L + T + 17, "geometric"), (3 * L + 1, "one"), (5 * L + 77, "long")):
        check(dev, wc.build(n, shape, "none", funcs="run", null_pct=null_pct, seed=null_pct), (n, shape, null_pct))


def test_a_partition_that_starts_with_nulls(dev):
    """the identity and RUN_COUNT 0 while the frame holds no value, then values; the second partition starts inside a chunk"""
    n = 2 * L + 9
    for dtype in (np.int32, np.uint32, np.int64, np.uint64):
        valid = np.ones(n, dtype=bool)
        valid[:T + 5] = valid[L + 100:L + T + 300] = False
        src = (np.arange(n) % 1000).astype(dtype) + 5
        part = (np.arange(n) >= L + 100).astype(U32)
        case = wc.Case(n, n, None, part, [], [wc.Func(op, src=src, valid=valid) for op in wc.RUN_OPS])
        got, _ = check(dev, case, dtype)
        signed = np.dtype(dtype).kind == "i"
        assert (got[0][:T + 5] == 0).all() and got[0][T + 5] == 1 and (got[0][L + 100:L + T + 300] == 0).all()
        assert (got[2][L + 100:L + T + 300] == ((1 << 63) - 1 if signed else wc.M64)).all() and (got[3][:T + 5] == ((1 << 63) if signed else 0)).all()


# ---- the definition by runs ----------------------------------------------------------------------------------------------------------------
def test_an_unsorted_permutation(dev):
    rng = np.random.default_rng(9)
    n, extra = 2 * L + T + 17, 50
    perm = rng.permutation(n + extra).astype(U32)
    part = rng.integers(0, 2, n + extra).astype(U32)
    order = [sc.Col(rng.integers(0, 2, n + extra).astype(np.uint8))]
    got, info = check(dev, wc.Case(n, n + extra, perm, part, order, wc.number_funcs()), "random runs")
    assert info["partitions"] > n // 4
    check(dev, wc.Case(n, n + extra, perm, part, [], wc.run_funcs(n + extra)), "random runs, running ops")


def test_entries_out_of_range(dev):
    """HJ_NO_ROW and rows >= nRows at position 0, at the last position, at the chunk seams and sprinkled in"""
    for n in (3, L + 1, 2 * L + T + 17):
        for shape in ("geometric", "one"):
            for funcs in (None, "run"):
                case = wc.build(n, shape, "runs", holes=n // 50 + 1, extra_rows=13, seed=n % 4, funcs=funcs)
                _, info = check(dev, case, ("holes", n, shape, funcs))
                assert info["skipped"] >= min(n, 2)
    case = wc.Case(10, 4, np.array([4, 5, wc.NO_ROW] * 3 + [9], dtype=U32), None, [], wc.number_funcs())
    _, info = check(dev, case, "all skipped")
    assert (info["partitions"], info["peer_runs"], info["skipped"]) == (0, 0, 10)


def test_rows_at_no_position_keep_the_sentinel(dev):
    n_pos, extra = L + 100, 3000
    for funcs in (None, "run"):
        case = wc.build(n_pos, "geometric", "runs", extra_rows=extra, seed=2, funcs=funcs)
        got, _ = check(dev, case, ("nPos < nRows", funcs))
        absent = np.setdiff1d(np.arange(n_pos + extra), case.perm[:n_pos].astype(np.int64))
        assert absent.size == extra and all((g[absent] == f.sentinel).all() for g, f in zip(got, case.funcs))


def test_perm_null(dev):
    for n in (1, T + 1, 2 * L + T + 17):
        check_both(dev, n, "identity", shape="geometric", peers="two", perm=None, extra_rows=5)
    case = wc.build(L + 1, "fixed65", "runs", perm=None)
    with_plane = wc.Case(case.n_pos, case.n_rows, np.arange(case.n_pos, dtype=U32), case.part, case.order, case.funcs)
    wc.same(on_device(dev, case)[0], on_device(dev, with_plane)[0], "dPerm NULL against the identity plane")


# ---- call structure ------------------------------------------------------------------------------------------------------------------------
def test_eight_functions_in_one_call_or_one_by_one(dev):
    for funcs in (None, "run"):
        case = wc.build(2 * L + T + 17, "geometric", "runs", seed=6, funcs=funcs)
        together, _ = check(dev, case, ("together", funcs))
        for i, f in enumerate(case.funcs):
            alone, info = on_device(dev, case, ("alone", i), funcs=[f])
            assert alone[0].tobytes() == together[i].tobytes(), (funcs, i)


def test_workspace_growth_and_reuse():
    """large then small, and small then large, each on a context of its own: the workspace grows once and is reused"""
    big, small = wc.build(1 << 16, "geometric", "runs"), wc.build(1000, "fixed3", "two", funcs="run")
    for order in ((big, small, big), (small, big, small)):
        d = Device()
        try:
            sizes = [check(d, case, ("reuse", case.n_pos))[1]["workspace_bytes"] for case in order]
            assert sizes[0] == sizes[2] != sizes[1]
        finally:
            d.close()


def test_no_positions_and_refused_calls(dev):
    case = wc.build(1000, "geometric", "runs")
    check(dev, case, "before")
    out = dev.put(np.full(8, wc.SENT32, dtype=U32))
    f_arr, _ = wc.func_array([wc.Func(W.HJ_WIN_RANK)], [(out, 0, 0)])
    assert lib.hj_window_rows_dev(dev.ctx._h, None, 8, 8, None, None, 0, f_arr, 0) == _lib.HJ_ERR_INVALID
    assert b"hj_window_rows_dev" in lib.hj_last_error(dev.ctx._h)
    assert dev.ctx.window_rows_info()["positions"] == 1000                                     # a refused call is no call
    dev.ctx.window_rows(0, 0, 8, 0, [], [(W.HJ_WIN_RANK, out)])
    assert list(dev.ctx.window_rows_info().values()) == [0] * 8
    assert (dev.get(out, 8) == wc.SENT32).all()
    dev.release()


# ---- the wrapper ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("null_keys", ["group", "drop"])
def test_window_rows_equals_its_host_form(null_keys):
    """a string partition key, an int64 DESC order column with NULLs first, lag of a string column, cumsum of a nullable int32"""
    t = wrapper_table(L + 333, 7)
    got, host = wrapper_call(hj.window_rows, t, null_keys), wrapper_call(hj.window_rows_host, t, null_keys)
    assert got.keys() == host.keys() and set(WRAPPER_FUNCS) < set(got)
    for name, h in host.items():
        g = got[name]
        if isinstance(h, hj.KeyColumn):
            assert isinstance(g, hj.KeyColumn) and g.to_list() == h.to_list(), name
        elif isinstance(h, np.ndarray):
            assert g.dtype == h.dtype and np.array_equal(g, h), name
        else:
            assert g == h, name
    if null_keys == "drop":
        assert got["null_rows"] > 0 and (got["rn"] == 0).sum() == got["null_rows"]
    wrapper_check(got, t, null_keys)


def test_window_rows_without_a_sort():
    v = np.arange(L + 5, dtype=np.int64)
    got = hj.window_rows({"rn": "row_number", "s": ("cumsum", "v"), "p": ("lag", "v", 2)}, cols={"v": v})
    assert np.array_equal(got["rn"], v + 1) and np.array_equal(got["s"].values, np.cumsum(v)) and got["n_partitions"] == 1
    assert got["p"].valid.tolist() == [False, False] + [True] * (L + 3) and np.array_equal(got["p"].values[2:], v[:-2])


# ---- stream order --------------------------------------------------------------------------------------------------------------------------
def test_stream_order(fl):
    """decoy content before the delay -- a dPerm of HJ_NO_ROW (nothing would be written), one partition id, zero values under
    an all-NULL plane -- and the real inputs behind it on the caller's stream"""
    n = 2 * L + 5
    funcs = [wc.Func(W.HJ_WIN_ROW_NUMBER), wc.Func(W.HJ_WIN_RANK), wc.Func(W.HJ_WIN_LAST_ROW), wc.Func(W.HJ_WIN_LEAD, 3)]
    case = wc.build(n, "geometric", "runs", seed=14, funcs=funcs)
    rng = np.random.default_rng(15)
    src, valid = rng.integers(-99, 99, n).astype(np.int32), rng.random(n) < 0.8
    case.funcs += [wc.Func(W.HJ_WIN_RUN_SUM, src=src, valid=valid), wc.Func(W.HJ_WIN_RUN_COUNT, src=src, valid=valid, width=4)]
    want, counts = wc.model(case)
    key, plane = case.order[0], case.funcs[4].plane(n)
    assert key.valid is None and counts[0] > 10
    vp = lambda p: C.c_void_p(p) if p else None     # noqa: E731
    with hj.HashJoinContext(0, stream=fl.handle) as ctx:
        st = so.Stage(fl.stream)
        b_perm = st.buf(np.full(n, so.NO_ROW, dtype=U32), real=case.perm, warm=np.roll(case.perm, 7))
        b_part = st.buf(np.zeros(n, dtype=U32), real=case.part, warm=np.roll(case.part, 3))
        b_key = st.buf(np.zeros_like(key.values), real=key.values, warm=key.values[::-1].copy())
        b_src = st.buf(np.zeros(n, dtype=np.int32), real=src, warm=src[::-1].copy())
        b_plane = st.buf(np.zeros_like(plane), real=plane, warm=~plane)
        outs = [st.out(n, f.dtype, f.sentinel) for f in case.funcs]

        def seq(which):
            order = (_lib.hj_sort_col * 1)()
            order[0].values, order[0].width, order[0].type = b_key.ptr, key.width, key.type
            arr, k = wc.func_array(case.funcs, [(o.ptr, b_src.ptr if f.run else 0, b_plane.ptr if f.run else 0) for f, o in zip(case.funcs, outs)])
            rc = lib.hj_window_rows_dev(ctx._h, vp(b_perm.ptr), n, n, vp(b_part.ptr), order, 1, arr, k)
            C.memset(order, 0, C.sizeof(order))               # both descriptors were read before the call returned
            C.memset(arr, 0, C.sizeof(arr))
            if rc != _lib.HJ_OK:
                raise hj.HashJoinError(rc, lib.hj_last_error(ctx._h).decode())

        assert so.contract()["hj_window_rows_dev"][0] == "asynchronous"
        so.run_delayed([st], seq, True, f"window_rows.{fl.name}")
        st.check_inputs_intact()
        info = ctx.window_rows_info()
    assert (info["positions"], info["partitions"], info["peer_runs"], info["skipped"]) == (n,) + counts
    wc.same([st.result(o, f.dtype, i) for i, (o, f) in enumerate(zip(outs, case.funcs))], want, "behind the delay")
