"""hj_sort_rows_dev / hj_sort_rows_info on an MI355X, through ctypes -> C ABI. At every case the device result equals the
host twin AND the model of sort_common (numpy ranks and np.lexsort) bit for bit, with guard words around dPerm intact. The
row counts come from hj_sort_layout_info (T = tile rows, L = chunk rows), not from constants. Then the wrappers against
numpy over the model's permutation, and one stream-order case. Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

from gpu_harness import Device, GuardedPlane, dev, fl  # noqa: F401
import sort_common as sc
import stream_order as so

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
GUARD = 64                       # words in front of and behind dPerm
SENT = 0xA5A5A5A5
T, L = sc.layout(1)[:2]          # at the sizes of this file the chunk is the smallest one
assert sc.layout(1 << 17)[:2] == (T, L) and L >= 2 * T
EDGES = (1, 2, 63, 64, 65, T - 1, T, T + 1, L - 1, L, L + 1, 2 * L + T + 17, 3 * L + 1, 1 << 16)
assert max(EDGES) <= 1 << 17


def sort_on_device(dev, cols, tag=None, garbage=None, release=True):
    """one hj_sort_rows_dev over the columns -> (the permutation, the info dict)"""
    n = cols[0].values.size
    desc = []
    for c in cols:
        plane = c.plane(garbage)
        desc.append((dev.put(c.values), dev.put(plane) if plane is not None else 0, c.width, c.type, c.flags))
    out = GuardedPlane(dev, n, sentinel=SENT, front=GUARD, behind=GUARD, what="a word outside dPerm was written")
    dev.ctx.sort_rows(desc, n, out.ptr)
    info = dev.ctx.sort_rows_info()
    got = out.read(n, tag)
    _, chunk, chunks, _ = sc.layout(n)
    assert (info["rows"], info["passes"], info["skipped"], info["reserved"]) == (n, sum(c.passes() for c in cols), 0, 0), (tag, info)
    assert (info["chunks"], info["chunk_rows"]) == (chunks, chunk) and info["workspace_bytes"] > 0, (tag, info)
    if release:
        dev.release()
    return got, info


def check(dev, cols, want, tag=None):
    """device == host twin == model"""
    garbage = np.random.default_rng(len(cols) + cols[0].values.size)
    got, info = sort_on_device(dev, cols, tag, garbage)
    sc.same(got, want, (tag, "device against the model"))
    sc.same(sc.host_perm(cols, garbage)[0], got, (tag, "host twin against the device"))
    return got, info


def check_family(dev, name, counts):
    for n in counts:
        cols, want = sc.case(name, n)
        check(dev, cols, want, (name, n))


# ---- ties and order ------------------------------------------------------------------------------------------------------------------
def test_all_keys_equal_at_every_edge(dev):
    """one bin holds the whole tile: the rank inside it reaches T - 1, every other bin is empty, the result is the identity"""
    for n in EDGES:
        cols, want = sc.case("equal", n)
        assert np.array_equal(want, np.arange(n, dtype=U32))
        check(dev, cols, want, ("equal", n))


def test_random_permutation_at_every_edge(dev):
    check_family(dev, "perm", EDGES)


@pytest.mark.parametrize("name", ["ascending", "descending", "alternating"])
def test_ordered_and_alternating_input(dev, name):
    check_family(dev, name, (65, T + 1, L + 1, 2 * L + T + 17, 3 * L + 1))


# ---- digits ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["low_byte", "high_byte", "ends", "small_i64"])
def test_digits(dev, name):
    """keys that differ in their lowest byte alone, in their highest alone, in digits 0x00 and 0xFF alone (the first and the
    last bin), and small values in a wide column (six passes in which one bin holds every row)"""
    check_family(dev, name, (64, T - 1, L, 2 * L + T + 17, 1 << 16))


# ---- types and values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sc.DTYPES)
def test_every_type_and_width(dev, dtype):
    """the whole range of the type with its corners: INT min, max, -1, 0; floats +-0.0, +-inf, denormals, NaNs of both signs"""
    check_family(dev, "type_" + dtype, (63, T + 1, 2 * L + T + 17))


@pytest.mark.parametrize("name", ["ties_f32", "ties_f64"])
def test_float_ties_keep_row_order(dev, name):
    """fourteen values, the specials: -0.0 and 0.0 tie, the NaNs tie whatever their sign and payload, and stay in row order"""
    for n in (65, L + 1, 2 * L + T + 17):                    # odd n: descending, see sort_common.make
        cols, want = sc.case(name, n)
        got, _ = check(dev, cols, want, (name, n))
        v = cols[0].values[got.astype(np.int64)]
        for cls in (np.isnan(v), v == 0):
            rows = got[cls]
            assert rows.size > 1 and (np.diff(rows.astype(np.int64)) > 0).all(), (name, n, "a tie is not in row order")
            run = np.flatnonzero(cls)
            assert run[-1] - run[0] + 1 == run.size, (name, n, "a tie class is not one run")


# ---- NULLs -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pct", [0, 10, 100])
@pytest.mark.parametrize("where", ["last", "first"])
@pytest.mark.parametrize("direction", ["asc", "desc"])
def test_nulls(dev, pct, where, direction):
    """random bytes under the NULLs, garbage in the plane's last word beyond nRows, both placements in both directions"""
    name = f"null{pct}_{where}_{direction}"
    for n in (33, T - 1, 2 * L + T + 17):
        cols, want = sc.case(name, n)
        got, _ = check(dev, cols, want, (name, n))
        nulls = ~cols[0].valid[got.astype(np.int64)]
        k = int(nulls.sum())
        assert k == (n if pct == 100 else 0 if pct == 0 else k)
        assert nulls[:k].all() if where == "first" else nulls[n - k:].all(), (name, n, "the NULLs are not where they belong")


# ---- multiple columns ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["multi2", "multi3", "multi4", "lead_const"])
def test_multiple_columns(dev, name):
    """few distinct values in the leading columns: later columns, and finally the row number, decide"""
    check_family(dev, name, (65, T + 1, L - 1, 2 * L + T + 17, 1 << 16))


# ---- fuzz --------------------------------------------------------------------------------------------------------------------------------
def test_fuzz(dev):
    for seed in range(40):
        cols = sc.fuzz_case(seed)
        check(dev, cols, sc.model_perm(cols), ("fuzz", seed, [(c.values.dtype.name, c.valid is not None, c.desc, c.nulls) for c in cols]))


# ---- repeatability -----------------------------------------------------------------------------------------------------------------------
def test_workspace_growth_and_reuse():
    """large then small, and small then large, each on a context of its own: the workspace grows once and is reused"""
    big, small = sc.case("multi3", 1 << 16), sc.case("type_int16", 1000)
    for order in ((big, small, big), (small, big, small)):
        d = Device()
        try:
            sizes = []
            for cols, want in order:
                _, info = check(d, cols, want, ("reuse", cols[0].values.size))
                sizes.append(info["workspace_bytes"])
            assert sizes[0] == sizes[2] != sizes[1]
        finally:
            d.close()


def test_identical_calls_give_identical_words(dev):
    cols, want = sc.case("multi4", 2 * L + T + 17)
    first, _ = sort_on_device(dev, cols, "first")
    again, _ = sort_on_device(dev, cols, "again")
    assert first.tobytes() == again.tobytes()
    sc.same(first, want, "multi4 twice")


def test_no_rows_and_refused_calls(dev):
    cols, want = sc.case("perm", 1000)
    check(dev, cols, want, "before")
    arr, k = sc.sort_col_array(cols, [(0, 0)])
    assert lib.hj_sort_rows_dev(dev.ctx._h, arr, 0, 1000, None) == _lib.HJ_ERR_INVALID
    assert b"hj_sort_rows_dev" in lib.hj_last_error(dev.ctx._h)
    assert dev.ctx.sort_rows_info()["rows"] == 1000                                           # a refused call is no call
    dev.ctx.sort_rows([(0, 0, 4, _lib.HJ_VAL_INT, 0)], 0, 0)
    assert list(dev.ctx.sort_rows_info().values()) == [0] * 8


# ---- the wrappers ------------------------------------------------------------------------------------------------------------------------
def test_sort_rows_wrapper():
    for name in ("multi4", "null10_first_desc", "type_float32"):
        cols, want = sc.case(name, L + 1)
        got = hj.sort_rows([c.key() for c in cols], descending=[c.desc for c in cols], nulls=[c.nulls for c in cols])
        sc.same(got, want, name)


def test_sort_by_columns_with_payload_and_limit():
    n = 2 * L + T + 17
    cols, want = sc.case("multi3", n)
    rng = np.random.default_rng(3)
    words = [None if i % 11 == 0 else "w%d" % (i * 7919 % 1000) * (i % 3) for i in range(n)]
    pv, pvalid = sc.nullable(rng, rng.integers(-1 << 40, 1 << 40, n), 0.2)
    payload = {"s": hj.KeyColumn.from_list(words), "v": hj.KeyColumn(pv, pvalid), "f": rng.random(n), "b": rng.integers(0, 256, n).astype(np.uint8)}
    kw = dict(descending=[c.desc for c in cols], nulls=[c.nulls for c in cols])
    for limit in (None, 0, 1, 1000, n + 5):
        m = n if limit is None else min(limit, n)
        got = hj.sort_by_columns([c.key() for c in cols], payload, limit=limit, **kw)
        rows = want[:m].astype(np.int64)
        sc.same(got["rows"], want[:m], ("rows", limit)) if m == n else np.testing.assert_array_equal(got["rows"], want[:m])
        for c, k in zip(cols, got["keys"]):
            assert isinstance(k, hj.KeyColumn) and k.rows == m
            valid = np.ones(m, dtype=bool) if c.valid is None else c.valid[rows]
            assert np.array_equal(k.valid if k.valid is not None else np.ones(m, dtype=bool), valid)
            assert k.values[valid].tobytes() == c.values[rows][valid].tobytes()
        assert got["cols"]["s"].to_list() == [None if words[i] is None else words[i].encode() for i in rows]
        assert got["cols"]["f"].tobytes() == payload["f"][rows].tobytes() and np.array_equal(got["cols"]["b"], payload["b"][rows])
        v = got["cols"]["v"]
        assert np.array_equal(v.valid if v.valid is not None else np.ones(m, dtype=bool), pvalid[rows])
        assert np.array_equal(v.values[pvalid[rows]], pv[rows][pvalid[rows]])


def test_sort_pairs():
    rng = np.random.default_rng(5)
    n = L + T + 3
    s, r = rng.integers(0, 500, n).astype(U32), rng.integers(0, 50, n).astype(U32)
    s[rng.random(n) < 0.05] = hj.NO_ROW
    r[rng.random(n) < 0.05] = hj.NO_ROW
    order = np.lexsort((r, s))
    got_s, got_r = hj.sort_pairs(s, r)
    assert got_s.dtype == U32 and np.array_equal(got_s, s[order]) and np.array_equal(got_r, r[order])
    assert (got_s[-int((s == hj.NO_ROW).sum()):] == hj.NO_ROW).all()


def test_sort_pairs_on_a_full_outer_join():
    """the canonical order of a join's maps: the device-sorted pairs equal the host-sorted ones, the outer tail last"""
    rng = np.random.default_rng(6)
    relR = rng.integers(1, 2000, 3000).astype(U64)                       # key tuples: duplicates on both sides, keys only in R and only in S
    relS = rng.integers(1000, 3000, 5000).astype(U64)
    res = hj.join_tables(relR, relS, how="full")
    s, r = res["s_idx"], res["r_idx"]
    assert (s == hj.NO_ROW).any() and (r == hj.NO_ROW).any()
    order = np.lexsort((r, s))
    got_s, got_r = hj.sort_pairs(s, r)
    assert np.array_equal(got_s, s[order]) and np.array_equal(got_r, r[order])
    tail = int((s == hj.NO_ROW).sum())
    assert (got_s[-tail:] == hj.NO_ROW).all() and (np.diff(got_r[-tail:].astype(np.int64)) > 0).all()


# ---- stream order ------------------------------------------------------------------------------------------------------------------------
def test_stream_order(fl):
    """decoy keys (ascending: the identity) and an all-NULL decoy plane before the delay, the real ones behind it on the
    caller's stream: a call that read early answers with the identity"""
    n = 2 * L + 5
    rng = np.random.default_rng(14)
    real = sc.Col(rng.integers(-300, 300, n).astype(np.int32), rng.random(n) < 0.9, desc=True, nulls="first")
    warm = sc.Col(rng.integers(0, 77, n).astype(np.int32), rng.random(n) < 0.5)
    want = sc.model_perm([real])
    assert not np.array_equal(want, np.arange(n, dtype=U32))
    vp = lambda p: C.c_void_p(p) if p else None     # noqa: E731
    with hj.HashJoinContext(0, stream=fl.handle) as ctx:
        st = so.Stage(fl.stream)
        keys = st.buf(np.arange(n, dtype=np.int32), real=real.values, warm=warm.values)
        plane = st.buf(np.zeros_like(real.plane()), real=real.plane(), warm=warm.plane())
        perm = st.out(n, U32, so.SENT32)

        def seq(which):
            cols = (_lib.hj_sort_col * 1)()
            cols[0].values, cols[0].valid, cols[0].width, cols[0].type, cols[0].flags = keys.ptr, plane.ptr, 4, _lib.HJ_VAL_INT, real.flags
            rc = lib.hj_sort_rows_dev(ctx._h, cols, 1, n, vp(perm.ptr))
            C.memset(cols, 0, C.sizeof(cols))
            if rc != _lib.HJ_OK:
                raise hj.HashJoinError(rc, lib.hj_last_error(ctx._h).decode())

        assert so.contract()["hj_sort_rows_dev"][0] == "asynchronous"
        so.run_delayed([st], seq, True, f"sort_rows.{fl.name}")
        st.check_inputs_intact()
        info = ctx.sort_rows_info()
    assert (info["rows"], info["passes"]) == (n, 5)
    sc.same(st.result(perm, U32, "perm"), want, "behind the delay")
