"""hj_key_groups_dev / hj_key_groups_info on an MI355X, through ctypes -> C ABI. At every shape the device result equals the
host twin AND the model of groups_common (a dict on the key's bytes) bit for bit -- rep, group, the first rows, the counts --
with guard words around every output intact and the failure word 0. Then group_by_columns and distinct_on against numpy
over the model's groups, and one stream-order case. Run with -m gpu."""
import ctypes as C
import functools

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

from gpu_harness import GuardedPlane, dev, fl  # noqa: F401
import groups_common as gc
import keys2_common as k2
import stream_order as so

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
NO_ROW = gc.NO_ROW
GUARD = 64                       # words in front of and behind every output
SENT = 0xA5A5A5A5


def out_plane(dev, n):
    """an output plane of n words on the device between two guards"""
    return GuardedPlane(dev, n, sentinel=SENT, front=GUARD, behind=GUARD, what="a word outside the output was written")


def groups_on_device(dev, keys, nulls, key_mask=0, capacity=None, tag=None, release=True):
    """one hj_key_groups_dev over the KeyColumns `keys` -> (the dict key_groups_host returns, the info dict)"""
    n = keys[0].rows
    flags = [hj.HJ_KEY_NULLS_EQUAL if nulls == "group" or c.nulls_equal else 0 for c in keys]
    desc = []
    for c, f in zip(keys, flags):
        v, off, valid = dev.column(c)
        desc.append((v, 0, c.width, off, 0, valid, 0, f))
    cap = n if capacity is None else capacity
    rep, group, first = out_plane(dev, n), out_plane(dev, n), out_plane(dev, cap)
    dev.ctx.key_groups(desc, hj.HJ_KEY_SIDE_S, n, rep.ptr, group.ptr, first.ptr if cap else 0, cap, key_mask)
    info = dev.ctx.key_groups_info()
    assert info["failure"] == 0, (tag, info)
    assert info["written"] == min(info["groups"], cap) and info["slots"] >= 2 * n and info["slots"] & (info["slots"] - 1) == 0, (tag, info)
    got = {"rep": rep.read(n, tag), "group": group.read(n, tag), "first_rows": first.read(info["written"], tag),
           "n_groups": info["groups"], "null_rows": info["null_rows"]}
    if release:
        dev.release()
    return got, info


def check(dev, keys, want, nulls="group", key_mask=0, capacity=None, tag=None):
    """device == host twin == model"""
    got, info = groups_on_device(dev, keys, nulls, key_mask, capacity, tag)
    if capacity is not None:
        want = dict(want, first_rows=want["first_rows"][:capacity])
    gc.same(got, want, (tag, "device against the model"))
    gc.same(hj.key_groups_host(keys, nulls=nulls, key_mask=key_mask, capacity=capacity), got, (tag, "host twin against the device"))
    return info


# ---- tables, each with the model's answer computed once ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(name):
    """-> (the key columns as numpy arrays, the model's groups)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "distinct":                                                      # 2^18 rows, all distinct, 8 bytes
        a = (np.arange(1 << 18, dtype=U64) * U64(0x9E3779B97F4A7C15)) ^ U64(0x5555)
        assert np.unique(a).size == a.size
        cols = [a]
    elif name == "thousand":                                                    # 200 000 rows, 1000 keys
        cols = [rng.integers(0, 1 << 62, 1000, dtype=np.int64).astype(U64)[rng.permutation(np.arange(200_000) % 1000)]]
    elif name == "one":                                                         # 100 000 rows of one key: one slot for all
        cols = [np.full(100_000, 0xDEADBEEFCAFE, dtype=U64)]
    elif name == "zipf":
        cols = [(hj.generate_data("zipf", 150_000, 20_000, 16, 1.0) & U64(0xFFFFFFFF)).astype(U32)]
    elif name == "collide":                                                     # 50 000 rows, 5000 keys, two columns
        pick = rng.permutation(np.concatenate([np.arange(5000), rng.integers(0, 5000, 45_000)]))
        cols = [rng.integers(0, 1 << 62, 5000, dtype=np.int64).astype(U64)[pick], (pick % 7).astype(np.uint16)]
    else:
        raise KeyError(name)
    return cols, gc.model_groups(gc.array_keys(cols))


def columns(arrays):
    return [hj.KeyColumn(a) for a in arrays]


# ---- the shapes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025])
def test_lane_wavefront_and_workgroup_edges(dev, n):
    """a fixed column, and a nullable string next to a nullable fixed column, in both NULL modes"""
    rng = np.random.default_rng(n)
    a = rng.integers(0, n // 3 + 1, n).astype(U64) << U64(35)
    info = check(dev, columns([a]), gc.model_groups(gc.array_keys([a])), tag=("fixed", n))
    assert info["null_rows"] == 0
    cols = [gc.string_col(rng, n, n // 8 + 1, nulls=0.1), k2.fixed_col(rng, 4, n, nulls=0.1, distinct=3)]
    for nulls in ("group", "drop"):
        check(dev, gc.key_columns(cols), gc.model_groups(gc.model_keys(cols, nulls)), nulls=nulls, key_mask=0xFFFF, tag=("mixed", n, nulls))


@pytest.mark.parametrize("name", ["distinct", "thousand", "one", "zipf"])
def test_large_tables(dev, name):
    cols, want = table(name)
    info = check(dev, columns(cols), want, tag=name)
    if name == "distinct":
        assert want["n_groups"] == 1 << 18 and info["slots"] == 1 << 19
    if name == "one":
        assert want["n_groups"] == 1 and info["probe_steps"] == 0 and info["collisions"] == 0


def test_word_collisions_under_a_weak_mask(dev):
    """16 join words for 5000 keys: the compare that finds another key runs, and nothing in the result shows it"""
    cols, want = table("collide")
    assert want["n_groups"] == 5000
    info = check(dev, columns(cols), want, key_mask=0xF, tag="collide")
    assert info["collisions"] > 0 and info["probe_steps"] > 0
    for key_mask in (0, 0x1):
        check(dev, columns(cols), want, key_mask=key_mask, tag=("collide", key_mask))


@pytest.mark.parametrize("nulls", ["group", "drop"])
def test_strings_and_nulls(dev, nulls):
    """20 000 rows: strings of 0 to 40 bytes at unaligned offsets, alone and next to fixed columns, 10 % NULLs"""
    n = 20_000
    rng = np.random.default_rng(20)
    for tag, cols in (("strings", [gc.string_col(rng, n, 1500, nulls=0.1)]),
                      ("mixed", [k2.fixed_col(rng, 2, n, nulls=0.1, distinct=9), gc.string_col(rng, n, 300, nulls=0.1),
                                 k2.fixed_col(rng, 16, n, distinct=4)]),
                      ("widths", [k2.fixed_col(rng, 1, n, nulls=0.1, distinct=30), k2.fixed_col(rng, 8, n, distinct=40)])):
        want = gc.model_groups(gc.model_keys(cols, nulls))
        assert (want["null_rows"] > n // 20) == (nulls == "drop") and want["n_groups"] > 100
        check(dev, gc.key_columns(cols), want, nulls=nulls, tag=(tag, nulls))
        check(dev, gc.key_columns(cols), want, nulls=nulls, key_mask=0xF, tag=(tag, nulls, 0xF))


def test_capacity_below_the_group_count(dev):
    cols, want = table("thousand")
    assert want["n_groups"] == 1000
    for capacity in (0, 1, 333, 999, 1000):
        info = check(dev, columns(cols), want, capacity=capacity, tag=("capacity", capacity))
        assert (info["groups"], info["written"]) == (1000, capacity)


def test_optional_outputs(dev):
    """no group plane, no first rows: rep alone, and the count of the groups all the same"""
    cols, want = table("thousand")
    a = cols[0]
    rep = out_plane(dev, a.size)
    dev.ctx.key_groups([(dev.put(a), 0, 8)], hj.HJ_KEY_SIDE_S, a.size, rep.ptr)
    info = dev.ctx.key_groups_info()
    assert (info["groups"], info["written"], info["failure"]) == (1000, 0, 0)
    assert np.array_equal(rep.read(a.size, "rep alone"), want["rep"])
    dev.release()


def test_two_calls_on_one_context(dev):
    """a large table, then a small one with other keys: no slot of the first leaks into the second, the workspace is reused"""
    cols, want = table("thousand")
    check(dev, columns(cols), want, tag="large")
    rng = np.random.default_rng(2)
    small = [rng.integers(0, 40, 3000).astype(U64) + U64(1 << 50)]
    check(dev, columns(small), gc.model_groups(gc.array_keys(small)), tag="small after large")
    check(dev, columns(small), gc.model_groups(gc.array_keys(small)), key_mask=0x1, tag="small after large, one word")
    assert hj.lib.hj_key_groups_dev(dev.ctx._h, None, 0, 0, 0, 0, None, None, None, 0) == _lib.HJ_ERR_INVALID
    info = dev.ctx.key_groups_info()                                            # a refused call is no call
    assert info["groups"] == 40 and info["failure"] == 0


def test_identical_calls_give_identical_bytes(dev):
    cols, want = table("zipf")
    first, _ = groups_on_device(dev, columns(cols), "group", tag="first")
    again, _ = groups_on_device(dev, columns(cols), "group", tag="again")
    for k in ("rep", "group", "first_rows"):
        assert first[k].tobytes() == again[k].tobytes(), k
    gc.same(first, want)


def test_no_rows(dev):
    dev.ctx.key_groups([(0, 0, 8)], hj.HJ_KEY_SIDE_S, 0, 0)
    info = dev.ctx.key_groups_info()
    assert [info[k] for k in ("groups", "written", "null_rows", "slots", "probe_steps", "collisions", "failure")] == [0] * 7


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------
def numpy_aggregates(want, values, valid, signed):
    """COUNT(*), COUNT(col), SUM, MIN, MAX of `values` per group of the model's ids, by numpy"""
    m, ids = want["n_groups"], want["group"]
    rows = np.flatnonzero(ids != NO_ROW)
    ok = rows if valid is None else rows[valid[rows]]
    wide = values.astype(np.int64 if signed else U64)
    count, seen = np.bincount(ids[rows], minlength=m).astype(U64), np.bincount(ids[ok], minlength=m).astype(U64)
    total = np.zeros(m, dtype=wide.dtype)
    np.add.at(total, ids[ok], wide[ok])
    info = np.iinfo(wide.dtype)
    lo, hi = np.full(m, info.max, dtype=wide.dtype), np.full(m, info.min, dtype=wide.dtype)
    np.minimum.at(lo, ids[ok], wide[ok])
    np.maximum.at(hi, ids[ok], wide[ok])
    return count, seen, total, lo, hi


def same_column(got, want_values, want_valid, tag):
    assert isinstance(got, hj.KeyColumn), tag
    valid = got.valid if got.valid is not None else np.ones(got.rows, dtype=bool)
    assert np.array_equal(valid, want_valid), tag
    assert np.array_equal(got.values[valid], want_values[want_valid]) and (got.values[~valid] == 0).all(), tag


@pytest.mark.parametrize("nulls", ["group", "drop"])
def test_group_by_columns_and_distinct_on(nulls):
    n = 30_000
    rng = np.random.default_rng(30)
    cols = [k2.fixed_col(rng, 8, n, nulls=0.1, distinct=60), gc.string_col(rng, n, 25, nulls=0.1)]
    keys = gc.key_columns(cols)
    want = gc.model_groups(gc.model_keys(cols, nulls))
    m = want["n_groups"]
    assert 500 < m < 3000 and (want["null_rows"] > 0) == (nulls == "drop")
    sources = {"i32": rng.integers(-1 << 31, 1 << 31, n).astype(np.int32), "u32": rng.integers(0, 1 << 32, n).astype(U32),
               "i64": rng.integers(-1 << 62, 1 << 62, n), "u64": rng.integers(0, 1 << 63, n).astype(U64) * U64(2)}
    valid = {"i32": rng.random(n) < 0.7, "u64": rng.random(n) < 0.5}
    table_cols = {k: hj.KeyColumn(v, valid[k]) if k in valid else v for k, v in sources.items()}
    aggs = {"rows": ("count", None)}
    for k in sources:
        aggs.update({f"n_{k}": ("count", k), f"sum_{k}": ("sum", k), f"min_{k}": ("min", k), f"max_{k}": ("max", k)})
    got = hj.group_by_columns(keys, table_cols, aggs, nulls=nulls, key_mask=0xFFF)
    assert (got["n_groups"], got["null_rows"]) == (m, want["null_rows"]) and np.array_equal(got["first_rows"], want["first_rows"])
    for k, v in sources.items():
        count, seen, total, lo, hi = numpy_aggregates(want, v, valid.get(k), signed=v.dtype.kind == "i")
        assert np.array_equal(got["count"], count) and np.array_equal(got["rows"], count) and np.array_equal(got[f"n_{k}"], seen), k
        for name, ref in ((f"sum_{k}", total), (f"min_{k}", lo), (f"max_{k}", hi)):
            assert got[name].values.dtype == ref.dtype, name
            same_column(got[name], ref, seen > 0, (name, nulls))
    # the keys of the groups, and distinct_on with payload columns through the same first rows
    payload = {"p2": rng.integers(0, 1 << 16, n).astype(np.uint16), "ps": k2.key_column(gc.string_col(rng, n, 50, nulls=0.2)),
               "pf": rng.random(n)}
    d = hj.distinct_on(keys, payload, nulls=nulls)
    first = want["first_rows"].astype(np.int64)
    assert np.array_equal(d["first_rows"], want["first_rows"]) and (d["n_groups"], d["null_rows"]) == (m, want["null_rows"])
    for res in (got, d):
        for c, k in zip(cols, res["keys"]):
            assert isinstance(k, hj.KeyColumn) and k.to_list() == [c.items[i] for i in first]
    assert d["cols"]["p2"].dtype == np.uint16 and np.array_equal(d["cols"]["p2"], payload["p2"][first])
    assert d["cols"]["pf"].tobytes() == payload["pf"][first].tobytes()
    strings = payload["ps"].to_list()
    assert d["cols"]["ps"].to_list() == [strings[i] for i in first]
    gc.same(hj.key_groups(keys, nulls=nulls), want, "key_groups")


def test_everything_dropped():
    """every row NULL-keyed: no group, nothing to aggregate into"""
    keys = hj.KeyColumn(np.arange(100, dtype=U32), valid=np.zeros(100, dtype=bool))
    got = hj.group_by_columns(keys, {"v": np.arange(100, dtype=np.int64)}, {"s": ("sum", "v")}, nulls="drop")
    assert got["n_groups"] == 0 and got["null_rows"] == 100 and got["count"].size == 0 and got["s"].rows == 0 and got["keys"][0].rows == 0
    d = hj.distinct_on(keys, {"v": np.arange(100, dtype=np.int64)}, nulls="drop")
    assert d["first_rows"].size == 0 and d["cols"]["v"].size == 0
    one = hj.group_by_columns(keys, {"v": np.arange(100, dtype=np.int64)}, {"s": ("sum", "v")}, nulls="group")
    assert one["n_groups"] == 1 and one["count"].tolist() == [100] and one["s"].values.tolist() == [4950] and one["keys"][0].to_list() == [None]


# ---- stream order ----------------------------------------------------------------------------------------------------------------
def test_stream_order(fl):
    """decoy keys (all distinct) before the delay, the real keys (few, repeated) behind it on the caller's stream: a call
    that read early, or a table filled out of order, answers for the decoys"""
    n = 1 << 14
    rng = np.random.default_rng(14)
    real = rng.integers(0, 300, n).astype(U64) << U64(33)
    warm = rng.integers(0, 77, n).astype(U64) + U64(1 << 60)
    decoy = np.arange(n, dtype=U64) + U64(1 << 40)
    want = gc.model_groups(gc.array_keys([real]))
    m = want["n_groups"]
    assert m == 300
    vp = lambda p: C.c_void_p(p) if p else None     # noqa: E731
    with hj.HashJoinContext(0, stream=fl.handle) as ctx:
        st = so.Stage(fl.stream)
        keys = st.buf(decoy, real=real, warm=warm)
        rep, group, first = st.out(n, U32, so.SENT32), st.out(n, U32, so.SENT32), st.out(n, U32, so.SENT32)

        def seq(which):
            cols = (_lib.hj_key_col2 * 1)()
            cols[0].s, cols[0].width = keys.ptr, 8
            rc = lib.hj_key_groups_dev(ctx._h, cols, 1, _lib.HJ_KEY_SIDE_S, n, 0, vp(rep.ptr), vp(group.ptr), vp(first.ptr), n)
            C.memset(cols, 0, C.sizeof(cols))
            if rc != _lib.HJ_OK:
                raise hj.HashJoinError(rc, lib.hj_last_error(ctx._h).decode())

        assert so.contract()["hj_key_groups_dev"][0] == "asynchronous"
        so.run_delayed([st], seq, True, f"key_groups.{fl.name}")
        st.check_inputs_intact()
        info = ctx.key_groups_info()
    assert (info["groups"], info["written"], info["failure"]) == (m, m, 0)
    assert np.array_equal(st.result(rep, U32, "rep"), want["rep"]) and np.array_equal(st.result(group, U32, "group"), want["group"])
    rows = st.result(first, U32, "first rows")
    assert np.array_equal(rows[:m], want["first_rows"]) and (rows[m:] == so.SENT32).all()
