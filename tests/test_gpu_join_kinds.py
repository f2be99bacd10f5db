"""Left-outer, semi and anti joins out of the materialising table probes (hj_probe_join_dev) through ctypes -> C ABI on an
MI355X. Expected rows never come from the library: the inner pairs are computed HERE with numpy / plain Python
(join_expected, walk_expected: restated from test_gpu_pairs.py), and every kind is derived from them --
matched = the unique S rows of the inner pairs, left = inner + (s, NO_ROW) for the unmatched s of the slice, semi =
matched, anti = the rest of the slice. LEFT is compared as sorted s << 32 | r, SEMI and ANTI as sorted s, element for
element. Every plane has sentinel words behind its capacity; SEMI and ANTI must leave the whole R plane alone. found,
the unmatched count of hj_pairs_info and totalMatches (the INNER count, whatever the kind) are asserted on every call.
Run with -m gpu."""
import functools

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from oracle import oracle

pytestmark = pytest.mark.gpu

from gpu_harness import Device, ctx, status  # noqa: F401
from join_kinds_common import (SENTINEL, GUARD, U64, INNER, LEFT, SEMI, ANTI, KINDS, NAMES, NO_ROW, Calls, derive, matched_rows,
                               zipf,
                               planes)
from r_marks_common import join_expected, walk_expected, inner_expected


def run_all_kinds(ctx, algo, R, S, inner, probe_length=4, kinds=KINDS, offset=0, tag=None, **reserve):
    """build R, then every kind over S passed at dS + 8 * offset bytes (S = buf[offset:])"""
    with Device(ctx) as dev:
        ctx.reserve(algo, R.size, max(S.size, 1), probeLength=probe_length, keepRowIds=True, **reserve)
        buf = np.concatenate([np.zeros(offset, dtype=U64), S])
        dR, dS = dev.put(R), dev.put(buf)
        ctx.build(dR, R.size)
        calls = Calls(ctx, dev)
        for kind in kinds:
            calls.call(kind, dS + 8 * offset, S.size, inner, tag=tag)


# ---------------------------------------------------------------------------------------------------------------------
# htm: bucket plus the whole chain
# ---------------------------------------------------------------------------------------------------------------------
def _htm_case(name):
    g = oracle.generate_data
    if name == "uniform_1000_x_sorted_1500":                  # rSize not a power of two; S keys absent from R
        return g("uniform", 1 << 10, 1 << 10, 16)[:1000], g("sorted", 2048)[:1500]
    if name == "random_2p16_x_self_and_sorted":               # 32-bit keys; half of S is absent from R
        R = g("random", 1 << 16, 1 << 16, 16)
        return R, np.concatenate([R[::2], g("sorted", 1 << 15)[:30000]])
    raise KeyError(name)


@pytest.mark.parametrize("name", ["uniform_1000_x_sorted_1500", "random_2p16_x_self_and_sorted"])
def test_htm_all_kinds(ctx, name):
    R, S = _htm_case(name)
    inner = join_expected(R, S)
    assert 0 < matched_rows(inner).size < S.size
    run_all_kinds(ctx, "htm", R, S, inner, tag=name)


def test_htm_long_chains(ctx):
    """A chain of more than 1000 buckets, met by: its hot key (every bucket matches: SEMI must write one row, not one per
    bucket), keys of the same bucket that R does not hold (the chain is walked to its end without a match: LEFT and ANTI
    must write one row, at the end, not one per bucket), and Zipf draws."""
    R = zipf(1 << 16, 1 << 12, 1.0, 12345)
    counts = np.bincount(R.astype(np.int64))
    hot = int(counts.argmax())
    assert counts[hot] > 3000                                 # 3 tuples per bucket: more than 1000 buckets
    buckets = 1 << int(np.ceil(np.log2(R.size // 3 + 1)))     # nextpow2(rSize / 3 + 1), HTMHashBuild.hpp:61-62
    # the hot key's bucket is (hot / 3) & (buckets - 1): keys k above the 2^12 alphabet with k / 3 = hot / 3 + j * buckets
    absent = np.array([3 * (hot // 3 + j * buckets) + d for j in (1, 2, 5) for d in (0, 1, 2)], dtype=U64)
    near = np.array([k for k in range(3 * (hot // 3), 3 * (hot // 3) + 3) if k and (k >= counts.size or counts[k] == 0)], dtype=U64)
    assert absent.min() > 1 << 12 and absent.max() < 1 << 32 and not np.isin(absent, R).any()
    S = np.concatenate([np.array([hot], dtype=U64), absent, near, zipf(1 << 12, 1 << 12, 1.0, 12345),
                        np.array([hot], dtype=U64), absent[:1]])
    inner = join_expected(R, S)
    with Device(ctx) as dev:
        ctx.reserve("htm", R.size, S.size)
        dR, dS = dev.put(R), dev.put(S)
        ctx.build(dR, R.size)
        assert ctx.fetch()["htmBuckets"] == buckets
        calls = Calls(ctx, dev)
        for kind in KINDS:
            calls.call(kind, dS, S.size, inner, tag="long_chains")


# ---------------------------------------------------------------------------------------------------------------------
# open addressing: the reference's walk, both walk instantiations
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("probe_length", [1, 2, 4, 8])
@pytest.mark.parametrize("dist", ["uniform", "random"])
@pytest.mark.parametrize("n", [1 << 10, 1 << 14])
def test_open_addressing_all_kinds(ctx, dist, n, probe_length):
    """duplicate keys in R (several rows per S tuple), R tuples that ran out of budget (an S tuple whose key R holds and the
    table does not is unmatched), S keys absent from R"""
    R = oracle.generate_data(dist, n, n, 16)
    S = np.concatenate([R[: n // 2 + 1], oracle.generate_data("sorted", n)])
    inner = walk_expected(R, S, probe_length)
    assert inner.size == oracle.build_probe_seq(R, S, probe_length)["totalMatches"]
    assert 0 < matched_rows(inner).size < S.size
    run_all_kinds(ctx, "atomic", R, S, inner, probe_length, tag=(dist, n, probe_length))


# ---------------------------------------------------------------------------------------------------------------------
# lanes without an element are not unmatched rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,probe_length", [("htm", 4), ("atomic", 4), ("atomic", 8)])      # 8: the walk with the early exit
@pytest.mark.parametrize("offset", [1, 0])
@pytest.mark.parametrize("n", [1, 2, 3, 1023, 1025, 2049])
def test_padding_lanes_write_no_rows(ctx, n, offset, algo, probe_length):
    """offset 1: S starts 8 bytes behind a 16-byte boundary, so S[0] is the head element (and with an even n there is a
    tail element too); offset 0 with an odd n: S[n - 1] is the tail element. Both are read by one thread of workgroup 0
    while 255 threads hold nothing, and the last round of the body is padded. S[0] and S[n - 1] are absent from R."""
    R = oracle.generate_data("sorted", 1 << 11)
    S = oracle.generate_data("sorted", 1 << 12)[:n].copy()
    S[1::3] += U64(5000)                                      # a third of the body is absent as well
    S[0] = U64(7001)
    S[n - 1] = U64(7003)
    inner = inner_expected(algo, R, S, probe_length)
    assert not np.isin(matched_rows(inner), [0, n - 1]).any()
    run_all_kinds(ctx, algo, R, S, inner, probe_length, offset=offset, tag=(algo, n, offset))


# ---------------------------------------------------------------------------------------------------------------------
# nothing and everything
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_nothing_and_everything(ctx, algo):
    """S entirely absent from R: INNER and SEMI produce nothing and leave both planes untouched (Calls.call checks every
    word of them), LEFT is all NO_ROW, ANTI is all of S. S = R: ANTI produces nothing."""
    n = 1 << 12
    R = oracle.generate_data("shuffle", n, n, 16)
    absent = oracle.generate_data("sorted", 4 * n)[3 * n: 3 * n + n - 3]
    none = inner_expected(algo, R, absent)
    assert none.size == 0
    run_all_kinds(ctx, algo, R, absent, none, tag="nothing")
    every = inner_expected(algo, R, R)
    assert matched_rows(every).size == n
    run_all_kinds(ctx, algo, R, R, every, tag="everything")


# ---------------------------------------------------------------------------------------------------------------------
# more rows per workgroup than a stage holds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [LEFT, ANTI])
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_stage_flushes_mid_run(ctx, algo, kind):
    """2^23 S tuples of which all but 2^10 are unmatched: thousands of rows per workgroup, so the stage flushes many times.
    Checked without sorting pairs: every S row once, its R row where it belongs."""
    nr, ns = 1 << 10, 1 << 23
    R = oracle.generate_data("sorted", nr)
    S = oracle.generate_data("sorted", ns)
    assert np.array_equal(R, np.arange(1, nr + 1, dtype=U64)) and np.array_equal(S, np.arange(1, ns + 1, dtype=U64))
    # key k sits in R row k - 1; for open addressing in slot k of 2048, and a key above 1024 meets other keys or empty slots
    want_r = np.full(ns, 0xFFFFFFFF, dtype=np.uint32)
    want_r[:nr] = np.arange(nr, dtype=np.uint32)
    rows = ns if kind == LEFT else ns - nr
    with Device(ctx) as dev:
        ctx.reserve(algo, nr, ns, keepRowIds=True)
        dR, dS = dev.put(R), dev.put(S)
        ctx.build(dR, nr)
        ds, dr = (p.ptr for p in planes(dev, rows))
        ctx.probe_pairs(dS, ns, ds, dr, rows, kind=kind)
        found, written, _us, unmatched = ctx.pairs_info()
        s, r = dev.get(ds, rows + GUARD), dev.get(dr, rows + GUARD)
        got = ctx.fetch()
    assert (found, written, unmatched) == (rows, rows, ns - nr)
    assert (got["totalMatches"], got["sSize"]) == (nr, ns)
    assert (s[rows:] == SENTINEL).all()
    count = np.bincount(s[:rows], minlength=ns)
    if kind == LEFT:
        assert count.size == ns and (count == 1).all()
        assert (r[rows:] == SENTINEL).all()
        by_s = np.empty(ns, dtype=np.uint32)
        by_s[s[:rows]] = r[:rows]
        assert np.array_equal(by_s, want_r)
    else:
        assert (r == SENTINEL).all()
        assert count.size == ns and (count[:nr] == 0).all() and (count[nr:] == 1).all()


# ---------------------------------------------------------------------------------------------------------------------
# capacity
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_capacity_cuts_the_output_and_nothing_else(ctx, algo, kind):
    n = 1 << 16
    R, S, inner = _capacity_case(algo)
    want = derive(kind, inner, n)
    assert want.size > 2
    with Device(ctx) as dev:
        ctx.reserve(algo, n, n, keepRowIds=True)
        dR, dS = dev.put(R), dev.put(S)
        ctx.build(dR, n)
        calls = Calls(ctx, dev)
        for capacity in (want.size, want.size + 1, want.size - 1, want.size // 2, 1, 0):
            rows = calls.call(kind, dS, n, inner, capacity=capacity, tag=algo)
            assert rows.size == min(want.size, capacity)
        ctx.probe_pairs(dS, n, 0, 0, 0, kind=kind)           # capacity 0 with NULL planes: counts only
        info = ctx.pairs_info()
        assert info[:2] == (want.size, 0) and info[3] == (0 if kind == INNER else n - matched_rows(inner).size)
        got = ctx.fetch()
    assert (got["totalMatches"], got["sSize"]) == (7 * inner.size, 7 * n)


@functools.lru_cache(maxsize=2)
def _capacity_case(algo):
    n = 1 << 16
    R = oracle.generate_data("uniform", n, n, 16)            # duplicate keys; about a third of 1..n is absent
    S = oracle.generate_data("sorted", n)
    return R, S, inner_expected(algo, R, S)


# ---------------------------------------------------------------------------------------------------------------------
# tuples outside the layout are unmatched rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_tuples_outside_the_layout_are_unmatched(ctx, algo):
    n = 1 << 12
    R = oracle.generate_data("sorted", n)
    S = oracle.generate_data("sorted", n).copy()
    S[5] = 0
    S[6] |= U64(1) << U64(32)
    S[7] = U64(7) << U64(32)
    S[n - 1] |= U64(1) << U64(63)
    outside = np.array([5, 6, 7, n - 1], dtype=U64)
    for off in (0, 1):                                     # 16-byte aligned start, and a start on the odd tuple
        Sx = S[off:]
        inner = join_expected(R, Sx)
        assert inner.size == n - 4 - off
        out_rows = outside - U64(off)
        assert np.array_equal(derive(ANTI, inner, Sx.size), out_rows)
        assert not np.isin(out_rows, derive(SEMI, inner, Sx.size)).any()
        assert np.isin((out_rows << U64(32)) | NO_ROW, derive(LEFT, inner, Sx.size)).all()
        run_all_kinds(ctx, algo, R, Sx, inner, offset=off, tag=("outside", off))


# ---------------------------------------------------------------------------------------------------------------------
# slices
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_ragged_slices_add_up_to_the_whole(ctx, algo):
    n = 1 << 15
    R = oracle.generate_data("uniform", n, n, 16)
    S = oracle.generate_data("uniform", n, 2 * n, 16)[: n - 5]            # half of the key range is absent from R
    whole = inner_expected(algo, R, S)
    cuts = [0, 1001, 1001 + 20000, 1001 + 20000 + 1, S.size]              # unequal slices; three start at odd rows
    with Device(ctx) as dev:
        ctx.reserve(algo, n, S.size, keepRowIds=True)
        dR, dS = dev.put(R), dev.put(S)
        ctx.build(dR, n)
        calls = Calls(ctx, dev)
        for kind in KINDS:
            parts = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                lo, hi = np.searchsorted(whole, [U64(a) << U64(32), U64(b) << U64(32)])
                parts.append(calls.call(kind, dS + 8 * a, b - a, whole[lo:hi], s_base=a, tag=algo))
            assert np.array_equal(np.sort(np.concatenate(parts)), derive(kind, whole, S.size)), (algo, kind)


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    n = 1 << 12
    R = oracle.generate_data("local_shuffle", n, n, 16)
    S = oracle.generate_data("sorted", 2 * n)[n // 2: n // 2 + n]
    with hj.HashJoinContext(0) as ctx, Device(ctx) as dev:
        dR, dS = dev.put(R), dev.put(S)
        ds, dr = (p.ptr for p in planes(dev, n))
        for kind in KINDS:
            # a PRJ context, with and without a resident R
            ctx.reserve("prj", n, n, keepRowIds=True)
            assert status(ctx.probe_pairs, dS, n, ds, dr, n, kind=kind) == _lib.HJ_ERR_STATE
            ctx.prj_build(dR, n)
            assert status(ctx.probe_pairs, dS, n, ds, dr, n, kind=kind) == _lib.HJ_ERR_STATE
            # open addressing without the flag: refused before and after the build, and nothing is counted
            ctx.reserve("atomic", n, n)
            assert status(ctx.probe_pairs, dS, n, ds, dr, n, kind=kind) == _lib.HJ_ERR_STATE
            ctx.build(dR, n)
            assert status(ctx.probe_pairs, dS, n, ds, dr, n, kind=kind) == _lib.HJ_ERR_STATE
            got = ctx.fetch()
            assert (got["totalMatches"], got["sSize"]) == (0, 0)
        # with the flag
        ctx.reserve("atomic", n, n, keepRowIds=True)
        ctx.build(dR, n)
        for kind in (4, 5, 0xFFFFFFFF):
            assert status(ctx.probe_pairs, dS, n, ds, dr, n, kind=kind) == _lib.HJ_ERR_INVALID
            assert status(ctx.probe_pairs, dS, n, 0, 0, 0, kind=kind) == _lib.HJ_ERR_INVALID
        for kind in KINDS:
            assert status(ctx.probe_pairs, dS, n, 0, dr, n, kind=kind) == _lib.HJ_ERR_INVALID
            assert status(ctx.probe_pairs, dS, n, ds, dr, n, s_idx_base=(1 << 32) - n, kind=kind) == _lib.HJ_ERR_INVALID
        for kind in (INNER, LEFT):                            # the R plane is needed where it is written ...
            assert status(ctx.probe_pairs, dS, n, ds, 0, n, kind=kind) == _lib.HJ_ERR_INVALID
        got = ctx.fetch()
        assert (got["totalMatches"], got["sSize"]) == (0, 0)                 # nothing of the refused calls was counted
        assert (dev.get(ds, n + GUARD) == SENTINEL).all() and (dev.get(dr, n + GUARD) == SENTINEL).all()
        inner = walk_expected(R, S, 4)
        for k, kind in enumerate((SEMI, ANTI)):               # ... and may be NULL where it is not
            assert status(ctx.probe_pairs, dS, n, ds, 0, n, kind=kind) == _lib.HJ_OK
            found, written = ctx.pairs_info()[:2]
            want = derive(kind, inner, n)
            assert found == written == want.size
            assert np.array_equal(np.sort(dev.get(ds, n)[:written].astype(U64)), want)
            # sSize 0: a no-op for every kind
            before = ctx.fetch()
            ctx.probe_pairs(dS, 0, ds, dr, n, kind=kind)
            ctx.probe_pairs(0, 0, 0, 0, 0, kind=kind)
            after = ctx.fetch()
            assert (after["totalMatches"], after["sSize"]) == (before["totalMatches"], before["sSize"]) == ((k + 1) * inner.size, (k + 1) * n)
            assert ctx.pairs_info()[:2] == (found, written)
        assert (dev.get(dr, n + GUARD) == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------------------------
# inner is inner
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_inner_is_the_pairs_probe(ctx, algo):
    n = 1 << 14
    R = oracle.generate_data("uniform", n, n, 16)
    S = oracle.generate_data("uniform", n, 2 * n, 16)[: n - 3]
    want = inner_expected(algo, R, S)
    got = []
    with Device(ctx) as dev:
        ctx.reserve(algo, n, S.size, keepRowIds=True)
        dR, dS = dev.put(R), dev.put(S)
        ctx.build(dR, n)
        ctx.probe_pairs(dS, S.size, 0, 0, 0, kind=LEFT)      # a kind call in front: its unmatched count must not stick
        assert ctx.pairs_info()[3] == S.size - matched_rows(want).size
        for entry in ("hj_probe_join_dev", "hj_probe_pairs_dev"):
            ds, dr = (p.ptr for p in planes(dev, want.size + 64))
            args = (ds, dr, want.size + 64)
            if entry == "hj_probe_join_dev":
                rc = hj.lib.hj_probe_join_dev(ctx._h, INNER, dS, S.size, 0, *args)
            else:
                rc = hj.lib.hj_probe_pairs_dev(ctx._h, dS, S.size, 0, *args)
            assert rc == _lib.HJ_OK
            info = ctx.pairs_info()
            s, r = dev.get(ds, want.size + 64 + GUARD), dev.get(dr, want.size + 64 + GUARD)
            assert (s[info[1]:] == SENTINEL).all() and (r[info[1]:] == SENTINEL).all()
            got.append((info[:2], info[3], np.sort((s[:info[1]].astype(U64) << U64(32)) | r[:info[1]].astype(U64))))
        res = ctx.fetch()
    assert got[0][0] == got[1][0] == (want.size, want.size) and got[0][1] == got[1][1] == 0
    assert np.array_equal(got[0][2], want) and np.array_equal(got[1][2], want)
    assert res["totalMatches"] == 3 * want.size and res["sSize"] == 3 * S.size


# ---------------------------------------------------------------------------------------------------------------------
# host-buffer convenience
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_join_pairs_round_trip(algo):
    n = 1 << 13
    R = oracle.generate_data("uniform", n, n // 4, 16)
    S = oracle.generate_data("uniform", n, n // 2, 16)[: n - 7]           # ~4 R copies per key, half of the keys absent from R
    inner = inner_expected(algo, R, S, 2)
    assert derive(LEFT, inner, S.size).size > S.size         # more rows than the |S| the outputs start with: they grow once
    for kind in KINDS:
        s_idx, r_idx = hj.join_pairs(R, S, algo=algo, probeLength=2, how=NAMES[kind])
        want = derive(kind, inner, S.size)
        assert s_idx.dtype == np.uint32 and s_idx.size == want.size
        if kind in (SEMI, ANTI):
            assert r_idx is None
            assert np.array_equal(np.sort(s_idx.astype(U64)), want)
            continue
        assert r_idx.dtype == np.uint32 and r_idx.size == s_idx.size
        assert np.array_equal(np.sort((s_idx.astype(U64) << U64(32)) | r_idx), want)
        hit = r_idx != hj.NO_ROW
        assert np.array_equal(S[s_idx[hit]], R[r_idx[hit]])                # the gather maps do what they are for
        assert hit.all() if kind == INNER else (~hit).sum() == S.size - matched_rows(inner).size
