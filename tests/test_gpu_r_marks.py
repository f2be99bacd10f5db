"""R-side match marks on the table paths (HJ_FLAG_TRACK_R_MATCHES, hj_r_rows_dev, hj_r_marks_clear) through ctypes -> C ABI
on an MI355X. Expected values never come from the library: the inner pairs are computed with numpy / plain Python
(r_marks_common), the matched R rows are their unique R words, the unmatched ones the rest of [base, base + rSize). Every
probe call goes through join_kinds_common.Calls, which checks its rows, hj_pairs_info and hj_result (totalMatches, sSize)
exactly as on a context without the flag; every sweep has sentinel words behind its capacity. Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from oracle import oracle

from gpu_harness import Device, ctx, status  # noqa: F401
from r_marks_common import (SENTINEL, GUARD, U64, INNER, LEFT, SEMI, ANTI, UNMATCHED, MATCHED, SWEEP_ROWS, Calls, Marks, zipf,
                            inner_expected, join_expected, r_rows_of)

pytestmark = pytest.mark.gpu


def tracked(ctx, dev, algo, R, s_max, probe_length=4, idx_base=0):
    """reserve with the flag, build R -> (dR, Calls, Marks)"""
    ctx.reserve(algo, R.size, max(s_max, 1), probeLength=probe_length, keepRowIds=True, trackRMatches=True)
    dR = dev.put(R)
    ctx.build(dR, R.size, idx_base)
    return dR, Calls(ctx, dev), Marks(ctx, dev, R.size, idx_base)


# ---------------------------------------------------------------------------------------------------------------------
# the last word of the plane
# ---------------------------------------------------------------------------------------------------------------------
# open addressing takes a power of two only (hj_reserve): 1 and 32 of the sizes asked for, and 1024 for 1000
@pytest.mark.parametrize("algo,n", [("htm", n) for n in (1, 31, 32, 33, 1000)] + [("atomic", n) for n in (1, 32, 1024)])
def test_last_word_of_the_plane(ctx, algo, n):
    """no probe: every row unmatched, none beyond rSize; every second row probed; every row probed: the complement of a
    full plane must not invent the rows of the last word's unused bits"""
    R = np.arange(1, n + 1, dtype=U64)
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, algo, R, 2 * n)
        marks.check((algo, n, "no probe"))
        for S in (np.concatenate([R[::2], R[:1] + U64(5000)]), R):
            inner = inner_expected(algo, R, S)
            calls.call(INNER, dev.put(S), S.size, inner, tag=(algo, n))
            marks.add(inner)
            marks.check((algo, n, S.size))
        assert marks.expected(UNMATCHED).size == 0 and marks.expected(MATCHED).size == n


# ---------------------------------------------------------------------------------------------------------------------
# row base; open addressing's dropped tuples
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_row_base(ctx, algo):
    """idxBase 5000: the rows come back with the base, the bit index has it subtracted; sIdxBase 77777 stays in the S plane"""
    n, r_base, s_base = 1 << 10, 5000, 77777
    R = oracle.generate_data("uniform", n, n, 16)
    S = oracle.generate_data("sorted", 2 * n)[5: n + 300]
    inner = inner_expected(algo, R, S, r_base=r_base, s_base=s_base)
    assert r_rows_of(inner).min() >= r_base and 0 < r_rows_of(inner).size < n
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, algo, R, S.size, idx_base=r_base)
        calls.call(LEFT, dev.put(S), S.size, inner, s_base=s_base, tag=algo)
        marks.add(inner)
        marks.check(algo)
        assert marks.expected(UNMATCHED).min() >= r_base and marks.expected(UNMATCHED).max() < r_base + n


@pytest.mark.parametrize("probe_length", [4, 1, 8])
def test_open_addressing_dropped_tuples_are_unmatched(ctx, probe_length):
    """a `uniform` R of 2^10 has duplicate keys and conflicts; S holds every key of R. What the build dropped, and what
    the walk does not reach, is unmatched. probeLength 1 and 8 take the generic walk."""
    n = 1 << 10
    R = oracle.generate_data("uniform", n, n, 16)
    S = np.concatenate([np.unique(R), oracle.generate_data("sorted", n)[::7]])
    inner = inner_expected("atomic", R, S, probe_length)
    conflicts = oracle.build_probe_seq(R, S, probe_length)["conflicts"]
    assert conflicts > 0 or probe_length == 8
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, "atomic", R, S.size, probe_length)
        calls.call(INNER, dev.put(S), S.size, inner, tag=probe_length)
        marks.add(inner)
        assert marks.expected(UNMATCHED).size >= conflicts        # every key of R was probed: the dropped tuples are in here
        marks.check(probe_length)
        assert ctx.fetch()["conflicts"] == conflicts


# ---------------------------------------------------------------------------------------------------------------------
# htm: bucket plus the whole chain
# ---------------------------------------------------------------------------------------------------------------------
def test_htm_1000_x_1500(ctx):
    g = oracle.generate_data
    R, S = g("uniform", 1 << 10, 1 << 10, 16)[:1000], g("sorted", 2048)[:1500]
    inner = join_expected(R, S)
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, "htm", R, S.size)
        calls.call(INNER, dev.put(S), S.size, inner)
        marks.add(inner)
        marks.check("1000x1500")


def test_htm_long_chains(ctx):
    """2^16 tuples over 2^12 keys: every duplicate of a probed key is marked, also the rows that sit deep in a chain of
    more than 1000 buckets; the keys S does not draw leave their rows unmatched"""
    R = zipf(1 << 16, 1 << 12, 1.0, 12345)
    S = zipf(1 << 10, 1 << 12, 1.0, 54321)
    counts = np.bincount(R.astype(np.int64))
    hot = int(counts.argmax())
    assert counts[hot] > 3000 and (S == hot).any()
    inner = join_expected(R, S)
    rows = r_rows_of(inner)
    assert np.array_equal(rows, np.flatnonzero(np.isin(R, S)).astype(U64)) and rows.size < R.size
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, "htm", R, S.size)
        calls.count_only(INNER, dev.put(S), S.size, inner.size, np.unique(inner >> U64(32)).size)
        marks.add(inner)
        marks.check("long chains")


# ---------------------------------------------------------------------------------------------------------------------
# accumulation over slices; the calls that must not mark
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_marks_accumulate_over_inner_and_left_slices_only(ctx, algo):
    n = 1 << 12
    R = oracle.generate_data("shuffle", n, n, 16)
    keys = oracle.generate_data("sorted", 2 * n)
    slices = [keys[0:900], keys[1000:1700], keys[2500:3001]]             # INNER, LEFT, INNER
    other = np.concatenate([keys[3200:3900], keys[n + 5: n + 50]])       # SEMI, ANTI, counting: rows no slice above names
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, algo, R, 1024)
        d_other, inner_other = dev.put(other), inner_expected(algo, R, other)
        assert inner_other.size > 0
        off = 0
        for step, (kind, S) in enumerate(zip((INNER, LEFT, INNER), slices)):
            inner = inner_expected(algo, R, S, s_base=off)
            assert not np.isin(r_rows_of(inner), marks.seen).any() and inner.size > 0
            calls.call(kind, dev.put(S), S.size, inner, s_base=off, tag=(algo, step))
            marks.add(inner)
            marks.check((algo, step))
            off += S.size
            # in between: none of these touches the marks
            if step == 0:
                calls.call(SEMI, d_other, other.size, inner_other, tag="semi")
            elif step == 1:
                calls.call(ANTI, d_other, other.size, inner_other, tag="anti")
            else:
                ctx.probe(d_other, other.size)
                calls.matches += inner_other.size
                calls.s += other.size
                got = ctx.fetch()
                assert (got["totalMatches"], got["sSize"]) == (calls.matches, calls.s)
            marks.check((algo, step, "after a call that does not mark"))
        assert not np.isin(r_rows_of(inner_other), marks.seen).any()


# ---------------------------------------------------------------------------------------------------------------------
# capacity on the probe: rows that are not written mark too
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_rows_cut_by_the_capacity_mark_too(ctx, algo):
    n = 1 << 13
    R = oracle.generate_data("uniform", n, n // 4, 16)                   # ~4 rows per key
    S = oracle.generate_data("uniform", n, n // 2, 16)[: n - 7]
    inner = inner_expected(algo, R, S)
    assert inner.size > 3000                                             # far more rows than the capacities below
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, algo, R, S.size)
        dS = dev.put(S)
        marks.add(inner)
        calls.count_only(INNER, dS, S.size, inner.size, np.unique(inner >> U64(32)).size, tag="capacity 0")
        marks.check((algo, "capacity 0, NULL planes"))
        for kind, capacity in ((INNER, inner.size // 3), (LEFT, 1)):
            ctx.r_marks_clear()
            calls.call(kind, dS, S.size, inner, capacity=capacity, tag=(algo, capacity))
            marks.check((algo, "capacity", capacity))


# ---------------------------------------------------------------------------------------------------------------------
# capacity on the sweep; a sweep of several workgroups
# ---------------------------------------------------------------------------------------------------------------------
def test_sweep_capacity_and_several_blocks(ctx):
    """rSize 100003: 13 workgroups of the sweep, the last word and the last workgroup partial. A capacity below the rows
    yields the first `capacity` rows ascending -- cut inside a workgroup's run, at its end, and inside the first one."""
    n = 100003
    assert n > 12 * SWEEP_ROWS and n % 32
    rng = np.random.default_rng(20261018)
    R = rng.permutation(np.arange(1, n + 1, dtype=U64))
    S = np.arange(1, n + 1, dtype=U64)[rng.random(n) < 0.6]
    inner = join_expected(R, S)
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, "htm", R, S.size)
        calls.count_only(INNER, dev.put(S), S.size, inner.size, S.size)
        marks.add(inner)
        marks.check("100003")
        for which in (UNMATCHED, MATCHED):
            want = marks.expected(which)
            first_run = int((want < SWEEP_ROWS).sum())                    # rows of the first workgroup's run
            for capacity in (want.size - 1, want.size // 2, first_run, 5, 1):
                produced, written, got = marks.sweep(which, capacity)          # no word behind the rows written: Marks.sweep
                print(which, capacity, produced, written)
                assert (produced, written) == (want.size, capacity) and produced > written
                assert np.array_equal(got.astype(U64), want[:capacity])
            assert marks.sweep(which, 0, null_plane=True)[:2] == (want.size, 0)       # only the count comes back
            produced, written, got = marks.sweep(which, 0)
            assert (produced, written) == (want.size, 0) and got.size == 0
        marks.check("after the truncated sweeps")                       # a sweep changes no mark


# ---------------------------------------------------------------------------------------------------------------------
# extremes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_nothing_and_everything(ctx, algo):
    n = 1 << 12
    R = oracle.generate_data("shuffle", n, n, 16)
    absent = oracle.generate_data("sorted", 4 * n)[3 * n: 3 * n + n - 3]
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, algo, R, n)
        marks.check((algo, "no probe at all"))
        none = inner_expected(algo, R, absent)
        assert none.size == 0
        calls.call(LEFT, dev.put(absent), absent.size, none, tag="nothing")
        marks.check((algo, "no S key in R"))
        assert marks.expected(UNMATCHED).size == n
        every = inner_expected(algo, R, R)
        calls.call(INNER, dR, n, every, tag="everything")
        marks.add(every)
        assert marks.expected(UNMATCHED).size == 0
        marks.check((algo, "every row matched"))                        # UNMATCHED: 0 rows, the whole plane untouched


# ---------------------------------------------------------------------------------------------------------------------
# contention: many concurrent marks on one word
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_zipf_probe_marks_exactly(ctx, algo):
    n = 1 << 12
    R = oracle.generate_data("sorted", n)                                # unique keys: key k is row k - 1
    S = zipf(1 << 16, n, 1.0, 54321)
    inner = inner_expected("htm", R, S)                                  # unique keys 1..n: the walk finds each in its home slot
    assert np.bincount((inner & U64(0xFFFFFFFF)).astype(np.int64)).max() > 3000 and r_rows_of(inner).size < n
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, algo, R, S.size)
        calls.call(INNER, dev.put(S), S.size, inner, tag="zipf")
        marks.add(inner)
        marks.check((algo, "zipf"))


# ---------------------------------------------------------------------------------------------------------------------
# clearing
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_clearing(ctx, algo):
    n = 1 << 11
    R = oracle.generate_data("shuffle", n, n, 16)
    S = oracle.generate_data("sorted", n)[100:1500]
    inner = inner_expected(algo, R, S)
    with Device(ctx) as dev:
        dR, calls, marks = tracked(ctx, dev, algo, R, S.size)
        dS = dev.put(S)
        calls.call(INNER, dS, S.size, inner)
        marks.add(inner)
        marks.check("first")
        marks.check("the same rows twice in a row")
        ctx.r_marks_clear()
        marks.clear()
        marks.check("after hj_r_marks_clear")
        got = ctx.fetch()
        assert (got["totalMatches"], got["sSize"]) == (inner.size, S.size)   # the clear and the sweeps touched no counter
        calls.call(LEFT, dS, S.size, inner)
        marks.add(inner)
        marks.check("marked again")
        ctx.build(dR, n)                                                # a rebuild on the same context
        marks.clear()
        marks.check("after a rebuild")
        assert marks.sweep(UNMATCHED)[:2] == (n, n)


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    n = 1 << 10
    R = oracle.generate_data("sorted", n)
    with hj.HashJoinContext(0) as c, Device(c) as dev:
        dR = dev.put(R)
        d_rows = dev.put(np.full(n + GUARD, SENTINEL, dtype=np.uint32))
        d_keys = dev.put(R.astype(np.uint32))
        # open addressing with the flag but without the row ids: refused at hj_reserve; htm takes the flag alone
        for algo in ("atomic", "nocc"):
            assert status(c.reserve, algo, n, n, trackRMatches=True) == _lib.HJ_ERR_INVALID
        assert status(c.reserve, "htm", n, n, trackRMatches=True) == _lib.HJ_OK
        # reserved without the flag
        for algo in ("atomic", "htm"):
            c.reserve(algo, n, n, keepRowIds=True)
            c.build(dR, n)
            assert status(c.r_rows, UNMATCHED, d_rows, n) == _lib.HJ_ERR_STATE
            assert status(c.r_rows_info) == _lib.HJ_ERR_STATE
            assert status(c.r_marks_clear) == _lib.HJ_ERR_STATE
        # with the flag: no build yet
        with hj.HashJoinContext(0) as fresh:
            fresh.reserve("atomic", n, n, keepRowIds=True, trackRMatches=True)
            assert status(fresh.r_rows, UNMATCHED, 0, 0) == _lib.HJ_ERR_STATE
        c.reserve("atomic", n, n, keepRowIds=True, trackRMatches=True)
        assert status(c.build_keys, d_keys, n, 0, 2 * n) == _lib.HJ_ERR_STATE
        c.build(dR, n)
        assert status(c.r_rows, 2, d_rows, n) == _lib.HJ_ERR_INVALID
        assert status(c.r_rows, 0xFFFFFFFF, d_rows, n) == _lib.HJ_ERR_INVALID
        assert status(c.r_rows, UNMATCHED, 0, n) == _lib.HJ_ERR_INVALID          # NULL plane with capacity > 0
        assert status(c.build_keys, d_keys, n, 0, 2 * n) == _lib.HJ_ERR_STATE
        assert c.r_rows_info() == (0, 0, 0, n)                                    # no sweep ran
        assert (dev.get(d_rows, n + GUARD) == SENTINEL).all()
        c.r_rows(UNMATCHED, d_rows, n)
        assert c.r_rows_info()[:2] == (n, n) and np.array_equal(dev.get(d_rows, n), np.arange(n, dtype=np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# host-buffer convenience
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["htm", "atomic"])
def test_outer_join_pairs_end_to_end(algo):
    """2^12 x 2^12: half of S is absent from R, a quarter of R is not probed"""
    n = 1 << 12
    R = oracle.generate_data("shuffle", n, n, 16)
    keys = np.concatenate([np.arange(1, 3 * n // 4 + 1, dtype=U64)[::2][: n // 2], np.arange(2 * n + 1, 2 * n + n // 2 + 1, dtype=U64)])
    S = np.random.default_rng(7).permutation(np.concatenate([keys, keys[: n - keys.size]]))[:n]
    inner = inner_expected(algo, R, S)
    matched = r_rows_of(inner)
    unmatched = np.setdiff1d(np.arange(n, dtype=U64), matched, assume_unique=True)
    assert unmatched.size >= n // 4 and np.unique(inner >> U64(32)).size <= n // 2 + 1
    no_row = U64(hj.NO_ROW)
    left = np.sort(np.concatenate([inner, (np.setdiff1d(np.arange(n, dtype=U64), np.unique(inner >> U64(32))) << U64(32)) | no_row]))
    for how, head, tail in (("right", inner, unmatched), ("full", left, unmatched)):
        s_idx, r_idx = hj.outer_join_pairs(R, S, algo=algo, how=how)
        assert s_idx.dtype == r_idx.dtype == np.uint32 and s_idx.size == r_idx.size == head.size + tail.size
        k = head.size
        assert np.array_equal(np.sort((s_idx[:k].astype(U64) << U64(32)) | r_idx[:k]), head), how
        assert (s_idx[k:] == hj.NO_ROW).all() and np.array_equal(r_idx[k:].astype(U64), tail), how
    for how, want in (("right_semi", matched), ("right_anti", unmatched)):
        s_idx, r_idx = hj.outer_join_pairs(R, S, algo=algo, how=how)
        assert s_idx is None and r_idx.dtype == np.uint32 and np.array_equal(r_idx.astype(U64), want), how
