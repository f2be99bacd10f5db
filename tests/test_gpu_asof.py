"""hj_pairs_asof_dev / hj_asof_info through ctypes -> C ABI on an MI355X, against the model of asof_common.py and against
hj_pairs_asof_host on the same buffers. Every output plane, mark plane and best plane has sentinel words around it that
must survive; the maps are unwritten. Run with -m gpu.

hj_asof.hip: a workgroup of each of the three kernels takes kFilterBlockPairs = 1024 consecutive pairs, a wavefront 256 of
them as four steps of 64 -- the pair counts below are the lane step, the wavefront's share, the workgroup's share and more
than four workgroups, each with its neighbours. k_asof_best combines the pairs of one S row that are neighbours within a
step of 64 before it issues an atomic: the runs below cross steps, wavefronts and workgroups, and come scattered too."""
import ctypes as C

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

import asof_common as ac
import where_common as wc
from gpu_harness import Device, GuardedPlane, check_pair_filter, ctx, plane_words, status  # noqa: F401

pytestmark = pytest.mark.gpu

U32, U64, NO_ROW = np.uint32, np.uint64, wc.NO_ROW
GUARD = 64                      # sentinel words around a plane
N_PAIRS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
N_S, N_R = 1500, 1100           # rows of the relations: neither a multiple of 32
INVALID = _lib.HJ_ERR_INVALID


def run(ctx, map_s, map_r, base, s_rows, r_rows, term, capacity=None, marks=True, offset=0, tag=None):
    """one hj_pairs_asof_dev over numpy inputs, checked in full against the model and the host form -> the model's dict"""
    n = map_s.size
    want = ac.model_call(map_s, map_r, base, s_rows, r_rows, term, capacity)
    cap = n if capacity is None else capacity
    s, op, r, s_valid, r_valid = term
    host = None
    if s_rows == s.size and r_rows == r.size:
        host = lambda: hj.pairs_asof_host(map_s, map_r, base, (hj.KeyColumn(s, s_valid), op, hj.KeyColumn(r, r_valid)), capacity=cap, marks=True)   # noqa: E731
    with Device(ctx) as dev:
        d_term = (dev.put(s), dev.put(r), s.dtype.itemsize, wc.TYPE_OF[s.dtype.kind], _lib.CMP_OPS[op],
                  dev.put(plane_words(s_valid)) if s_valid is not None else 0, dev.put(plane_words(r_valid)) if r_valid is not None else 0)
        # the best planes hold junk before the call: it initialises them itself. bestVal: 64-bit words behind a guard of 64 words
        outside = "a word outside a best plane was written"
        best = [("best_val", GuardedPlane(dev, 2 * s_rows, front=GUARD, behind=GUARD, body=0x33333333, what=outside), None, None),
                ("best_row", GuardedPlane(dev, s_rows, front=GUARD, behind=GUARD, body=0, what=outside), want["best_row"],
                 "bestRow: the left-outer as-of map")]
        call = lambda ms, mr, os, o_r, c, ps, pr, bv, br: ctx.pairs_asof(ms, mr, n, base, s_rows, r_rows, d_term, bv, br, os, o_r, c, ps, pr)   # noqa: E731
        check_pair_filter(dev, call, ctx.asof_info, map_s, map_r, s_rows, r_rows, want, cap, GUARD, offset=offset, marks=marks, extra=best,
                          host=host, tag=tag)
    return want


def relation(rng, dtype, n, span=12):
    """n values of dtype around the middle of a small range: every op finds eligible pairs, rejects others and meets ties"""
    dtype = np.dtype(dtype)
    v = rng.integers(0, span, n)
    return (v - span // 2).astype(dtype) if dtype.kind != "u" else v.astype(dtype)


def unique_pairs(rng, n, n_s=N_S, n_r=N_R, base=0):
    """n distinct (s, r), as a join gives them, in random order"""
    cells = rng.choice(n_s * n_r, n, replace=False)
    return (base + cells // n_r).astype(U32), (cells % n_r).astype(U32)


@pytest.mark.parametrize("base", [0, 7])
@pytest.mark.parametrize("n", N_PAIRS)
def test_every_pair_count(ctx, n, base):
    """the lane step, the wavefront's share, the workgroup's share, more than four workgroups: one 4-byte term"""
    rng = np.random.default_rng(n)
    s, r = relation(rng, np.int32, N_S), relation(rng, np.int32, N_R)
    map_s, map_r = unique_pairs(rng, n, base=base)
    order = np.argsort(map_s, kind="stable")        # the S rows' pairs side by side, as a probe leaves them
    want = run(ctx, map_s[order], map_r[order], base, N_S, N_R, wc.term_of(s, ">=", r), tag=("count", n, base))
    assert n < 64 or 0 < want["info"][0] < n


@pytest.mark.parametrize("run_len", [2, 64, 65, 257, 1025])
def test_one_s_row_owning_a_run(ctx, run_len):
    """the pairs of one S row as one run that crosses lane steps, wavefronts and workgroups, in front of it 37 pairs of other
    rows so that it starts inside a step; then the same pairs scattered through a shuffled list"""
    rng = np.random.default_rng(run_len)
    hot, n_r = 777, 1100
    r = rng.integers(-500, 500, n_r).astype(np.int64)
    s = np.full(N_S, 100, dtype=np.int64)
    lead_s, lead_r = unique_pairs(rng, 37, n_s=700)                  # rows below `hot`
    run_r = rng.choice(n_r, run_len, replace=False).astype(U32)
    tail_s, tail_r = unique_pairs(rng, 300, n_s=700)
    map_s = np.concatenate([lead_s, np.full(run_len, hot, U32), tail_s + U32(800)])
    map_r = np.concatenate([lead_r, run_r, tail_r])
    for op in (">=", "<"):
        want = run(ctx, map_s, map_r, 0, N_S, N_R, wc.term_of(s, op, r), tag=("run", run_len, op))
        p = rng.permutation(map_s.size)
        mixed = run(ctx, map_s[p], map_r[p], 0, N_S, N_R, wc.term_of(s, op, r), tag=("scattered", run_len, op))
        assert np.array_equal(want["kept"], mixed["kept"]) and np.array_equal(want["best_row"], mixed["best_row"])
        if run_len >= 64:
            assert want["best_row"][hot] != NO_ROW


@pytest.mark.parametrize("case", ["all tied", "none eligible", "one pair per S row", "key 0 is the maximum", "tie with the lowest row last"])
def test_directed_cases(ctx, case):
    rng = np.random.default_rng(17)
    n = 1300
    if case == "all tied":
        s, r = np.full(N_S, 5, np.uint16), np.full(N_R, 5, np.uint16)
        map_s, map_r = unique_pairs(rng, 4097)
        want = run(ctx, map_s, map_r, 0, N_S, N_R, wc.term_of(s, ">=", r), tag=case)
        # per S row its lowest R row
        for si in np.unique(map_s)[:50]:
            assert want["best_row"][si] == map_r[map_s == si].min()
    elif case == "none eligible":
        s, r = np.zeros(N_S, np.int8), np.ones(N_R, np.int8)
        map_s, map_r = unique_pairs(rng, 2500)
        want = run(ctx, map_s, map_r, 0, N_S, N_R, wc.term_of(s, ">=", r), tag=case)
        assert want["info"][0] == 0 and (want["best_row"] == NO_ROW).all()
    elif case == "one pair per S row":
        s, r = relation(rng, np.float32, N_S), relation(rng, np.float32, N_R)
        map_s, map_r = rng.permutation(n).astype(U32), rng.integers(0, N_R, n).astype(U32)
        want = run(ctx, map_s, map_r, 0, N_S, N_R, wc.term_of(s, "<=", r), tag=case)
        assert 0 < want["info"][0] < n and want["info"][0] == int(wc.holds(wc.term_of(s, "<=", r), map_s.astype(np.int64), map_r.astype(np.int64)).sum())
    elif case == "key 0 is the maximum":
        # unsigned 0 under >= is the smallest order key there is, and the plane starts at it: the pair must still be kept;
        # likewise the largest value under <=, whose complemented key is 0
        for dtype, op, val in ((np.uint64, ">=", 0), (np.uint8, ">=", 0), (np.uint32, "<=", 0xFFFFFFFF), (np.uint64, "<=", (1 << 64) - 1)):
            s, r = np.full(N_S, val, dtype), np.full(N_R, val, dtype)
            map_s, map_r = unique_pairs(rng, n)
            want = run(ctx, map_s, map_r, 0, N_S, N_R, wc.term_of(s, op, r), tag=(case, str(np.dtype(dtype)), op))
            assert want["info"][0] == np.unique(map_s).size
    else:
        # the winner of every S row stands behind its rivals in the list
        s, r = np.full(N_S, 9, np.int32), rng.integers(7, 9, N_R).astype(np.int32)
        map_s, map_r = unique_pairs(rng, 3000)
        order = np.lexsort((-map_r.astype(np.int64), map_s))
        run(ctx, map_s[order], map_r[order], 0, N_S, N_R, wc.term_of(s, ">", r), tag=case)


@pytest.mark.parametrize("dtype", wc.DTYPES, ids=str)
@pytest.mark.parametrize("planes", [False, True], ids=["plain", "nullable"])
def test_every_width_and_type(ctx, dtype, planes):
    """the ladder against itself under the four ops, on the device: the pairs are the ladder's cross product, repeated with a
    rotation to fill more than one workgroup (a repeated pair: each copy of a winner is kept)"""
    v = wc.ladder(dtype)
    k = v.size
    s, r = np.divmod(np.arange(k * k, dtype=np.int64), k)
    reps = -(-1100 // (k * k))
    map_s, map_r = np.tile(s, reps).astype(U32), np.tile(r, reps).astype(U32)
    sv, rv = (np.arange(k) % 4 != 1, np.arange(k) % 5 != 2) if planes else (None, None)
    for op in ac.ASOF_OPS:
        want = run(ctx, map_s, map_r, 0, k, k, wc.term_of(v, op, v.copy(), sv, rv), tag=(str(dtype), op, planes))
        assert 0 < want["info"][0] <= reps * k


def test_dropped_entries_and_a_row_base(ctx):
    rng = np.random.default_rng(21)
    n, base = 5000, 777
    s, r = relation(rng, np.float64, N_S), relation(rng, np.float64, N_R)
    term = wc.term_of(s, "<", r, rng.random(N_S) < 0.9, rng.random(N_R) < 0.9)
    map_s, map_r = unique_pairs(rng, n, base=base)
    map_s[::7] = NO_ROW
    map_r[3::11] = NO_ROW
    map_s[5::13] = base + N_S           # the first row behind S
    map_s[6::17] = rng.integers(0, base, map_s[6::17].size)      # below the base
    map_r[8::19] = N_R + rng.integers(0, 1 << 20, map_r[8::19].size)
    want = run(ctx, map_s, map_r, base, N_S, N_R, term, tag="dropped")
    assert want["info"][3] > n // 4 and 0 < want["info"][0] < N_S
    # a relation without rows: every pair is dropped and nothing is read
    none = np.zeros(0, dtype=np.float64)
    assert run(ctx, map_s, map_r, 0, 0, N_R, wc.term_of(none, "<", r), tag="no S rows")["info"] == (0, 0, 0, n)
    assert run(ctx, map_s, map_r, 0, N_S, 0, wc.term_of(s, "<", none), tag="no R rows")["info"] == (0, 0, 0, n)


def test_capacity_cut_and_the_mark_only_pass(ctx):
    rng = np.random.default_rng(31)
    s, r = relation(rng, np.int64, N_S), relation(rng, np.int64, N_R)
    term = wc.term_of(s, "<=", r, rng.random(N_S) < 0.95, None)
    map_s, map_r = unique_pairs(rng, 6000)
    kept = run(ctx, map_s, map_r, 0, N_S, N_R, term, offset=3, tag="misaligned planes")["info"][0]
    assert kept > 1100
    for cap in (kept - 1, 1030, 1):             # the cut inside a workgroup's run, behind the first workgroups, in the first one
        run(ctx, map_s, map_r, 0, N_S, N_R, term, capacity=cap, offset=1, tag=("cut", cap))
    run(ctx, map_s, map_r, 0, N_S, N_R, term, capacity=0, tag="mark only")
    run(ctx, map_s, map_r, 0, N_S, N_R, term, marks=False, tag="no planes")


def test_a_second_call_resets_planes_and_cursor(ctx):
    rng = np.random.default_rng(41)
    s, r = relation(rng, np.uint16, N_S), relation(rng, np.uint16, N_R)
    map_s, map_r = unique_pairs(rng, 3000)
    first = run(ctx, map_s, map_r, 0, N_S, N_R, wc.term_of(s, ">", r), tag="first")
    where_before = ctx.where_info()
    second = run(ctx, map_s[:1000], map_r[:1000], 0, N_S, N_R, wc.term_of(s, "<", r), tag="second")
    assert ctx.asof_info()[0] == second["info"][0] != first["info"][0]
    run(ctx, map_s[:0], map_r[:0], 0, N_S, N_R, wc.term_of(s, "<", r), tag="no pairs")
    assert ctx.asof_info()[:2] == (0, 0) and ctx.asof_info()[3] == 0
    assert ctx.where_info() == where_before       # other calls' records are their own
    # preset mark bits survive a call
    sw, rw = -(-N_S // 32), -(-N_R // 32)
    pre_s, pre_r = rng.integers(0, 1 << 32, sw).astype(U32), rng.integers(0, 1 << 32, rw).astype(U32)
    with Device(ctx) as dev:
        d_ps, d_pr = dev.put(pre_s), dev.put(pre_r)
        d_term = (dev.put(s), dev.put(r), 2, _lib.HJ_VAL_UINT, _lib.CMP_OPS[">"], 0, 0)
        ctx.pairs_asof(dev.put(map_s), dev.put(map_r), map_s.size, 0, N_S, N_R, d_term, dev.alloc(8 * N_S), dev.alloc(4 * N_S), 0, 0, 0, d_ps, d_pr)
        assert ctx.asof_info()[:2] == (first["info"][0], 0)
        assert np.array_equal(dev.get(d_ps, sw), pre_s | first["s_marks"]) and np.array_equal(dev.get(d_pr, rw), pre_r | first["r_marks"])


def test_what_the_device_form_refuses(ctx):
    with Device(ctx) as dev:
        d = dev.alloc(4096)
        good = (d, d, 8, _lib.HJ_VAL_INT, _lib.HJ_CMP_LT, d, d)
        call = lambda term, n=16, s_rows=8, r_rows=8, ms=d, mr=d, bv=d, br=d, os=d, o_r=d, cap=16: status(      # noqa: E731
            ctx.pairs_asof, ms, mr, n, 0, s_rows, r_rows, term, bv, br, os, o_r, cap)
        before = ctx.asof_info()
        edit = lambda i, v: good[:i] + (v,) + good[i + 1:]        # noqa: E731
        for term in (edit(2, 3), edit(2, 16), edit(3, 3), edit(4, 6), edit(4, _lib.HJ_CMP_EQ), edit(4, _lib.HJ_CMP_NE), edit(0, 0), edit(1, 0),
                     edit(0, d + 4), edit(1, d + 2), edit(5, d + 2), edit(6, d + 1), (d, d, 2, _lib.HJ_VAL_FLOAT, _lib.HJ_CMP_LT, 0, 0)):
            assert call(term) == INVALID, term
        assert call(good, ms=0) == INVALID and call(good, mr=0) == INVALID and call(good, os=0) == INVALID and call(good, o_r=0) == INVALID
        assert call(good, bv=0) == INVALID and call(good, br=0) == INVALID and call(good, bv=d + 4) == INVALID and call(good, br=d + 2) == INVALID
        assert call(good, n=1 << 32) == INVALID and call(good, s_rows=1 << 32) == INVALID and call(good, r_rows=1 << 32) == INVALID
        t = _lib.hj_asof_term()
        t.s, t.r, t.width, t.op, t.reserved = d, d, 4, _lib.HJ_CMP_GE, 1
        vp = C.c_void_p
        assert lib.hj_pairs_asof_dev(ctx._h, vp(d), vp(d), 4, 0, 8, 8, C.byref(t), vp(d), vp(d), None, None, 0, None, None) == INVALID
        assert lib.hj_pairs_asof_dev(ctx._h, vp(d), vp(d), 4, 0, 8, 8, None, vp(d), vp(d), None, None, 0, None, None) == INVALID
        assert b"hj_pairs_asof_dev" in lib.hj_last_error(ctx._h)
        assert ctx.asof_info() == before       # a refused call enqueues nothing and leaves the record alone
