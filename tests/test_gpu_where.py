"""hj_pairs_where_dev / hj_where_info through ctypes -> C ABI on an MI355X, against the numpy model of where_common.py and
against hj_pairs_where_host on the same buffers. Every output plane and every marks plane has sentinel words around it that
must survive. Run with -m gpu.

hj_where.hip: a workgroup of k_pairs_where takes kFilterBlockPairs = 1024 consecutive pairs, a wavefront 256 of them as four
steps of 64 -- the pair counts below are the lane step, the wavefront's share, the workgroup's share and more than four
workgroups, each with its neighbours."""
import ctypes as C

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

import where_common as wc
from gpu_harness import Device, check_pair_filter, ctx, plane_words, status  # noqa: F401

pytestmark = pytest.mark.gpu

U32, NO_ROW = np.uint32, wc.NO_ROW
GUARD = 64                      # sentinel words around a plane
N_PAIRS = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)
INVALID = _lib.HJ_ERR_INVALID


def run(ctx, map_s, map_r, base, s_rows, r_rows, terms, capacity=None, marks=True, offset=0, tag=None):
    """one hj_pairs_where_dev over numpy inputs, checked in full against the model and the host form -> the model's dict"""
    n = map_s.size
    want = wc.model_call(map_s, map_r, base, s_rows, r_rows, terms, capacity)
    cap = n if capacity is None else capacity
    host = None
    if s_rows == terms[0][0].size and r_rows == terms[0][2].size:
        host = lambda: hj.pairs_where_host(map_s, map_r, base, [(hj.KeyColumn(s, sv), op, hj.KeyColumn(r, rv)) for s, op, r, sv, rv in terms],      # noqa: E731
                                           capacity=cap, marks=True)
    with Device(ctx) as dev:
        d_terms = []
        for s, op, r, s_valid, r_valid in terms:
            d_terms.append((dev.put(s), dev.put(r), s.dtype.itemsize, wc.TYPE_OF[s.dtype.kind], _lib.CMP_OPS[op],
                            dev.put(plane_words(s_valid)) if s_valid is not None else 0,
                            dev.put(plane_words(r_valid)) if r_valid is not None else 0))
        call = lambda ms, mr, os, o_r, c, ps, pr: ctx.pairs_where(ms, mr, n, base, s_rows, r_rows, d_terms, os, o_r, c, ps, pr)        # noqa: E731
        check_pair_filter(dev, call, ctx.where_info, map_s, map_r, s_rows, r_rows, want, cap, GUARD, offset=offset, marks=marks, host=host, tag=tag)
    return want


def relation(rng, dtype, n, span=6):
    """n values of dtype around the middle of a small range, so that every op keeps some pairs and rejects others"""
    dtype = np.dtype(dtype)
    v = rng.integers(0, span, n)
    return (v - span // 2).astype(dtype) if dtype.kind != "u" else v.astype(dtype)


N_S, N_R = 1500, 1100           # rows of the relations: neither a multiple of 32


@pytest.mark.parametrize("n", N_PAIRS)
def test_every_pair_count(ctx, n):
    """the lane step, the wavefront's share, the workgroup's share, more than four workgroups: one 4-byte term"""
    rng = np.random.default_rng(n)
    s, r = relation(rng, np.int32, N_S), relation(rng, np.int32, N_R)
    map_s, map_r = rng.integers(0, N_S, n).astype(U32), rng.integers(0, N_R, n).astype(U32)
    want = run(ctx, map_s, map_r, 0, N_S, N_R, [wc.term_of(s, "<", r)], tag=("count", n))
    assert n < 64 or 0 < want["info"][0] < n


@pytest.mark.parametrize("which", ["all", "none", "every other", "only the last"])
def test_which_pairs_are_kept(ctx, which):
    n = 4097
    rng = np.random.default_rng(11)
    s, r = np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32)      # pair k is (k, k): the term decides per pair
    map_s, map_r = np.arange(n, dtype=U32), rng.permutation(n).astype(U32)
    r_of = np.empty(n, dtype=np.int64)
    r_of[map_r] = np.arange(n)                                               # the pair an R row belongs to
    lim = {"all": np.full(n, n, np.uint32), "none": np.zeros(n, np.uint32), "every other": np.where(np.arange(n) % 2 == 0, n, 0).astype(np.uint32),
           "only the last": np.where(np.arange(n) == n - 1, n, 0).astype(np.uint32)}[which]
    want = run(ctx, map_s, map_r, 0, n, n, [wc.term_of(s, "<", lim[r_of])], tag=which)
    assert want["info"][0] == {"all": n, "none": 0, "every other": (n + 1) // 2, "only the last": 1}[which]
    if which == "only the last":
        assert want["kept"][0] == (np.uint64(n - 1) << np.uint64(32)) | np.uint64(map_r[n - 1])


@pytest.mark.parametrize("dtype", wc.DTYPES, ids=str)
@pytest.mark.parametrize("planes", [False, True], ids=["plain", "nullable"])
def test_one_term_of_every_width_and_type(ctx, dtype, planes):
    """the ladder against itself under every op, on the device: the pairs are the ladder's cross product, repeated to fill
    more than one workgroup"""
    v = wc.ladder(dtype)
    k = v.size
    s, r = np.divmod(np.arange(k * k, dtype=np.int64), k)
    reps = -(-2100 // (k * k))
    map_s, map_r = np.tile(s, reps).astype(U32), np.tile(r, reps).astype(U32)
    sv, rv = (np.arange(k) % 4 != 1, np.arange(k) % 5 != 2) if planes else (None, None)
    for op in wc.OPS:
        want = run(ctx, map_s, map_r, 0, k, k, [wc.term_of(v, op, v.copy(), sv, rv)], tag=(str(dtype), op, planes))
        assert 0 < want["info"][0] < map_s.size


def four_terms(rng, n_s, n_r, planes):
    nulls = (lambda n: rng.random(n) < 0.9) if planes else (lambda n: None)
    return [wc.term_of(relation(rng, np.uint8, n_s, 4), "<=", relation(rng, np.uint8, n_r, 4), nulls(n_s), None),
            wc.term_of(relation(rng, np.int16, n_s), ">=", relation(rng, np.int16, n_r)),
            wc.term_of(relation(rng, np.float32, n_s, 3), "!=", relation(rng, np.float32, n_r, 3), None, nulls(n_r)),
            wc.term_of(relation(rng, np.float64, n_s, 8), "<", relation(rng, np.float64, n_r, 8), nulls(n_s), nulls(n_r))]


@pytest.mark.parametrize("planes", [False, True], ids=["plain", "nullable"])
def test_four_terms_dropped_entries_and_a_row_base(ctx, planes):
    rng = np.random.default_rng(21 + planes)
    n, base = 5000, 777
    terms = four_terms(rng, N_S, N_R, planes)
    map_s, map_r = (base + rng.integers(0, N_S, n)).astype(U32), rng.integers(0, N_R, n).astype(U32)
    map_s[::7] = NO_ROW
    map_r[3::11] = NO_ROW
    map_s[5::13] = base + N_S           # the first row behind S
    map_s[6::17] = rng.integers(0, base, map_s[6::17].size)      # below the base
    map_r[8::19] = N_R + rng.integers(0, 1 << 20, map_r[8::19].size)
    want = run(ctx, map_s, map_r, base, N_S, N_R, terms, tag=("four", planes))
    assert want["info"][3] > n // 4 and 0 < want["info"][0] < n // 8
    for k in (1, 2, 3):
        assert run(ctx, map_s, map_r, base, N_S, N_R, terms[:k], tag=("prefix", k))["info"][0] >= want["info"][0]


def test_capacity_cut_and_the_mark_only_pass(ctx):
    rng = np.random.default_rng(31)
    n = 4500
    s, r = relation(rng, np.int64, N_S), relation(rng, np.int64, N_R)
    terms = [wc.term_of(s, "<=", r, rng.random(N_S) < 0.95, None)]
    map_s, map_r = rng.integers(0, N_S, n).astype(U32), rng.integers(0, N_R, n).astype(U32)
    kept = run(ctx, map_s, map_r, 0, N_S, N_R, terms, offset=3, tag="misaligned planes")["info"][0]
    assert kept > 2000
    for cap in (kept - 1, 1030, 1):             # the cut inside a workgroup's run, at its start, in the first one
        run(ctx, map_s, map_r, 0, N_S, N_R, terms, capacity=cap, offset=1, tag=("cut", cap))
    run(ctx, map_s, map_r, 0, N_S, N_R, terms, capacity=0, tag="mark only")
    run(ctx, map_s, map_r, 0, N_S, N_R, terms, marks=False, tag="no planes")
    # a relation without rows: every pair is dropped and nothing is read
    none = np.zeros(0, dtype=np.int64)
    assert run(ctx, map_s, map_r, 0, 0, N_R, [wc.term_of(none, "<", r)], tag="no S rows")["info"] == (0, 0, 0, n)
    assert run(ctx, map_s, map_r, 0, N_S, 0, [wc.term_of(s, "<", none)], tag="no R rows")["info"] == (0, 0, 0, n)


def test_a_second_call_resets_the_cursor_and_bits_only_go_up(ctx):
    rng = np.random.default_rng(41)
    n = 3000
    s, r = relation(rng, np.uint16, N_S), relation(rng, np.uint16, N_R)
    map_s, map_r = rng.integers(0, N_S, n).astype(U32), rng.integers(0, N_R, n).astype(U32)
    first = run(ctx, map_s, map_r, 0, N_S, N_R, [wc.term_of(s, ">", r)], tag="first")
    second = run(ctx, map_s[:1000], map_r[:1000], 0, N_S, N_R, [wc.term_of(s, "==", r)], tag="second")
    assert ctx.where_info()[0] == second["info"][0] != first["info"][0]
    run(ctx, map_s[:0], map_r[:0], 0, N_S, N_R, [wc.term_of(s, "==", r)], tag="no pairs")
    assert ctx.where_info()[:2] == (0, 0) and ctx.where_info()[3] == 0
    # preset bits survive a call
    sw, rw = -(-N_S // 32), -(-N_R // 32)
    pre_s, pre_r = rng.integers(0, 1 << 32, sw).astype(U32), rng.integers(0, 1 << 32, rw).astype(U32)
    with Device(ctx) as dev:
        d_ps, d_pr = dev.put(pre_s), dev.put(pre_r)
        d_terms = [(dev.put(s), dev.put(r), 2, _lib.HJ_VAL_UINT, _lib.CMP_OPS[">"], 0, 0)]
        ctx.pairs_where(dev.put(map_s), dev.put(map_r), n, 0, N_S, N_R, d_terms, 0, 0, 0, d_ps, d_pr)
        assert ctx.where_info()[:2] == (first["info"][0], 0)
        assert np.array_equal(dev.get(d_ps, sw), pre_s | first["s_marks"]) and np.array_equal(dev.get(d_pr, rw), pre_r | first["r_marks"])
        # other calls' records are their own
        verify_before = ctx.verify_info()
        ctx.pairs_where(dev.put(map_s), dev.put(map_r), n, 0, N_S, N_R, d_terms, 0, 0, 0)
        assert ctx.verify_info() == verify_before


def test_what_the_device_form_refuses(ctx):
    with Device(ctx) as dev:
        d = dev.alloc(4096)
        good = (d, d, 8, _lib.HJ_VAL_INT, _lib.HJ_CMP_LT, d, d)
        call = lambda terms, n=16, s_rows=8, r_rows=8, ms=d, mr=d, os=d, o_r=d, cap=16: status(      # noqa: E731
            ctx.pairs_where, ms, mr, n, 0, s_rows, r_rows, terms, os, o_r, cap)
        before = ctx.where_info()
        edit = lambda i, v: [good[:i] + (v,) + good[i + 1:]]        # noqa: E731
        for terms in ([], [good] * 5, edit(2, 3), edit(2, 16), edit(3, 3), edit(4, 6), edit(0, 0), edit(1, 0), edit(0, d + 4), edit(1, d + 2),
                      edit(5, d + 2), edit(6, d + 1), [(d, d, 2, _lib.HJ_VAL_FLOAT, 0, 0, 0)]):
            assert call(terms) == INVALID, terms
        assert call([good], ms=0) == INVALID and call([good], mr=0) == INVALID and call([good], os=0) == INVALID and call([good], o_r=0) == INVALID
        assert call([good], n=1 << 32) == INVALID and call([good], s_rows=1 << 32) == INVALID and call([good], r_rows=1 << 32) == INVALID
        arr = (_lib.hj_where_term * 1)()
        arr[0].s, arr[0].r, arr[0].width, arr[0].reserved = d, d, 4, 1
        assert lib.hj_pairs_where_dev(ctx._h, C.c_void_p(d), C.c_void_p(d), 4, 0, 8, 8, arr, 1, None, None, 0, None, None) == INVALID
        assert lib.hj_pairs_where_dev(ctx._h, C.c_void_p(d), C.c_void_p(d), 4, 0, 8, 8, None, 1, None, None, 0, None, None) == INVALID
        assert b"hj_pairs_where_dev" in lib.hj_last_error(ctx._h)
        assert ctx.where_info() == before       # a refused call enqueues nothing and leaves the record alone
