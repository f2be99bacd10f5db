"""gpu_harness.py on host memory: the harness is what stands between a kernel bug and a green run, so the guarded plane and
check_pair_filter are tested themselves. The stand-in context below has the four memory calls of a HashJoinContext over
ctypes buffers, so a "device pointer" is a host address, and its pairs_where / pairs_asof run hj_pairs_where_host /
hj_pairs_asof_host -- the host twins, which share the kernels' compare and order bodies -- on those addresses. The check
must accept them as they are and reject each fault that a wrapped call injects. Needs no GPU and touches none."""
import ctypes as C

import numpy as np
import pytest

from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib
from htm_hashjoin_amd.engine import _terms_arr

import asof_common as ac
import where_common as wc
from gpu_harness import SENTINEL, Device, GuardedPlane, check_pair_filter, plane_bits, plane_words, row_bits

U32, U64 = np.uint32, np.uint64
GUARD = 64
N_S, N_R = 150, 110              # rows of the relations: neither a multiple of 32


class HostContext:
    """the memory calls of a HashJoinContext on host memory, and the two filters as their host twins"""

    def __init__(self):
        self.bufs, self.info = {}, None

    def dev_alloc(self, nbytes):
        buf = (C.c_uint8 * nbytes)()
        self.bufs[C.addressof(buf)] = buf
        return C.addressof(buf)

    def dev_free(self, ptr):
        del self.bufs[ptr]

    def copy_h2d(self, dst_ptr, src_np):
        src_np = np.ascontiguousarray(src_np)
        C.memmove(dst_ptr, src_np.ctypes.data, src_np.nbytes)

    def copy_d2h(self, dst_np, src_ptr):
        C.memmove(dst_np.ctypes.data, src_ptr, dst_np.nbytes)

    def words(self, ptr, n, dtype=U32):
        """n entries at a "device" address as a numpy array over the same memory: what a fault writes through"""
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), (n * np.dtype(dtype).itemsize,)).view(dtype)

    def pairs_where(self, ms, mr, n, base, s_rows, r_rows, terms, out_s, out_r, cap, s_marks=0, r_marks=0):
        arr, k = _terms_arr(terms)
        info = (C.c_uint64 * 4)()
        rc = lib.hj_pairs_where_host(ms, mr, n, base, s_rows, r_rows, arr, k, out_s or None, out_r or None, cap, s_marks or None, r_marks or None, info)
        assert rc == _lib.HJ_OK, rc
        self.info = tuple(int(x) for x in info)

    def pairs_asof(self, ms, mr, n, base, s_rows, r_rows, term, best_val, best_row, out_s, out_r, cap, s_marks=0, r_marks=0):
        info = (C.c_uint64 * 4)()
        rc = lib.hj_pairs_asof_host(ms, mr, n, base, s_rows, r_rows, _terms_arr([term], _lib.hj_asof_term)[0], best_val, best_row,
                                    out_s or None, out_r or None, cap, s_marks or None, r_marks or None, info)
        assert rc == _lib.HJ_OK, rc
        self.info = tuple(int(x) for x in info)

    def filter_info(self):
        return self.info


# ---- the device buffers and the bit planes ------------------------------------------------------------------------------------------
def test_device_allocates_whole_words_and_frees_what_it_holds():
    ctx = HostContext()
    with Device(ctx) as dev:
        sizes = [len(ctx.bufs[dev.alloc(n)]) for n in (0, 1, 16, 17, 21)]
        assert sizes == [16, 16, 16, 20, 24]
        p = dev.put(np.arange(5, dtype=np.uint16))
        assert dev.get(p, 5, np.uint16).tolist() == [0, 1, 2, 3, 4] and len(ctx.bufs[p]) == 16
        dev.free(p)
        assert p not in ctx.bufs and len(ctx.bufs) == 5
    assert not ctx.bufs and not dev.owns
    dev = Device(ctx)
    dev.put(np.zeros(3, U64))
    dev.release()
    assert not ctx.bufs and dev.ptrs == []


@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, 150])
def test_bit_planes_there_and_back(n):
    bits = np.random.default_rng(n).random(n) < 0.4
    words = plane_words(bits)
    assert words.dtype == U32 and words.size == -(-n // 32)
    for i in range(n):
        assert bool(int(words[i >> 5]) >> (i & 31) & 1) == bool(bits[i])
    assert n % 32 == 0 or int(words[-1]) >> (n % 32) == 0, "a bit behind the last row is set"
    assert np.array_equal(plane_bits(words, n), bits)
    assert np.array_equal(row_bits(np.flatnonzero(bits), n), bits)


# ---- the guarded plane ------------------------------------------------------------------------------------------------------------------
PLANES = [(U32, SENTINEL), (U64, 0xA5A5A5A5A5A5A5A5), (np.int64, -(0x5A5A5A5A5A5A5A5B))]


@pytest.mark.parametrize("dtype,sentinel", PLANES, ids=["uint32", "uint64", "int64"])
def test_guarded_plane_passes_what_stays_inside(dtype, sentinel):
    ctx = HostContext()
    with Device(ctx) as dev:
        plane = GuardedPlane(dev, 10, dtype, sentinel, front=GUARD, behind=GUARD)
        assert plane.ptr == plane.base + GUARD * np.dtype(dtype).itemsize
        assert (plane.read(0, "untouched") == sentinel).all()
        ctx.words(plane.ptr, 10, dtype)[:7] = 3
        assert plane.read(7, "seven").tolist() == [3] * 7
        assert plane.read(None, "whole").tolist() == [3] * 7 + [sentinel] * 3
        assert plane.read(10, "whole").size == 10
        zeros = GuardedPlane(dev, 5, dtype, sentinel, front=GUARD, behind=GUARD, body=0)
        assert zeros.read(None, "a body of its own").tolist() == [0] * 5
        assert GuardedPlane(dev, 0, dtype, sentinel, front=3, behind=GUARD).read(0, "no entries").size == 0
        bare = GuardedPlane(dev, 4, dtype, sentinel, behind=4096)
        assert bare.ptr == bare.base and bare.read(0, "no front guard").size == 0


@pytest.mark.parametrize("where", ["the last word in front", "the first word in front", "the first word behind", "the last word behind",
                                   "the body behind written", "the body's last entry"])
@pytest.mark.parametrize("dtype,sentinel", PLANES, ids=["uint32", "uint64", "int64"])
def test_guarded_plane_raises_for_a_word_outside(dtype, sentinel, where):
    n, written = 10, 7
    at = {"the last word in front": -1, "the first word in front": -GUARD, "the first word behind": n, "the last word behind": n + GUARD - 1,
          "the body behind written": written, "the body's last entry": n - 1}[where]
    ctx = HostContext()
    with Device(ctx) as dev:
        plane = GuardedPlane(dev, n, dtype, sentinel, front=GUARD, behind=GUARD, what="outside")
        ctx.words(plane.ptr, written, dtype)[:] = 1
        plane.read(written, where)
        ctx.words(plane.base, n + 2 * GUARD, dtype)[GUARD + at] = 1
        with pytest.raises(AssertionError, match="outside"):
            plane.read(written, where)
        if 0 <= at < n:
            plane.read(n, "inside the body once all of it counts as written")


# ---- check_pair_filter --------------------------------------------------------------------------------------------------------------------
def relation(rng, n, span=12):
    return (rng.integers(0, span, n) - span // 2).astype(np.int32)


def case(n, kind):
    """n pairs over the two relations, some of them dropped entries; every S row's pairs are in the list once"""
    rng = np.random.default_rng(100 + n)
    s, r = relation(rng, N_S), relation(rng, N_R)
    cells = rng.choice(N_S * N_R, n, replace=False)
    map_s, map_r = (cells // N_R).astype(U32), (cells % N_R).astype(U32)
    if kind == "where":                 # a repeated pair: kept as often as it stands in the list
        map_s[n // 2:n // 2 + n // 8], map_r[n // 2:n // 2 + n // 8] = map_s[:n // 8], map_r[:n // 8]
    map_s[5::13] = wc.NO_ROW
    map_r[7::17] = N_R
    return map_s, map_r, wc.term_of(s, "<=", r, rng.random(N_S) < 0.9, None)


def run(kind, map_s, map_r, term, capacity=None, fault=None, marks=True, offset=0):
    """check_pair_filter over the stand-in, as test_gpu_where.run and test_gpu_asof.run call it over a GPU; `fault` gets the
    context and the arguments of the call behind the call itself and writes what a broken kernel would"""
    ctx = HostContext()
    cap = map_s.size if capacity is None else capacity
    s, op, r, s_valid, r_valid = term
    with Device(ctx) as dev:
        d_term = (dev.put(s), dev.put(r), s.dtype.itemsize, wc.TYPE_OF[s.dtype.kind], _lib.CMP_OPS[op],
                  dev.put(plane_words(s_valid)) if s_valid is not None else 0, dev.put(plane_words(r_valid)) if r_valid is not None else 0)
        if kind == "where":
            want, extra = wc.model_call(map_s, map_r, 0, N_S, N_R, [term], capacity), []

            def call(ms, mr, out_s, out_r, c, ps, pr):
                ctx.pairs_where(ms, mr, map_s.size, 0, N_S, N_R, [d_term], out_s, out_r, c, ps, pr)
                if fault:
                    fault(ctx, dict(n=map_s.size, ms=ms, mr=mr, out_s=out_s, out_r=out_r, ps=ps, pr=pr))
        else:
            want = ac.model_call(map_s, map_r, 0, N_S, N_R, term, capacity)
            extra = [("best_val", GuardedPlane(dev, 2 * N_S, front=GUARD, behind=GUARD, body=0x33333333, what="a word outside a best plane was written"),
                      None, None),
                     ("best_row", GuardedPlane(dev, N_S, front=GUARD, behind=GUARD, body=0, what="a word outside a best plane was written"),
                      want["best_row"], "bestRow: the left-outer as-of map")]

            def call(ms, mr, out_s, out_r, c, ps, pr, bv, br):
                ctx.pairs_asof(ms, mr, map_s.size, 0, N_S, N_R, d_term, bv, br, out_s, out_r, c, ps, pr)
                if fault:
                    fault(ctx, dict(n=map_s.size, ms=ms, mr=mr, out_s=out_s, out_r=out_r, ps=ps, pr=pr, bv=bv, br=br))
        check_pair_filter(dev, call, ctx.filter_info, map_s, map_r, N_S, N_R, want, cap, GUARD, offset=offset, marks=marks, extra=extra,
                          tag=(kind, map_s.size, capacity))
    assert not ctx.bufs
    return want


@pytest.mark.parametrize("n", [0, 1, 64, 257])
@pytest.mark.parametrize("kind", ["where", "asof"])
def test_check_accepts_the_host_twin(kind, n):
    map_s, map_r, term = case(n, kind)
    want = run(kind, map_s, map_r, term)
    assert n < 64 or 0 < want["info"][0] < n
    assert n < 64 or want["info"][3] > 0
    run(kind, map_s, map_r, term, marks=False, offset=3)


@pytest.mark.parametrize("kind", ["where", "asof"])
def test_check_accepts_the_host_twin_under_a_cut_and_at_capacity_0(kind):
    map_s, map_r, term = case(257, kind)
    kept = run(kind, map_s, map_r, term)["info"][0]
    assert kept > 8
    for cap in (kept - 1, kept // 2, 1):
        assert run(kind, map_s, map_r, term, capacity=cap, offset=1)["info"][:2] == (kept, cap)
    assert run(kind, map_s, map_r, term, capacity=0)["info"][:2] == (kept, 0)


def _info_off_by_one(ctx, a):
    ctx.info = (ctx.info[0] + 1,) + ctx.info[1:]


def _foreign_pair(ctx, a):
    ctx.words(a["out_r"], 1)[0] ^= 1            # the first kept pair's R row becomes its neighbour


def _one_pair_too_often(ctx, a):
    """under a cut: the first written pair stands in the output once more than the list holds it"""
    out_s, out_r = ctx.words(a["out_s"], ctx.info[1]), ctx.words(a["out_r"], ctx.info[1])
    times = int(((ctx.words(a["ms"], a["n"]) == out_s[0]) & (ctx.words(a["mr"], a["n"]) == out_r[0])).sum())
    out_s[1:times + 1], out_r[1:times + 1] = out_s[0], out_r[0]
    if int(((out_s == out_s[0]) & (out_r == out_r[0])).sum()) != times + 1:
        raise RuntimeError("the fault is not the one the test is about")


def _flip(plane, bit):
    def fault(ctx, a):
        ctx.words(a[plane], bit // 32 + 1)[bit // 32] ^= U32(1 << (bit % 32))
    return fault


def _map_word(which):
    def fault(ctx, a):
        ctx.words(a[which], 3)[2] += U32(1)
    return fault


def _best_row(ctx, a):
    ctx.words(a["br"], N_S)[N_S - 1] ^= U32(1)


def _behind_the_run(ctx, a):
    ctx.words(a["out_s"], ctx.info[1] + 1)[ctx.info[1]] = 0


FAULTS = {"info's kept count off by one": (_info_off_by_one, None), "a foreign pair in the output": (_foreign_pair, None),
          "a kept pair once more than it was kept, under a cut": (_one_pair_too_often, "cut"),
          "an S mark bit set": (_flip("ps", N_S - 1), None), "an S mark bit in the plane's spare bits": (_flip("ps", N_S), None),
          "an R mark bit flipped": (_flip("pr", 0), None), "a word of map S overwritten": (_map_word("ms"), None),
          "a word of map R overwritten": (_map_word("mr"), None), "a word behind the run written": (_behind_the_run, "cut")}


@pytest.mark.parametrize("name", list(FAULTS))
@pytest.mark.parametrize("kind", ["where", "asof"])
def test_check_rejects_each_fault(kind, name):
    fault, cut = FAULTS[name]
    map_s, map_r, term = case(257, kind)
    kept = run(kind, map_s, map_r, term)["info"][0]
    capacity = kept // 2 if cut else None
    run(kind, map_s, map_r, term, capacity=capacity)            # the same call without the fault passes
    with pytest.raises(AssertionError):
        run(kind, map_s, map_r, term, capacity=capacity, fault=fault)


def test_check_rejects_a_changed_best_row_entry():
    map_s, map_r, term = case(257, "asof")
    with pytest.raises(AssertionError, match="bestRow"):
        run("asof", map_s, map_r, term, fault=_best_row)


def test_check_compares_the_host_form():
    """a host form that disagrees in one mark word, or in one pair, fails the check"""
    map_s, map_r, term = case(64, "where")
    ctx = HostContext()
    want = wc.model_call(map_s, map_r, 0, N_S, N_R, [term])
    good = {"info": want["info"], "s_idx": map_s[want["keep"]], "r_idx": map_r[want["keep"]], "s_marks": want["s_marks"], "r_marks": want["r_marks"]}
    bad_marks = dict(good, r_marks=want["r_marks"] ^ U32(1))
    bad_pairs = dict(good, r_idx=good["r_idx"] ^ U32(1))
    for host, ok in ((good, True), (bad_marks, False), (bad_pairs, False), (dict(good, info=(0, 0, 0, 0)), False)):
        with Device(ctx) as dev:
            s, op, r, s_valid, _ = term
            d_term = (dev.put(s), dev.put(r), 4, _lib.HJ_VAL_INT, _lib.CMP_OPS[op], dev.put(plane_words(s_valid)), 0)
            call = lambda ms, mr, os, o_r, c, ps, pr: ctx.pairs_where(ms, mr, 64, 0, N_S, N_R, [d_term], os, o_r, c, ps, pr)   # noqa: E731
            args = (dev, call, ctx.filter_info, map_s, map_r, N_S, N_R, want, 64, GUARD)
            if ok:
                check_pair_filter(*args, host=lambda: host)
            else:
                with pytest.raises(AssertionError):
                    check_pair_filter(*args, host=lambda: host)
