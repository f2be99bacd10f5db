"""The one device harness of the GPU tests: the only place in tests/ that allocates device memory for a test. Device buffers
that are freed at the end, planes between guard words that are checked when they are read, the one-bit-per-row plane in both
directions, the fixtures every GPU file shares, and the full check of one pair-filter call (verify, verify2, where, as-of).
No test in here, and nothing that asks the library what a result should be; test_gpu_harness.py tests this module on host
memory, without a GPU."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

import stream_order as so

SENTINEL = 0xA5A5A5A5
U32, U64 = np.uint32, np.uint64


# ---- device buffers -------------------------------------------------------------------------------------------------------------
def alloc(ctx, nbytes):
    """the one allocation rule: whole 32-bit words, 16 bytes at least. For a buffer the caller frees itself with ctx.dev_free"""
    return ctx.dev_alloc(max((int(nbytes) + 3) & ~3, 16))


class Device:
    """the device buffers of one test on a context: the caller's (`with Device(ctx) as dev:` frees them at the end), or one
    of its own (Device(); release() frees the buffers, close() the context too)"""

    def __init__(self, ctx=None):
        self.owns = ctx is None
        self.ctx, self.ptrs = hj.HashJoinContext(0) if ctx is None else ctx, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

    def alloc(self, nbytes):
        self.ptrs.append(alloc(self.ctx, nbytes))
        return self.ptrs[-1]

    def free(self, *ptrs):
        for p in ptrs:
            self.ptrs.remove(p)
            self.ctx.dev_free(p)

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = self.alloc(a.nbytes)
        if a.nbytes:
            self.ctx.copy_h2d(p, a)
        return p

    def get(self, ptr, n, dtype=U32):
        out = np.empty(n, dtype=dtype)
        if n:
            self.ctx.copy_d2h(out, ptr)
        return out

    def column(self, col):
        """(values, offsets, validity) of a KeyColumn on the device, 0 for what it has none of"""
        return tuple(self.put(a) if a is not None else 0 for a in col.take(0, col.rows))

    def release(self):
        for p in self.ptrs:
            self.ctx.dev_free(p)
        self.ptrs = []

    def close(self):
        self.release()
        if self.owns:
            self.ctx.close()


class GuardedPlane:
    """n entries of `dtype` on the device, `front` guard entries before them and `behind` after them. Every guard entry holds
    the sentinel, and so does the body unless `body` gives its content (a mark plane starts as zeros, a plane the call
    initialises itself as junk). ptr is the body's address. One upload, and one download per read()."""

    def __init__(self, dev, n, dtype=U32, sentinel=SENTINEL, front=0, behind=0, body=None, what="a word outside the plane was written"):
        self.dev, self.n, self.dtype, self.sentinel, self.front, self.behind, self.what = dev, int(n), np.dtype(dtype), sentinel, front, behind, what
        image = np.full(front + self.n + behind, sentinel, dtype=self.dtype)
        if body is not None:
            image[front:front + self.n] = body
        self.base = dev.put(image)
        self.ptr = self.base + front * self.dtype.itemsize

    def read(self, written=None, tag=None):
        """the first `written` entries of the body (default: all n). Asserts that both guards and the body behind `written`
        still hold the sentinel"""
        written = self.n if written is None else int(written)
        assert 0 <= written <= self.n, (tag, written, self.n)
        a = self.dev.get(self.base, self.front + self.n + self.behind, self.dtype)
        assert (a[:self.front] == self.sentinel).all() and (a[self.front + written:] == self.sentinel).all(), (tag, self.what)
        return a[self.front:self.front + written]

    def free(self):
        self.dev.free(self.base)


# ---- the one-bit-per-row plane: bit i & 31 of word i >> 5 -----------------------------------------------------------------------
def plane_words(bits):
    """one bool per row -> the plane as uint32 words, the bits behind the last row clear"""
    bits = np.asarray(bits, dtype=bool)
    padded = np.zeros(-(-bits.size // 32) * 32, dtype=bool)
    padded[:bits.size] = bits
    return np.packbits(padded, bitorder="little").view(U32).copy()


def plane_bits(words, n):
    """the plane's words -> one bool per row for its first n rows"""
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:n].astype(bool)


def row_bits(rows, n):
    """one bool per row of n rows: exactly `rows` are set"""
    bits = np.zeros(n, dtype=bool)
    bits[np.asarray(rows, dtype=np.int64)] = True
    return bits


# ---- pairs ------------------------------------------------------------------------------------------------------------------------
def packed(s, r):
    """the pairs (s[k], r[k]) as s << 32 | r, sorted: a multiset that compares with array_equal"""
    return np.sort((np.asarray(s).astype(U64) << U64(32)) | np.asarray(r).astype(U64))


def assert_sub_multiset(got, kept, tag=None):
    """every pair of `got` is one of `kept`, each at most as often as it was kept (both packed)"""
    pool, counts = np.unique(kept, return_counts=True)
    mine, mine_counts = np.unique(got, return_counts=True)
    at = np.searchsorted(pool, mine)
    assert (at < pool.size).all() and np.array_equal(pool[at], mine) and (mine_counts <= counts[at]).all(), (tag, "cut: not a sub-multiset of the kept pairs")


def status(call, *args, **kw):
    """the status a call of the library ends with"""
    try:
        call(*args, **kw)
    except hj.HashJoinError as e:
        return e.status
    return _lib.HJ_OK


# ---- the shared fixtures: a test module gets one by importing its name, and with it an instance of its own ----------------------
@pytest.fixture(scope="module")
def ctx():
    c = hj.HashJoinContext(0)
    yield c
    c.close()


@pytest.fixture(name="ctx")
def ctx_per_test():
    """`ctx` for a module whose every test starts on a context of its own: the module imports this name instead of ctx"""
    with hj.HashJoinContext(0) as c:
        yield c


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


@pytest.fixture(scope="module", params=so.FLAVOURS)
def fl(request):
    f = so.Flavour(request.param)
    assert so.witness(f)         # misused on purpose, the harness sees the decoy: the cases of the module cannot pass vacuously
    return f


# ---- the full check of one pair-filter call -----------------------------------------------------------------------------------------
def check_pair_filter(dev, call, read_info, map_s, map_r, s_rows, r_rows, want, capacity, guard, offset=0, marks=True, extra=(), host=None,
                      tag=None):
    """One call of a pair filter (hj_pairs_verify_dev, hj_pairs_verify2_dev, hj_pairs_where_dev, hj_pairs_asof_dev) over the
    maps, checked in full. The caller has its columns on `dev` already and makes the call itself:

        call(d_map_s, d_map_r, d_out_s, d_out_r, capacity, d_s_marks, d_r_marks, *[p.ptr for _, p, _, _ in extra])

    with 0 for the output planes at capacity 0 and for the mark planes with marks=False; read_info() gives the call's record
    (kept, written, us, dropped). want: the expectation as where_common.model_call gives it -- "kept" (packed, sorted), "info"
    (kept, written, 0, dropped), "s_marks" / "r_marks" (the planes a call on cleared planes leaves). The output planes have
    `offset` sentinel words in front of them (a misaligned plane) and `guard` behind, the mark planes `guard` on either side.
    extra: (key, GuardedPlane, its expected body or None, the message when it differs) per further plane of the call; host: a
    function without arguments that gives the host form's dict for the same input, or None.

    Asserted: the info triple; no word outside the written run, the mark planes or an extra plane; the marks bit for bit; the
    extra planes; the maps unwritten; the kept multiset, or under a cut a sub-multiset of it; then the host form's info, marks,
    extra planes and, without a cut, pairs. -> (the S entries and the R rows as written, the S and the R mark plane or None)"""
    n, sw, rw = map_s.size, -(-s_rows // 32), -(-r_rows // 32)
    kept, written = want["info"][0], want["info"][1]
    d_ms, d_mr = dev.put(map_s), dev.put(map_r)
    outs = [GuardedPlane(dev, capacity, front=offset, behind=guard, what="a word outside the run was written") for _ in range(2)] if capacity else None
    planes = [GuardedPlane(dev, words, front=guard, behind=guard, body=0, what="a word outside the marks plane was written")
              for words in (sw, rw)] if marks else None
    call(d_ms, d_mr, *([o.ptr for o in outs] if outs else [0, 0]), capacity, *([p.ptr for p in planes] if planes else [0, 0]),
         *[p.ptr for _, p, _, _ in extra])
    info = read_info()
    print(tag, "pairs", n, "info", info, "model", want["info"])
    assert (info[0], info[1], info[3]) == (kept, written, want["info"][3]), (tag, info, want["info"])
    got_s, got_r = (o.read(written, tag) for o in outs) if outs else (np.empty(0, dtype=U32), np.empty(0, dtype=U32))
    got_ps = got_pr = None
    if planes:
        got_ps, got_pr = (p.read(None, tag) for p in planes)
        assert np.array_equal(got_ps, want["s_marks"]), (tag, "S marks")      # bit for bit, cut pairs included
        assert np.array_equal(got_pr, want["r_marks"]), (tag, "R marks")
    got_extra = {}
    for key, plane, expected, message in extra:
        got_extra[key] = plane.read(None, tag)
        if expected is not None:
            assert np.array_equal(got_extra[key], expected), (tag, message)
    assert np.array_equal(dev.get(d_ms, n), map_s) and np.array_equal(dev.get(d_mr, n), map_r), (tag, "a map was written")
    got = packed(got_s, got_r)
    if written == kept:
        assert np.array_equal(got, want["kept"]), (tag, "the kept pairs")
    else:       # cut by the capacity: any `written` of the kept pairs, each at most as often as it was kept
        assert got.size == written, (tag, "cut")
        assert_sub_multiset(got, want["kept"], tag)
    if host is not None:        # the same code in a host loop: the same multiset, the same planes, the same words
        h = host()
        assert h["info"] == tuple(want["info"]), (tag, h["info"])
        if written == kept:
            assert np.array_equal(packed(h["s_idx"], h["r_idx"]), got), (tag, "host and device disagree")
        assert np.array_equal(h["s_marks"], want["s_marks"]) and np.array_equal(h["r_marks"], want["r_marks"]), (tag, "host marks")
        for key, plane_got in got_extra.items():
            if key in h:
                assert np.array_equal(h[key], plane_got), (tag, key, "host and device disagree")
    return got_s, got_r, got_ps, got_pr
