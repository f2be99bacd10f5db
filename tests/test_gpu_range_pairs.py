"""hj_range_index_dev / hj_range_pairs_dev on the device against the numpy model of range_common and the host twins: both
search levels and their seam (index sizes from hj_range_layout_info), runs of equal keys over pivots, every bracket, pick and
extreme, NULLs and NaNs, the expansion's tile and chunk edges, the capacity cuts, the 64-bit total and the two mark planes.
Every plane the calls write lies between guard words."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from gpu_harness import Device, GuardedPlane, SENTINEL, U32, ctx, plane_bits  # noqa: F401

import range_common as rc

pytestmark = pytest.mark.gpu
GUARD = 8
BRACKETS = [(a, b) for a in (False, True) for b in (False, True)]


def _plane(a):
    return None if a is None else rc.plane_words(a)


class Index:
    """R's column and its index on the device, the three planes between guard words, checked against the model once"""

    def __init__(self, dev, r, r_valid=None, tag=None):
        self.dev, self.r, self.r_valid, self.n = dev, np.ascontiguousarray(r), r_valid, r.size
        self.width, self.type = self.r.dtype.itemsize, rc.val_type(self.r.dtype)
        self.kdt = np.uint64 if self.width == 8 else U32
        self.perm = GuardedPlane(dev, self.n, front=GUARD, behind=GUARD)
        self.keys = GuardedPlane(dev, self.n, dtype=self.kdt, sentinel=int(SENTINEL) * (0x100000001 if self.width == 8 else 1), front=GUARD, behind=GUARD)
        self.head = GuardedPlane(dev, 4, front=GUARD, behind=GUARD)
        d_r, d_valid = dev.put(self.r), (dev.put(_plane(r_valid)) if r_valid is not None else 0)
        dev.ctx.range_index((d_r if self.n else 0, d_valid, self.width, self.type), self.n, self.perm.ptr if self.n else 0, self.keys.ptr if self.n else 0,
                            self.head.ptr)
        model = rc.model_index(self.r, r_valid)
        info = dev.ctx.range_index_info()
        head = self.head.read(None, tag)
        assert tuple(head) == model["head"] + (4 if self.width < 8 else 8,), (tag, head, model["head"])
        assert (info[0], info[1], info[3]) == model["head"], (tag, info)
        assert np.array_equal(self.perm.read(None, tag), model["perm"]), (tag, "perm")
        got = self.keys.read(None, tag)[:model["head"][0]]
        assert np.array_equal(np.unique(got, return_inverse=True)[1], np.unique(model["keys"], return_inverse=True)[1]), (tag, "keys")
        assert (got[1:] >= got[:-1]).all(), (tag, "the key plane ascends")


def check_call(dev, idx, lo, hi, lo_valid=None, hi_valid=None, lo_open=False, hi_open=False, pick="all", base=0, capacity=None, marks=True, pre=None,
               host=True, tag=None):
    """one range call on the index, checked in full against the model: the info words, the pairs (a sub-multiset under a cut),
    both mark planes bit for bit over what they held before (pre: (S words, R words)), the guard words of every plane; then the
    host twin. capacity None: the model's total. -> the model's dict"""
    ctx = dev.ctx
    n_s = (lo if lo is not None else hi).size
    want = rc.model_call(idx.r, lo, hi, idx.r_valid, lo_valid, hi_valid, lo_open, hi_open, pick, base)
    total = want["info"][0]
    capacity = total if capacity is None else capacity
    written = min(total, capacity)
    mine = []
    put = lambda a: 0 if a is None else (mine.append(dev.put(a)) or mine[-1])       # noqa: E731
    flags = (hj.HJ_RANGE_LO_OPEN if lo_open else 0) | (hj.HJ_RANGE_HI_OPEN if hi_open else 0)
    term = (put(lo), put(hi), idx.width, idx.type, flags, hj.RANGE_PICKS[pick], put(_plane(lo_valid)), put(_plane(hi_valid)))
    outs = [GuardedPlane(dev, capacity, front=3, behind=GUARD, what="a word outside the run was written") for _ in range(2)] if capacity else None
    sw, rw = -(-n_s // 32), -(-idx.n // 32)
    pre = pre or (np.zeros(sw, dtype=U32), np.zeros(rw, dtype=U32))
    planes = [GuardedPlane(dev, w, front=GUARD, behind=GUARD, body=p, what="a word outside the marks plane was written") for w, p in zip((sw, rw), pre)] if marks else None
    ctx.range_pairs(idx.keys.ptr if idx.n else 0, idx.perm.ptr if idx.n else 0, idx.head.ptr, idx.n, term, n_s, base, *([o.ptr for o in outs] if outs else [0, 0]),
                    capacity, *([p.ptr for p in planes] if planes else [0, 0]))
    info = ctx.range_pairs_info()
    print(tag, "rows", idx.n, n_s, "info", info, "model", want["info"])
    assert info[:2] == (total, written) and info[3:] == want["info"][3:], (tag, info, want["info"])
    got_s, got_r = (o.read(written, tag) for o in outs) if outs else (np.empty(0, dtype=U32), np.empty(0, dtype=U32))
    got = rc.packed(got_s, got_r)
    if written == total:
        assert np.array_equal(got, want["kept"]), (tag, "the pairs")
    else:
        assert got.size == written and np.unique(got).size == written and np.isin(got, want["kept"]).all(), (tag, "cut: not a sub-multiset")
    if planes:
        got_ps, got_pr = (p.read(None, tag) for p in planes)
        assert np.array_equal(got_ps, want["s_marks"] | pre[0]), (tag, "S marks")
        assert np.array_equal(got_pr, want["r_marks"] | pre[1]), (tag, "R marks")
    idx.head.read(None, tag), idx.perm.read(None, tag), idx.keys.read(None, tag)          # the index is read, never written
    if host:
        col = lambda a, v: None if a is None else hj.KeyColumn(a, v)      # noqa: E731
        h = hj.range_pairs_host(col(idx.r, idx.r_valid), col(lo, lo_valid), col(hi, hi_valid), lo_open, hi_open, pick, None, base)
        assert h["info"] == want["info"] and np.array_equal(rc.packed(h["s_idx"], h["r_idx"]), want["kept"]), (tag, "host twin")
        assert np.array_equal(h["s_marks"], want["s_marks"]) and np.array_equal(h["r_marks"], want["r_marks"]), (tag, "host marks")
    for o in (outs or []) + (planes or []):
        o.free()
    dev.free(*mine)
    return want


def _bounds(rng, r, n_s):
    """bounds that hit a key, fall between two keys, lie below the first and above the last"""
    pool = np.concatenate([r, r[:8] + 1, r[:8] - 1, np.array([-5, 1 << 30], dtype=r.dtype)]).astype(np.int64)
    lo = rng.choice(pool, n_s)
    hi = lo + rng.integers(-2, 12, n_s)                        # narrow ranges, some of them reversed
    wide = rng.choice(n_s, 3, replace=False)                    # and three that take everything
    lo[wide], hi[wide] = np.iinfo(r.dtype).min, np.iinfo(r.dtype).max
    return lo.astype(r.dtype), hi.astype(r.dtype)


def _sizes():
    small = hj.range_layout_info(1)
    stride = small["stride"]
    full = (small["lds_bytes"] // 8) * stride                   # the most rows the smallest stride takes
    big = hj.range_layout_info(full + 4000)
    assert big["stride"] == 2 * stride
    seam = big["pivots"] * big["stride"]
    return [0, 1, 2, stride - 1, stride, stride + 1, full - 1, full, full + 1, seam - 1, seam + 1]


@pytest.mark.parametrize("n", _sizes())
def test_index_sizes_around_both_search_levels_and_their_seam(ctx, n):
    rng = np.random.default_rng(n)
    r = (rng.integers(0, max(n // 2, 3), n) * 3).astype(np.int32)      # duplicates, and gaps to fall into
    with Device(ctx) as dev:
        idx = Index(dev, r, tag=n)
        lo, hi = _bounds(rng, r, 1500)
        for k, ((lo_open, hi_open), pick) in enumerate(zip(BRACKETS, ("all", "first", "last", "all"))):
            check_call(dev, idx, lo, hi, lo_open=lo_open, hi_open=hi_open, pick=pick, base=k * 1000, host=n <= 4096, tag=(n, lo_open, hi_open, pick))


def test_runs_of_equal_keys_over_the_pivots(ctx):
    stride = hj.range_layout_info(1)["stride"]
    with Device(ctx) as dev:
        for r in (np.full(5 * stride + 3, 7, dtype=np.uint16),                                    # all keys equal
                  np.repeat(np.arange(40, dtype=np.uint16) * 2, stride - 3),                       # runs that drift over the pivots
                  np.repeat(np.arange(9, dtype=np.uint16) * 2, 3 * stride + 1)):                   # runs longer than a stride
            idx = Index(dev, r[np.random.default_rng(1).permutation(r.size)])
            pts = np.arange(0, 84, dtype=np.uint16)
            lo, hi = np.repeat(pts, 12), np.tile(pts[::7], 84)
            for lo_open, hi_open in BRACKETS:
                for pick in rc.PICKS:
                    check_call(dev, idx, lo, hi, lo_open=lo_open, hi_open=hi_open, pick=pick, tag=(r.size, lo_open, hi_open, pick))


@pytest.mark.parametrize("dtype", rc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_directed_cases_of_every_type(ctx, dtype):
    """bounds on, between, below and above the keys; lo > hi; lo == hi open and closed; the type's extremes (INT64_MIN,
    UINT64_MAX, +-inf) as open and closed bounds; -0.0 against 0.0; NULL and NaN bounds and elements; a base"""
    r, lo, hi = rc.directed(dtype)
    rng = np.random.default_rng(3)
    with Device(ctx) as dev:
        idx = Index(dev, r)
        for lo_open, hi_open in BRACKETS:
            for pick in rc.PICKS:
                check_call(dev, idx, lo, hi, lo_open=lo_open, hi_open=hi_open, pick=pick, base=77, tag=(lo_open, hi_open, pick))
        check_call(dev, idx, lo, None, lo_open=True, tag="hi unbounded")
        check_call(dev, idx, None, hi, hi_open=True, pick="last", tag="lo unbounded: the keyless as-of")
        r_valid, lo_valid, hi_valid = rng.random(r.size) > 0.3, rng.random(lo.size) > 0.1, rng.random(lo.size) > 0.1
        if np.dtype(dtype).kind == "f":
            r, lo = np.concatenate([r, [np.nan, -np.nan, -0.0, 0.0]]).astype(dtype), lo.copy()
            r_valid = np.concatenate([r_valid, [True] * 4])
            lo[::5] = np.nan
        idx = Index(dev, r, r_valid)
        for pick in rc.PICKS:
            want = check_call(dev, idx, lo, hi, lo_valid, hi_valid, pick=pick, tag=("NULLs and NaNs", pick))
            assert want["info"][4] >= (~lo_valid).sum() and not (plane_bits(want["r_marks"], r.size) & ~r_valid).any()


def test_expansion_over_tile_and_chunk_edges(ctx):
    l = hj.range_layout_info(1, 1)
    tile, chunk = l["tile"], l["chunk_rows"]
    n_r, n_s = 3 * tile + 500, 2 * chunk + 100
    r = np.random.default_rng(2).permutation(n_r).astype(np.uint32)
    with Device(ctx) as dev:
        idx = Index(dev, r)
        lo, hi = np.full(n_s, 9, dtype=np.uint32), np.zeros(n_s, dtype=np.uint32)                 # empty: lo > hi
        for row, (a, b) in {0: (0, 0), chunk - 1: (5, 9), chunk + 5: (0, n_r), 2 * chunk - 1: (n_r - 1, n_r - 1), 2 * chunk: (3, 700), n_s - 1: (1, 1)}.items():
            lo[row], hi[row] = a, b                     # one row spans more than three tiles, between runs of empty rows
        want = check_call(dev, idx, lo, hi, base=5, tag="one row over three tiles")
        assert want["info"][0] > 3 * tile
        # totals of exactly a tile multiple and one to either side: rows of 1, 2, 3.. pairs, trimmed
        for delta in (-1, 0, 1):
            cnt = np.zeros(n_s, dtype=np.int64)
            cnt[::3] = np.arange(cnt[::3].size) % 5
            at = np.flatnonzero(cnt)
            excess = int(cnt.sum()) - (2 * tile + delta)
            assert excess > 0
            for row in at[::-1]:
                take = min(excess, int(cnt[row]))
                cnt[row] -= take
                excess -= take
                if not excess:
                    break
            lo = (np.arange(n_s) % 1000).astype(np.uint32)
            hi = (lo + cnt - 1).astype(np.uint32)
            lo[cnt == 0], hi[cnt == 0] = 9, 0
            want = check_call(dev, idx, lo, hi, tag=("tile multiple", delta))
            assert want["info"][0] == 2 * tile + delta


def test_capacity_cuts(ctx):
    rng = np.random.default_rng(4)
    r = rng.integers(0, 300, 900).astype(np.int16)
    lo = rng.integers(0, 300, 700).astype(np.int16)
    hi = (lo + rng.integers(0, 6, 700)).astype(np.int16)
    with Device(ctx) as dev:
        idx = Index(dev, r)
        total = rc.model_call(r, lo, hi)["info"][0]
        assert total > 4096
        for cap in (0, 1, total // 2, 2048, 2049, total - 1, total, total + 9):       # a cut in the middle of a row and at a tile edge
            check_call(dev, idx, lo, hi, capacity=cap, host=False, tag=("capacity", cap))
        check_call(dev, idx, lo, hi, pick="last", capacity=100, host=False, tag="capacity under a pick")


def test_the_total_is_exact_in_64_bits(ctx):
    """65 537 S rows that each match all of 65 537 R rows: 2^32 + 131 073 pairs, 4097 of them written; no per-pair work"""
    n, cap = 65537, 4097
    r = np.random.default_rng(6).integers(-50, 50, n).astype(np.int32)
    with Device(ctx) as dev:
        idx = Index(dev, r)
        d_lo = dev.put(np.full(n, -1000, dtype=np.int32))
        outs = [GuardedPlane(dev, cap, front=GUARD, behind=GUARD) for _ in range(2)]
        planes = [GuardedPlane(dev, -(-n // 32), front=GUARD, behind=GUARD, body=0) for _ in range(2)]
        ctx.range_pairs(idx.keys.ptr, idx.perm.ptr, idx.head.ptr, n, (d_lo, 0, 4, hj.HJ_VAL_INT), n, 0, outs[0].ptr, outs[1].ptr, cap, planes[0].ptr, planes[1].ptr)
        info = ctx.range_pairs_info()
        print("64-bit total", info)
        assert info[0] == n * n == (1 << 32) + 131073 and info[1] == cap and info[3:6] == (n, 0, n)
        got_s, got_r = outs[0].read(), outs[1].read()
        assert (got_s < n).all() and (got_r < n).all() and np.unique(rc.packed(got_s, got_r)).size == cap
        for p in planes:
            assert plane_bits(p.read(), n).all() and np.array_equal(p.read(), rc.plane_words(np.ones(n, dtype=bool)))


def test_mark_planes(ctx):
    """overlapping, adjacent, identical and empty ranges; position 0 and the last indexed position; bits set before the call
    survive; a mark-only pass equals the full pass; FIRST / LAST mark winners only, ties to the lowest R row"""
    r = np.array([10, 20, 20, 30, 40, 40, 40, 50, 60, 70] * 7, dtype=np.int64)
    r_valid = np.ones(r.size, dtype=bool)
    r_valid[[3, 69]] = False
    lo = np.array([10, 20, 20, 30, 41, 45, 70, 10, 60, 5, 80, 40, 40], dtype=np.int64)
    hi = np.array([20, 30, 30, 39, 49, 44, 70, 10, 65, 9, 90, 40, 40], dtype=np.int64)
    rng = np.random.default_rng(8)
    with Device(ctx) as dev:
        idx = Index(dev, r, r_valid)
        pre = (rng.integers(0, 1 << 32, 1, dtype=np.uint64).astype(U32), rng.integers(0, 1 << 32, 3, dtype=np.uint64).astype(U32) & U32(0x11111111))
        for pick in rc.PICKS:
            for lo_open, hi_open in BRACKETS:
                full = check_call(dev, idx, lo, hi, lo_open=lo_open, hi_open=hi_open, pick=pick, tag=("marks", pick, lo_open, hi_open))
                only = check_call(dev, idx, lo, hi, lo_open=lo_open, hi_open=hi_open, pick=pick, capacity=0, pre=pre, host=False, tag=("mark-only", pick))
                assert np.array_equal(full["r_marks"], only["r_marks"]) and np.array_equal(full["s_marks"], only["s_marks"])
        last = rc.model_call(r, lo[11:12], hi[11:12], r_valid, pick="last")
        assert np.flatnonzero(plane_bits(last["r_marks"], r.size)).tolist() == [4]        # the lowest row of the 21 that hold 40
        check_call(dev, idx, lo, hi, marks=False, tag="no planes")


@pytest.mark.parametrize("dtype", rc.DTYPES, ids=lambda d: np.dtype(d).name)
def test_device_host_and_model_agree_on_a_seeded_fuzz(ctx, dtype):
    with Device(ctx) as dev:
        for seed, ((lo_open, hi_open), pick) in enumerate(zip(BRACKETS, ("all", "last", "first", "all"))):
            r, rv, lo, hi, lv, hv = rc.fuzz_case(200 + seed, dtype, 3000, 2500)
            idx = Index(dev, r, rv, tag=seed)
            check_call(dev, idx, lo, hi, lv, hv, lo_open, hi_open, pick, base=seed * 4099, tag=(seed, lo_open, hi_open, pick))
            check_call(dev, idx, None, hi, None, hv, hi_open=hi_open, pick="last", capacity=50, host=False, tag=(seed, "as-of, cut"))
