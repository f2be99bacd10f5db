"""hj_window_frames_dev / hj_window_frames_info on an MI355X, through ctypes -> C ABI. At every case the device result equals
the host twin (a running window and a deque) AND the model of frames_common (cumulative sums and slices) bit for bit, every
output lies between guard words that are checked, and the info fields equal the model's partitions and skipped entries.
The sizes come from hj_frames_layout_info (T = tile positions, L = chunk positions), not from constants; n is at most
5 L + 77. Run with -m gpu."""
import numpy as np
import pytest

from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

from gpu_harness import Device, GuardedPlane, dev  # noqa: F401
import frames_common as fc
import window_common as wc

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
A = _lib
GUARD = 64                       # entries in front of and behind every output
T, L = fc.layout(1)[:2]          # at the sizes of this file the chunk is the smallest one
assert fc.layout(1 << 17)[:2] == (T, L) and L >= 2 * T
N = 2 * L + T + 17               # three chunks, the last one short, no multiple of anything
FAR = fc.FAR
WIDTHS = (1, 2, 63, 64, 65, 512, T - 1, T, T + 1, L - 1, L, L + 1, 2 * L + 5, N - 1, N, N + 1, FAR)
SINGLES = [(-1, -1), (0, 0), (1, 1), (-(L + 1), -(L + 1)), (-FAR, FAR)]


def on_device(dev, case, tag=None, garbage=None, funcs=None, release=True):
    """one hj_window_frames_dev -> ([one array per function], the info dict)"""
    funcs = case.funcs if funcs is None else funcs
    d_perm = dev.put(case.perm) if case.perm is not None else 0
    d_part = dev.put(case.part) if case.part is not None else 0
    outs, desc = [GuardedPlane(dev, case.n_rows, U64, fc.SENT64, front=GUARD, behind=GUARD, what="an entry outside out was written") for _ in funcs], []
    for f, o in zip(funcs, outs):
        plane = f.plane(case.n_rows, garbage)
        desc.append((f.op, o.ptr, f.lo, f.hi, dev.put(f.src) if f.src is not None else 0, dev.put(plane) if plane is not None else 0, f.width, f.flags))
    dev.ctx.window_frames(d_perm, case.n_pos, case.n_rows, d_part, desc)
    info = dev.ctx.window_frames_info()
    got = [o.read(case.n_rows, tag) for o in outs]
    if release:
        dev.release()
    return got, info


def check(dev, case, tag=None):
    """device == host twin == model, and the info fields"""
    garbage = np.random.default_rng(case.n_pos + len(case.funcs))
    want, counts = fc.model(case)
    got, info = on_device(dev, case, tag, garbage)
    fc.same(got, want, (tag, "device against the model"))
    host, host_info = fc.host_call(case, garbage)
    fc.same(host, got, (tag, "host twin against the device"))
    fc.check_info(list(info.values()), case, counts, tag)
    assert list(info.values())[:3] + list(info.values())[4:] == host_info[:3] + host_info[4:], (tag, info, host_info)
    return got, info


# ---- widths ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", WIDTHS)
def test_every_width_placed_four_ways(dev, w):
    """trailing, leading, centred, clear of the row on both sides; three of the one-position frames and the widest one beside them"""
    k = WIDTHS.index(w)
    frames = fc.placements(w) + [SINGLES[(k + i) % len(SINGLES)] for i in range(3)]
    frames = [(max(lo, -FAR), min(hi, FAR)) for lo, hi in frames]
    check(dev, fc.build(N, fc.rotate(frames, k), "one", seed=k), ("one partition", w))
    check(dev, fc.build(N, fc.rotate(frames, k + 3), "geometric", seed=k + 1), ("geometric", w))


@pytest.mark.parametrize("w", [2, 64, 65, T + 1, L])
def test_partitions_of_the_block_size_and_one_off(dev, w):
    """partitions of W - 1, W and W + 1 positions: block borders fall on, before and behind the partition heads"""
    frames = fc.placements(w) + [(-(w - 1), 1), (-1, w - 2 if w > 2 else 0), (0, 0)]
    for i, k in enumerate((w - 1, w, w + 1)):
        check(dev, fc.build(N, fc.rotate(frames, i), f"fixed{k}", seed=i), ("fixed", w, k))


@pytest.mark.parametrize("shape", ["seams", "each", "one", "geometric"])
def test_partition_shapes(dev, shape):
    frames = [(-6, 0), (-63, 0), (0, 64), (-(T - 1), 0), (-T // 2, L), (-(L + 1), -1), (2, 2 * L), (-3, -1)]
    for i, n in enumerate((L, N)):
        check(dev, fc.build(n, fc.rotate(frames, 3 * i), shape, seed=i), (shape, n))


def test_a_block_carry_over_chunks_without_a_head(dev):
    """one partition over at least three whole chunks, W = 2 L + 5 and W = L: the carry of a block crosses chunks that hold no
    head, forwards for G and backwards for H"""
    n = 5 * L + 77
    frames = fc.placements(2 * L + 5)[:4] + fc.placements(L)[:4]
    for i, perm in enumerate(("random", None)):
        check(dev, fc.build(n, fc.rotate(frames, 4 * i + 1), "long", perm=perm, seed=i), ("long", perm))
    ids = wc.shape_ids("long", n)
    assert (np.bincount(ids)[1] >= 3 * L) and ids[L] == ids[4 * L] == 1


# ---- unbounded sides and empty frames ------------------------------------------------------------------------------------------------
def test_unbounded_sides(dev):
    """each side unbounded with the other at 0, 1 and L + 1 on either side of the row, and both"""
    a = [(None, 0), (None, 1), (None, L + 1), (None, -1), (None, -(L + 1)), (None, None), (0, None), (1, None)]
    b = [(L + 1, None), (-1, None), (-(L + 1), None), (None, None), (0, None), (None, 0), (None, 1), (-1, None)]
    for i, (n, shape) in enumerate(((5 * L + 77, "long"), (N, "geometric"), (N, "one"), (N, f"fixed{L + 3}"))):
        for j, frames in enumerate((a, b)):
            check(dev, fc.build(n, fc.rotate(frames, i + 4 * j), shape, seed=i), ("unbounded", n, shape, j))


def test_empty_frames_at_the_head_and_the_tail_of_every_partition(dev):
    """partitions of 7 positions and frames clear of the row: the identity and COUNT 0 where the frame leaves the partition"""
    n, k = L + T + 5, 7
    part = (np.arange(n) // k).astype(U32)
    rng = np.random.default_rng(5)
    src = rng.integers(-1 << 62, 1 << 62, n).astype(np.int64)
    frames = [(-5, -3), (3, 5), (None, -3), (3, None)]
    funcs = [fc.Func(A.HJ_AGG_COUNT, lo, hi) for lo, hi in frames] + [fc.Func(A.HJ_AGG_MIN, -5, -3, src), fc.Func(A.HJ_AGG_MAX, 3, 5, src),
                                                                     fc.Func(A.HJ_AGG_SUM, -5, -3, src), fc.Func(A.HJ_AGG_MAX, L + 1, L + 2, src)]
    got, _ = check(dev, fc.Case(n, n, None, part, funcs), "empty frames")
    at, size = np.arange(n) % k, np.minimum(k, n - np.arange(n) // k * k)
    before, behind = at < 3, size - 1 - at < 3
    assert (got[0][before] == 0).all() and (got[2][before] == 0).all() and (got[0][~before] > 0).all()
    assert (got[1][behind] == 0).all() and (got[3][behind] == 0).all() and (got[1][~behind] > 0).all()
    assert (got[4][before] == (1 << 63) - 1).all() and (got[5][behind] == 1 << 63).all() and (got[6][before] == 0).all()
    assert (got[7] == 1 << 63).all()                                    # a frame a chunk away from a partition of 7


# ---- perms, holes, rows at no position -----------------------------------------------------------------------------------------------
MIXED = [(-6, 0), (0, 6), (-3, -1), (None, None), (-(T + 1), 0), (-1, L), (None, 0), (-FAR, FAR)]


@pytest.mark.parametrize("perm", ["random", "identity", None])
def test_permutations(dev, perm):
    for i, n in enumerate((1, T + 1, N)):
        check(dev, fc.build(n, fc.rotate(MIXED, i), "geometric", perm=perm, extra_rows=5, seed=i), ("perm", perm, n))
    if perm is None:
        case = fc.build(L + 1, MIXED, "fixed65", perm=None)
        with_plane = fc.Case(case.n_pos, case.n_rows, np.arange(case.n_pos, dtype=U32), case.part, case.funcs)
        fc.same(on_device(dev, case)[0], on_device(dev, with_plane)[0], "dPerm NULL against the identity plane")


def test_entries_out_of_range(dev):
    """HJ_NO_ROW and rows >= nRows at position 0, at the last position, at the chunk seams and sprinkled in: they cut the runs"""
    for n in (3, L + 1, N):
        for shape in ("geometric", "one"):
            case = fc.build(n, fc.rotate(MIXED, n % 8), shape, holes=n // 50 + 1, extra_rows=13, seed=n % 4)
            _, info = check(dev, case, ("holes", n, shape))
            assert info["skipped"] >= min(n, 2)
    funcs = [fc.Func(A.HJ_AGG_COUNT, -1, 1), fc.Func(A.HJ_AGG_COUNT, None, None)]
    _, info = check(dev, fc.Case(10, 4, np.array([4, 5, fc.NO_ROW] * 3 + [9], dtype=U32), None, funcs), "all skipped")
    assert (info["partitions"], info["peer_runs"], info["skipped"]) == (0, 0, 10)


def test_rows_at_no_position_keep_the_sentinel(dev):
    n_pos, extra = L + 100, 3000
    case = fc.build(n_pos, MIXED, "geometric", extra_rows=extra, seed=2)
    got, _ = check(dev, case, "nPos < nRows")
    absent = np.setdiff1d(np.arange(n_pos + extra), case.perm[:n_pos].astype(np.int64))
    assert absent.size == extra and all((g[absent] == fc.SENT64).all() for g in got)


def test_an_unsorted_permutation(dev):
    rng = np.random.default_rng(9)
    n, extra = N, 50
    perm = rng.permutation(n + extra).astype(U32)
    part = rng.integers(0, 2, n + extra).astype(U32)
    base = fc.build(n + extra, MIXED, "one", perm=None)
    _, info = check(dev, fc.Case(n, n + extra, perm, part, base.funcs), "random runs")
    assert info["partitions"] > n // 4


# ---- data ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("null_pct", [0, 10, 100])
def test_source_types_and_nulls(dev, null_pct):
    """int32, uint32, int64, uint64: sums that wrap 2^64, the extremes of the signed types, counts with and without a plane"""
    for i, (n, shape) in enumerate(((65, "fixed3"), (N, "geometric"), (3 * L + 1, "one"))):
        for k in (0, 3):
            check(dev, fc.build(n, fc.rotate(MIXED, k + i), shape, null_pct=null_pct, seed=null_pct + i), (n, shape, null_pct, k))


# ---- call structure ------------------------------------------------------------------------------------------------------------------
def test_eight_functions_with_eight_frames_in_one_call_or_one_by_one(dev):
    frames = [(-6, 0), (0, T), (-(L + 1), L + 1), (None, None), (3, 9), (None, -2), (-64, 63), (0, None)]
    assert len(set(frames)) == 8
    case = fc.build(N, frames, "geometric", seed=6)
    together, _ = check(dev, case, "together")
    for i, f in enumerate(case.funcs):
        alone, _ = on_device(dev, case, ("alone", i), funcs=[f])
        assert alone[0].tobytes() == together[i].tobytes(), i


def test_workspace_growth_and_reuse():
    """large then small, and small then large, each on a context of its own: the workspace grows once and is reused"""
    big, small = fc.build(1 << 15, MIXED[:4], "geometric"), fc.build(1000, MIXED[4:], "fixed3")
    for order in ((big, small, big), (small, big, small)):
        d = Device()
        try:
            sizes = [check(d, case, ("reuse", case.n_pos))[1]["workspace_bytes"] for case in order]
            assert sizes[0] == sizes[2] != sizes[1]
        finally:
            d.close()


def test_no_positions_and_refused_calls(dev):
    case = fc.build(1000, MIXED, "geometric")
    check(dev, case, "before")
    out = dev.put(np.full(8, fc.SENT64, dtype=U64))
    f_arr, _ = fc.func_array([fc.Func(A.HJ_AGG_COUNT, -1, 0)], [(out, 0, 0)])
    assert lib.hj_window_frames_dev(dev.ctx._h, None, 8, 8, None, f_arr, 0) == _lib.HJ_ERR_INVALID
    assert b"hj_window_frames_dev" in lib.hj_last_error(dev.ctx._h)
    f_arr[0].lo, f_arr[0].hi = 1, 0
    assert lib.hj_window_frames_dev(dev.ctx._h, None, 8, 8, None, f_arr, 1) == _lib.HJ_ERR_INVALID
    assert dev.ctx.window_frames_info()["positions"] == 1000                                    # a refused call is no call
    assert (dev.get(out, 8, U64) == fc.SENT64).all()
    dev.ctx.window_frames(0, 0, 8, 0, [(A.HJ_AGG_COUNT, out, -1, 0)])
    assert list(dev.ctx.window_frames_info().values()) == [0] * 8
    assert (dev.get(out, 8, U64) == fc.SENT64).all()
    dev.release()
