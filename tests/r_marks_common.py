"""What the tests of the R-side match marks share (test_gpu_r_marks.py, test_gpu_prj_r_marks.py): the references for the
inner pairs (restated from test_gpu_join_kinds.py / test_gpu_prj_join_kinds.py: numpy and plain Python, never the
library), and Marks, which keeps in numpy what a tracking context must remember and checks hj_r_rows_dev against it.
Unmatched R = setdiff1d(arange(base, base + n), unique(inner & 0xFFFFFFFF)). No test in here."""
import numpy as np

from gpu_harness import GuardedPlane
from join_kinds_common import SENTINEL, GUARD, U64, INNER, LEFT, SEMI, ANTI, Calls, zipf  # noqa: F401

UNMATCHED, MATCHED = 0, 1
LOW = U64(0xFFFFFFFF)
# hj_r_marks.hip: a workgroup of the sweep takes kSweepWords = 256 words of the plane = 8192 rows; the scan of the block
# counts (launch_exclusive_scan_u32, hj_scan.hip) works in tiles of kScanTile = 4096 entries
SWEEP_ROWS = 32 * 256
SCAN_TILE = 4096


def valid_s(S):
    return ((S >> U64(32)) == 0) & (S != 0)


def join_expected(R, S, r_base=0, s_base=0, any_key=False):
    """all (i, j) with S[i] == R[j], packed s << 32 | r and sorted: sort R, searchsorted S, expand the runs. any_key (the
    radix join): the key is the low word, 0 included; otherwise tuples outside the DataGen layout match nothing"""
    if any_key:
        R, S = R & LOW, S & LOW
    order = np.argsort(R, kind="stable")
    Rs = R[order]
    lo = np.searchsorted(Rs, S, "left")
    cnt = np.searchsorted(Rs, S, "right") - lo
    if not any_key:
        cnt[~valid_s(S)] = 0
    total = int(cnt.sum())
    s_idx = np.repeat(np.arange(S.size, dtype=np.int64), cnt)
    within = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    r_idx = order[np.repeat(lo, cnt) + within]
    return np.sort(((s_idx + s_base).astype(U64) << U64(32)) | (r_idx + r_base).astype(U64))


def walk_expected(R, S, probe_length, r_base=0, s_base=0):
    """open addressing, plain Python: sequential insert in input order keeping (index, key) per slot
    (NoCCHashBuild.hpp:43-59, the walk wraps; a tuple that exhausts probeLength is dropped), then the probe walk (:70-79:
    at most probeLength slots from the home slot, no wrap, stop at the first empty one)"""
    n = R.size
    mask = 2 * n - 1
    keys, idx = [0] * (2 * n + 16), [0] * (2 * n + 16)
    for i, k in enumerate(R.tolist()):
        cur, budget = k & mask, probe_length
        while budget:
            if keys[cur] == 0:
                keys[cur], idx[cur] = k, i
                break
            cur = (cur + 1) & mask
            budget -= 1
    out = []
    for i, s in enumerate(S.tolist()):
        if s == 0 or s >> 32:
            continue
        cur = s & mask
        for _ in range(probe_length):
            if keys[cur] == 0:
                break
            if keys[cur] == s:
                out.append(((i + s_base) << 32) | (idx[cur] + r_base))
            cur += 1
    return np.sort(np.array(out, dtype=U64))


def inner_expected(algo, R, S, probe_length=4, r_base=0, s_base=0):
    if algo == "prj":
        return join_expected(R, S, r_base, s_base, any_key=True)
    if algo == "htm":
        return join_expected(R, S, r_base, s_base)
    return walk_expected(R, S, probe_length, r_base, s_base)


def r_rows_of(inner):
    return np.unique(inner & LOW)


def unmatched_r(inner, n, base=0):
    return np.setdiff1d(np.arange(base, base + n, dtype=U64), r_rows_of(inner), assume_unique=True)


class Marks:
    """What the marks of a context must be since its last build of n R rows from `base`: every R row of the inner pairs
    of its INNER / LEFT calls. sweep() is one hj_r_rows_dev with guard words behind the capacity; check() both `which`
    values at full capacity, element for element."""

    def __init__(self, ctx, dev, n, base=0):
        self.ctx, self.dev, self.n, self.base = ctx, dev, n, base
        self.seen = np.empty(0, dtype=U64)

    def add(self, inner):
        self.seen = np.union1d(self.seen, inner & LOW)

    def clear(self):
        self.seen = np.empty(0, dtype=U64)

    def expected(self, which):
        if which == MATCHED:
            return self.seen
        return np.setdiff1d(np.arange(self.base, self.base + self.n, dtype=U64), self.seen, assume_unique=True)

    def sweep(self, which, capacity=None, null_plane=False):
        """-> (produced, written, the rows written); no word behind them was written"""
        cap = self.n + 64 if capacity is None else capacity
        plane = None if null_plane else GuardedPlane(self.dev, cap, behind=GUARD, what="a word behind the last row was written")
        self.ctx.r_rows(which, plane.ptr if plane else 0, cap)
        produced, written, _us, rows = self.ctx.r_rows_info()
        assert rows == self.n, (rows, self.n)
        got = None
        if plane:
            got = plane.read(written, which)
            plane.free()
        return produced, written, got

    def check(self, tag=None):
        for which in (UNMATCHED, MATCHED):
            want = self.expected(which)
            produced, written, got = self.sweep(which)
            print(tag, "which", which, "produced", produced, "written", written, "want", want.size)
            assert produced == written == want.size, (tag, which, produced, written, want.size)
            assert np.array_equal(got.astype(U64), want), (tag, which)      # ascending, without holes
