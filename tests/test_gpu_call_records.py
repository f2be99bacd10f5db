"""What the five *_info calls remember, and for how long (hj_pairs_info, hj_r_rows_info, hj_gather_info, hj_verify_info,
hj_mark_rows_info), through ctypes -> C ABI on an MI355X. One context per table kind, reserved with HJ_FLAG_KEEP_ROW_IDS |
HJ_FLAG_TRACK_R_MATCHES; |R| = 1024 unique keys, |S| = 1500. One call of each of the five kinds with a capacity below what
it finds, then a second build, then an hj_reserve that replaces the marks plane:

    record      a new build                                  hj_reserve replacing the plane
    pairs       words 0, 1, 3 stay; the time (word 2) is 0   --
    R rows      (0, 0, 0, rows of the build)                 HJ_ERR_STATE, as hj_r_rows_dev
    gather      stays                                        stays
    verify      stays                                        stays
    mark rows   stays                                        stays

Every expected word comes from numpy (join_kinds_common.derive, r_marks_common.inner_expected). Run with -m gpu."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib

from gpu_harness import Device, plane_bits, status
from r_marks_common import U64, LOW, INNER, LEFT, SEMI, ANTI, UNMATCHED, MATCHED, inner_expected, r_rows_of
from join_kinds_common import derive, matched_rows, planes

pytestmark = pytest.mark.gpu

N_R, N_S, BITS = 1024, 1500, 5
N_R_LARGER = 1 << 16                 # its marks plane (8 KiB) does not fit the one reserved for 1024 rows (128 bytes)
NO_ROW = np.uint32(0xFFFFFFFF)
PAIRS_CAP, R_ROWS_CAP, VERIFY_CAP, MARK_CAP = 100, 10, 50, 5


def relations():
    """R: the keys 1 .. 1024 shuffled (in a table of 2048 slots every key sits in its home slot); S: 1500 draws from
    1 .. 2048, so about half of S and of R go without a partner"""
    rng = np.random.default_rng(31)
    R = rng.permutation(np.arange(1, N_R + 1, dtype=U64))
    S = rng.integers(1, 2 * N_R + 1, N_S).astype(U64)
    return R, S


def bits_set(words, rows):
    return int(plane_bits(words, rows).sum())


class Scenario:
    """the calls of one context and what their info vectors must hold (time words apart)"""

    def __init__(self, ctx, dev, algo, kind):
        self.ctx, self.dev, self.algo, self.kind = ctx, dev, algo, kind
        self.prj = algo == "prj"
        self.R, self.S = relations()
        self.inner = inner_expected(algo, self.R, self.S)
        self.dR, self.dS = dev.put(self.R), dev.put(self.S)

    def reserve(self, r_size):
        self.ctx.reserve(self.algo, r_size, N_S, radixBits=BITS if self.prj else 0, keepRowIds=True, trackRMatches=True)

    def build(self):
        (self.ctx.prj_build if self.prj else self.ctx.build)(self.dR, N_R)

    def probe_pairs(self, kind, d_s, d_r, cap):
        (self.ctx.prj_probe_pairs if self.prj else self.ctx.probe_pairs)(self.dS, N_S, d_s, d_r, cap, 0, kind=kind)

    def pairs(self):
        """an INNER call that only counts (it marks R rows all the same), then the call of `kind` cut by its capacity"""
        self.probe_pairs(INNER, 0, 0, 0)
        d_s, d_r = (p.ptr for p in planes(self.dev, PAIRS_CAP))
        self.probe_pairs(self.kind, d_s, d_r, PAIRS_CAP)
        found = derive(self.kind, self.inner, N_S).size
        assert found > PAIRS_CAP
        return found, PAIRS_CAP, 0 if self.kind == INNER else N_S - matched_rows(self.inner).size

    def r_rows(self):
        d = self.dev.alloc(4 * R_ROWS_CAP)
        self.ctx.r_rows(UNMATCHED, d, R_ROWS_CAP)
        lone = N_R - r_rows_of(self.inner).size
        assert lone > R_ROWS_CAP
        return lone, R_ROWS_CAP, N_R

    def gather(self):
        rng = np.random.default_rng(32)
        n = 300
        m = rng.integers(0, N_R, n).astype(np.uint32)
        m[3::11] = N_R + 7                                        # out of range
        m[::7] = NO_ROW
        d_dst = self.dev.alloc(8 * n)
        self.ctx.gather(self.dev.put(m), n, N_R, [(self.dR, d_dst, 8, 0)])
        nulls, stray = int((m == NO_ROW).sum()), int(((m != NO_ROW) & (m >= N_R)).sum())
        assert nulls and stray
        return n, nulls, stray

    def verify(self):
        """the relations as one 8-byte key column: the inner pairs of the key word are kept, each of them once more with the
        R row behind (another key: R's are unique) is rejected, and twelve candidates are dropped unread"""
        s, r = (self.inner >> U64(32)).astype(np.uint32), (self.inner & LOW).astype(np.uint32)
        assert np.array_equal(self.S[s], self.R[r])
        map_s = np.concatenate([s, s, np.full(7, NO_ROW), np.zeros(5, dtype=np.uint32)])
        map_r = np.concatenate([r, (r + 1) % N_R, np.zeros(7, dtype=np.uint32), np.full(5, 5000, dtype=np.uint32)])
        d_s, d_r = (p.ptr for p in planes(self.dev, VERIFY_CAP))
        self.ctx.pairs_verify(self.dev.put(map_s), self.dev.put(map_r), map_s.size, 0, N_S, N_R, [(self.dS, self.dR, 8)], d_s, d_r,
                              VERIFY_CAP)
        assert self.inner.size > VERIFY_CAP
        return self.inner.size, VERIFY_CAP, 12

    def mark_rows(self):
        rows = 777
        words = np.random.default_rng(33).integers(0, 1 << 32, (rows + 31) // 32 + 8).astype(np.uint32)
        self.ctx.mark_rows(self.dev.put(words), rows, 40, MATCHED, self.dev.alloc(4 * MARK_CAP), MARK_CAP)
        produced = bits_set(words, rows)
        assert produced > MARK_CAP
        return produced, MARK_CAP, rows

    def infos(self):
        c = self.ctx
        return {"pairs": c.pairs_info(), "gather": c.gather_info(), "verify": c.verify_info(), "mark_rows": c.mark_rows_info()}


def words013(info):
    return info[0], info[1], info[3]


def lifetimes(algo, kind, counting_probe=False):
    with hj.HashJoinContext(0) as ctx, Device(ctx) as dev:
        sc = Scenario(ctx, dev, algo, kind)
        # 1. nothing has been called
        for name in ("gather_info", "verify_info", "mark_rows_info"):
            assert getattr(ctx, name)() == (0, 0, 0, 0), name
        # 2. build, one call of each kind, every capacity below what the call finds
        sc.reserve(N_R)
        sc.build()
        want = {"pairs": sc.pairs()}
        if counting_probe:
            # the counting probe of a rows context runs the pairs join with a cursor of its own: no pairs call
            before = ctx.pairs_info()
            ctx.prj_probe(sc.dS, N_S)
            assert ctx.pairs_info() == before
        want["r_rows"] = sc.r_rows()
        want["gather"], want["verify"], want["mark_rows"] = sc.gather(), sc.verify(), sc.mark_rows()
        first = sc.infos()
        first["r_rows"] = ctx.r_rows_info()
        print(algo, "want", want, "got", first)
        for name, info in first.items():
            assert words013(info) == want[name], (name, info, want[name])
        # 3. a second build on the same context
        sc.build()
        second = sc.infos()
        print(algo, "after the second build", second, ctx.r_rows_info())
        for name in ("gather", "verify", "mark_rows"):
            assert words013(second[name]) == want[name] and second[name][2] != 0, (name, second[name])
        assert ctx.r_rows_info() == (0, 0, 0, N_R)
        assert words013(second["pairs"]) == want["pairs"] and second["pairs"][2] == 0, second["pairs"]
        # 4. a reserve that replaces the marks plane: the marks describe no build any more
        sc.reserve(N_R_LARGER)
        assert status(ctx.r_rows, UNMATCHED, 0, 0) == _lib.HJ_ERR_STATE
        assert status(ctx.r_rows_info) == _lib.HJ_ERR_STATE
        third = sc.infos()
        for name in ("gather", "verify", "mark_rows"):
            assert words013(third[name]) == want[name] and third[name][2] != 0, (name, third[name])


def test_atomic_context():
    lifetimes("atomic", LEFT)


def test_htm_context():
    lifetimes("htm", SEMI)


def test_prj_resident_context():
    lifetimes("prj", ANTI, counting_probe=True)
