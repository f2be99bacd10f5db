"""Case table and plain references for the resident-R radix join (hj_prj_build_dev / hj_prj_probe_dev).

No GPU and no pytest fixtures in here: test_prj_resident_cases.py checks on the CPU that the table reaches every branch it
claims to reach, test_gpu_prj_resident_edges.py runs it on the device. The expected values come from numpy alone
(reference_matches, expected_plan); the host-side planner (hj_prj_fragment_info) is only asked which layout it plans.

A case is a list of steps on ONE context: build R, probe a slice, probe an empty slice, reserve again. Every relation is
generated from a fixed seed when the case is asked for its steps, so importing this module costs nothing."""
import collections
import ctypes
import functools
import os

import numpy as np

import htm_hashjoin_amd as hj

# the three constants the join's work items depend on (hj_prj.h / hj_prj_impl.h)
ITEM_S = 1 << 16              # kPrjItemS: S tuples per work item at most
JOIN_BLOCK_TUPLES = 24576     # kJoinBlockTuples: R tuples of one hashed LDS table
COUNTER_MAX = 65535           # the DIRECT kernel's 16-bit counters (radixBits >= 16): R tuples per partition they can hold
PREFETCH = 1024 * 16          # keys of a partition the register prefetch covers (kJoinThreads x kJoinPre), over all C2 fragments

BOUNDARY_SIZES = (ITEM_S - 1, ITEM_S, ITEM_S + 1, 2 * ITEM_S, 2 * ITEM_S + 1)
BOUNDARY_ITEMS = (1, 1, 2, 2, 3)

U64 = np.uint64


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def key_counts(a):
    """(sorted distinct keys, their multiplicities) of a relation"""
    return np.unique(np.ascontiguousarray(a, dtype=U64), return_counts=True)


def reference_matches(R, S, r_counts=None):
    """Join cardinality |{(r, s): r.key == s.key}| from numpy alone: sum over the common keys of the products of their
    multiplicities, as a Python int. r_counts = key_counts(R) computed earlier (R is probed by many slices)."""
    kr, cr = key_counts(R) if r_counts is None else r_counts
    ks, cs = key_counts(S)
    if kr.size == 0 or ks.size == 0:
        return 0
    pos = np.searchsorted(kr, ks)
    pos[pos == kr.size] = kr.size - 1
    hit = kr[pos] == ks
    a, b = cr[pos[hit]].astype(U64), cs[hit].astype(U64)
    if int(a.max(initial=0)) * int(b.max(initial=0)) * a.size < 1 << 64:     # the sum of products cannot wrap in 64 bits
        return int(np.sum(a * b, dtype=U64))
    return sum(int(x) * int(y) for x, y in zip(a.tolist(), b.tolist()))


def partition_sizes(a, bits):
    """tuples per final partition: the radix join partitions on the low `bits` key bits"""
    P = 1 << bits
    return np.bincount((np.asarray(a, dtype=U64) & U64(P - 1)).astype(np.int64), minlength=P)


def expected_plan(R, S_slice, bits):
    """What one probe must report (hj_prj_resident_info) and which LDS mode each of its work items takes, from the two
    partition histograms: an item is a partition that holds R and S tuples and at most ITEM_S of its S tuples.
    cells[(mode, split)] = items of partitions in that mode whose S side is split over several items (or is not)."""
    hr, hs = partition_sizes(R, bits), partition_sizes(S_slice, bits)
    items = np.where((hr > 0) & (hs > 0), (hs + ITEM_S - 1) // ITEM_S, 0)
    direct = (hr <= COUNTER_MAX) if bits >= 16 else np.zeros(hr.size, dtype=bool)
    hashed = ~direct & (hr <= JOIN_BLOCK_TUPLES)
    cells = collections.Counter()
    for name, sel in (("direct", direct), ("hashed", hashed), ("blocks", ~direct & ~hashed)):
        for split in (False, True):
            n = int(items[sel & ((items > 1) == split)].sum())
            if n:
                cells[(name, split)] = n
    return {"items": int(items.sum()), "splitPartitions": int((items > 1).sum()),
            "maxSPartition": int(hs.max()) if hs.size else 0, "cells": cells, "sSizes": hs, "itemsPerPartition": items}


def _fragment_info(n, bits, mode):
    out = (ctypes.c_uint64 * 13)()
    assert hj.lib.hj_prj_fragment_info(n, 0, bits, mode, out) == 0
    return out


def resolved_bits(n_reserved, bits):
    """the radix bits hj_reserve settles on (bits = 0: its own pick for that |R|)"""
    out = _fragment_info(n_reserved, bits, 1)
    return int(out[11] + out[12])


Planned = collections.namedtuple("Planned", "planned C2 cap2 tail")


def planned(n, bits, mode):
    """Whether the histogram-free passes are planned for a relation of n tuples (R at the build, a slice at its probe:
    both plan the relation on its own), its fragments per partition and their capacity; tail = a fragment can hold more
    keys than the join's register prefetch covers, so the loop behind the prefetch can run."""
    out = _fragment_info(n, bits, mode)
    C1, C2, cap2 = int(out[1]), int(out[4]), int(out[5])
    if C1 == 0:
        return Planned(False, 0, 0, False)
    return Planned(True, C2, cap2, cap2 > PREFETCH // C2)


def one_shot_planned(n_r, n_s, bits, mode):
    """hj_prj_join_dev takes the histogram-free passes only when both relations qualify"""
    out = (ctypes.c_uint64 * 13)()
    assert hj.lib.hj_prj_fragment_info(n_r, n_s, bits, mode, out) == 0
    return out[0] != 0


# ---------------------------------------------------------------------------------------------------------------------
# relations (fixed seeds)
# ---------------------------------------------------------------------------------------------------------------------
def _rng(*seed):
    return np.random.default_rng([20261016, *seed])


@functools.lru_cache(maxsize=2)
def unique_shuffled(n, seed=1):
    """the keys 1..n, each once, in random order"""
    a = _rng(1, n, seed).permutation(np.arange(1, n + 1, dtype=U64))
    a.setflags(write=False)
    return a


def uniform(n, hi, *seed):
    """n draws from 1..hi"""
    return _rng(2, n, hi, *seed).integers(1, hi + 1, size=n, dtype=U64)


def const_low_bits(n, hi, c, *seed):
    """n draws from the keys (x << 8) | c, x in 1..hi: pass 1 of the histogram-free passes meets one bin and gives up"""
    return (_rng(3, n, hi, c, *seed).integers(1, hi + 1, size=n, dtype=U64) << U64(8)) | U64(c)


def hot_keys(p, bits, j_lo, count):
    """count distinct keys of partition p: p + j * 2^bits, j = j_lo .. j_lo + count - 1"""
    keys = U64(p) + (np.arange(j_lo, j_lo + count, dtype=U64) << U64(bits))
    assert int(keys[-1]) < 1 << 32
    return keys


def shuffled(parts, *seed):
    a = np.concatenate([np.asarray(x, dtype=U64) for x in parts])
    _rng(4, *seed).shuffle(a)
    return a


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
# op: "build" (arr = R, paths = allowed prjPath / rPath), "probe" (arr = slice, paths = allowed sPath),
#     "empty" (prj_probe(dS, 0)), "reserve" (hj_reserve again with the sizes of the first one: R stays resident)
Step = collections.namedtuple("Step", "op arr paths")


def build(R, paths):
    return Step("build", np.ascontiguousarray(R, dtype=U64), frozenset(paths))


def probe(S, paths):
    return Step("probe", np.ascontiguousarray(S, dtype=U64), frozenset(paths))


EMPTY = Step("empty", None, frozenset())
RESERVE = Step("reserve", None, frozenset())


class Case:
    """name, radixBits (0 = the engine's pick), prjMode, and make() -> list of steps. one_shot: R and the first slice are also joined
    through hj_run (k_prj_join). oracle_total: the CPU oracle's radix join is affordable on the concatenated slices.
    must_tail: sizes whose plan must be tail-capable -- asserted by the tests, so that a change of the fragment geometry
    cannot silently empty the case."""

    def __init__(self, name, bits, mode, make, one_shot=False, oracle_total=True, must_tail=(), memo=None):
        self.name, self.bits, self.mode, self._make = name, bits, mode, make
        self.memo = {} if memo is None else memo          # host references by step: shared by cases that differ in the mode alone
        self.one_shot, self.oracle_total, self.must_tail = one_shot, oracle_total, tuple(must_tail)

    def steps(self):
        return self._make(self)

    def once(self, key, fn):
        """fn() the first time `key` is asked for (a host reference that does not depend on the mode)"""
        if key not in self.memo:
            self.memo[key] = fn()
        return self.memo[key]

    def __repr__(self):
        return f"Case({self.name}, bits={self.bits}, mode={self.mode})"

    def path(self, n, ok):
        """allowed path of a relation of n tuples: 0 when the histogram-free passes are not planned, else `ok`"""
        bits = self.bits if self.bits else 14          # the engine's pick below 2^28 tuples
        return (0,) if not planned(n, bits, self.mode).planned else ok


def reserve_sizes(steps):
    """(rSize, sSize) of the case's hj_reserve: the largest R and the largest slice of its steps"""
    return (max(s.arr.size for s in steps if s.op == "build"), max(s.arr.size for s in steps if s.op == "probe"))


def _frag_tail(c):
    n = 1 << (14 + c.bits)                          # bits 9: 2^23, bits 10: 2^24 -- 1024 keys per fragment on average
    R = unique_shuffled(n)
    S = uniform(n + n // 2, n + n // 8, 10)         # an eighth of the domain is absent from R
    return [build(R, c.path(n, (1,))), probe(S[:n], c.path(n, (1,))), probe(S[n:], c.path(n // 2, (1,)))]


def _c2_sweep(log2n):
    def make(c):
        n = 1 << log2n
        R = unique_shuffled(n)
        S = uniform(n + 4321, n + n // 4, 11, c.bits)
        cut = n // 3
        return [build(R, c.path(n, (1,))), probe(S[:cut], c.path(cut, (1,))), probe(S[cut:], c.path(S.size - cut, (1,)))]
    return make


def _hot_partition(reps):
    """2^20 dense keys and one R partition of 40000 distinct keys, each `reps` times; the first slice puts 3 * 2^16 + 1
    draws from those keys into that partition (4 work items, the last one short), the second slice next to none.
    bits 16: the hot keys reach up to 65535 * 2^16 + p, so that key >> 16 uses the last of the direct counters."""
    def make(c):
        p, n = 777, 1 << 20
        hot = hot_keys(p, c.bits, (1 << (32 - c.bits)) - 40000, 40000)
        R = shuffled([np.arange(1, n + 1, dtype=U64)] + [hot] * reps, 20, c.bits, reps)
        S1 = shuffled([uniform(n, n + n // 4, 21, c.bits), hot[_rng(22, c.bits).integers(0, hot.size, size=3 * ITEM_S + 1)]], 23, c.bits)
        S2 = shuffled([uniform(n // 2, n, 24, c.bits), hot[-3:], hot[:2]], 25, c.bits)
        return [build(R, (0,)), probe(S1, (0,)), probe(S2, (0,))]
    return make


def _boundaries(c):
    """Five partitions whose S side holds exactly 2^16 - 1, 2^16, 2^16 + 1, 2^17, 2^17 + 1 tuples (1, 1, 2, 2, 3 items),
    drawn from 300 keys each that R holds; every other S tuple falls into another partition."""
    n, P = 1 << 20, 1 << c.bits
    parts = boundary_partitions(c.bits)
    hots = [hot_keys(p, c.bits, 64, 300) for p in parts]
    R = shuffled([np.arange(1, n + 1, dtype=U64)] + hots, 30, c.bits)
    rest = uniform(n, n + n // 4, 31, c.bits)
    rest = rest[~np.isin(rest & U64(P - 1), np.array(parts, dtype=U64))]
    rng = _rng(32, c.bits)
    S = shuffled([rest] + [h[rng.integers(0, h.size, size=m)] for h, m in zip(hots, BOUNDARY_SIZES)], 33, c.bits)
    return [build(R, (0,)), probe(S, (0,))]


def boundary_partitions(bits):
    return [(1 << bits) - 1, 0, 4097, 12345, 1 << (bits - 1)]


def _sparse(nr):
    """Few R tuples (most partitions hold none), none of them with key & 15 == 5; slices with keys absent from R, a slice
    of one tuple, an empty probe, a slice that falls into the partitions without R only (no work item at all)."""
    def make(c):
        dom = 1 << 24
        rng = _rng(40, nr)
        R = np.unique(rng.integers(1, dom, size=2 * nr, dtype=U64))
        rng.shuffle(R)
        R = R[:nr]
        assert R.size == nr
        R = np.where((R & U64(15)) == U64(5), R + U64(1), R)                 # may repeat a key: fine
        rng = _rng(41, nr, c.bits)
        S1 = shuffled([R[rng.integers(0, nr, size=30000)], uniform(30001, dom, 42, nr)], 43, nr)
        nowhere = (uniform(20000, dom >> 4, 44, nr) << U64(4)) | U64(5)      # partitions p with p & 15 == 5: no R tuple
        S3 = shuffled([R[rng.integers(0, nr, size=777)], nowhere[:999]], 45, nr)
        return [build(R, (0,)), probe(S1, (0,)), probe(R[7:8], (0,)), EMPTY, probe(nowhere, (0,)), probe(S3, (0,)),
                probe(uniform(1, dom, 46, nr), (0,))]
    return make


def _narrow(log2n):
    """single-pass radix widths (<= 8) and 11: R with duplicates, at 4 bits several LDS blocks per R partition"""
    def make(c):
        n = 1 << log2n
        R = uniform(n, n // 2, 50, c.bits)
        S = uniform(n + n // 2 + 17, n // 2 + n // 8, 51, c.bits)
        return [build(R, c.path(n, (1,))), probe(S[:n], c.path(n, (1,))), probe(S[n:], c.path(S.size - n, (1,)))]
    return make


def _mixed(r_falls_back):
    """slices that take the three S paths in turn against an R that keeps the histogram-free layout (or falls back itself)"""
    def make(c):
        n, low = 1 << 23, 0x5A
        if r_falls_back:
            R = (unique_shuffled(n) << U64(8)) | U64(low)                   # low 8 bits constant: pass 1 gives up
        else:
            R = unique_shuffled(n)
        hi = n >> 8 if not r_falls_back else n
        return [build(R, (2,) if r_falls_back else (1,)),
                probe(uniform(n, n, 60), c.path(n, (1,))),
                probe(const_low_bits(n // 2, hi, low, 61), c.path(n // 2, (2,))),
                probe(R[1000:1000 + (1 << 18)] if r_falls_back else uniform(1 << 18, n + n // 2, 62), c.path(1 << 18, (1,))),
                probe(uniform(n // 2, n, 63), c.path(n // 2, (1,)))]
    return make


def _regrow(c):
    """R too small for the histogram-free passes, reserved for slices that get them: the first probe's plan holds
    fragment counters the reserved workspace has no room for, so hj_prj_probe_dev replaces the workspace. A later
    hj_reserve with the same sizes reallocates nothing, so R stays resident (htm_hashjoin.h: only an hj_reserve that
    reallocated drops it)."""
    n, big = 1 << 20, 1 << 23
    R = unique_shuffled(n)
    return [build(R, c.path(n, (1,))), probe(uniform(big, 2 * n, 70), c.path(big, (1,))), probe(uniform(1000, 2 * n, 71), (0,)),
            RESERVE, probe(uniform(big // 2, 2 * n, 72), c.path(big // 2, (1,))), probe(uniform(big, 3 * n, 73), c.path(big, (1,)))]


def _rebuild(c):
    """one context: an R of the histogram-free layout, an R of the exact passes with an oversized partition, the first
    one again -- every build over what the previous one left in the resident offsets and fragment counters"""
    n1, n2 = 1 << 23, 1 << 20
    R1 = unique_shuffled(n1)
    hot = hot_keys(777, c.bits, 64, 40000)
    R2 = shuffled([np.arange(1, n2 + 1, dtype=U64), hot], 80)
    S2 = shuffled([uniform(n2, 2 * n2, 81), hot[_rng(82).integers(0, hot.size, size=2 * ITEM_S + 5)]], 83)
    return [build(R1, c.path(n1, (1,))), probe(uniform(n1 // 2, n1 + n1 // 4, 84), c.path(n1 // 2, (1,))),
            build(R2, c.path(R2.size, (1,))), probe(S2, c.path(S2.size, (1,))), probe(uniform(n1, n1, 85), c.path(n1, (1,))),
            build(R1, c.path(n1, (1,))), probe(uniform(n1, n1 + n1 // 4, 86), c.path(n1, (1,)))]


# The fragment-with-a-tail geometry also exists at 10 bits and 2^24 tuples; the table leaves it at the smallest size.
CASES = [
    Case("frag-tail-b9", 9, 2, _frag_tail, one_shot=True, must_tail=(1 << 23,)),
    Case("frag-c2-4-b11", 11, 2, _c2_sweep(21)),
    Case("frag-c2-8-b11", 11, 2, _c2_sweep(22)),
    Case("frag-c2-16-b11", 11, 2, _c2_sweep(23)),
    Case("frag-c2-1-b15", 15, 2, _c2_sweep(23)),
    Case("blocks-split-hashed-m0", 14, 0, _hot_partition(1), oracle_total=False),
    Case("blocks-split-hashed-m1", 14, 1, _hot_partition(1), oracle_total=False),
    Case("direct-large-partition", 16, 1, _hot_partition(1), oracle_total=False),
    Case("direct-kernel-blocks", 16, 1, _hot_partition(2), oracle_total=False),
    Case("boundaries-b14", 14, 1, _boundaries, oracle_total=False),
    Case("boundaries-b16", 16, 1, _boundaries, oracle_total=False),
    Case("sparse-1000-b14", 14, 2, _sparse(1000)),
    Case("sparse-1000-b16", 16, 0, _sparse(1000)),
    Case("sparse-1000-auto", 0, 1, _sparse(1000)),
    Case("sparse-70001-b14", 14, 0, _sparse(70001)),
    Case("sparse-70001-b16", 16, 2, _sparse(70001)),
    Case("sparse-70001-auto", 0, 2, _sparse(70001)),
    Case("narrow-b4", 4, 1, _narrow(20)),
    Case("narrow-b8", 8, 2, _narrow(19)),
    Case("narrow-b11", 11, 2, _narrow(20)),
    Case("mixed-paths-r-frag", 14, 2, _mixed(False)),
    Case("mixed-paths-r-fallback", 14, 2, _mixed(True)),
    Case("workspace-regrow", 14, 2, _regrow),
    Case("rebuild", 14, 2, _rebuild, oracle_total=False),
]
CASE_IDS = [c.name for c in CASES]


# ---------------------------------------------------------------------------------------------------------------------
# seeded random cases
# ---------------------------------------------------------------------------------------------------------------------
FUZZ_BLOCKS = 4
FUZZ_BITS = (0, 4, 8, 9, 11, 12, 14, 16)
FUZZ_SHAPES = ("dense", "31-bit", "const-low-bits", "const-middle-bits", "repeated")


def fuzz_case_count():
    """HJ_FUZZ_CASES as in test_gpu_fuzz.py: the number of random cases (default 36); every case runs the three modes"""
    return int(os.environ.get("HJ_FUZZ_CASES", "36"))


def ragged(rng, n, k):
    """k >= 1 slice lengths >= 1 that add up to n, at random"""
    k = min(k, n)
    cuts = np.sort(rng.choice(np.arange(1, n), size=k - 1, replace=False)) if k > 1 else np.array([], dtype=np.int64)
    return [int(x) for x in np.diff(np.concatenate([[0], cuts, [n]]))]


def random_relations(block, index):
    """(R, S, slice lengths, bits, shape) of random case `index` of `block`: |R| in [2^10, 2^21) of any size, 1..7 slices
    of ragged lengths, the key domains of test_radix_join_on_random_relations"""
    rng = np.random.default_rng([20265000, block, index])
    nr = int(rng.integers(1 << 10, 1 << 21))
    ns = int(rng.integers(1 << 10, 1 << 21))
    shape = FUZZ_SHAPES[int(rng.integers(0, len(FUZZ_SHAPES)))]
    if shape == "dense":
        hi = max(nr, ns)
        R = rng.integers(1, hi + 1, size=nr, dtype=U64); S = rng.integers(1, hi + 1, size=ns, dtype=U64)
    elif shape == "31-bit":                          # few matches but those S tuples that are copies of R's
        R = rng.integers(1, 1 << 31, size=nr, dtype=U64)
        S = np.concatenate([R[: min(nr, ns) // 2], rng.integers(1, 1 << 31, size=ns - min(nr, ns) // 2, dtype=U64)])
        rng.shuffle(S)
    elif shape == "const-low-bits":                  # one pass-1 bin takes everything
        low = U64(int(rng.integers(0, 256)))
        R = (rng.integers(1, 1 << 20, size=nr, dtype=U64) << U64(8)) | low; S = (rng.integers(1, 1 << 20, size=ns, dtype=U64) << U64(8)) | low
    elif shape == "const-middle-bits":               # bits 8..15 are zero: pass 2 cannot spread a partition
        R = (rng.integers(1, 1 << 12, size=nr, dtype=U64) << U64(16)) | rng.integers(0, 256, size=nr, dtype=U64)
        S = (rng.integers(1, 1 << 12, size=ns, dtype=U64) << U64(16)) | rng.integers(0, 256, size=ns, dtype=U64)
    else:                                            # repeated keys, ~2 ... 64 tuples per key
        d = int(rng.integers(max(nr, ns) // 64 + 1, max(nr, ns)))
        R = rng.integers(1, d + 1, size=nr, dtype=U64); S = rng.integers(1, d + 1, size=ns, dtype=U64)
    bits = int(rng.choice(FUZZ_BITS))
    lens = ragged(rng, ns, int(rng.integers(1, 8)))
    return np.ascontiguousarray(R), np.ascontiguousarray(S), lens, bits, shape


def random_cases(block):
    """the random cases of one block: indices block, block + FUZZ_BLOCKS, ... below HJ_FUZZ_CASES, each in modes 0, 1, 2"""
    for index in range(block, fuzz_case_count(), FUZZ_BLOCKS):
        R, S, lens, bits, shape = random_relations(block, index)
        # a relation of independent draws keeps the histogram-free layout (a fragment holds its mean + 7 sigma); constant
        # key bits inside the radix overflow a fragment in pass 1 (low bits) or pass 2 (middle bits)
        ok = (2,) if shape.startswith("const") else (1,)
        memo = {}
        for mode in (0, 1, 2):
            def make(c, R=R, S=S, lens=lens, ok=ok):
                steps, off = [build(R, c.path(R.size, ok))], 0
                for m in lens:
                    steps.append(probe(S[off:off + m], c.path(m, ok)))
                    off += m
                return steps
            yield Case(f"random-{block}-{index}-{shape}-n{R.size}-b{bits}-m{mode}", bits, mode, make,
                       oracle_total=shape in ("dense", "31-bit"), memo=memo)
