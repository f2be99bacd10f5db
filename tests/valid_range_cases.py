"""Relations for the valid-slot-range tests (test_valid_range_cases.py on the CPU, test_gpu_valid_range.py on the device).

An LDS build writes only the slots [validLo, validHiEx + 512) of the table (hj_common.h, Counters); everything else keeps
what an earlier build on the same context left there. The builders here put a relation R on a chosen BAND of home slots,
a POISON relation on every other slot of the same table, and a probe side that asks for every poison key and for keys homed
right at the edges of the range the device reported. What R alone joins to -- the sequential oracle's answer -- is then what
every reader of the table must give, whatever lies outside the range.

Two table geometries share the slot numbering (8-byte slots of one table buffer):
  open addressing   home = (key >> shift) & (table - 1), table = 2 * n
  bucketised (htm)  home = 4 * ((key / 3) & (table / 4 - 1)), table = 4 * nextpow2(n / 3 + 1)   (= 2 * n for n = 2^16, 2^18)
Fixed seed, plain numpy, no device. No test in here."""
from collections import namedtuple

import numpy as np

from oracle import oracle

U64 = np.uint64
SEED = 20270131
BLOCK = 512                     # the granularity of the range (set_valid_range: 512 slots of defined contents behind it)
# the room the fixed placements leave between the band and the table's edges, far more than any build's rounding takes
MARGIN = 8 * BLOCK
REACH_UP = 2 * BLOCK            # how far above the last slot a tuple can land on validHiEx may lie at most (classify)

Band = namedtuple("Band", "R twins n table a copies shift htm lo hi_ex period")


def htm_table(n):
    nb = 1
    while nb < n // 3 + 1:
        nb *= 2
    return 4 * nb


def homes(keys, table, shift=0, htm=False):
    keys = np.asarray(keys, dtype=U64) & U64(0xFFFFFFFF)
    if htm:
        return ((keys // U64(3)) << U64(2)) & U64(table - 1)
    return (keys >> U64(shift)) & U64(table - 1)


def band_relation(n, table, a, copies=1, shuffle=0, high_bits=True, shift=0, htm=False, seed=SEED):
    """n tuples whose home slots are the band [lo, hi_ex) (hi_ex > table: the band wraps past the table's end).
    Open addressing: lo = a, one key per slot, each `copies` times, adjacent: hi_ex = a + n / copies.
    htm: keys from 3 * (a / 4) on (from 1 for a < 4), each `copies` times: the buckets from slot a & ~3 on, three keys each.
    shuffle: a local shuffle of that width. high_bits: one tuple in 16 gets key + j * period, j = 1..3 -- the same home
    slot, another key; `twins` are keys + 4 * period of one tuple in 8: they share a home with a member and are no member.
    shift: the home shift of a radix shard (hj_build_keys_dev); the low bits are random."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=U64) // U64(copies)
    span = n // copies
    if htm:
        assert shift == 0 and table == htm_table(n)
        k0 = max(1, 3 * (a >> 2))
        keys = U64(k0) + i
        period = 3 * (table // 4)
        lo, hi_ex = 4 * (k0 // 3), 4 * ((k0 + span - 1) // 3) + 4
    else:
        assert a >= 1
        keys = (U64(a) + i) << U64(shift)
        if shift:
            keys |= rng.integers(0, 1 << shift, size=n, dtype=U64)
        period = table << shift
        lo, hi_ex = a, a + span
    assert hi_ex - lo <= table
    twins = keys[rng.random(n) < 1 / 8] + U64(4 * period)
    if high_bits:
        j = np.where(rng.random(n) < 1 / 16, rng.integers(1, 4, size=n), 0).astype(U64)
        keys = keys + j * U64(period)
    if shuffle > 1:
        keys = keys[np.argsort(np.arange(n) + rng.uniform(0, shuffle, size=n), kind="stable")]
    assert int(keys.max()) < 0xFFFFFFFF and int(twins.max()) < 0xFFFFFFFF
    return Band(np.ascontiguousarray(keys), np.ascontiguousarray(twins), n, table, a, copies, shift, htm, lo, hi_ex, period)


def outside_slots(band):
    """the slots of the table outside the band, from its top on, wrapping past the table's end"""
    return (np.arange(band.hi_ex, band.lo + band.table, dtype=np.int64)) % band.table


def poison_for(band, order="perm", htm=None, chains=True, seed=SEED + 1):
    """Unique keys (none a member of the band's relation or one of its twins), one homed on every slot outside the band --
    htm: one in every bucket that lies wholly outside it -- wrapping past the table's end. order "perm": a random
    permutation (no locality: global atomics, packed slots); "sorted": by home slot (the rings).
    htm (default: the band's own geometry): the geometry the POISON is built in; both share the table buffer.
    chains (htm poison): as many keys as the table size allows are there FIVE times, so that their buckets overflow and
    slot 3 of those buckets links into the overflow area."""
    htm = band.htm if htm is None else htm
    T = band.table
    if htm:
        nb = T // 4
        first, last = -(-band.hi_ex // 4), (band.lo + T) // 4          # buckets wholly outside, unwrapped
        b = np.arange(first, last, dtype=np.int64) % nb
        keys = (3 * b + 3 * nb + (np.arange(b.size) % 3)).astype(U64)
        if chains:
            # the poison must size the same table: nextpow2(count / 3 + 1) == nb, i.e. count <= 3 * nb - 3
            fives = max(0, min(b.size, (3 * nb - 3 - b.size) // 4))
            keys = np.concatenate([np.repeat(keys[:fives], 5), keys[fives:]])
            assert htm_table(keys.size) == T, (keys.size, T)
    else:
        shift = band.shift if not band.htm else 0
        s = outside_slots(band)
        keys = ((s + T).astype(U64)) << U64(shift)
    if order == "perm":
        keys = np.random.default_rng(seed).permutation(keys)
    else:
        assert order == "sorted"
        keys = np.sort(keys, kind="stable")
    return np.ascontiguousarray(keys)


def edge_slots(lo, hi_ex, table):
    """the slots around the reported range whose keys the probe side asks for, where they lie inside the table"""
    want = (lo - 1, lo, hi_ex - 1, hi_ex, hi_ex + BLOCK - 1, hi_ex + BLOCK, hi_ex + BLOCK + 1)
    return [s for s in want if 0 <= s < table]


def keys_homed_at(band, slots):
    """member-or-not keys with these home slots: the plain key of the slot, and one with high bits no relation uses"""
    out = []
    for s in slots:
        if band.htm:
            base = [3 * (s >> 2) + k for k in range(3)]
        else:
            base = [s << band.shift]
        out += [k for k in base if k] + [k + 5 * band.period for k in base]
    return np.array(out, dtype=U64)


def probe_side(band, P, lo, hi_ex, key32=False):
    """All of R and all of P (every stale key is asked for), keys homed at the edges of the reported range [lo, hi_ex),
    the high-bit twins and -- for 8-byte probe tuples -- a few tuples outside the DataGen layout (payload bits, zero)."""
    parts = [band.R, np.asarray(P, dtype=U64), keys_homed_at(band, edge_slots(lo, hi_ex, band.table)), band.twins]
    if not key32:
        parts.append(np.concatenate([band.R[:5] | U64(1 << 32), np.asarray(P[:5], dtype=U64) | U64(7 << 32), np.zeros(2, dtype=U64)]))
    return np.ascontiguousarray(np.concatenate(parts))


def expected(band, S, probe_length=4):
    """the sequential oracle on R ALONE: counters and the table (htm: the buckets and their chains)"""
    if band.htm:
        return oracle.htm_build_probe_seq(band.R, S, want_buckets=True)
    if band.shift or band.n * 2 != band.table:
        return oracle.build_probe_seq_ts(band.R, S, band.table, band.shift, probe_length, want_table=True)
    return oracle.build_probe_seq(band.R, S, probe_length, want_table=True)


def classify(band, probe_length=4):
    """What the band's place says about the range a build must report, by arithmetic alone:
    "whole"    the home slots reach the table's last block (or wrap): set_valid_range makes the whole table valid
    "interior" 0 < validLo and validHiEx + 512 < table must both hold
    "control"  the band starts in block 0 (today's relations: keys from 1), the top is interior: validLo = 0
    "device"   neither: that close to an edge the build's own rounding decides
    The upper side is sharp. Every home slot of R is probed, so validHiEx >= hi_ex, and hi_ex + 512 >= table forces the
    whole table. And no build reaches further than REACH_UP above `top`, one past the last slot a tuple of R can land on
    (hi_ex + probeLength - 1; htm: hi_ex): the window build declares the blocks up to the last one touched + 1 probed
    (k_finalize_range: validHiEx = (block + 2) * 512 <= top - 1 + 1024), the deferred phases of the rings the same, and the
    rings own up to one ring (8 granules = 1024 slots) from the granule their window stands on, which the last home slot
    is not below (k_build_wave: ownHiEx = (winLoG + 8) * 128 <= top - 1 + 1024). So top + REACH_UP + 512 <= table forces an
    interior top. The lower side keeps MARGIN: where the rings' pre-pass puts the first seam is its own business."""
    T = band.table
    if band.hi_ex + BLOCK >= T:
        return "whole"
    top = band.hi_ex + (0 if band.htm else probe_length - 1)
    if top + REACH_UP + BLOCK > T:
        return "device"
    if band.lo >= MARGIN:
        return "interior"
    return "control" if band.lo < BLOCK else "device"


# ---- the placements every path is run on: name -> (a, copies) for a table of T slots ------------------------------------
def placements(T):
    return {
        "control": (1, 1),                          # keys from 1: validLo = 0
        "mid": (T // 4, 1),                         # table / 2 inside the band
        "below": (MARGIN, 2),                       # wholly below table / 2: tableSumHalf == tableSumFull
        "above": (T // 2 + MARGIN, 2),              # wholly above: tableSumHalf == 0
        "straddle": (T - T // 4, 1),                # the tuples wrap past the table's end: whole
    }


def band_slots(n, copies=1, htm=False):
    """slots between the first and the last home slot of a band of n tuples (htm: to within a bucket)"""
    span = n // copies
    return 4 * -(-span // 3) if htm else span


def top_sweep(T, slots):
    """where a band of that many slots starts so that its top lies in each of the last six blocks of the table, lowest first"""
    return [T - k * BLOCK + 40 - slots for k in range(6, 0, -1)]


def bottom_sweep():
    """band bottoms in blocks 0 to 3"""
    return [k * BLOCK + 5 for k in range(4)]
