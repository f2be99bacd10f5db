"""Case table and plain references for the seams of the ring builds (buildVariant 3 and 4, hj_build_wave.hip).

No GPU and no pytest fixtures in here: test_wave_cases.py checks on the CPU that every constructor produces the property it
is named for, test_gpu_wave_seams.py runs the table on the device. What a build must give comes from the sequential oracle;
where its seams must lie comes from expected_seams, a numpy restatement of the pre-pass (k_wave_seams, k_wave_bounds_scan)
written from the rules in the kernels' comments. The zone widths are never written down here: they come from
hj_wave_layout_info, which reports the kernel's own constants.

A relation is described by its HOME SLOTS (an int64 array, one per position): relation(homes, shift) turns them into keys
with home = (key >> shift) & (tableSize - 1). A case names its seam by the chunk number c, the nominal seam p = c * chunkLen,
the seam's position q = starts[c] and the first slot of chunk c's range, L = bounds[c] * granule.

Three bases, all sorted, all such that the compact build holds on them:
  dense   homes 1 .. n: every slot taken -- a walk that is displaced by one slot displaces every later tuple up to the
          relation's end, so the displacement enters the shadow granule of the NEXT seam from below, where nobody simulates
          it: bit 4 there, by design (case R). The base of the cases without a walk (E, F, G).
  gapped  homes 1, 2, ... without the slots = 16 (mod 32): dense enough that the 960 positions before a seam span less than
          a ring (so a tuple homed at L - 1 placed q - shadow - 1 positions early still sits in the previous wavefront's ring,
          case B), with a free slot every 32 to end a displacement well inside the chunk.
  odd     homes 1, 3, ..., 2n - 1: the whole table at 64 tuples per granule, a free slot next to every tuple. A tile spans
          exactly one ring there, and chunk 0 (which has no shadow zone) cuts its tiles 64 positions before the others do:
          copies of the key homed at L - 1 that sit before the NOMINAL seam 1 are outside its ring (bit 0), which is why
          case A runs on this base at the middle and the last seam only.
"""
import collections

import numpy as np

import htm_hashjoin_amd as hj

U64 = np.uint64
I64 = np.int64

# hj_result.compactFallback
BIT_OUTSIDE, BIT_CROSSERS, BIT_EMPTY_PATTERN, BIT_BELOW, BIT_SEAM = 1, 2, 4, 8, 16

SAMPLE = 64             # tuples from the nominal seam whose lowest home slot names the seam's granule: one per lane of a wavefront


def layout(n, compute_units):
    """hj_wave_layout_info without a device: chunk geometry for n tuples + the kernel's zone constants"""
    return hj.wave_layout_info(n, compute_units)


# ---------------------------------------------------------------------------------------------------------------------
# relations
# ---------------------------------------------------------------------------------------------------------------------
def relation(homes, shift=0):
    """keys whose home slot is homes[i]: home << shift | (all ones below the shift), so that no key is 0"""
    return (np.asarray(homes, dtype=I64).astype(U64) << U64(shift)) | U64((1 << shift) - 1)


def homes_of(rel, table_size, shift=0, htm=False):
    """home slot per tuple (int64) and which tuples are valid (upper word 0, not 0). htm: the bucketised table's home, the
    first of the four slots of bucket (key / 3) & (table_size / 4 - 1)"""
    rel = np.asarray(rel, dtype=U64)
    valid = ((rel >> U64(32)) == 0) & (rel != 0)
    if htm:
        return ((((rel & U64(0xFFFFFFFF)) // U64(3)) << U64(2)) & U64(table_size - 1)).astype(I64), valid
    return (((rel & U64(0xFFFFFFFF)) >> U64(shift)) & U64(table_size - 1)).astype(I64), valid


def base_dense(n):
    return np.arange(1, n + 1, dtype=I64)


def base_odd(n):
    return 2 * np.arange(n, dtype=I64) + 1


def base_gapped(n):
    s = np.arange(1, 2 * n, dtype=I64)
    return s[s % 32 != 16][:n]


BASES = {"dense": base_dense, "gapped": base_gapped, "odd": base_odd}


# ---------------------------------------------------------------------------------------------------------------------
# the pre-pass, restated
# ---------------------------------------------------------------------------------------------------------------------
def expected_seams(rel, lay, table_size, home_shift=0, htm=False):
    """(starts[nChunks + 1], bounds[nChunks + 1]) as int64, from the rules of k_wave_seams and k_wave_bounds_scan:
      * nominal seam p = c * chunkLen; m = the lowest valid home slot among the SAMPLE tuples from p;
      * chunk c > 0 starts at the first position in [p, p + look) whose (valid) home slot lies at or beyond the first slot
        of the granule after m's, and its range starts at that granule; without such a position (or when that slot is
        2^32, which wraps to 0) it starts at p, in m's granule; chunk 0 starts at 0 in m's granule;
      * a chunk c > 0 with fewer than `look` positions left (p + look > n) starts at n and owns the table from the granule
        after the highest valid home slot among those positions;
      * bounds = prefix maximum of those granules over the chunks that had a valid tuple in their sample; a chunk without
        one inherits, chunks before the first one take the first one's (0 if there is none); never above the table's
        granules; bounds[nChunks] = granules of the table, starts[nChunks] = n.
    htm: the same rules on the bucketised table's home slots (table_size = 4 slots per bucket)."""
    home, valid = homes_of(rel, table_size, home_shift, htm)
    n = home.size
    gran, look, chunk_len, n_chunks = lay["granuleSlots"], lay["look"], lay["chunkLen"], lay["nChunks"]
    assert n_chunks == -(-n // chunk_len)
    starts = np.empty(n_chunks + 1, dtype=I64)
    raw = np.full(n_chunks, -1, dtype=I64)
    for c in range(n_chunks):
        p = c * chunk_len
        hs, vs = home[p:p + SAMPLE], valid[p:p + SAMPLE]
        m = int(hs[vs].min()) if vs.any() else -1
        start, g = p, (m // gran if m >= 0 else -1)
        hl, vl = home[p:p + look], valid[p:p + look]
        if c > 0 and p + look > n:
            start = n
            if m >= 0:
                g = int(hl[vl].max()) // gran + 1
        elif c > 0 and m >= 0:
            edge = (m // gran + 1) * gran
            if edge < 1 << 32:
                hit = np.flatnonzero(vl & (hl >= edge))
                if hit.size:
                    start, g = p + int(hit[0]), edge // gran
        starts[c], raw[c] = start, g
    starts[n_chunks] = n
    num_gran = table_size // gran
    bounds = np.empty(n_chunks + 1, dtype=I64)
    have = raw >= 0
    first = int(raw[have][0]) if have.any() else 0
    run, seen = 0, False
    for c in range(n_chunks):
        if have[c]:
            run, seen = max(run, int(raw[c])), True
        bounds[c] = min(run if seen else first, num_gran)
    bounds[n_chunks] = num_gran
    return starts, bounds


Seam = collections.namedtuple("Seam", "c p q L")


def seam_of(starts, bounds, lay, c):
    return Seam(c, c * lay["chunkLen"], int(starts[c]), int(bounds[c]) * lay["granuleSlots"])


def seams_to_test(lay):
    """seam 1, a middle seam, the last seam"""
    return (1, lay["nChunks"] // 2, lay["nChunks"] - 1)


# ---------------------------------------------------------------------------------------------------------------------
# the directed perturbations: each overwrites a few positions of a base near one seam, n stays
# ---------------------------------------------------------------------------------------------------------------------
def crossers(base, sm, k):
    """case A: k copies of the key homed at L - 1 in the k positions before q (the last of them is the base's own): the
    first keeps L - 1, the other k - 1 walk on to L (probeLength >= 2)"""
    h = base.copy()
    assert h[sm.q - 1] == sm.L - 1 and k <= sm.q
    h[sm.q - k:sm.q] = sm.L - 1
    return h, list(range(sm.q - k, sm.q))


def shadow_reach(base, sm, lay, seen):
    """case B: one more copy of the key homed at L - 1, q - shadow positions before... the seam (the first position the next
    wavefront reads) or one position earlier (which it does not)"""
    h = base.copy()
    pos = sm.q - lay["shadow"] - (0 if seen else 1)
    assert pos >= 0 and h[sm.q - 1] == sm.L - 1
    h[pos] = sm.L - 1
    return h, [pos]


def head_straggler(base, sm, lay, inside, slot_below):
    """case C: a tuple homed slot_below slots below L (inside the granule below the range) at the last position of the
    head zone, q + overlap - 1, or at the first one past it"""
    h = base.copy()
    assert 1 <= slot_below <= lay["granuleSlots"]
    pos = sm.q + lay["overlap"] - (1 if inside else 0)
    h[pos] = sm.L - slot_below
    return h, [pos]


def below_in_seam_tile(base, sm, lay, slot_below):
    """case H: a tuple homed slot_below slots below L, the first slot of chunk c's range, at the first position of chunk c's
    OWN tail zone, (c + 1) * chunkLen - tail: a whole chunk past the head zone, in a tile that holds a zone edge and
    therefore runs the zone tests"""
    h = base.copy()
    pos = sm.p + lay["chunkLen"] - lay["tail"]
    assert pos < h.size
    h[pos] = sm.L - slot_below
    return h, [pos]


def early_arrival(base, sm, lay, inside, slot_above):
    """case D: a tuple of the NEXT range, homed at L + slot_above, at the first position of the tail zone, p - tail, or one
    position before it"""
    h = base.copy()
    pos = sm.p - lay["tail"] - (0 if inside else 1)
    h[pos] = sm.L + slot_above
    return h, [pos]


def empty_pattern(n, twin):
    """case E (8-byte tuples, table of 2n slots): the n sorted keys up to 0xFFFFFFFF, the compact table's empty pattern --
    or, the twin on which it holds, up to 0xFFFFFFFE: homes n .. 2n - 1, respectively n - 1 .. 2n - 2"""
    top = 0xFFFFFFFF - (1 if twin else 0)
    return np.arange(top - (n - 1), top + 1, dtype=U64)


def run_over_chunks(n, lay):
    """case F: the dense base with one key repeated 2 * chunkLen + 100 times from the middle of a chunk on: chunks whose
    range is empty, seams without a crossing"""
    h = base_dense(n)
    a = 5 * lay["chunkLen"] + 37
    h[a:a + 2 * lay["chunkLen"] + 100] = h[a]
    return h


def last_granule(n, lay):
    """the odd base with everything from a little before the last nominal seam on homed in the table's last granule: the
    last chunk's sample lies there, the slot after its granule is the table's end, and no home reaches it"""
    h = base_odd(n)
    a = (lay["nChunks"] - 1) * lay["chunkLen"] - 100
    g = lay["granuleSlots"]
    h[a:] = 2 * n - g + (np.arange(n - a) * 7) % g
    return h


def crossers_in_table(table, rel, table_size, shift, L, probe_length):
    """From a table in the reference's format (value = key, 0 = empty): tuples homed below L that sit at or beyond L, plus
    tuples homed below L that are in no slot at all and whose last try, home + probeLength - 1, is at or beyond L (the
    base relations have no conflicts and the walks of a directed case stay far from the table's ends)."""
    th, tv = homes_of(table, table_size, shift)
    slot = np.arange(table_size)
    placed_beyond = int(np.count_nonzero(tv & (th < L) & (slot >= L)))
    rh, rv = homes_of(rel, table_size, shift)
    keys_in, cnt_in = np.unique(np.asarray(table, dtype=U64)[tv], return_counts=True)
    keys_r, cnt_r = np.unique(np.asarray(rel, dtype=U64)[rv & (rh < L) & (rh + probe_length - 1 >= L)], return_counts=True)
    dropped = 0
    for key, cnt in zip(keys_r.tolist(), cnt_r.tolist()):
        at = np.searchsorted(keys_in, U64(key))
        there = int(cnt_in[at]) if at < keys_in.size and keys_in[at] == U64(key) else 0
        dropped += cnt - there
    return placed_beyond + dropped


# ---------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------
# family   A crossers, A1 = A' (probeLength 1), B shadow reach, C head / overlap, D tail / early arrival, H below the range
#          in a seam tile, R ripple
# base     name in BASES; homes = the perturbed home slots; moved = the positions overwritten
# probe    probeLength; shift = homeShift (0 for 8-byte tuples; bare keys: 0 or 3); keys32 = through hj_build_keys_dev
# variant, cause   what buildVariant 4 must report: (4, 0) = the compact build held, (3, bit) = it handed over for exactly
#          that cause, (3, 0) = not tried
# crossing walks across the seam the compact build must have counted where it held (None: not a case of family A)
Case = collections.namedtuple("Case", "name family base seam homes moved probe shift keys32 variant cause crossing")


def _case(name, family, base, sm, homes, moved, probe, variant, cause, shift=0, keys32=False, crossing=None):
    return Case(name, family, base, sm, homes, moved, probe, shift, keys32, variant, cause, crossing)


def base_seams(name, n, lay, table_size):
    return expected_seams(relation(BASES[name](n)), lay, table_size)


def cases(n, lay, full=True):
    """The directed cases for a relation of n tuples in a table of 2n slots. full = False: one repeat of A to D (the
    thresholds alone), for a second size."""
    out = []
    table_size = 2 * n
    cap, pmax = lay["crosserCap"], lay["compactMaxProbeLength"]
    homes = {b: f(n) for b, f in BASES.items()}
    seams = {b: expected_seams(relation(h), lay, table_size) for b, h in homes.items()}
    first, middle, last = seams_to_test(lay)

    def a_expect(x):
        return (4, 0) if x <= cap else (3, BIT_CROSSERS)

    for c in (first, middle, last):
        tag = {first: "seam1", middle: "middle", last: "last"}[c]
        g, o = seam_of(*seams["gapped"], lay, c), seam_of(*seams["odd"], lay, c)
        # A: k - 1 walks cross; at the cap, one below it, one above it and far above it
        for x in (1, cap - 1, cap, cap + 1, 200):
            for probe in ((2, 4, 8) if full and x in (1, cap, cap + 1) else (4,)):
                h, mv = crossers(homes["gapped"], g, x + 1)
                out.append(_case(f"A-{tag}-gapped-x{x}-p{probe}", "A", "gapped", g, h, mv, probe, *a_expect(x), crossing=x))
        if c != first:
            for x in ((1, cap, cap + 1) if full else (cap,)):
                for probe in (4, pmax):
                    h, mv = crossers(homes["odd"], o, x + 1)
                    out.append(_case(f"A-{tag}-odd-x{x}-p{probe}", "A", "odd", o, h, mv, probe, *a_expect(x), crossing=x))
        h, mv = crossers(homes["gapped"], g, 100)
        out.append(_case(f"A1-{tag}-gapped", "A1", "gapped", g, h, mv, 1, 4, 0, crossing=0))
        # B: the shadow zone's first position against the one before it
        for seen in (True, False):
            h, mv = shadow_reach(homes["gapped"], g, lay, seen)
            out.append(_case(f"B-{tag}-{'seen' if seen else 'unseen'}", "B", "gapped", g, h, mv, 4,
                             *((4, 0) if seen else (3, BIT_SEAM)), crossing=1 if seen else None))
        # C: the head zone's last position against the first one past it; the tuple goes to a free slot of the granule
        # below the range (gapped: its first free slot; odd: an even one). Shadow zone + head zone are exactly the first
        # tile, so the first position past the head zone opens a FULL tile, and full tiles skip the zone tests (bit 3 among
        # them): the tuple is simply outside the ring, whose shadow granule is gone by then -- bit 0.
        for base, sm, below in (("gapped", g, lay["granuleSlots"] - 16), ("odd", o, 10)):
            for inside in (True, False):
                h, mv = head_straggler(homes[base], sm, lay, inside, below)
                out.append(_case(f"C-{tag}-{base}-{'in' if inside else 'out'}", "C", base, sm, h, mv, 4,
                                 *((4, 0) if inside else (3, BIT_OUTSIDE))))
            # H: where bit 3 does fire -- the same tuple a chunk further on, in the tile that holds chunk c's tail zone
            if c != last:
                h, mv = below_in_seam_tile(homes[base], sm, lay, below)
                out.append(_case(f"H-{tag}-{base}", "H", base, sm, h, mv, 4, 3, BIT_BELOW))
        # D: the tail zone's first position against the one before it; a tuple homed at L and one at L + 5
        for base, sm in (("gapped", g), ("odd", o)):
            for above in (0, 5):
                for inside in (True, False):
                    h, mv = early_arrival(homes[base], sm, lay, inside, above)
                    out.append(_case(f"D-{tag}-{base}-L{above}-{'in' if inside else 'out'}", "D", base, sm, h, mv, 4,
                                     *((4, 0) if inside else (3, BIT_OUTSIDE))))
    if not full:
        return out
    g = seam_of(*seams["gapped"], lay, middle)
    # A once above the largest probeLength the compact build takes: not tried
    h, mv = crossers(homes["gapped"], g, 3)
    out.append(_case("A-middle-gapped-x2-above-pmax", "A", "gapped", g, h, mv, pmax + 1, 3, 0))
    # A and B through the bare-key build, home shift 0 and 3
    for shift in (0, 3):
        for x in (cap, cap + 1):
            h, mv = crossers(homes["gapped"], g, x + 1)
            out.append(_case(f"A-middle-keys-s{shift}-x{x}", "A", "gapped", g, h, mv, 4, *a_expect(x), shift=shift, keys32=True,
                             crossing=x))
        for seen in (True, False):
            h, mv = shadow_reach(homes["gapped"], g, lay, seen)
            out.append(_case(f"B-middle-keys-s{shift}-{'seen' if seen else 'unseen'}", "B", "gapped", g, h, mv, 4,
                             *((4, 0) if seen else (3, BIT_SEAM)), shift=shift, keys32=True, crossing=1 if seen else None))
    # R: case B's seen copy on the dense base. The seam itself checks out; the one-slot displacement then runs through every
    # later tuple and enters the next seam's shadow granule from below, where the next wavefront cannot see it
    d = seam_of(*seams["dense"], lay, middle)
    h, mv = shadow_reach(homes["dense"], d, lay, True)
    out.append(_case("R-middle-dense-ripple", "R", "dense", d, h, mv, 4, 3, BIT_SEAM))
    return out


def short_last_chunk_sizes(lay, k=8):
    """case G: m = k * chunkLen + r bare keys with r around the look (r < look: the last chunk is too short for a seam)"""
    look = lay["look"]
    return [k * lay["chunkLen"] + r for r in (1, SAMPLE - 1, SAMPLE, look - 1, look, look + 1)]
