"""The planar retire of the classic ring build (buildVariant 3 on a context reserved without HJ_FLAG_KEEP_ROW_IDS,
hj_build_wave.hip): the table leaves as a plane of 4-byte keys -- what the probe reads -- and a plane of input indices that
only the deferred phase walks on; the keys of the slots those walks changed are written afterwards, from R, behind a kernel
boundary. Whatever road a build takes (planar, or the packed build behind it after a hand-over), table and counters must be
the sequential oracle's, slot for slot. The seam and deferral relations come from tests/wave_cases.py. Run with -m gpu on an
MI355X."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from gpu_harness import alloc, ctx  # noqa: F401
import wave_cases as wc
from oracle import oracle

pytestmark = pytest.mark.gpu

N = 1 << 16
COUNTERS = ("conflicts", "totalMatches", "inputSum", "tableSumHalf", "tableSumFull", "conflictSum")
LOG_OVERFLOW, EMPTY_PATTERN = 1, 2          # hj_wave_planar_info, out[1]


def probe_side(rel):
    """every third tuple, and a few keys next to the relation's that it does not hold"""
    return np.concatenate([rel[::3], rel[:64] + np.uint64(1 << 20)])


def build_probe(c, rel, S, probe=4, variant=3, shift=0, keys32=False, table_size=None, idx_base=0, keep=False):
    """one build + probe through the split API -> (result, exported table, hj_wave_planar_info)"""
    table_size = table_size or 2 * rel.size
    c.reserve("atomic", table_size // 2, S.size, probeLength=probe, buildVariant=variant, keepRowIds=keep)
    width, dtype = (4, np.uint32) if keys32 else (8, np.uint64)
    d_r, d_s = alloc(c, width * rel.size + 16), alloc(c, width * S.size + 16)
    try:
        c.copy_h2d(d_r, rel.astype(dtype))
        c.copy_h2d(d_s, S.astype(dtype))
        if keys32:
            c.build_keys(d_r, rel.size, shift, table_size)
            c.probe_keys(d_s, S.size)
        else:
            c.build(d_r, rel.size, idx_base)
            c.probe(d_s, S.size)
        c.checksums()
        got = c.fetch()
        return got, c.export_table(table_size), c.wave_planar_info()
    finally:
        c.dev_free(d_r)
        c.dev_free(d_s)


def check_exact(got, table, want, tag):
    for k in COUNTERS:
        assert got[k] == want[k], (tag, k, got[k], want[k])
    assert got["outputSum"] == want["outputSumAtomic"], tag
    assert np.array_equal(table, want["table"]), tag


def check_planar(got, info, tag):
    """variant 3, the planar road taken and kept: 4-byte table, no hand-over of either kind"""
    assert (got["buildVariant"], got["compactFallback"]) == (3, 0), tag
    assert info == {"planar": True, "planarFallback": 0, "tableFormat": 1}, (tag, info)


@pytest.mark.parametrize("log2n", (16, 18, 20))
def test_uniform_under_the_device_pick(ctx, log2n):
    """`uniform` (shuffle window 16), buildVariant 0: the sampler picks the classic rings, they retire planar, nothing hands
    over; probeLength 1, 2, 4, 8"""
    n = 1 << log2n
    rel = oracle.generate_data("uniform", n, n, 16)
    S = oracle.relS_for("uniform", rel)
    for probe in (1, 2, 4, 8):
        want = oracle.build_probe_seq(rel, S, probe, want_table=True)
        got = ctx.run("atomic", rel, S, probeLength=probe)
        info = ctx.wave_planar_info()
        table = ctx.export_table(2 * n)
        check_exact(got, table, want, (n, probe))
        check_planar(got, info, (n, probe))
        if probe > 1:
            assert got["buildDeferred"] > 0, (n, probe)       # the seams' stragglers: the walks on the index plane ran


@pytest.fixture(scope="module")
def world(ctx):
    lay = ctx.wave_layout_info(N)
    return {"lay": lay, "cases": wc.cases(N, lay, full=True)}


@pytest.mark.parametrize("family", ("A", "A1", "B", "C", "D", "H", "R"))
def test_seam_and_deferral_cases(ctx, world, family):
    """The directed cases of tests/wave_cases.py through buildVariant 3 and 0 without the row-id flag. A: up to 200 copies of
    one key right before a seam (more than probeLength of them) walk across it into slots later tuples have taken -- the
    deferred phase displaces those, carries them on and reads their keys back from R; B, C: stragglers on either side of a
    seam; D: early arrivals; H: a tuple below its chunk's range; R: a displacement that runs through every later slot (more
    than a dirty log holds: the hand-over by a single walk).
    As tuples and, where the table says so, as bare keys with a home shift."""
    todo = [c for c in world["cases"] if c.family == family]
    assert todo
    for case in todo:
        rel = wc.relation(case.homes, case.shift)
        S = probe_side(rel)
        want = oracle.build_probe_seq_ts(rel, S, 2 * N, case.shift, case.probe, want_table=True)
        for variant in (3, 0):
            got, table, info = build_probe(ctx, rel, S, case.probe, variant, case.shift, case.keys32)
            tag = (case.name, variant)
            check_exact(got, table, want, tag)
            if variant == 3 and family == "R":
                # one deferred tuple displaces every later tuple up to the relation's end: half the table's slots change in
                # one walk, several times what its slice's log holds -- the packed build redoes the table
                assert (got["buildVariant"], got["compactFallback"]) == (3, 0), tag
                assert info == {"planar": False, "planarFallback": LOG_OVERFLOW, "tableFormat": 0}, (tag, info)
            elif variant == 3:
                check_planar(got, info, tag)
                if family == "A" and case.crossing is not None:
                    assert got["buildDeferred"] >= case.crossing, tag          # every walk across the seam is a deferred tuple
            elif family != "R":
                assert info["planarFallback"] == 0, tag


def test_displaced_tuples_with_an_index_base(ctx, world):
    """case A with 200 crossers, built with idxBase != 0: the deferred phase finds a displaced tuple's key at
    R[index - idxBase]"""
    case = next(c for c in world["cases"] if c.name == "A-middle-gapped-x200-p4")
    rel = wc.relation(case.homes)
    S = probe_side(rel)
    want = oracle.build_probe_seq(rel, S, 4, want_table=True)
    for idx_base in (12345, 0xFFFFFFFF - N):
        got, table, info = build_probe(ctx, rel, S, 4, 3, idx_base=idx_base)
        check_exact(got, table, want, idx_base)
        check_planar(got, info, idx_base)
        assert got["buildDeferred"] >= 200


@pytest.mark.parametrize("shift", (0, 3))
def test_bare_keys_with_a_home_shift(ctx, shift):
    """hj_build_keys_dev (a radix shard's keys; their indices start at 0 by the ABI), home shift 0 and 3, one seeded `uniform`
    relation at 2^16: the keys of a shard share their low bits, so the relation is made of keys = home << shift | low bits"""
    rng = np.random.default_rng(20 + shift)
    base = oracle.generate_data("uniform", N, N, 16)
    rel = (base << np.uint64(shift)) | np.uint64((1 << shift) - 1)
    S = np.concatenate([rel[rng.integers(0, N, N // 2)], rel[:64] + np.uint64(1 << 22)])
    want = oracle.build_probe_seq_ts(rel, S, 2 * N, shift, 4, want_table=True)
    for variant in (3, 0):
        got, table, info = build_probe(ctx, rel, S, 4, variant, shift, True, 2 * N)
        check_exact(got, table, want, (shift, variant))
        check_planar(got, info, (shift, variant))
        assert got["buildDeferred"] > 0


def test_walks_at_the_table_end_and_runs_of_one_key(ctx, world):
    """everything from the last seam on homed in the table's last granule (walks that end at the table's last slot, and
    walks that wrap); one key repeated over more than two chunks (entries that outlive the ring, chunks with an empty
    range)"""
    lay = world["lay"]
    for name, homes in (("last granule", wc.last_granule(N, lay)), ("run over chunks", wc.run_over_chunks(N, lay))):
        rel = wc.relation(homes)
        S = probe_side(rel)
        for probe in (4, 8):
            want = oracle.build_probe_seq(rel, S, probe, want_table=True)
            got, table, info = build_probe(ctx, rel, S, probe, 3)
            check_exact(got, table, want, (name, probe))
            # both stay planar: the walks at and past the last slot, and the 2049 deferred copies of one key (which change
            # no more slots than probeLength), are the planar walker's work, not the packed build's
            check_planar(got, info, (name, probe))
            assert got["buildDeferred"] > 100, (name, probe)
    # one tuple homed at the table's last slot behind the sorted relation's own: its walk ends there
    homes = wc.base_odd(N)
    homes[-3:] = 2 * N - 1
    rel = wc.relation(homes)
    want = oracle.build_probe_seq(rel, probe_side(rel), 4, want_table=True)
    got, table, info = build_probe(ctx, rel, probe_side(rel), 4, 3)
    check_exact(got, table, want, "last slot")
    check_planar(got, info, "last slot")
    # six tuples homed there, probeLength 8: five walks wrap past the last slot into slots 0.., past what earlier tuples hold
    # there; a handful of changed slots, far below what a slice's log holds, so the planar walker itself has to get the wrap right
    homes = wc.base_odd(N)
    homes[-6:] = 2 * N - 1
    rel = wc.relation(homes)
    want = oracle.build_probe_seq(rel, probe_side(rel), 8, want_table=True)
    got, table, info = build_probe(ctx, rel, probe_side(rel), 8, 3)
    check_exact(got, table, want, "wrap")
    check_planar(got, info, "wrap")
    assert got["buildDeferred"] >= 5


def test_log_overflow_hands_over_and_the_flag_resets():
    """buildVariant 3 forced onto `shuffle` (no locality: nearly every tuple is deferred, the dirty logs cannot fit): the
    packed classic build redoes the table, exact; the next build on the same context (`uniform`) is planar again, and the
    one after it hands over again"""
    shuffled = oracle.generate_data("shuffle", N, N, 16)
    uniform = oracle.generate_data("uniform", N, N, 16)
    with hj.HashJoinContext(0) as c:
        for step, (rel, overflow) in enumerate(((shuffled, True), (uniform, False), (shuffled, True), (shuffled, True))):
            S = probe_side(rel)
            want = oracle.build_probe_seq(rel, S, 4, want_table=True)
            got, table, info = build_probe(c, rel, S, 4, 3)
            check_exact(got, table, want, step)
            assert (got["buildVariant"], got["compactFallback"]) == (3, 0), step
            if overflow:
                assert info == {"planar": False, "planarFallback": LOG_OVERFLOW, "tableFormat": 0}, (step, info)
                assert got["buildDeferred"] > N // 2, step
            else:
                check_planar(got, info, step)


def test_empty_pattern_key_hands_over(ctx, world):
    """key 0xFFFFFFFF cannot live in a table of 4-byte keys: the packed build takes the relation, at buildVariant 3, 4 (whose
    own hand-over leads to the classic rings) and 0; one key lower the planar table holds and its last slot matches nothing"""
    for twin in (False, True):
        rel = wc.empty_pattern(N, twin)
        S = np.concatenate([np.full(5, 0xFFFFFFFF, dtype=np.uint64), rel[-300:], rel[:10]])
        for probe in (1, 4):
            want = oracle.build_probe_seq(rel, S, probe, want_table=True)
            for variant in (3, 4, 0):
                got, table, info = build_probe(ctx, rel, S, probe, variant)
                tag = (twin, probe, variant)
                check_exact(got, table, want, tag)
                if twin:
                    assert info["planarFallback"] == 0, tag
                    assert got["buildVariant"] == 4 or info["planar"], tag
                else:
                    assert got["buildVariant"] == 3 and info == {"planar": False, "planarFallback": EMPTY_PATTERN, "tableFormat": 0}, (tag, info)
                if variant == 3:
                    assert got["compactFallback"] == 0, tag


def test_row_ids_keep_the_packed_slots(ctx):
    """reserved WITH the flag: 8-byte slots as before, and the materialising probe returns the join's pairs"""
    n = 1 << 12
    rel = oracle.generate_data("uniform", n, n, 16)
    S = oracle.relS_for("uniform", rel)
    want = oracle.build_probe_seq(rel, S, 4, want_table=True)
    for variant in (3, 0):
        got, table, info = build_probe(ctx, rel, S, 4, variant, keep=True)
        check_exact(got, table, want, variant)
        assert (got["buildVariant"], got["compactFallback"]) == (3, 0)
        assert info == {"planar": False, "planarFallback": 0, "tableFormat": 0}, info
    # pairs, on sorted unique keys (every tuple is in the table): S[i] = key k matches R row k - 1
    rel = oracle.generate_data("sorted", n)
    S = rel[::5].copy()
    cap = S.size + 8
    ctx.reserve("atomic", n, S.size, buildVariant=3, keepRowIds=True)
    d_r, d_s, d_os, d_or = alloc(ctx, 8 * n), alloc(ctx, 8 * S.size), alloc(ctx, 4 * cap), alloc(ctx, 4 * cap)
    try:
        ctx.copy_h2d(d_r, rel)
        ctx.copy_h2d(d_s, S)
        ctx.build(d_r, n)
        ctx.probe_pairs(d_s, S.size, d_os, d_or, cap)
        found, written = ctx.pairs_info()[:2]
        assert found == written == S.size
        s_rows, r_rows = np.empty(cap, dtype=np.uint32), np.empty(cap, dtype=np.uint32)
        ctx.copy_d2h(s_rows, d_os)
        ctx.copy_d2h(r_rows, d_or)
        order = np.argsort(s_rows[:written])
        assert np.array_equal(s_rows[:written][order], np.arange(S.size, dtype=np.uint32))
        assert np.array_equal(r_rows[:written][order], (S - np.uint64(1)).astype(np.uint32))
        assert ctx.wave_planar_info()["tableFormat"] == 0
    finally:
        for p in (d_r, d_s, d_os, d_or):
            ctx.dev_free(p)
