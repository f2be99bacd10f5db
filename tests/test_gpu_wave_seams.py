"""The seams of the ring builds, aimed at on purpose: every zone edge of the compact build (buildVariant 4) with a tuple one
position inside it and one position outside, every hand-over cause by name, and the pre-pass that places the seams against
its numpy restatement. tests/wave_cases.py holds the case table and the references, tests/test_wave_cases.py has shown on
the CPU that every case sits where it says and keeps its base's seams. Whatever the cause, every build must give the table
and the counters of the sequential oracle, slot for slot. Run with -m gpu on an MI355X."""
import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from gpu_harness import alloc, ctx  # noqa: F401
import wave_cases as wc
from oracle import oracle

pytestmark = pytest.mark.gpu

N = 1 << 16
COUNTERS = ("conflicts", "totalMatches", "inputSum", "tableSumHalf", "tableSumFull", "conflictSum")


def build_probe(ctx, rel, S, probe, variant, shift=0, keys32=False, table_size=None):
    """one build + probe on the device -> (result, exported table, (starts, bounds, pcounts) if the rings ran)"""
    table_size = table_size or 2 * rel.size
    if not keys32:
        got = ctx.run("atomic", rel, S, probeLength=probe, buildVariant=variant)
    else:
        ctx.reserve("atomic", table_size // 2, S.size, probeLength=probe, buildVariant=variant)
        d_r, d_s = alloc(ctx, 4 * rel.size + 16), alloc(ctx, 4 * S.size + 16)
        try:
            ctx.copy_h2d(d_r, rel.astype(np.uint32))
            ctx.copy_h2d(d_s, S.astype(np.uint32))
            ctx.build_keys(d_r, rel.size, shift, table_size)
            ctx.probe_keys(d_s, S.size)
            ctx.checksums()
            got = ctx.fetch()
        finally:
            ctx.dev_free(d_r)
            ctx.dev_free(d_s)
    table = ctx.export_table(table_size)
    seams = ctx.wave_seams() if got["buildVariant"] in (3, 4) else None
    return got, table, seams


def check_exact(got, table, want, tag):
    for k in COUNTERS:
        assert got[k] == want[k], (tag, k, got[k], want[k])
    assert got["outputSum"] == want["outputSumAtomic"], tag
    assert np.array_equal(table, want["table"]), tag


def check_seams(seams, expect, tag):
    assert seams is not None, tag
    assert np.array_equal(seams[0], expect[0]), (tag, "starts")
    assert np.array_equal(seams[1], expect[1]), (tag, "bounds")


def probe_side(rel):
    """every third tuple, and a few keys next to the relation's that it does not hold"""
    return np.concatenate([rel[::3], rel[:64] + np.uint64(1 << 20)])


@pytest.fixture(scope="module")
def world(ctx):
    """layout of this device, the case table, and per base: relation, oracle result, restated seams -- and the seams the
    device exports for the base itself, which every perturbed relation must reproduce"""
    out = {}
    for n in (N, N // 2):
        lay = ctx.wave_layout_info(n)
        base = {}
        for name, f in wc.BASES.items():
            rel = wc.relation(f(n))
            expect = wc.expected_seams(rel, lay, 2 * n)
            want = oracle.build_probe_seq(rel, probe_side(rel), 4, want_table=True)
            for variant in (3, 4):
                got, table, seams = build_probe(ctx, rel, probe_side(rel), 4, variant)
                check_exact(got, table, want, (name, n, variant))
                assert (got["buildVariant"], got["compactFallback"], got["buildDeferred"]) == (variant, 0, 0), (name, n, variant)
                check_seams(seams, expect, (name, n, variant))
            base[name] = {"rel": rel, "seams": expect}
        out[n] = {"lay": lay, "base": base, "cases": wc.cases(n, lay, full=n == N)}
    return out


def run_case(ctx, w, n, case, variants):
    """the unconditional part (table and counters against the oracle, exported seams against the restatement and against
    the base's) and what the case table says buildVariant 4 and 3 must report"""
    lay = w["lay"]
    rel = wc.relation(case.homes, case.shift)
    S = probe_side(rel)
    want = oracle.build_probe_seq_ts(rel, S, 2 * n, case.shift, case.probe, want_table=True)
    expect = wc.expected_seams(rel, lay, 2 * n, case.shift)
    assert np.array_equal(expect[0], w["base"][case.base]["seams"][0]) and np.array_equal(expect[1], w["base"][case.base]["seams"][1])
    report = None
    for variant in variants:
        tag = (case.name, n, variant)
        got, table, seams = build_probe(ctx, rel, S, case.probe, variant, case.shift, case.keys32)
        if variant == 4:
            report = (got["buildVariant"], got["compactFallback"])
            print(f"{case.name} n={n}: predicted (variant, cause) = {(case.variant, case.cause)}, device {report}")
        check_exact(got, table, want, tag)
        if variant == 4:
            assert report == (case.variant, case.cause), tag
            check_seams(seams, expect, tag)
            if got["compactFallback"] == 0 and got["buildVariant"] == 4:
                assert got["buildDeferred"] == 0, tag
                if case.crossing is not None:
                    assert int(seams[2][case.seam.c]) == case.crossing, (tag, "pcounts")
        elif variant == 3:
            assert (got["buildVariant"], got["compactFallback"]) == (3, 0), tag
            check_seams(seams, expect, tag)
        else:
            assert got["compactFallback"] == 0 or got["buildVariant"] == 3, tag
    return report


FAMILIES = ("A", "A1", "B", "C", "D", "H", "R")


@pytest.mark.parametrize("seam", ("seam1", "middle", "last"))
@pytest.mark.parametrize("family", FAMILIES)
def test_directed_cases(ctx, world, family, seam):
    """Every case of the table at 2^16 tuples under buildVariant 0, 3 and 4 (and 1, 2 for the first case of the family):
    cause and variant exactly as predicted, table and counters exact whatever the cause."""
    w = world[N]
    todo = [c for c in w["cases"] if c.family == family and f"-{seam}-" in c.name]
    if (family == "R" and seam != "middle") or (family == "H" and seam == "last"):
        assert not todo                      # R runs once; the last chunk has no tail zone for H
        return
    assert todo
    for k, case in enumerate(todo):
        run_case(ctx, w, N, case, (0, 3, 4) + ((1, 2) if k == 0 else ()))


def test_directed_cases_at_half_the_size(ctx, world):
    """one repeat of A to D at 2^15 tuples (16 chunks): the thresholds alone, buildVariant 3 and 4"""
    w = world[N // 2]
    assert w["lay"]["nChunks"] == wc.layout(N // 2, w["lay"]["computeUnits"])["nChunks"]
    for case in w["cases"]:
        run_case(ctx, w, N // 2, case, (3, 4))


def test_empty_pattern_key_and_its_holding_twin(ctx, world):
    """case E. A relation that holds key 0xFFFFFFFF cannot live in the compact table, whose empty slots carry that pattern:
    bit 2. One key lower it holds -- and then the table's last slot is empty and its 4 bytes equal the key 0xFFFFFFFF, which
    a probe must not take for a match, at any probeLength, as a tuple or as a bare key."""
    lay = world[N]["lay"]
    for twin, expect4 in ((False, (3, wc.BIT_EMPTY_PATTERN)), (True, (4, 0))):
        rel = wc.empty_pattern(N, twin)
        S = np.concatenate([np.full(5, 0xFFFFFFFF, dtype=np.uint64), rel[-300:], rel[:10], np.full(3, 0xFFFFFFFF, dtype=np.uint64)])
        seams_want = wc.expected_seams(rel, lay, 2 * N)
        for probe in (1, 2, 4, 8):
            want = oracle.build_probe_seq(rel, S, probe, want_table=True)
            # the twin's last slot is empty and key 0xFFFFFFFF matches nothing: 300 + 10 matches; the relation itself holds it once
            assert (want["totalMatches"], int(want["table"][-1])) == ((310, 0) if twin else (318, 0xFFFFFFFF))
            for variant in ((0, 1, 2, 3, 4) if probe == 4 else (3, 4)):
                got, table, seams = build_probe(ctx, rel, S, probe, variant)
                tag = (twin, probe, variant)
                if variant == 4:
                    print(f"E twin={twin} probeLength {probe}: predicted {expect4}, device {(got['buildVariant'], got['compactFallback'])}")
                check_exact(got, table, want, tag)
                if variant == 4:
                    assert (got["buildVariant"], got["compactFallback"]) == expect4, tag
                if variant in (3, 4):
                    check_seams(seams, seams_want, tag)
                if variant == 3:
                    assert (got["buildVariant"], got["compactFallback"]) == (3, 0), tag
            if not twin:
                continue
            # the bare-key probe against the compact table of the twin
            ctx.reserve("atomic", N, S.size, probeLength=probe, buildVariant=4)
            d_r, d_s, d_k = alloc(ctx, 8 * N), alloc(ctx, 8 * S.size), alloc(ctx, 4 * S.size)
            try:
                ctx.copy_h2d(d_r, rel)
                ctx.copy_h2d(d_s, S)
                ctx.copy_h2d(d_k, S.astype(np.uint32))
                ctx.build(d_r, N)
                ctx.probe_keys(d_k, S.size)
                got = ctx.fetch()
                assert (got["buildVariant"], got["compactFallback"], got["totalMatches"]) == (4, 0, want["totalMatches"]), probe
                ctx.probe(d_s, S.size)                                  # the two probes add up
                assert ctx.fetch()["totalMatches"] == 2 * want["totalMatches"], probe
            finally:
                for p in (d_r, d_s, d_k):
                    ctx.dev_free(p)


def test_run_over_chunks(ctx, world):
    """case F: one key repeated over more than two chunks inside a sorted relation -- chunks with an empty slot range, seams
    without a crossing. Table and counters; the cause is the build's own matter, but a hand-over says why."""
    lay = world[N]["lay"]
    rel = wc.relation(wc.run_over_chunks(N, lay))
    S = probe_side(rel)
    expect = wc.expected_seams(rel, lay, 2 * N)
    assert not np.array_equal(expect[0], world[N]["base"]["dense"]["seams"][0])
    for probe in (4, 8):
        want = oracle.build_probe_seq(rel, S, probe, want_table=True)
        assert want["conflicts"] >= 2 * lay["chunkLen"]
        for variant in (0, 1, 2, 3, 4):
            got, table, seams = build_probe(ctx, rel, S, probe, variant)
            check_exact(got, table, want, (probe, variant))
            if variant == 4:
                print(f"F probeLength {probe}: device {(got['buildVariant'], got['compactFallback'])}")
                assert (got["buildVariant"] == 4) == (got["compactFallback"] == 0)
            if variant in (3, 4):
                check_seams(seams, expect, (probe, variant))
            if variant == 3:
                assert (got["buildVariant"], got["compactFallback"]) == (3, 0)


@pytest.mark.parametrize("shift", (0, 3))
def test_short_last_chunk(ctx, world, shift):
    """case G: m = 8 * chunkLen + r sorted bare keys, r around the look: a last chunk with fewer tuples than the look has
    positions starts at the relation's end and only owns its part of the table. The compact build holds."""
    lay = world[N]["lay"]
    table_size = 1 << 16
    shapes = set()
    for m in wc.short_last_chunk_sizes(lay):
        rel = wc.relation(wc.base_dense(m), shift)
        S = probe_side(rel)
        lay_m = ctx.wave_layout_info(m)
        expect = wc.expected_seams(rel, lay_m, table_size, shift)
        shapes.add(bool(expect[0][-2] == m))
        want = oracle.build_probe_seq_ts(rel, S, table_size, shift, 4, want_table=True)
        for variant in (0, 1, 2, 3, 4):
            got, table, seams = build_probe(ctx, rel, S, 4, variant, shift, True, table_size)
            check_exact(got, table, want, (m, variant))
            if variant in (3, 4):
                assert (got["buildVariant"], got["compactFallback"], got["buildDeferred"]) == (variant, 0, 0), (m, variant)
                check_seams(seams, expect, (m, variant))
    assert shapes == {True, False}


def test_invalid_tuple_at_the_seam(ctx, world):
    """one invalid tuple (payload bits set, then key 0) in the shadow zone's last position, at the seam and in the head
    zone's last position: HJ_ERR_KEY_RANGE from every variant, and the next valid build on the same context is exact"""
    w = world[N]
    lay, rel = w["lay"], w["base"]["odd"]["rel"]
    sm = wc.seam_of(*w["base"]["odd"]["seams"], lay, lay["nChunks"] // 2)
    S = probe_side(rel)
    want = oracle.build_probe_seq(rel, S, 4, want_table=True)
    for pos in (sm.q - 1, sm.q, sm.q + lay["overlap"] - 1):
        for bad_value in (rel[pos] | (np.uint64(1) << np.uint64(40)), np.uint64(0)):
            bad = rel.copy()
            bad[pos] = bad_value
            for variant in (0, 1, 2, 3, 4):
                with pytest.raises(hj.HashJoinError) as e:
                    ctx.run("atomic", bad, S, buildVariant=variant)
                assert e.value.status == _lib.HJ_ERR_KEY_RANGE, (pos, variant)
        for variant in (3, 4):
            got, table, seams = build_probe(ctx, rel, S, 4, variant)
            check_exact(got, table, want, (pos, variant))
            assert (got["buildVariant"], got["compactFallback"]) == (variant, 0)
            check_seams(seams, w["base"]["odd"]["seams"], (pos, variant))


def _datagen(dist, n):
    return oracle.generate_data(dist, n, n, 16)


@pytest.mark.parametrize("n", (1 << 20, 1 << 22))
def test_pre_pass_against_its_restatement(ctx, n):
    """k_wave_seams and k_wave_bounds_scan alone: more than 256 chunks, so the prefix maximum runs across workgroups.
    DataGen's near-sorted distributions, a relation whose homes reach the table's last granule, and case F."""
    lay = ctx.wave_layout_info(n)
    assert lay["nChunks"] > 256
    rels = [(d, _datagen(d, n)) for d in ("uniform", "sorted", "local_shuffle")]
    rels.append(("last granule", wc.relation(wc.last_granule(n, lay))))
    rels.append(("run over chunks", wc.relation(wc.run_over_chunks(n, lay))))
    tail = wc.base_dense(n)
    tail[:3 * lay["chunkLen"]] = 0                       # leading chunks without a valid sample take the first valid one's
    tail[300 * lay["chunkLen"]:300 * lay["chunkLen"] + 64] = 0      # ... and one in a later workgroup inherits
    for name, rel in rels:
        expect = wc.expected_seams(rel, lay, 2 * n)
        got = ctx.run("atomic", rel, None, buildVariant=3)
        assert got["buildVariant"] == 3
        want = oracle.build_probe_seq(rel, None, 4)
        for k in COUNTERS:
            assert got[k] == want[k], (name, k)
        check_seams(ctx.wave_seams(), expect, (name, n))
    with pytest.raises(hj.HashJoinError) as e:
        ctx.run("atomic", tail.astype(np.uint64), None, buildVariant=3)
    assert e.value.status == _lib.HJ_ERR_KEY_RANGE
    check_seams(ctx.wave_seams(), wc.expected_seams(tail.astype(np.uint64), lay, 2 * n), ("no sample", n))


def test_seam_export_needs_the_rings(ctx, world):
    """hj_wave_seams: HJ_ERR_STATE before any build, after buildVariant 1 and 2, and after buildVariant 0 picked neither ring
    build; the seams after it picked one"""
    rel = world[N]["base"]["gapped"]["rel"]
    with hj.HashJoinContext(0) as fresh:
        with pytest.raises(hj.HashJoinError) as e:
            fresh.wave_seams()
        assert e.value.status == _lib.HJ_ERR_STATE
        assert fresh.wave_layout_info(N) == wc.layout(N, fresh.wave_layout_info(N)["computeUnits"])
    for variant in (1, 2):
        assert ctx.run("atomic", rel, None, buildVariant=variant)["buildVariant"] == variant
        with pytest.raises(hj.HashJoinError) as e:
            ctx.wave_seams()
        assert e.value.status == _lib.HJ_ERR_STATE
    shuffled = oracle.generate_data("shuffle", 1 << 20, 1 << 20, 16)
    with hj.HashJoinContext(0) as fresh:
        assert fresh.run("atomic", shuffled, None)["buildVariant"] == 1              # everything enqueued, global atomics picked
        with pytest.raises(hj.HashJoinError) as e:
            fresh.wave_seams()
        assert e.value.status == _lib.HJ_ERR_STATE
        if fresh.run("atomic", rel, None)["buildVariant"] in (3, 4):
            check_seams(fresh.wave_seams(), world[N]["base"]["gapped"]["seams"], "auto")
        else:
            with pytest.raises(hj.HashJoinError):
                fresh.wave_seams()
    got = ctx.run("atomic", rel, None, buildVariant=4)
    assert got["buildVariant"] == 4
    check_seams(ctx.wave_seams(), world[N]["base"]["gapped"]["seams"], "after 4")


def test_context_reused_across_hold_hand_over_hold(world):
    """A with 64, 65 and 64 crossers on ONE reserved context: each step exact, each step's compactFallback its own"""
    w = world[N]
    lay = w["lay"]
    cap = lay["crosserCap"]
    sm = wc.seam_of(*w["base"]["gapped"]["seams"], lay, lay["nChunks"] // 2)
    with hj.HashJoinContext(0) as c:
        c.reserve("atomic", N, N, buildVariant=4)
        d_r, d_s = alloc(c, 8 * N), alloc(c, 8 * N)
        try:
            for x, expect4 in ((cap, (4, 0)), (cap + 1, (3, wc.BIT_CROSSERS)), (cap, (4, 0))):
                rel = wc.relation(wc.crossers(wc.base_gapped(N), sm, x + 1)[0])
                S = np.resize(probe_side(rel), N)
                want = oracle.build_probe_seq(rel, S, 4, want_table=True)
                c.copy_h2d(d_r, rel)
                c.copy_h2d(d_s, S)
                c.build(d_r, N)
                c.probe(d_s, N)
                c.checksums()
                got = c.fetch()
                check_exact(got, c.export_table(2 * N), want, x)
                assert (got["buildVariant"], got["compactFallback"]) == expect4, x
                starts, bounds, pcounts = c.wave_seams()
                check_seams((starts, bounds), w["base"]["gapped"]["seams"], x)
                if x == cap:
                    assert got["buildDeferred"] == 0 and int(pcounts[sm.c]) == cap
        finally:
            c.dev_free(d_r)
            c.dev_free(d_s)
