"""Every stream-ordered entry point behind a delayed caller's stream (hj_create_on_stream), on an MI355X. Run with -m gpu.

The rest of the suite drives contexts with a private stream that is idle at the start of every call, so work on the wrong
stream, a host read that does not wait, a descriptor read after the call returned, or an undocumented synchronisation would
fail no test. Here every sequence is enqueued behind ONE bounded delay on the caller's stream (stream_order.py), with no
host synchronisation between the calls: when the library's calls are enqueued the inputs still hold decoys and the outputs
sentinels; the real inputs arrive behind the delay on the same stream and a torch copy on that stream takes the results.
Whatever left the stream's order computed on decoys and is wrong, never invalid. Results are compared after one final
synchronize, against the numpy / plain Python models of the other tests (r_marks_common, join_kinds_common, agg_common,
keys2_common, the gather models of test_gpu_gather2.py); the library is asked for nothing about what a result should be.
Where a later call needs a count as a host argument (gather rows, verify2 / pairs_agg pairs) it comes from the model.

Each sequence runs once as a warm-up on other valid inputs of the same sizes (buffers grow, the locality expectation
settles) and is followed by a sync; the delayed run is the steady state. Where every call of a sequence is classified
"asynchronous" in the Stream contract table of INTEGRATION.md, the delay must still be pending after the last enqueue: no
call blocked the host, and the decoys were still in place when every call was made. Both stream flavours: a
torch.cuda.Stream() (non-blocking) and handle 0, the legacy default stream. The module fixture runs the harness witness
first. The descriptor arrays of the resident, aggregation and key-column sequences are the test's own ctypes arrays, zeroed
the moment each call returns, while the stream is still delayed (the header: "read before the call returns")."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from htm_hashjoin_amd._lib import lib

import agg_common as ac
import keys2_common as k2
import stream_order as so
from gather_common import column, fill_of, fixed, rows_of, strings, want_of
from gpu_harness import fl, plane_words  # noqa: F401
from join_kinds_common import ANTI, LEFT, derive
from r_marks_common import LOW, inner_expected, join_expected, unmatched_r

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
NO_ROW = so.NO_ROW
SLACK = 64                       # map words behind the exact count: they keep the HJ_NO_ROW prefill

_CONTRACT = so.contract()


def all_async(*names):
    """whether every entry point of a sequence is asynchronous in the steady state, by the table of INTEGRATION.md"""
    return all(_CONTRACT[n][0] == "asynchronous" for n in names)


def ok(ctx, rc):
    if rc != _lib.HJ_OK:
        raise hj.HashJoinError(rc, lib.hj_last_error(ctx._h).decode())


def vp(p):
    return C.c_void_p(p) if p else None


def zero(arr):
    """a descriptor array the call has returned from: the caller reuses it at once"""
    C.memset(arr, 0, C.sizeof(arr))


def maps(st, count):
    """two map planes for `count` rows: HJ_NO_ROW everywhere (a valid map for whoever reads it early)"""
    return st.out(count + SLACK, U32, NO_ROW), st.out(count + SLACK, U32, NO_ROW)


def map_rows(st, b, count, tag):
    a = st.result(b, U32, tag)
    assert (a[count:] == NO_ROW).all(), (tag, "a word behind the last row was written")
    return a[:count]


def packed(s, r):
    return (s.astype(U64) << U64(32)) | r.astype(U64)


# ---------------------------------------------------------------------------------------------------------------------
# a. table count: build -> probe -> probe
# ---------------------------------------------------------------------------------------------------------------------
N = 1 << 16                      # what the directed tests of the ring builds use (test_gpu_wave_seams.N); 4 chunks of the window build
N1, N2 = 40001, 20003            # two S slices of unequal, odd length
PROBE = 4


def walk_table(R, probe_length=PROBE):
    """the open-addressing table after the sequential insert (NoCCHashBuild.hpp:43-59), as hj_export_table gives it, and
    the tuples dropped: r_marks_common.walk_expected's first half, restated"""
    n = R.size
    mask = 2 * n - 1
    keys, dropped = [0] * (2 * n), 0
    for k in R.tolist():
        cur = k & mask
        for _ in range(probe_length):
            if keys[cur] == 0:
                keys[cur] = k
                break
            cur = (cur + 1) & mask
        else:
            dropped += 1
    return np.array(keys, dtype=U64), dropped


@functools.lru_cache(maxsize=None)
def table_data():
    rng = np.random.default_rng(20240607)
    d = types.SimpleNamespace()
    d.R = hj.generate_data("local_shuffle", N, N, 16)                   # keys 1..N, shuffle window 16
    d.Rw = d.R.reshape(-1, 2)[:, ::-1].ravel().copy()                   # neighbours swapped: other content, the same locality class
    d.Rd = d.R + U64(2 * N)                                             # same home slots, keys 2N+1..3N: matches nothing of S
    d.S = rng.integers(1, N + N // 4, N1 + N2).astype(U64)              # a fifth of S has no partner
    d.Sw = rng.integers(1, N + N // 4, N1 + N2).astype(U64)
    d.Sd = U64(3 * N + 1) + np.arange(N1 + N2, dtype=U64)               # matches neither R nor its decoy
    d.inner1 = inner_expected("atomic", d.R, d.S[:N1], PROBE, 0, 0)
    d.inner2 = inner_expected("atomic", d.R, d.S[N1:], PROBE, 0, N1)
    d.table, d.dropped = walk_table(d.R)
    assert d.inner1.size and d.inner2.size and d.inner1.size < N1
    return d


def stage_table_inputs(st, d):
    bR = st.buf(d.Rd, real=d.R, warm=d.Rw)
    bS1 = st.buf(d.Sd[:N1], real=d.S[:N1], warm=d.Sw[:N1])
    bS2 = st.buf(d.Sd[N1:], real=d.S[N1:], warm=d.Sw[N1:])
    return bR, bS1, bS2


@pytest.mark.parametrize("variant", [1, 2, 3, 4, 0])
def test_a_table_build_probe_probe(fl, variant):
    """open addressing, every build variant: the table (hj_export_table) and the match total are exact. buildVariant 0 picks
    the compact rings on this R (shuffle window 16), on the device, behind the delay"""
    d = table_data()
    with hj.HashJoinContext(0, stream=fl.handle) as ctx:
        ctx.reserve("atomic", N, N1 + N2, buildVariant=variant, probeLength=PROBE)
        st = so.Stage(fl.stream)
        bR, bS1, bS2 = stage_table_inputs(st, d)

        def seq(which):
            ctx.build(bR.ptr, N)
            ctx.probe(bS1.ptr, N1)
            ctx.probe(bS2.ptr, N2)

        so.run_delayed([st], seq, all_async("hj_build_dev", "hj_probe_dev"), f"a.table_count.v{variant}.{fl.name}")
        got = ctx.fetch()
        table = ctx.export_table(2 * N)
        st.check_inputs_intact()
    print("variant", variant, {k: got[k] for k in ("buildVariant", "totalMatches", "conflicts", "sSize", "compactFallback")})
    assert got["buildVariant"] == (variant or 4), got["buildVariant"]
    assert (got["totalMatches"], got["sSize"], got["rSize"]) == (d.inner1.size + d.inner2.size, N1 + N2, N)
    assert got["conflicts"] == d.dropped
    assert np.array_equal(table, d.table), np.flatnonzero(table != d.table)[:8]


def test_a_two_builds_behind_one_delay_stale_expectation(fl):
    """buildVariant 0, two builds of different locality class queued behind the same delay: shuffle window 16, then uniformly
    shuffled. When the second build is enqueued the first has not run, so the expectation it reads from pinned memory
    (*hPreferred, "read here without waiting") is the stale one of the warm-up -- tight locality: only the rings are enqueued
    for an input that wants global atomics. "One slow step, never a wrong one": both tables and both match totals are exact.
    The first table is gone when the stream drains, so it is read through a pairs probe with every key 1..N and one with S's
    first slice (HJ_FLAG_KEEP_ROW_IDS: the rings are the tight pick); the second one also through hj_export_table."""
    d = table_data()
    RB = hj.generate_data("shuffle", N, N, 16)
    every = np.arange(1, N + 1, dtype=U64)
    innerA_all = inner_expected("atomic", d.R, every, PROBE)
    innerB_all = inner_expected("atomic", RB, every, PROBE)
    innerB1 = inner_expected("atomic", RB, d.S[:N1], PROBE)
    innerB2 = inner_expected("atomic", RB, d.S[N1:], PROBE, 0, N1)
    tableB, droppedB = walk_table(RB)
    with hj.HashJoinContext(0, stream=fl.handle) as ctx:
        ctx.reserve("atomic", N, N, buildVariant=0, probeLength=PROBE, keepRowIds=True)
        st = so.Stage(fl.stream)
        bRA = st.buf(d.Rd, real=d.R, warm=d.Rw)
        bRB = st.buf(d.Rd, real=RB, warm=d.R.reshape(-1, 4)[:, ::-1].ravel().copy())    # the warm-up leaves the expectation "tight"
        bAll = st.buf(every + U64(5 * N), real=every, warm=np.roll(every, 3))
        bS1 = st.buf(d.Sd[:N1], real=d.S[:N1], warm=d.Sw[:N1])
        bS2 = st.buf(d.Sd[N1:], real=d.S[N1:], warm=d.Sw[N1:])
        pA = maps(st, innerA_all.size)
        pA1 = maps(st, d.inner1.size)
        pB = maps(st, innerB_all.size)
        pB1 = maps(st, innerB1.size)

        def seq(which):
            ctx.build(bRA.ptr, N)
            ctx.probe_pairs(bAll.ptr, N, pA[0].ptr, pA[1].ptr, innerA_all.size + SLACK)
            ctx.probe_pairs(bS1.ptr, N1, pA1[0].ptr, pA1[1].ptr, d.inner1.size + SLACK)
            ctx.build(bRB.ptr, N)
            ctx.probe_pairs(bAll.ptr, N, pB[0].ptr, pB[1].ptr, innerB_all.size + SLACK)
            ctx.probe_pairs(bS1.ptr, N1, pB1[0].ptr, pB1[1].ptr, innerB1.size + SLACK)
            ctx.probe(bS2.ptr, N2)

        so.run_delayed([st], seq, all_async("hj_build_dev", "hj_probe_pairs_dev", "hj_probe_dev"), f"a.two_builds.{fl.name}")
        got = ctx.fetch()
        table = ctx.export_table(2 * N)
    print("second build:", {k: got[k] for k in ("buildVariant", "totalMatches", "conflicts", "buildDeferred")})
    for name, planes, want in (("A, every key", pA, innerA_all), ("A, slice 1", pA1, d.inner1), ("B, every key", pB, innerB_all),
                               ("B, slice 1", pB1, innerB1)):
        s, r = map_rows(st, planes[0], want.size, name), map_rows(st, planes[1], want.size, name)
        assert np.array_equal(np.sort(packed(s, r)), want), name
    assert (got["totalMatches"], got["sSize"]) == (innerB_all.size + innerB1.size + innerB2.size, N + N1 + N2)
    assert got["conflicts"] == droppedB
    assert np.array_equal(table, tableB), np.flatnonzero(table != tableB)[:8]
    # the pick is taken among the enqueued variants: with the stale expectation that is the rings and nothing else. (A
    # library that waited for the first build would have enqueued, and picked, global atomics for a shuffled R.)
    assert got["buildVariant"] == 3, got["buildVariant"]


def test_a_htm_build_probe_probe(fl):
    """the bucketised table: hj_build_dev reads the conflict count back (documented: not asynchronous), so correctness only --
    no pending() assertion. R has duplicate keys, so buckets overflow into chains and the read-back is used"""
    d = table_data()
    R = hj.generate_data("uniform", N, N, 16)
    want = join_expected(R, d.S[:N1]).size + join_expected(R, d.S[N1:]).size
    with hj.HashJoinContext(0, stream=fl.handle) as ctx:
        ctx.reserve("htm", N, N1 + N2)
        st = so.Stage(fl.stream)
        bR = st.buf(d.Rd, real=R, warm=np.roll(R, 4099))
        _, bS1, bS2 = stage_table_inputs(st, d)

        def seq(which):
            ctx.build(bR.ptr, N)
            ctx.probe(bS1.ptr, N1)
            ctx.probe(bS2.ptr, N2)

        so.run_delayed([st], seq, False, f"a.htm.{fl.name}")            # hj_build_dev under HTM waits for the stream
        got = ctx.fetch()
    assert got["conflicts"] > 0 and got["htmOverflowBuckets"] > 0, got
    assert (got["totalMatches"], got["sSize"], got["rSize"]) == (want, N1 + N2, N)


# ---------------------------------------------------------------------------------------------------------------------
# b. table pairs: build -> probe_pairs inner -> probe_pairs left -> r_rows -> gather through both maps
# ---------------------------------------------------------------------------------------------------------------------
def test_b_table_pairs_marks_gather(fl):
    d = table_data()
    rng = np.random.default_rng(5)
    left2 = derive(LEFT, d.inner2, N2, N1)
    lone_r = unmatched_r(np.concatenate([d.inner1, d.inner2]), N)
    c1, c2 = d.inner1.size, left2.size
    pay_r = rng.integers(0, 1 << 63, N, dtype=np.int64).view(U64)
    pay_s = rng.integers(0, 1 << 32, N2, dtype=np.int64).astype(U32)
    fill_r, fill_s = 0x1122334455667788, 0x99AABBCC
    with hj.HashJoinContext(0, stream=fl.handle) as ctx:
        ctx.reserve("atomic", N, N1 + N2, probeLength=PROBE, keepRowIds=True, trackRMatches=True)
        st = so.Stage(fl.stream)
        bR, bS1, bS2 = stage_table_inputs(st, d)
        bPr = st.buf(np.full(N, ac.POISON, dtype=U64), real=pay_r, warm=np.roll(pay_r, 1))
        bPs = st.buf(np.full(N2, ac.POISON >> 32, dtype=U32), real=pay_s, warm=np.roll(pay_s, 1))
        pI, pL = maps(st, c1), maps(st, c2)
        bLone = st.out(N, U32, so.SENT32)
        bGr, bGs = st.out(c2, U64, so.SENT64), st.out(c2, U32, so.SENT32)
        bGv = st.out((c2 + 31) // 32, U32, so.SENT32)

        def seq(which):
            ctx.build(bR.ptr, N)
            ctx.probe_pairs(bS1.ptr, N1, pI[0].ptr, pI[1].ptr, c1 + SLACK, s_idx_base=0, kind=0)
            ctx.probe_pairs(bS2.ptr, N2, pL[0].ptr, pL[1].ptr, c2 + SLACK, s_idx_base=N1, kind=LEFT)
            ctx.r_rows(0, bLone.ptr, N)
            ctx.gather(pL[1].ptr, c2, N, [(bPr.ptr, bGr.ptr, 8, fill_r)], d_valid=bGv.ptr)              # R's column, NULL rows
            ctx.gather(pL[0].ptr, c2, N2, [(bPs.ptr, bGs.ptr, 4, fill_s)], row_base=N1)                 # the slice's own column

        so.run_delayed([st], seq, all_async("hj_build_dev", "hj_probe_pairs_dev", "hj_probe_join_dev", "hj_r_rows_dev", "hj_gather_dev"),
                       f"b.table_pairs.{fl.name}")
        got = ctx.fetch()
        info = ctx.gather_info()
        st.check_inputs_intact()
    assert info[:2] == (c2, 0) and info[3] == 0, ("gather_info: the last gather alone, it has no NULL row", info)
    s1, r1 = map_rows(st, pI[0], c1, "inner S"), map_rows(st, pI[1], c1, "inner R")
    assert np.array_equal(np.sort(packed(s1, r1)), d.inner1)
    s2, r2 = map_rows(st, pL[0], c2, "left S"), map_rows(st, pL[1], c2, "left R")
    assert np.array_equal(np.sort(packed(s2, r2)), left2)
    lone = st.result(bLone, U32, "r_rows")
    assert np.array_equal(lone[:lone_r.size].astype(U64), lone_r) and (lone[lone_r.size:] == so.SENT32).all()
    has = r2 != NO_ROW
    want_r = np.where(has, pay_r[np.where(has, r2, 0)], U64(fill_r))
    assert np.array_equal(st.result(bGr, U64, "gather R"), want_r)
    assert np.array_equal(st.result(bGv, U32, "gather valid"), plane_words(has)) and not has.all()
    assert np.array_equal(st.result(bGs, U32, "gather S"), pay_s[s2 - N1])
    assert (got["totalMatches"], got["sSize"]) == (d.inner1.size + d.inner2.size, N1 + N2)


# ---------------------------------------------------------------------------------------------------------------------
# c. resident radix join, through _lib with the test's own descriptor arrays (f); g interleaves two of these
# ---------------------------------------------------------------------------------------------------------------------
NR, M1, M2 = (1 << 14) + 37, 9001, 5003
KEYS = 12000


def stage_strings(st, col, rng):
    """a variable-length source column: decoy = other bytes under all-zero offsets (every element empty) and an all-zero
    validity plane. -> (data, offsets, validity or None)"""
    data, off = col["data"], col["offsets"].astype(U32)
    bD = st.buf(rng.integers(0, 256, data.size, dtype=np.uint8), real=data, warm=rng.integers(0, 256, data.size, dtype=np.uint8))
    bO = st.buf(np.zeros(off.size, dtype=U32), real=off, warm=off)
    bV = None
    if col["valid"] is not None:
        w = plane_words(col["valid"])
        bV = st.buf(np.zeros(w.size, dtype=U32), real=w, warm=w)
    return bD, bO, bV


def g2_cols(descs):
    arr = (_lib.hj_gather_col2 * len(descs))()
    for c, d in zip(arr, descs):
        c.src, c.dst, c.srcOffsets, c.dstOffsets, c.srcValid, c.dstValid = (d.get(k) or None for k in
                                                                           ("src", "dst", "src_offsets", "dst_offsets", "src_valid", "dst_valid"))
        c.dstCapacity, c.width, c.flags = d.get("dst_capacity", 0), d.get("width", 0), 0
        fill = int.from_bytes(bytes(d.get("fill", b"\0" * 16)[:16]), "little")
        c.fill[0], c.fill[1] = fill & 0xFFFFFFFFFFFFFFFF, fill >> 64
    return arr


@functools.lru_cache(maxsize=None)
def resident_data(seed):
    rng = np.random.default_rng(seed)
    d = types.SimpleNamespace(rng=rng)
    d.R = rng.integers(0, KEYS, NR).astype(U64)                          # duplicate keys; key 0 is an ordinary key
    d.S = rng.integers(0, KEYS + KEYS // 4, M1 + M2).astype(U64)
    d.Rd = d.R + U64(2 * KEYS)                                           # disjoint from S and from S's decoy
    d.Sd = d.S + U64(4 * KEYS)
    d.Rw, d.Sw = np.roll(d.R, 5), np.roll(d.S, 11)
    d.inner1 = join_expected(d.R, d.S[:M1], 0, 0, any_key=True)
    d.inner2 = join_expected(d.R, d.S[M1:], 0, M1, any_key=True)
    d.anti2 = derive(ANTI, d.inner2, M2, M1)
    d.matched = np.unique(d.inner1 & LOW)                                # the inner call marks; counting and anti calls do not
    assert d.inner1.size > M1 // 2 and d.anti2.size and d.matched.size < NR
    # R's payload: a plain column, a nullable one, a string column; S's first slice: a string column
    d.plain = fixed(column(rng, NR, 8), 8, fill_of(8, 1))
    d.nullable = fixed(column(rng, NR, 4), 4, fill_of(4, 2), valid=rng.random(NR) < 0.7, dst_valid=True)
    lens = [k2.LENGTHS[(k * 7 + 3) % len(k2.LENGTHS)] for k in range(NR)]
    d.str_r = strings(rng, lens, valid=rng.random(NR) < 0.8, dst_valid=True)
    d.str_s = strings(rng, [k2.LENGTHS[(k * 5 + 1) % len(k2.LENGTHS)] for k in range(M1)])
    r_rows, s_rows = (d.inner1 & LOW).astype(np.int64), (d.inner1 >> U64(32)).astype(np.int64)
    ok_r = d.str_r["valid"][r_rows]
    d.bytes_r = int((d.str_r["offsets"][r_rows + 1] - d.str_r["offsets"][r_rows])[ok_r].sum())      # the map's order does not change the totals
    d.bytes_s = int((d.str_s["offsets"][s_rows + 1] - d.str_s["offsets"][s_rows]).sum())
    return d


class Resident:
    """sequence c on one context and one stage: prj_build -> prj_probe x 2 -> prj_probe_pairs (inner, then anti) -> r_rows ->
    gather2 (plain, nullable, string) -> gather2 (string) once more, the second scan reusing the context's workspace while the
    first is still pending"""

    CALLS = ("hj_prj_build_dev", "hj_prj_probe_dev", "hj_prj_probe_pairs_dev", "hj_prj_probe_join_dev", "hj_r_rows_dev", "hj_gather2_dev")

    def __init__(self, handle, stream, seed):
        self.d = d = resident_data(seed)
        self.ctx = hj.HashJoinContext(0, stream=handle)
        self.ctx.reserve("prj", NR, max(M1, M2), keepRowIds=True, trackRMatches=True)
        self.st = st = so.Stage(stream)
        rng = np.random.default_rng(seed + 1)
        self.bR = st.buf(d.Rd, real=d.R, warm=d.Rw)
        self.bS1 = st.buf(d.Sd[:M1], real=d.S[:M1], warm=d.Sw[:M1])
        self.bS2 = st.buf(d.Sd[M1:], real=d.S[M1:], warm=d.Sw[M1:])
        self.c1 = c1 = d.inner1.size
        self.pI = maps(st, c1)
        self.bAnti = st.out(d.anti2.size + SLACK, U32, NO_ROW)
        self.bMatched = st.out(NR, U32, so.SENT32)
        poison8 = np.full(NR, ac.POISON, dtype=U64)
        self.bPlain = st.buf(poison8, real=d.plain["src"], warm=np.roll(d.plain["src"].view(U64), 1))
        self.bNull = st.buf(np.full(NR, ac.POISON >> 32, dtype=U32), real=d.nullable["src"], warm=np.roll(d.nullable["src"].view(U32), 1))
        wv = plane_words(d.nullable["valid"])
        self.bNullV = st.buf(np.zeros(wv.size, dtype=U32), real=wv, warm=wv)
        self.sR, self.sS = stage_strings(st, d.str_r, rng), stage_strings(st, d.str_s, rng)
        # R's columns are gathered through the whole R plane, the SLACK words behind the pairs included: they keep the
        # HJ_NO_ROW prefill, so the call has NULL rows and leaves non-zero counters for the next call to clear in stream order
        self.g1 = g1 = c1 + SLACK
        words = (g1 + 31) // 32
        self.oPlain, self.oNull = st.out(g1, U64, so.SENT64), st.out(g1, U32, so.SENT32)
        self.oNullV, self.oRowV = st.out(words, U32, so.SENT32), st.out(words, U32, so.SENT32)
        self.oStrR, self.oStrROff, self.oStrRV = st.out(d.bytes_r, np.uint8, so.SENT_BYTE), st.out(g1 + 1, U32, so.SENT32), st.out(words, U32, so.SENT32)
        self.oStrS, self.oStrSOff = st.out(d.bytes_s, np.uint8, so.SENT_BYTE), st.out(c1 + 1, U32, so.SENT32)

    def close(self):
        self.ctx.close()

    def steps(self):
        """the calls of the sequence, one closure each"""
        ctx, h, d, c1 = self.ctx, self.ctx._h, self.d, self.c1

        def gather_r():
            cols = g2_cols([dict(src=self.bPlain.ptr, dst=self.oPlain.ptr, width=8, fill=d.plain["fill"]),
                            dict(src=self.bNull.ptr, dst=self.oNull.ptr, width=4, fill=d.nullable["fill"], src_valid=self.bNullV.ptr, dst_valid=self.oNullV.ptr),
                            dict(src=self.sR[0].ptr, dst=self.oStrR.ptr, src_offsets=self.sR[1].ptr, dst_offsets=self.oStrROff.ptr,
                                 src_valid=self.sR[2].ptr, dst_valid=self.oStrRV.ptr, dst_capacity=d.bytes_r)])
            ok(ctx, lib.hj_gather2_dev(h, vp(self.pI[1].ptr), self.g1, 0, NR, cols, 3, vp(self.oRowV.ptr)))
            zero(cols)

        def gather_s():
            cols = g2_cols([dict(src=self.sS[0].ptr, dst=self.oStrS.ptr, src_offsets=self.sS[1].ptr, dst_offsets=self.oStrSOff.ptr, dst_capacity=d.bytes_s)])
            ok(ctx, lib.hj_gather2_dev(h, vp(self.pI[0].ptr), c1, 0, M1, cols, 1, None))
            zero(cols)

        return [lambda: ok(ctx, lib.hj_prj_build_dev(h, vp(self.bR.ptr), NR)),
                lambda: ok(ctx, lib.hj_prj_probe_dev(h, vp(self.bS1.ptr), M1)),
                lambda: ok(ctx, lib.hj_prj_probe_dev(h, vp(self.bS2.ptr), M2)),
                lambda: ok(ctx, lib.hj_prj_probe_pairs_dev(h, vp(self.bS1.ptr), M1, 0, vp(self.pI[0].ptr), vp(self.pI[1].ptr), c1 + SLACK)),
                lambda: ok(ctx, lib.hj_prj_probe_join_dev(h, ANTI, vp(self.bS2.ptr), M2, M1, vp(self.bAnti.ptr), None, d.anti2.size + SLACK)),
                lambda: ok(ctx, lib.hj_r_rows_dev(h, 1, vp(self.bMatched.ptr), NR)),
                gather_r, gather_s]

    def check(self, tag):
        d, st, c1 = self.d, self.st, self.c1
        got = self.ctx.fetch()
        both = d.inner1.size + d.inner2.size
        assert (got["totalMatches"], got["sSize"], got["rSize"]) == (2 * both, 2 * (M1 + M2), NR), (tag, got)
        s, r = map_rows(st, self.pI[0], c1, tag), map_rows(st, self.pI[1], c1, tag)
        assert np.array_equal(np.sort(packed(s, r)), d.inner1), (tag, "inner pairs")
        assert np.array_equal(np.sort(map_rows(st, self.bAnti, d.anti2.size, tag)).astype(U64), d.anti2), (tag, "anti rows")
        matched = st.result(self.bMatched, U32, tag)
        assert np.array_equal(matched[:d.matched.size].astype(U64), d.matched) and (matched[d.matched.size:] == so.SENT32).all(), (tag, "r_rows")
        # the gathers, by the models of test_gpu_gather2.py over the map as it was written (its multiset is exact, above)
        g1 = self.g1
        i, null, _oor, has = rows_of(np.concatenate([r, np.full(SLACK, NO_ROW, dtype=U32)]), 0, NR)
        assert has[:c1].all() and null[c1:].all() and np.array_equal(st.result(self.oRowV, U32, tag), plane_words(has)), (tag, "dValid")
        el, raw, _ = want_of(d.plain, i, has, g1)
        assert st.result(self.oPlain, np.uint8, tag).tobytes() == raw, (tag, "plain column")
        el, raw, _ = want_of(d.nullable, i, has, g1)
        assert st.result(self.oNull, np.uint8, tag).tobytes() == raw, (tag, "nullable column")
        assert np.array_equal(st.result(self.oNullV, U32, tag), plane_words(el)), (tag, "nullable column, dstValid")
        el, raw, off = want_of(d.str_r, i, has, g1)
        assert len(raw) == d.bytes_r and st.result(self.oStrR, np.uint8, tag).tobytes() == raw, (tag, "string column of R")
        assert np.array_equal(st.result(self.oStrROff, U32, tag).astype(np.int64), off), (tag, "string column of R, offsets")
        assert np.array_equal(st.result(self.oStrRV, U32, tag), plane_words(el)), (tag, "string column of R, dstValid")
        i, _null, _oor, has = rows_of(s, 0, M1)
        el, raw, off = want_of(d.str_s, i, has, c1)
        assert len(raw) == d.bytes_s and st.result(self.oStrS, np.uint8, tag).tobytes() == raw, (tag, "string column of S")
        assert np.array_equal(st.result(self.oStrSOff, U32, tag).astype(np.int64), off), (tag, "string column of S, offsets")
        # the counters of the LAST gather2 alone: each call clears them on the stream, behind the call before
        info = self.ctx.gather2_info()
        assert info[:2] == (c1, 0) and info[3:] == (0, d.bytes_s) + (0,) * 7, (tag, "gather2_info", info)
        st.check_inputs_intact(tag)


def test_c_resident_radix_join(fl):
    c = Resident(fl.handle, fl.stream, 11)
    try:
        so.run_delayed([c.st], lambda which: [step() for step in c.steps()], all_async(*Resident.CALLS), f"c.resident.{fl.name}")
        c.check("c")
    finally:
        c.close()


# ---------------------------------------------------------------------------------------------------------------------
# g. two contexts live at once: on two delayed streams, interleaved call by call; and on one stream, as bench.py has them
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("streams", ["two streams", "one stream"])
def test_g_two_contexts_interleaved(fl, streams):
    other = so.Flavour("side") if streams == "two streams" else fl
    a, b = Resident(fl.handle, fl.stream, 21), Resident(other.handle, other.stream, 22)
    assert not np.array_equal(a.d.R, b.d.R) and not np.array_equal(a.d.S, b.d.S)
    try:
        def seq(which):
            for step_a, step_b in zip(a.steps(), b.steps()):
                step_a()
                step_b()

        so.run_delayed([a.st, b.st], seq, all_async(*Resident.CALLS), f"g.{streams.replace(' ', '_')}.{fl.name}")
        a.check(("g", streams, "first context"))
        b.check(("g", streams, "second context"))
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------------------------------------------------------------
# d. fused aggregation, then the reduction over the pairs
# ---------------------------------------------------------------------------------------------------------------------
def test_d_aggregating_joins(fl):
    """prj_agg_begin (4 columns, one nullable) -> prj_probe_agg x 2 -> prj_agg_rows; prj_agg_begin again (2 columns) -> one probe
    -> rows into other planes; then pairs_agg over the pairs of the first slice, with a count plane"""
    d = resident_data(11)
    rng = np.random.default_rng(3)
    ns = M1 + M2
    cols = [ac.Col(ac.SUM, rng.integers(-(1 << 62), 1 << 62, ns, dtype=np.int64)),
            ac.Col(ac.MAX, rng.integers(0, 1 << 32, ns, dtype=np.int64).astype(U32), valid=rng.random(ns) < 0.6),
            ac.Col(ac.MIN, rng.integers(0, 1 << 63, ns, dtype=np.int64).view(U64)),
            ac.Col(ac.COUNT)]
    cols2 = [cols[0], ac.Col(ac.COUNT)]
    want = ac.expected_join(NR, np.concatenate([d.inner1, d.inner2]), cols)
    want2 = ac.expected_join(NR, d.inner1, cols2)
    want_pairs = ac.expected_join(NR, d.inner1, [cols[0]])
    c1 = d.inner1.size
    with hj.HashJoinContext(0, stream=fl.handle) as ctx:
        h = ctx._h
        ctx.reserve("prj", NR, max(M1, M2), keepRowIds=True)
        st = so.Stage(fl.stream)
        bR = st.buf(d.Rd, real=d.R, warm=d.Rw)
        bS = [st.buf(d.Sd[:M1], real=d.S[:M1], warm=d.Sw[:M1]), st.buf(d.Sd[M1:], real=d.S[M1:], warm=d.Sw[M1:])]
        src = []                                # per slice, per column: (values, validity) buffers
        for lo, n in ((0, M1), (M1, M2)):
            row = []
            for c in cols:
                bv = bw = None
                if c.op != ac.COUNT:
                    v = np.ascontiguousarray(c.poisoned()[lo:lo + n])
                    bv = st.buf(np.full(n, ac.POISON >> (64 - 8 * c.width), dtype=v.dtype), real=v, warm=np.roll(v, 1))
                if c.valid is not None:
                    w = c.words(lo, n)
                    bw = st.buf(np.zeros(w.size, dtype=U32), real=w, warm=w)
                row.append((bv, bw))
            src.append(row)
        out = [st.out(NR, U64, so.SENT64) for _ in cols]
        out_count = st.out(NR, U64, so.SENT64)
        out2 = [st.out(NR, U64, so.SENT64) for _ in cols2]
        out2_count = st.out(NR, U64, so.SENT64)
        pI = maps(st, c1)
        zeros = np.zeros(NR, dtype=U64)                                 # the caller initialises: SUM and the count start at 0
        acc = st.buf(np.full(NR, so.SENT64, dtype=U64), real=zeros, warm=zeros, fetch=True)
        acc_count = st.buf(np.full(NR, so.SENT64, dtype=U64), real=zeros, warm=zeros, fetch=True)

        def begin(cc):
            specs = (_lib.hj_agg_spec * len(cc))()
            for a, c in zip(specs, cc):
                a.op, a.width, a.flags = c.spec
            ok(ctx, lib.hj_prj_agg_begin(h, specs, len(cc)))
            zero(specs)

        def probe(k, which_cols):
            srcs = (_lib.hj_agg_src * len(which_cols))()
            for a, j in zip(srcs, which_cols):
                bv, bw = src[k][j]
                a.src, a.srcValid = (bv.ptr if bv else None), (bw.ptr if bw else None)
            ok(ctx, lib.hj_prj_probe_agg_dev(h, vp(bS[k].ptr), (M1, M2)[k], srcs, len(which_cols)))
            zero(srcs)

        def rows(planes, count):
            ptrs = (C.c_void_p * len(planes))(*[p.ptr for p in planes])
            ok(ctx, lib.hj_prj_agg_rows_dev(h, ptrs, vp(count.ptr)))
            zero(ptrs)

        def pairs_agg():
            col = (_lib.hj_agg_col * 1)()
            col[0].src, col[0].acc = src[0][0][0].ptr, acc.ptr
            col[0].op, col[0].width, col[0].flags = cols[0].spec
            ok(ctx, lib.hj_pairs_agg_dev(h, vp(pI[1].ptr), vp(pI[0].ptr), c1, 0, NR, 0, M1, col, 1, vp(acc_count.ptr)))
            zero(col)

        def seq(which):
            ok(ctx, lib.hj_prj_build_dev(h, vp(bR.ptr), NR))
            begin(cols)
            probe(0, range(4))
            probe(1, range(4))
            rows(out, out_count)
            begin(cols2)
            probe(0, (0, 3))
            rows(out2, out2_count)
            ok(ctx, lib.hj_prj_probe_pairs_dev(h, vp(bS[0].ptr), M1, 0, vp(pI[0].ptr), vp(pI[1].ptr), c1 + SLACK))
            pairs_agg()

        so.run_delayed([st], seq, all_async("hj_prj_build_dev", "hj_prj_agg_begin", "hj_prj_probe_agg_dev", "hj_prj_agg_rows_dev",
                                            "hj_prj_probe_pairs_dev", "hj_pairs_agg_dev"), f"d.aggregation.{fl.name}")
        st.check_inputs_intact()
    for name, planes, count, (want_count, want_planes), cc in (("first", out, out_count, want, cols), ("second", out2, out2_count, want2, cols2),
                                                              ("pairs", [acc], acc_count, want_pairs, [cols[0]])):
        got_count = st.result(count, U64, name)
        assert np.array_equal(got_count, want_count), (name, "count", np.flatnonzero(got_count != want_count)[:8])
        for i, (p, w) in enumerate(zip(planes, want_planes)):
            g = st.result(p, U64, name)
            assert np.array_equal(g, w), (name, "column", i, cc[i].spec, np.flatnonzero(g != w)[:8])
    s, r = map_rows(st, pI[0], c1, "d"), map_rows(st, pI[1], c1, "d")
    assert np.array_equal(np.sort(packed(s, r)), d.inner1)


# ---------------------------------------------------------------------------------------------------------------------
# e. key columns: hash2 -> prj_build -> prj_probe_pairs -> verify2 -> gather2 of the string key
# ---------------------------------------------------------------------------------------------------------------------
KR, KS, POOL = 3001, 4003, 1200
KEY_MASK = 0xFF                  # 256 join words for thousands of rows: the verify step has something to reject


def arrow(c):
    """a keys2_common.ModelCol as numpy buffers: (values or bytes, uint32 offsets or None, validity words or None)"""
    valid = np.array([e is not None for e in c.items], dtype=bool)
    words = None if valid.all() else plane_words(valid)
    if c.width:
        raw = b"".join(b"\xA5" * c.width if e is None else e for e in c.items)
        return np.frombuffer(raw, dtype=np.uint8).copy(), None, words
    lens = [0 if e is None else len(e) for e in c.items]
    off = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(U32)
    data = np.frombuffer(b"".join(e or b"" for e in c.items) + b"\xEE" * 4, dtype=np.uint8).copy()
    return data, off, words


@functools.lru_cache(maxsize=None)
def key_data():
    rng = np.random.default_rng(77)
    d = types.SimpleNamespace()
    pool_s = [rng.integers(0, 256, k2.LENGTHS[(k * 7 + 3) % len(k2.LENGTHS)], dtype=np.uint8).tobytes() for k in range(POOL + 300)]
    pool_i = [rng.integers(0, 256, 8, dtype=np.uint8).tobytes() for _ in range(POOL + 300)]

    def side(n, hi):
        pick = rng.integers(0, hi, n)
        gone = rng.random(n) < 0.1
        return [k2.ModelCol(0, [None if g else pool_s[p] for p, g in zip(pick, gone)], True),      # a NULL string equals a NULL string
                k2.ModelCol(8, [pool_i[p] for p in pick], False)]

    d.r, d.s = side(KR, POOL), side(KS, POOL + 300)
    words_r, words_s = k2.model_words(d.r, KEY_MASK), k2.model_words(d.s, KEY_MASK)
    d.cand = join_expected(words_r, words_s, any_key=True)              # the candidate pairs: equal join words
    kept = k2.inner_pairs(k2.row_keys(d.r), k2.row_keys(d.s))
    d.kept = np.sort(np.array([(s << 32) | r for s, r in kept], dtype=U64))
    assert 0 < d.kept.size < d.cand.size // 4, (d.kept.size, d.cand.size)
    d.words_r, d.words_s = words_r, words_s
    return d


def test_e_key_columns(fl):
    d = key_data()
    rng = np.random.default_rng(9)
    n_cand, n_kept = d.cand.size, d.kept.size
    with hj.HashJoinContext(0, stream=fl.handle) as ctx:
        h = ctx._h
        ctx.reserve("prj", KR, KS, keepRowIds=True)
        st = so.Stage(fl.stream)
        staged = {}
        for name, side in (("r", d.r), ("s", d.s)):
            data, off, words = arrow(side[0])
            bD = st.buf(rng.integers(0, 256, data.size, dtype=np.uint8), real=data, warm=rng.integers(0, 256, data.size, dtype=np.uint8))
            bO = st.buf(np.zeros(off.size, dtype=U32), real=off, warm=off)
            bV = st.buf(np.zeros(words.size, dtype=U32), real=words, warm=words)
            ints, _, _ = arrow(side[1])
            bI = st.buf(np.full(ints.size // 8, ac.POISON, dtype=U64), real=ints, warm=np.roll(ints, 8))
            staged[name] = (bD, bO, bV, bI)
        # the hashed tuples: written by hash2, read by the radix join. Before the delay: keys outside the mask, R's and S's apart
        tR = st.buf(np.full(KR, 0x1000, dtype=U64), fetch=True)
        tS = st.buf(np.full(KS, 0x2000, dtype=U64), fetch=True)
        pC, pK = maps(st, n_cand), maps(st, n_kept)
        str_s = dict(width=0, offsets=arrow(d.s[0])[1].astype(np.int64), data=arrow(d.s[0])[0],
                     valid=np.array([e is not None for e in d.s[0].items]))
        i_kept = (d.kept >> U64(32)).astype(np.int64)
        total = int((str_s["offsets"][i_kept + 1] - str_s["offsets"][i_kept]).sum())                # a NULL's range is empty
        oStr, oOff, oValid = st.out(total, np.uint8, so.SENT_BYTE), st.out(n_kept + 1, U32, so.SENT32), st.out((n_kept + 31) // 32, U32, so.SENT32)

        def key_cols():
            arr = (_lib.hj_key_col2 * 2)()
            (sD, sO, sV, sI), (rD, rO, rV, rI) = staged["s"], staged["r"]
            arr[0].s, arr[0].r, arr[0].sOffsets, arr[0].rOffsets, arr[0].sValid, arr[0].rValid = sD.ptr, rD.ptr, sO.ptr, rO.ptr, sV.ptr, rV.ptr
            arr[0].width, arr[0].flags = 0, _lib.HJ_KEY_NULLS_EQUAL
            arr[1].s, arr[1].r, arr[1].width, arr[1].flags = sI.ptr, rI.ptr, 8, 0
            return arr

        def seq(which):
            for side, n, out in ((_lib.HJ_KEY_SIDE_R, KR, tR), (_lib.HJ_KEY_SIDE_S, KS, tS)):
                cols = key_cols()
                ok(ctx, lib.hj_key_hash2_dev(h, cols, 2, side, n, KEY_MASK, vp(out.ptr)))
                zero(cols)
            ok(ctx, lib.hj_prj_build_dev(h, vp(tR.ptr), KR))
            ok(ctx, lib.hj_prj_probe_pairs_dev(h, vp(tS.ptr), KS, 0, vp(pC[0].ptr), vp(pC[1].ptr), n_cand + SLACK))
            cols = key_cols()
            ok(ctx, lib.hj_pairs_verify2_dev(h, vp(pC[0].ptr), vp(pC[1].ptr), n_cand, 0, KS, KR, cols, 2, vp(pK[0].ptr), vp(pK[1].ptr),
                                             n_kept + SLACK, None, None))
            zero(cols)
            g = g2_cols([dict(src=staged["s"][0].ptr, dst=oStr.ptr, src_offsets=staged["s"][1].ptr, dst_offsets=oOff.ptr,
                              src_valid=staged["s"][2].ptr, dst_valid=oValid.ptr, dst_capacity=total)])
            ok(ctx, lib.hj_gather2_dev(h, vp(pK[0].ptr), n_kept, 0, KS, g, 1, None))
            zero(g)

        so.run_delayed([st], seq, all_async("hj_key_hash2_dev", "hj_prj_build_dev", "hj_prj_probe_pairs_dev", "hj_pairs_verify2_dev", "hj_gather2_dev"),
                       f"e.key_columns.{fl.name}")
        st.check_inputs_intact()
    assert np.array_equal(st.result(tR, U64, "hash R"), d.words_r) and np.array_equal(st.result(tS, U64, "hash S"), d.words_s)
    s, r = map_rows(st, pC[0], n_cand, "candidates"), map_rows(st, pC[1], n_cand, "candidates")
    assert np.array_equal(np.sort(packed(s, r)), d.cand)
    s, r = map_rows(st, pK[0], n_kept, "kept"), map_rows(st, pK[1], n_kept, "kept")
    assert np.array_equal(np.sort(packed(s, r)), d.kept)
    i, _null, _oor, has = rows_of(s, 0, KS)
    el, raw, off = want_of(str_s, i, has, n_kept)
    assert len(raw) == total and st.result(oStr, np.uint8, "string key").tobytes() == raw
    assert np.array_equal(st.result(oOff, U32, "string key").astype(np.int64), off)
    assert np.array_equal(st.result(oValid, U32, "string key"), plane_words(el))


# ---------------------------------------------------------------------------------------------------------------------
# h. the Zipf stream
# ---------------------------------------------------------------------------------------------------------------------
def test_h_zipf_three_slices(fl):
    """hj_zipf_next_dev three times in a row: the third call waits, by design, for the event of the first (the pinned buffer
    pair is reused), so it blocks until the delay has run out -- correctness only, no pending() assertion. The warm-up's
    draws come first in the one rand() stream"""
    alphabet, theta, slices = 1 << 12, 0.9, (1001, 333, 2047)
    total = sum(slices)
    want = hj.generate_data("zipf", 2 * total, alphabet, 16, zipf_theta=theta)
    with hj.HashJoinContext(0, stream=fl.handle) as ctx:
        ctx.zipf_open(alphabet, theta, 0)
        st = so.Stage(fl.stream)
        out = st.out(total, U64, so.SENT64)

        def seq(which):
            off = 0
            for m in slices:
                ctx.zipf_next(m, out.ptr + 8 * off)
                off += m

        so.run_delayed([st], seq, False, f"h.zipf.{fl.name}")           # the third hj_zipf_next_dev waits for the first
        ctx.zipf_close()
    assert np.array_equal(st.result(out, U64, "zipf"), want[total:])


# ---------------------------------------------------------------------------------------------------------------------
# i. timing on a caller's stream: the probe's time is its own
# ---------------------------------------------------------------------------------------------------------------------
def test_i_probe_time_on_a_callers_stream(fl):
    """build, a second delay of known length D2, probe: on a caller's stream hj_probe_dev records the start of its own time
    (EV_PROBE0), so probe_us does not span the second delay. The probe of 2^15 tuples takes microseconds; D2 / 2 is far above
    it and far below build-end to probe-end"""
    n, ns = 1 << 15, (1 << 15) - 1
    R = hj.generate_data("local_shuffle", n, n, 16)
    rng = np.random.default_rng(1)
    S = rng.integers(1, n + 1, ns).astype(U64)
    want = inner_expected("atomic", R, S, PROBE).size
    d2_ms = so.DELAY_MS
    with hj.HashJoinContext(0, stream=fl.handle) as ctx:
        ctx.reserve("atomic", n, ns, probeLength=PROBE)
        st = so.Stage(fl.stream)
        bR = st.buf(R + U64(2 * n), real=R, warm=np.roll(R, 5))
        bS = st.buf(S + U64(4 * n), real=S, warm=np.roll(S, 5))
        st.arm()
        st.load("warm")
        ctx.build(bR.ptr, n)
        ctx.probe(bS.ptr, ns)
        fl.stream.synchronize()
        st.arm()
        try:
            first = so.Delayed(fl.stream)
            st.load("real")
            ctx.build(bR.ptr, n)
            second = so.Delayed(fl.stream, d2_ms)
            ctx.probe(bS.ptr, ns)
            still = first.pending() and second.pending()
        finally:
            fl.stream.synchronize()
        got = ctx.fetch()
    print("probe_us", got["probe_us"], "build_us", got["build_us"], "D2 us", d2_ms * 1e3)
    assert still, "the delays had run out before the probe was enqueued"
    assert got["totalMatches"] == want
    assert 0 < got["probe_us"] < d2_ms * 1e3 / 2, got["probe_us"]
    assert got["build_us"] > 0, got["build_us"]
