"""PRJ with a resident R: hj_prj_build_dev partitions R once, hj_prj_probe_dev joins S slice by slice against it
(skew-split join, k_prj_probe_items), hj_prj_resident_info reports paths and work items. Checked against the CPU oracle
(oracle.prj_join: the fork's PRO, oracle.true_cardinality: the join cardinality)."""
import ctypes

import numpy as np
import pytest

import htm_hashjoin_amd as hj
from htm_hashjoin_amd import _lib
from oracle import oracle

from gpu_harness import alloc, ctx_per_test  # noqa: F401  (every test of this file starts on a context of its own)

pytestmark = pytest.mark.gpu

ITEM_S = 1 << 16          # kPrjItemS: S tuples per join work item at most


@pytest.fixture(scope="module")
def zipf_s():
    """2^24 Zipf(0.9) draws over 2^22 keys (generated once: the host generator takes seconds)"""
    return hj.generate_data("zipf", 1 << 24, 1 << 22, 16, zipf_theta=0.9)


def upload(c, a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    d = alloc(c, max(a.size, 1) * 8)
    c.copy_h2d(d, a)
    return d


def ragged(n, k):
    """k slice lengths that add up to n, all different (k = 1: one slice)"""
    if k == 1:
        return [n]
    w = np.arange(1, k + 1, dtype=np.float64)
    cuts = np.floor(np.cumsum(w) / w.sum() * n).astype(np.int64)
    return [int(x) for x in np.diff(np.concatenate([[0], cuts]))]


def build_and_probe(c, dR, nR, S, slices, **kw):
    """reserve for the largest slice, build, probe every slice; returns (result after the build, result at the end)"""
    lens = ragged(S.size, slices)
    c.reserve("prj", nR, max(lens), **kw)
    c.prj_build(dR, nR)
    after_build = c.fetch()
    dS = alloc(c, max(lens) * 8)
    off = 0
    for m in lens:
        c.copy_h2d(dS, S[off:off + m])
        c.prj_probe(dS, m)
        off += m
    got = c.fetch()
    c.dev_free(dS)
    return after_build, got


def r_qualifies(n, bits, mode):
    """hj_prj_fragment_info: R's histogram-free passes are planned at all"""
    out = (ctypes.c_uint64 * 13)()
    assert hj.lib.hj_prj_fragment_info(n, 0, bits, mode, out) == 0
    return out[1] != 0


CASES = [(dist, bits, mode) for dist in ("shuffle", "local_shuffle", "uniform") for bits in (14, 15, 16) for mode in (1, 2)]


@pytest.mark.parametrize("dist,bits,mode", CASES)
def test_batches_equal_one_shot(ctx, dist, bits, mode):
    n = 1 << (22 + CASES.index((dist, bits, mode)) % 3)
    R = hj.generate_data(dist, n, n, 1024)
    S = hj.generate_data("uniform", n + n // 2 + 12345, n, 16)
    want = oracle.prj_join(R, S, bits)
    want_r = oracle.prj_join(R, None, bits)
    dR = upload(ctx, R)
    for slices in (1, 3, 7):
        b, got = build_and_probe(ctx, dR, n, S, slices, radixBits=bits, prjMode=mode)
        assert (b["totalMatches"], b["prjChecksum"], b["sSize"]) == (0, want_r["checksum"], 0), (slices, b)
        assert b["radixBits"] == bits and b["prjPartitions"] == 1 << bits
        assert got["totalMatches"] == want["matches"], (slices, got["totalMatches"], want["matches"])
        assert got["prjChecksum"] == want["checksum"] and got["sSize"] == S.size, (slices, got)
        if not r_qualifies(n, bits, mode):
            assert got["prjPath"] == 0
        else:                                                   # dense keys never overflow a fragment
            assert got["prjPath"] in ((1,) if dist != "uniform" else (1, 2))
        info = ctx.prj_resident_info()
        assert info["rPath"] == got["prjPath"]
        assert info["items"] >= 1 and info["maxSPartition"] <= ITEM_S and info["splitPartitions"] == 0, info
    ctx.dev_free(dR)


@pytest.mark.parametrize("bits", (14, 16))
def test_zipf_skew_is_split(ctx, zipf_s, bits):
    n = 1 << 22
    R = hj.generate_data("shuffle", n)
    dR = upload(ctx, R)
    b, got = build_and_probe(ctx, dR, n, zipf_s, 1, radixBits=bits)
    assert got["totalMatches"] == zipf_s.size                   # R holds every key of the alphabet once
    assert got["prjChecksum"] == oracle.prj_join(R, None, bits)["checksum"]
    info = ctx.prj_resident_info()
    assert info["splitPartitions"] >= 1 and info["maxSPartition"] > ITEM_S, info
    assert info["items"] > info["splitPartitions"], info
    ctx.dev_free(dR)


def skewed_r(kind, n, reps):
    if kind == "nonunique":
        return hj.generate_relation("nonunique", n, n, seed=12345)
    rng = np.random.default_rng(7)
    R = np.concatenate([np.arange(1, n + 1, dtype=np.uint64), np.full(reps, 4097, dtype=np.uint64)])
    rng.shuffle(R)
    return R


@pytest.mark.parametrize("kind,reps", (("nonunique", 0), ("repeated", 30000), ("repeated", 70000)))
@pytest.mark.parametrize("bits", (14, 16))                     # hashed LDS table / DIRECT counters (radixBits >= 16)
def test_skewed_r(ctx, kind, reps, bits):
    n = 1 << 22
    R = skewed_r(kind, n, reps)
    S = hj.generate_relation("fk", 3 * n, n, seed=54321)
    S = np.concatenate([S, np.full(1000, 4097, dtype=np.uint64)])   # the repeated key on the S side too
    want = oracle.true_cardinality(R, S)
    dR = upload(ctx, R)
    _, got = build_and_probe(ctx, dR, R.size, S, 3, radixBits=bits)
    assert got["totalMatches"] == want, (kind, reps, bits, got["totalMatches"], want)
    assert got["prjChecksum"] == oracle.prj_join(R, None, bits)["checksum"]
    ctx.dev_free(dR)


def test_r_stays_resident_after_dr_is_overwritten_and_freed(ctx):
    n = 1 << 22
    R = hj.generate_data("shuffle", n)
    S = hj.generate_data("uniform", 2 * n, n, 16)
    want = oracle.prj_join(R, S, 14)
    dR = upload(ctx, R)
    ctx.reserve("prj", n, n, radixBits=14)
    ctx.prj_build(dR, n)
    ctx.copy_h2d(dR, np.full(n, 77, dtype=np.uint64))
    ctx.synchronize()
    ctx.dev_free(dR)
    dS = alloc(ctx, n * 8)
    for k in range(2):
        ctx.copy_h2d(dS, S[k * n:(k + 1) * n])
        ctx.prj_probe(dS, n)
    got = ctx.fetch()
    ctx.dev_free(dS)
    assert (got["totalMatches"], got["prjChecksum"], got["sSize"]) == (want["matches"], want["checksum"], 2 * n)


def expect_state(fn, *a):
    with pytest.raises(hj.HashJoinError) as e:
        fn(*a)
    assert e.value.status == _lib.HJ_ERR_STATE, e.value


def test_state_errors(ctx):
    n = 1 << 20
    R = hj.generate_data("shuffle", n)
    dR = upload(ctx, R)
    S = hj.generate_data("uniform", 2 * n, n, 16)
    dS = upload(ctx, S)
    ctx.reserve("prj", n, n)
    expect_state(ctx.prj_probe, dS, n)                          # before any build
    expect_state(ctx.prj_resident_info)
    ctx.prj_build(dR, n)
    expect_state(ctx.prj_probe, dS, n + 1)                      # larger than the reserved slice
    ctx.prj_probe(dS, 0)                                        # empty slice: a no-op
    r = ctx.fetch()
    assert (r["totalMatches"], r["sSize"]) == (0, 0)
    ctx.prj_probe(dS, n)
    ctx.prj_join(dR, n, dS, n)                                  # the one-shot join replaces the resident R
    expect_state(ctx.prj_probe, dS, n)
    ctx.prj_build(dR, n)
    ctx.reserve("atomic", n, n)
    ctx.build(dR, n)                                            # a table build does too
    expect_state(ctx.prj_probe, dS, n)
    ctx.reserve("prj", n, n)
    ctx.prj_build(dR, n)
    ctx.prj_probe(dS, n)
    ctx.reserve("prj", 2 * n, 2 * n)                            # grows the buffers
    expect_state(ctx.prj_probe, dS, n)
    ctx.prj_build(dR, n)                                        # ... and a new build is fine again
    ctx.prj_probe(dS, 2 * n)
    assert ctx.fetch()["totalMatches"] == oracle.prj_join(R, S, 14)["matches"]
    ctx.dev_free(dR); ctx.dev_free(dS)


def test_histogram_free_r_survives_a_falling_back_s(ctx, zipf_s):
    n = 1 << 22
    R = hj.generate_data("shuffle", n)
    U = hj.generate_data("uniform", 1 << 23, n, 16)
    dR = upload(ctx, R)
    ctx.reserve("prj", n, zipf_s.size, radixBits=14, prjMode=2)
    ctx.prj_build(dR, n)
    assert ctx.fetch()["prjPath"] == 1
    dS = alloc(ctx, zipf_s.size * 8)
    ctx.copy_h2d(dS, zipf_s)
    ctx.prj_probe(dS, zipf_s.size)                              # Zipf: S's histogram-free passes fall back
    info = ctx.prj_resident_info()
    assert (info["rPath"], info["sPath"]) == (1, 2), info
    assert ctx.fetch()["totalMatches"] == zipf_s.size
    ctx.copy_h2d(dS, U)
    ctx.prj_probe(dS, U.size)                                   # and a slice that keeps them: both layouts fragmented
    info = ctx.prj_resident_info()
    assert (info["rPath"], info["sPath"]) == (1, 1), info
    got = ctx.fetch()
    assert got["prjPath"] == 1
    assert got["totalMatches"] == zipf_s.size + oracle.prj_join(R, U, 14)["matches"]
    assert got["prjChecksum"] == oracle.prj_join(R, None, 14)["checksum"]
    ctx.dev_free(dR); ctx.dev_free(dS)


def test_config5_full_size_resident_prj():
    """BASELINE configs[4] through the resident radix join: |R| = 2^28 unique keys, 16 slices of 2^28 Zipf(0.9) draws
    (hj_zipf_next_dev) probed against R partitioned once: totalMatches = 2^32, as test_config5_skew_stress_full_size
    checks for the tables."""
    n, slices, per = 1 << 28, 16, 1 << 28
    R = hj.generate_data("local_shuffle", n, n, 1024)
    with hj.HashJoinContext(0) as c:
        dR = alloc(c, n * 8); c.copy_h2d(dR, R)
        del R
        dS = alloc(c, per * 8)
        c.reserve("prj", n, per)
        c.prj_build(dR, n)
        c.synchronize()
        c.dev_free(dR)
        c.zipf_open(n, 0.9, 0)
        split = 0
        for _ in range(slices):
            c.zipf_next(per, dS)
            c.prj_probe(dS, per)
            split = max(split, c.prj_resident_info()["splitPartitions"])
        c.zipf_close()
        r = c.fetch()
        c.dev_free(dS)
    assert (r["sSize"], r["totalMatches"]) == (slices * per, slices * per)
    assert r["radixBits"] == 14 and split >= 1                  # auto bits: 2^28 / 2^14 R tuples per partition
