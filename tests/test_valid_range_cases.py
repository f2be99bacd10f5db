"""The builders of valid_range_cases.py, checked on the CPU: what test_gpu_valid_range.py takes for granted about its own
inputs -- band and poison tile the table, the oracle's table of R is empty outside the band's reach, no poison key joins
with R, and the interior / whole / control label of every case follows from where the band lies."""
import numpy as np
import pytest

import r_marks_common as rm
import valid_range_cases as vc
from oracle import oracle

U64 = np.uint64
N = 1 << 12                    # the arithmetic does not depend on the size; the device tests use 2^16 and 2^18
T = 2 * N

GEOMETRIES = {"oa": dict(), "oa_shift3": dict(shift=3), "htm": dict(htm=True)}


def bands(geo, n=N):
    T = vc.htm_table(n) if geo == "htm" else 2 * n
    for name, (a, copies) in vc.placements(T).items():
        yield name, vc.band_relation(n, T, a, copies=copies, shuffle=16, **GEOMETRIES[geo])


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_band_and_poison_homes_tile_the_table(geo):
    for name, band in bands(geo):
        T = band.table
        h = vc.homes(band.R, T, band.shift, band.htm).astype(np.int64)
        inside = ((h - band.lo) % T) < (band.hi_ex - band.lo)
        assert inside.all(), (geo, name)
        assert np.array_equal(vc.homes(band.twins, T, band.shift, band.htm), vc.homes(band.twins - U64(4 * band.period), T, band.shift, band.htm))
        assert not np.isin(band.twins, band.R).any(), (geo, name)
        for order in ("perm", "sorted"):
            P = vc.poison_for(band, order, chains=False)
            assert np.unique(P).size == P.size and not np.isin(P, band.R).any() and not np.isin(P, band.twins).any(), (geo, name)
            hp = vc.homes(P, T, band.shift, band.htm).astype(np.int64)
            step = 4 if band.htm else 1
            band_homes = np.arange(band.lo, band.hi_ex, step, dtype=np.int64) % T
            assert np.intersect1d(hp, band_homes).size == 0, (geo, name, order)
            # together they cover the table exactly: every slot (htm: every bucket) outside the band is some poison key's home
            assert np.array_equal(np.sort(np.concatenate([hp, band_homes])), np.arange(0, T, step)), (geo, name, order)
            assert np.array_equal(np.sort(P), np.sort(vc.poison_for(band, "perm", chains=False))), (geo, name)
        if order == "sorted":
            assert (np.diff(P.astype(np.int64)) > 0).all()


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_cross_geometry_poison_stays_outside_the_band(geo):
    """an htm poison under an open-addressing band and the other way round: whole buckets / slots outside, none inside"""
    for name, band in bands(geo):
        P = vc.poison_for(band, "perm", htm=not band.htm, chains=False)
        hp = vc.homes(P, band.table, 0, not band.htm).astype(np.int64)
        width = 4 if not band.htm else 1                    # an htm poison key occupies its whole bucket
        for off in range(width):
            assert ((((hp + off) - band.lo) % band.table) >= band.hi_ex - band.lo).all(), (geo, name)
        assert hp.size >= (band.table - (band.hi_ex - band.lo)) // (4 if not band.htm else 1) - 2, (geo, name)


def test_htm_chain_poison_sizes_the_same_table_and_overflows():
    for name, band in bands("htm"):
        P = vc.poison_for(band, "perm")
        assert vc.htm_table(P.size) == band.table, name
        res = oracle.htm_build_probe_seq(P, None)
        assert res["overflowBuckets"] > 0 and res["numBuckets"] == band.table // 4, (name, res)


@pytest.mark.parametrize("geo", GEOMETRIES)
@pytest.mark.parametrize("probe", (4, 8))
def test_oracle_table_of_r_is_empty_outside_the_bands_reach(geo, probe):
    for name, band in bands(geo):
        T = band.table
        want = vc.expected(band, None, probe)
        if band.htm:
            occupied = 4 * np.nonzero(want["buckets"]["count"])[0]
            reach = band.hi_ex - band.lo
        else:
            occupied = np.nonzero(want["table"])[0]
            reach = band.hi_ex - band.lo + probe
        assert occupied.size and (((occupied - band.lo) % T) < reach).all(), (geo, name, probe)


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_no_poison_key_and_no_twin_joins_with_r(geo):
    for name, band in bands(geo):
        P = vc.poison_for(band, "perm")
        lo, hi_ex = (band.lo // vc.BLOCK) * vc.BLOCK, min(band.table, (band.hi_ex // vc.BLOCK + 2) * vc.BLOCK)
        S = vc.probe_side(band, P, lo, hi_ex, key32=bool(band.shift))
        assert S.size >= band.R.size + P.size + band.twins.size
        strangers = np.concatenate([P, band.twins])
        assert vc.expected(band, strangers)["totalMatches"] == 0, (geo, name)
        full, alone = vc.expected(band, S), vc.expected(band, band.R)
        # the edge keys may be members; everything else the probe side adds matches nothing
        edges = vc.keys_homed_at(band, vc.edge_slots(lo, hi_ex, band.table))
        assert full["totalMatches"] == alone["totalMatches"] + vc.expected(band, edges)["totalMatches"], (geo, name)


@pytest.mark.parametrize("geo", ("oa", "htm"))
def test_the_numpy_pair_references_agree_with_the_oracle(geo):
    """r_marks_common's references give the pairs; their count must be the oracle's totalMatches on the same inputs,
    tuples outside the DataGen layout included"""
    for name, band in bands(geo, 1 << 10):
        P = vc.poison_for(band, "perm")
        S = vc.probe_side(band, P, band.lo, min(band.hi_ex, band.table))
        inner = rm.inner_expected("htm" if band.htm else "atomic", band.R, S, 4)
        assert inner.size == vc.expected(band, S)["totalMatches"], (geo, name)


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_classification_follows_from_the_placement(geo):
    for n in (1 << 16, 1 << 18):
        T = vc.htm_table(n) if geo == "htm" else 2 * n
        assert T == 2 * n
        want = {"control": "control", "mid": "interior", "below": "interior", "above": "interior", "straddle": "whole"}
        for name, (a, copies) in vc.placements(T).items():
            band = vc.band_relation(n, T, a, copies=copies, **GEOMETRIES[geo])
            assert vc.classify(band) == want[name], (geo, n, name, band.lo, band.hi_ex)
            if name == "mid":
                assert band.lo < T // 2 < band.hi_ex
            if name == "below":
                assert band.hi_ex + vc.MARGIN <= T // 2
            if name == "above":
                assert band.lo >= T // 2 + vc.MARGIN
            if name == "straddle":
                assert band.hi_ex > T
        slots = vc.band_slots(n, 1, geo == "htm")
        tops, labels = [], []
        for a in vc.top_sweep(T, slots):
            band = vc.band_relation(n, T, a, **GEOMETRIES[geo])
            tops.append((T - band.hi_ex) // vc.BLOCK)
            labels.append(vc.classify(band))
            assert band.lo >= vc.MARGIN, (geo, n, a)
        assert tops == [5, 4, 3, 2, 1, 0], (geo, n, tops)             # one top in each of the last six blocks
        # three blocks of room: interior whatever the build; the last block: whole; between them the build's rounding decides
        assert labels == ["interior", "interior", "interior", "device", "device", "whole"], (geo, n, labels)
        for k, a in enumerate(vc.bottom_sweep()):
            band = vc.band_relation(n, T, a, **GEOMETRIES[geo])
            assert band.lo // vc.BLOCK == k and band.hi_ex + vc.MARGIN <= T, (geo, n, a)
            assert vc.classify(band) == ("control" if k == 0 else "device"), (geo, n, a)


def test_classification_is_sharp_at_the_upper_edge():
    """top = one past the last slot a tuple can land on: top + 1536 <= table is interior, hi_ex + 512 >= table is whole"""
    n, T = 1 << 16, 1 << 17
    for probe in (4, 8):
        a = T - (vc.REACH_UP + vc.BLOCK) - (probe - 1) - n                  # top + 1536 == T
        assert vc.classify(vc.band_relation(n, T, a), probe) == "interior"
        assert vc.classify(vc.band_relation(n, T, a + 1), probe) == "device"
    assert vc.classify(vc.band_relation(n, T, T - vc.BLOCK - n - 1)) == "device"
    assert vc.classify(vc.band_relation(n, T, T - vc.BLOCK - n)) == "whole"
