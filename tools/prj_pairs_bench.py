#!/usr/bin/env python3
"""Times the materialising radix join against its two yardsticks on the same R and S, through the C ABI, no torch:
development tool.

    python tools/prj_pairs_bench.py [--log2n 27] [--reps 10] [--radix-bits 0] [--s sorted,uniform,zipf] [--yardsticks-only]
                                    [--how left,semi,anti] [--absent-half] [--track-r]

|R| = |S| = 2^log2n, R = the keys 1..n shuffled (unique), so every S tuple matches once. S = sorted, uniform draws, or
Zipf(theta) over n keys. Per S one JSON line with the median HIP-event times over `reps` launches after one warm-up of
  (a) hj_prj_probe_dev, R resident as bare keys (no flag)                     -> count_us (count_join_us: its join kernel)
  (b) htm build + hj_probe_pairs_dev: the only other way to the same pairs    -> htm_pairs_us
  (c) hj_prj_probe_pairs_dev, R resident as {key, row} (HJ_FLAG_KEEP_ROW_IDS) -> pairs_us (pairs_join_us: its join kernel)
and ratio_a = (c) / (a), ratio_b = (c) / (b), out_GBps = 8 B x pairs / (c), build_us of both resident forms.
--how: after (c), the same launches through hj_prj_probe_join_dev for each listed join kind -> <kind>_us, <kind>_rows and
<kind>_ratio = its median / (c)'s, (c) being the INNER join of the same process and input; (c) itself always goes through
hj_prj_probe_pairs_dev, the entry point older checkouts have. --absent-half: every second tuple of S gets n added to its
key, which R does not hold, so half of S is unmatched (and (a)'s and (c)'s pair counts halve).
--track-r: behind (c) and the kinds, R is built once more on a context reserved with HJ_FLAG_TRACK_R_MATCHES as well and
INNER (and LEFT, when --how lists it) is timed again -> track_<kind>_us (track_<kind>_join_us: its join kernel) and
track_<kind>_ratio = its median / the median of the same kind without the flag, timed just before in this process;
track_marked = R rows the marks then hold. On the sorted S without --absent-half it also times hj_r_rows_dev (HJ_R_MATCHED)
with a quarter, a half and all of R's rows marked -> sweep_<rows>_us, sweep_<rows>_GBps = (4 B x rows + 2 x the plane of
n / 8 B) / its median.
--yardsticks-only runs (a) and (b) alone and uses nothing newer than hj_prj_probe_dev / hj_probe_pairs_dev: the same
script times the yardsticks on a checkout that has no materialising radix join."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import htm_hashjoin_amd as hj  # noqa: E402
from htm_hashjoin_amd import _lib  # noqa: E402


def med(xs):
    return round(statistics.median(xs[1:]), 1)          # [0] is the warm-up launch


def track_r(c, a, row, dR, dS, n, dOutS, dOutR, kinds, sweep):
    """--track-r: INNER / LEFT on a tracking context against row's medians of the same kinds, then the sweep"""
    c.reserve("prj", n, n, radixBits=a.radix_bits, keepRowIds=True, trackRMatches=True)
    c.prj_build(dR, n)
    for how in ["inner"] + [k for k in kinds if k == "left"]:
        us, join_us = [], []
        for _ in range(a.reps + 1):
            c.r_marks_clear()                               # every launch meets clear bits and sets them: the atomics are timed
            c.prj_probe_pairs(dS, n, dOutS, dOutR, n, kind=_lib.JOIN_KINDS[how])
            found, written, t, _ = c.pairs_info()
            assert found == written <= n, (how, found, written)
            us.append(t); join_us.append(c.fetch()["join_us"])
        base = row["pairs_us" if how == "inner" else "left_us"]
        row.update({"track_" + how + "_us": med(us), "track_" + how + "_us_min": min(us[1:]), "track_" + how + "_join_us": med(join_us),
                    "track_" + how + "_ratio": round(med(us) / base, 3)})
    c.r_rows(_lib.HJ_R_MATCHED, 0, 0)
    row["track_marked"] = c.r_rows_info()[0]
    if not sweep:
        return
    for part in (4, 2, 1):                                  # sorted S, unique R: its first n / part tuples mark that many rows
        c.r_marks_clear()
        c.prj_probe_pairs(dS, n // part, 0, 0, 0)           # a mark-only pass
        us = []
        for _ in range(a.reps + 1):
            c.r_rows(_lib.HJ_R_MATCHED, dOutR, n)
            produced, written, t, _ = c.r_rows_info()
            assert produced == written, (produced, written)
            us.append(t)
        row.update({"sweep_%d_us" % produced: med(us), "sweep_%d_GBps" % produced: round((4.0 * produced + 2.0 * n / 8) / max(med(us), 1) / 1e3, 1)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--theta", type=float, default=0.9)
    ap.add_argument("--radix-bits", type=int, default=0)
    ap.add_argument("--s", default="sorted,uniform,zipf")
    ap.add_argument("--yardsticks-only", action="store_true")
    ap.add_argument("--no-htm", action="store_true", help="skip yardstick (b)")
    ap.add_argument("--tag", default="")
    ap.add_argument("--how", default="", help="comma list of left, semi, anti")
    ap.add_argument("--absent-half", action="store_true")
    ap.add_argument("--track-r", action="store_true", help="also time INNER / LEFT and the sweep with HJ_FLAG_TRACK_R_MATCHES")
    a = ap.parse_args()
    n = 1 << a.log2n
    kinds = [k for k in a.how.split(",") if k]
    want = n // 2 if a.absent_half else n               # pairs per probe
    with hj.HashJoinContext(0) as c:
        dR, dS = c.dev_alloc(n * 8), c.dev_alloc(n * 8)
        c.copy_h2d(dR, hj.generate_data("shuffle", n, n))
        dOutS, dOutR = c.dev_alloc(4 * n + 16), c.dev_alloc(4 * n + 16)
        for sname in a.s.split(","):
            if sname in ("sorted", "uniform"):
                S = (np.arange(1, n + 1, dtype=np.uint64) if sname == "sorted"
                     else np.random.default_rng(54321).integers(1, n + 1, size=n, dtype=np.uint64))
                if a.absent_half:
                    S[1::2] += np.uint64(n)
                c.copy_h2d(dS, S)
                del S
            else:
                c.zipf_open(n, a.theta, 54321)
                c.zipf_next(n, dS)
                c.zipf_close()
            c.synchronize()
            row = {"tag": a.tag, "S": sname, "log2n": a.log2n}
            # (a) the counting probe against bare keys
            c.reserve("prj", n, n, radixBits=a.radix_bits)
            c.prj_build(dR, n)
            row["count_build_us"] = round(c.fetch()["build_us"], 1)
            us, join_us = [], []
            for _ in range(a.reps + 1):
                c.prj_probe(dS, n)
                res = c.fetch()
                us.append(res["probe_us"]); join_us.append(res["join_us"])
            info = c.prj_resident_info()
            row.update({"radixBits": res["radixBits"], "matches_per_probe": res["totalMatches"] // (a.reps + 1),
                        "count_us": med(us), "count_us_min": round(min(us[1:]), 1), "count_join_us": med(join_us),
                        "count_paths": [info["rPath"], info["sPath"]], "items": info["items"],
                        "maxSPartition": info["maxSPartition"]})
            assert row["matches_per_probe"] == want or sname == "zipf", row
            # (b) the bucketised table's materialising probe
            if not a.no_htm:
                c.reserve("htm", n, n)
                c.build(dR, n)
                row["htm_build_us"] = round(c.fetch()["build_us"], 1)
                us = []
                for _ in range(a.reps + 1):
                    c.probe_pairs(dS, n, dOutS, dOutR, n)
                    found, written, t, _ = c.pairs_info()
                    assert found == written == row["matches_per_probe"], (found, written)
                    us.append(t)
                row.update({"htm_pairs_us": med(us), "htm_pairs_us_min": min(us[1:])})
            # (c) the materialising radix join
            if not a.yardsticks_only:
                c.reserve("prj", n, n, radixBits=a.radix_bits, keepRowIds=True)
                c.prj_build(dR, n)
                row["pairs_build_us"] = round(c.fetch()["build_us"], 1)
                us, join_us = [], []
                for _ in range(a.reps + 1):
                    c._check(hj.lib.hj_prj_probe_pairs_dev(c._h, dS, n, 0, dOutS, dOutR, n))
                    found, written, t, _ = c.pairs_info()
                    assert found == written == row["matches_per_probe"], (found, written)
                    us.append(t); join_us.append(c.fetch()["join_us"])
                row.update({"pairs_us": med(us), "pairs_us_min": min(us[1:]), "pairs_join_us": med(join_us),
                            "ratio_a": round(med(us) / row["count_us"], 3), "out_GBps": round(8.0 * n / med(us) / 1e3, 1),
                            "residentBytes": c.prj_resident_info()["residentBytes"]})
                if not a.no_htm:
                    row["ratio_b"] = round(med(us) / row["htm_pairs_us"], 3)
                for how in kinds:                                   # at most n rows each on these inputs: the planes do
                    kind = _lib.JOIN_KINDS[how]
                    kus, kjoin = [], []
                    for _ in range(a.reps + 1):
                        c.prj_probe_pairs(dS, n, dOutS, dOutR, n, kind=kind)
                        found, written, t, _ = c.pairs_info()
                        assert found == written <= n, (how, found, written)
                        kus.append(t); kjoin.append(c.fetch()["join_us"])
                    row.update({how + "_rows": found, how + "_us": med(kus), how + "_us_min": min(kus[1:]),
                                how + "_join_us": med(kjoin), how + "_ratio": round(med(kus) / row["pairs_us"], 3)})
                if a.track_r:
                    track_r(c, a, row, dR, dS, n, dOutS, dOutR, kinds, sname == "sorted" and not a.absent_half)
            print(json.dumps(row), flush=True)
        for p in (dR, dS, dOutS, dOutR):
            c.dev_free(p)


if __name__ == "__main__":
    main()
