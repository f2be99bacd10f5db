#!/usr/bin/env python3
"""Times the materialising probe against the counting probe on the same table and the same S, through the C ABI, no
torch: development tool.

    python tools/pairs_bench.py [--log2n 27] [--reps 10] [--counting-only] [--how left,semi,anti] [--absent-half] [--track-r]

One context, |R| = |S| = 2^log2n, R = local_shuffle W=16. Per configuration one JSON line with the median HIP-event
times over `reps` launches after one warm-up launch of
  (a) hj_probe_dev                                   -> probe_us
  (b) hj_probe_pairs_dev into two |pairs|-sized maps -> pairs_us, ratio = (b) / (a), out_GBps = 8 B x pairs / (b)
Configurations: atomic (HJ_FLAG_KEEP_ROW_IDS) x sorted S and htm x sorted S (every S tuple matches once: the
write-heaviest unique-key case), htm x Zipf(0.9) S.
claims = output runs claimed from the cursor per launch, from the kernel's geometry: a workgroup claims when its LDS stage
of 4096 pairs cannot take the next round, and once more at its end (pairs / 4096 + workgroups when every round is full).
--how: after (b), the same launches through hj_probe_join_dev for each listed join kind -> <kind>_us, <kind>_rows and
<kind>_ratio = its median / (b)'s, (b) being the INNER join of the same process and input; (b) itself always goes through
hj_probe_pairs_dev, the entry point older checkouts have. --absent-half: every second tuple of the sorted S gets a key
above R's (n + its key), so half of S is unmatched.
--track-r: behind the launches above, the same table is built once more on a context reserved with
HJ_FLAG_TRACK_R_MATCHES and INNER (and LEFT, when --how lists it) is timed again -> track_<kind>_us and track_<kind>_ratio =
its median / the median of the same kind without the flag, timed just before in this process; track_marked = R rows the
marks then hold. On the sorted S without --absent-half it also times hj_r_rows_dev (HJ_R_MATCHED) with a quarter, a half
and all of R's rows marked -> sweep_<rows>_us, sweep_<rows>_GBps = (4 B x rows + 2 x the plane of n / 8 B) / its median.
--counting-only runs (a) alone and uses nothing newer than hj_probe_dev (the 8-byte table is then asked for with
buildVariant 3): the same script times the yardstick on a checkout that has no materialising probe."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import htm_hashjoin_amd as hj  # noqa: E402
from htm_hashjoin_amd import _lib  # noqa: E402

STAGE_PAIRS, WORKGROUPS = 4096, 256 * 4


def track_r(c, a, row, algo, dR, dProbe, n, kinds, sweep):
    """--track-r: INNER / LEFT on a tracking context against row's medians of the same kinds, then the sweep"""
    c.reserve(algo, n, n, keepRowIds=True, trackRMatches=True)
    c.build(dR, n)
    for how in ["inner"] + [k for k in kinds if k == "left"]:
        kind, rows = _lib.JOIN_KINDS[how], row["pairs" if how == "inner" else "left_rows"]
        dOutS, dOutR = c.dev_alloc(4 * rows + 16), c.dev_alloc(4 * rows + 16)
        us = []
        for _ in range(a.reps + 1):
            c.r_marks_clear()                               # every launch meets clear bits and sets them: the atomics are timed
            c.probe_pairs(dProbe, n, dOutS, dOutR, rows, kind=kind)
            found, written, t, _ = c.pairs_info()
            assert found == written == rows, (how, found, written, rows)
            us.append(t)
        c.dev_free(dOutS)
        c.dev_free(dOutR)
        med, base = statistics.median(us[1:]), row["pairs_us" if how == "inner" else "left_us"]
        row.update({"track_" + how + "_us": med, "track_" + how + "_us_min": min(us[1:]), "track_" + how + "_ratio": round(med / base, 3)})
    c.r_rows(_lib.HJ_R_MATCHED, 0, 0)
    row["track_marked"] = c.r_rows_info()[0]
    if not sweep:
        return
    dRows = c.dev_alloc(4 * n + 16)
    for part in (4, 2, 1):                                  # sorted S: its first n / part tuples mark that many rows
        c.r_marks_clear()
        c.probe_pairs(dProbe, n // part, 0, 0, 0)           # a mark-only pass
        us = []
        for _ in range(a.reps + 1):
            c.r_rows(_lib.HJ_R_MATCHED, dRows, n)
            produced, written, t, _ = c.r_rows_info()
            assert produced == written, (produced, written)
            us.append(t)
        med = statistics.median(us[1:])
        row.update({"sweep_%d_us" % produced: med, "sweep_%d_GBps" % produced: round((4.0 * produced + 2.0 * n / 8) / max(med, 1) / 1e3, 1)})
    c.dev_free(dRows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--theta", type=float, default=0.9)
    ap.add_argument("--counting-only", action="store_true")
    ap.add_argument("--tag", default="")
    ap.add_argument("--how", default="", help="comma list of left, semi, anti")
    ap.add_argument("--absent-half", action="store_true")
    ap.add_argument("--track-r", action="store_true", help="also time INNER / LEFT and the sweep with HJ_FLAG_TRACK_R_MATCHES")
    a = ap.parse_args()
    n = 1 << a.log2n
    kinds = [k for k in a.how.split(",") if k]
    with hj.HashJoinContext(0) as c:
        dR, dS, dZ = c.dev_alloc(n * 8), c.dev_alloc(n * 8), c.dev_alloc(n * 8)
        R = hj.generate_data("local_shuffle", n, n, 16)
        c.copy_h2d(dR, R)
        del R
        S = np.arange(1, n + 1, dtype=np.uint64)
        if a.absent_half:
            S[1::2] += np.uint64(n)
        c.copy_h2d(dS, S)
        del S
        c.zipf_open(n, a.theta, 54321)
        c.zipf_next(n, dZ)
        c.zipf_close()
        c.synchronize()
        configs = [("atomic", "sorted", dS), ("htm", "sorted", dS), ("htm", "zipf", dZ)]
        if a.counting_only:
            configs.insert(0, ("atomic-default", "sorted", dS))
        for algo, sname, dProbe in configs:
            if algo == "atomic-default":
                c.reserve("atomic", n, n)                           # the device's pick: the compact 4-byte table here
            elif algo == "atomic":
                kw = {"buildVariant": 3} if a.counting_only else {"keepRowIds": True}
                c.reserve("atomic", n, n, **kw)
            else:
                c.reserve("htm", n, n)
            c.build(dR, n)
            probe_us = []
            for _ in range(a.reps + 1):
                c.probe(dProbe, n)
                probe_us.append(c.fetch()["probe_us"])
            res = c.fetch()
            row = {"tag": a.tag, "algo": algo, "S": sname, "log2n": a.log2n, "buildVariant": res["buildVariant"],
                   "matches_per_probe": res["totalMatches"] // (a.reps + 1),
                   "probe_us": round(statistics.median(probe_us[1:]), 1), "probe_us_min": round(min(probe_us[1:]), 1)}
            if not a.counting_only:
                pairs = row["matches_per_probe"]
                dOutS, dOutR = c.dev_alloc(4 * pairs + 16), c.dev_alloc(4 * pairs + 16)
                pairs_us = []
                for _ in range(a.reps + 1):
                    c._check(hj.lib.hj_probe_pairs_dev(c._h, dProbe, n, 0, dOutS, dOutR, pairs))
                    found, written, us, _ = c.pairs_info()
                    assert found == written == pairs, (found, written, pairs)
                    pairs_us.append(us)
                c.dev_free(dOutS)
                c.dev_free(dOutR)
                med = statistics.median(pairs_us[1:])
                for how in kinds:
                    kind = _lib.JOIN_KINDS[how]
                    c.probe_pairs(dProbe, n, 0, 0, 0, kind=kind)             # capacity 0: the kind's row count
                    rows = c.pairs_info()[0]
                    dOutS = c.dev_alloc(4 * rows + 16)
                    dOutR = c.dev_alloc(4 * rows + 16) if kind <= _lib.HJ_JOIN_LEFT else 0
                    kind_us = []
                    for _ in range(a.reps + 1):
                        c.probe_pairs(dProbe, n, dOutS, dOutR, rows, kind=kind)
                        found, written, us, _ = c.pairs_info()
                        assert found == written == rows, (how, found, written, rows)
                        kind_us.append(us)
                    c.dev_free(dOutS)
                    if dOutR:
                        c.dev_free(dOutR)
                    kmed = statistics.median(kind_us[1:])
                    row.update({how + "_rows": rows, how + "_us": kmed, how + "_us_min": min(kind_us[1:]),
                                how + "_ratio": round(kmed / med, 3)})
                row.update({"pairs": pairs, "pairs_us": med, "pairs_us_min": min(pairs_us[1:]),
                            "ratio": round(med / row["probe_us"], 3), "out_GBps": round(8.0 * pairs / med / 1e3, 1),
                            "claims": pairs // STAGE_PAIRS + min(WORKGROUPS, (n // 2 + 256) // 256)})
                if a.track_r:
                    track_r(c, a, row, algo, dR, dProbe, n, kinds, sname == "sorted" and not a.absent_half)
            print(json.dumps(row), flush=True)
        for p in (dR, dS, dZ):
            c.dev_free(p)


if __name__ == "__main__":
    main()
