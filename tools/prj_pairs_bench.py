#!/usr/bin/env python3
"""Times the materialising radix join against its two yardsticks on the same R and S, through the C ABI, no torch:
development tool.

    python tools/prj_pairs_bench.py [--log2n 27] [--reps 10] [--radix-bits 0] [--s sorted,uniform,zipf] [--yardsticks-only]

|R| = |S| = 2^log2n, R = the keys 1..n shuffled (unique), so every S tuple matches once. S = sorted, uniform draws, or
Zipf(theta) over n keys. Per S one JSON line with the median HIP-event times over `reps` launches after one warm-up of
  (a) hj_prj_probe_dev, R resident as bare keys (no flag)                     -> count_us (count_join_us: its join kernel)
  (b) htm build + hj_probe_pairs_dev: the only other way to the same pairs    -> htm_pairs_us
  (c) hj_prj_probe_pairs_dev, R resident as {key, row} (HJ_FLAG_KEEP_ROW_IDS) -> pairs_us (pairs_join_us: its join kernel)
and ratio_a = (c) / (a), ratio_b = (c) / (b), out_GBps = 8 B x pairs / (c), build_us of both resident forms.
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


def med(xs):
    return round(statistics.median(xs[1:]), 1)          # [0] is the warm-up launch


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
    a = ap.parse_args()
    n = 1 << a.log2n
    with hj.HashJoinContext(0) as c:
        dR, dS = c.dev_alloc(n * 8), c.dev_alloc(n * 8)
        c.copy_h2d(dR, hj.generate_data("shuffle", n, n))
        dOutS, dOutR = c.dev_alloc(4 * n + 16), c.dev_alloc(4 * n + 16)
        for sname in a.s.split(","):
            if sname == "sorted":
                c.copy_h2d(dS, np.arange(1, n + 1, dtype=np.uint64))
            elif sname == "uniform":
                c.copy_h2d(dS, np.random.default_rng(54321).integers(1, n + 1, size=n, dtype=np.uint64))
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
            assert row["matches_per_probe"] == n, row
            # (b) the bucketised table's materialising probe
            if not a.no_htm:
                c.reserve("htm", n, n)
                c.build(dR, n)
                row["htm_build_us"] = round(c.fetch()["build_us"], 1)
                us = []
                for _ in range(a.reps + 1):
                    c.probe_pairs(dS, n, dOutS, dOutR, n)
                    found, written, t, _ = c.pairs_info()
                    assert found == written == n, (found, written)
                    us.append(t)
                row.update({"htm_pairs_us": med(us), "htm_pairs_us_min": min(us[1:])})
            # (c) the materialising radix join
            if not a.yardsticks_only:
                c.reserve("prj", n, n, radixBits=a.radix_bits, keepRowIds=True)
                c.prj_build(dR, n)
                row["pairs_build_us"] = round(c.fetch()["build_us"], 1)
                us, join_us = [], []
                for _ in range(a.reps + 1):
                    c.prj_probe_pairs(dS, n, dOutS, dOutR, n)
                    found, written, t, _ = c.pairs_info()
                    assert found == written == n, (found, written)
                    us.append(t); join_us.append(c.fetch()["join_us"])
                row.update({"pairs_us": med(us), "pairs_us_min": min(us[1:]), "pairs_join_us": med(join_us),
                            "ratio_a": round(med(us) / row["count_us"], 3), "out_GBps": round(8.0 * n / med(us) / 1e3, 1),
                            "residentBytes": c.prj_resident_info()["residentBytes"]})
                if not a.no_htm:
                    row["ratio_b"] = round(med(us) / row["htm_pairs_us"], 3)
            print(json.dumps(row), flush=True)
        for p in (dR, dS, dOutS, dOutR):
            c.dev_free(p)


if __name__ == "__main__":
    main()
