#!/usr/bin/env python3
"""Times the steps of join_on -- hash, candidate join, verify, sweep -- against the candidate join alone: development tool.

    python tools/bench_join_on.py [--log2n 27] [--reps 5] [--weak-mask 0x3FFFFFF] [--out FILE]

|R| = |S| = n = 2^log2n, unique uint64 keys 1..n in two different random orders (generate_relation "pk"): below 2^32, so
the same relations are valid input for the radix join on the key word, which is the yardstick -- prj_build + prj_probe_pairs
on the relations themselves, what radix_join_pairs runs on the device: code this path does not change, on the same
commit, in the same process, alternating with the sequence measured. Everything is resident on the device before
anything is timed; no map visits the host.
Per key_mask (0 = the full join word, then --weak-mask, which keeps fewer bits and so makes more candidates), after one
warm-up of every step, `reps` rounds of
  yardstick   prj_build(R) + prj_probe_pairs(S)                              host clock around the stream, synchronised
  join_on     key_hash(R), prj_build, key_hash(S), prj_probe_pairs, pairs_verify, mark_rows(S plane, unmatched)
              the same clock around the whole sequence; per step the device time of the call's own *_info counter
              (pairs_info, verify_info, mark_rows_info) and, for key_hash and prj_build, which have none, the host clock
              around the synchronised call
One JSON line per round, then one summary line per mask: median (min..max) per step, the yardstick's spread, hash + verify
+ sweep as an overhead over the yardstick, and pairs_verify's achieved bytes/s under the byte model of
profiles/join_on.md (8 B of maps + 2 x 8 B of key elements per candidate, 8 B per kept pair)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import htm_hashjoin_amd as hj  # noqa: E402

WIDTH = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--weak-mask", type=lambda v: int(v, 0), default=0x3FFFFFF)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = 1 << a.log2n
    words = (n + 31) // 32
    sink = open(a.out, "w") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    R = hj.generate_relation("pk", n, seed=12345)
    S = hj.generate_relation("pk", n, seed=54321)
    with hj.HashJoinContext(0) as c:
        held = []

        def alloc(nbytes):
            held.append(c.dev_alloc(nbytes))
            return held[-1]

        def wall_us(fn):
            c.synchronize()
            t0 = time.perf_counter()
            fn()
            c.synchronize()
            return (time.perf_counter() - t0) * 1e6

        try:
            d_r, d_s, d_tr, d_ts = (alloc(8 * n) for _ in range(4))
            d_marks_s, d_marks_r, d_lone = alloc(4 * words), alloc(4 * words), alloc(4 * n)
            c.copy_h2d(d_r, R)
            c.copy_h2d(d_s, S)
            zeros = np.zeros(words, dtype=np.uint32)
            cols = [(d_s, d_r, WIDTH)]
            c.reserve("prj", n, n, keepRowIds=True)
            for mask in (0, a.weak_mask):
                # how many candidates this mask makes: a counting probe (capacity 0), then planes of that size
                c.key_hash(cols, hj.HJ_KEY_SIDE_R, n, d_tr, mask)
                c.key_hash(cols, hj.HJ_KEY_SIDE_S, n, d_ts, mask)
                c.prj_build(d_tr, n)
                c.prj_probe_pairs(d_ts, n, 0, 0, 0)
                candidates = c.pairs_info()[0]
                d_ms, d_mr, d_ks, d_kr = (alloc(4 * candidates) for _ in range(4))
                t = {}

                def yardstick():
                    c.prj_build(d_r, n)
                    c.prj_probe_pairs(d_s, n, d_ms, d_mr, candidates)

                def sequence():
                    t["hash_r_us"] = wall_us(lambda: c.key_hash(cols, hj.HJ_KEY_SIDE_R, n, d_tr, mask))
                    t["build_us"] = wall_us(lambda: c.prj_build(d_tr, n))
                    t["hash_s_us"] = wall_us(lambda: c.key_hash(cols, hj.HJ_KEY_SIDE_S, n, d_ts, mask))
                    c.prj_probe_pairs(d_ts, n, d_ms, d_mr, candidates)
                    found, written, t["probe_us"] = c.pairs_info()[:3]
                    assert found == written == candidates, (found, written, candidates)
                    c.copy_h2d(d_marks_s, zeros)
                    c.copy_h2d(d_marks_r, zeros)
                    c.pairs_verify(d_ms, d_mr, candidates, 0, n, n, cols, d_ks, d_kr, candidates, d_marks_s, d_marks_r)
                    kept, wrote, t["verify_us"], dropped = c.verify_info()
                    assert (kept, wrote, dropped) == (n, n, 0), (kept, wrote, dropped)      # unique keys 1..n on both sides
                    c.mark_rows(d_marks_s, n, 0, 0, d_lone, n)
                    lone, _, t["mark_rows_us"], _ = c.mark_rows_info()
                    assert lone == 0, lone

                def chained():
                    """the same calls with nothing between them but the stream"""
                    c.key_hash(cols, hj.HJ_KEY_SIDE_R, n, d_tr, mask)
                    c.prj_build(d_tr, n)
                    c.key_hash(cols, hj.HJ_KEY_SIDE_S, n, d_ts, mask)
                    c.prj_probe_pairs(d_ts, n, d_ms, d_mr, candidates)
                    c.pairs_verify(d_ms, d_mr, candidates, 0, n, n, cols, d_ks, d_kr, candidates, d_marks_s, d_marks_r)
                    c.mark_rows(d_marks_s, n, 0, 0, d_lone, n)

                yardstick(), sequence(), chained()                  # warm-up of every shape
                c.synchronize()
                rounds = []
                for rep in range(a.reps):
                    row = {"mask": hex(mask), "rep": rep, "n": n, "candidates": candidates}
                    row["yardstick_us"] = round(wall_us(yardstick), 1)
                    c.copy_h2d(d_marks_s, zeros)
                    c.copy_h2d(d_marks_r, zeros)
                    row["join_on_us"] = round(wall_us(chained), 1)
                    sequence()
                    row.update({k: round(float(v), 1) for k, v in t.items()})
                    emit(row)
                    rounds.append(row)
                keys = [k for k in rounds[0] if k.endswith("_us")]
                summary = {"mask": hex(mask), "summary": True, "n": n, "candidates": candidates, "kept": n, "reps": a.reps}
                for k in keys:
                    v = [r[k] for r in rounds]
                    summary[k] = [round(statistics.median(v), 1), min(v), max(v)]
                med = {k: summary[k][0] for k in keys}
                extra = med["hash_r_us"] + med["hash_s_us"] + med["verify_us"] + med["mark_rows_us"]
                summary["hash_verify_sweep_us"] = round(extra, 1)
                summary["overhead_over_yardstick"] = round(extra / med["yardstick_us"], 3)
                summary["join_on_over_yardstick"] = round(med["join_on_us"] / med["yardstick_us"], 3)
                summary["yardstick_spread"] = round((summary["yardstick_us"][2] - summary["yardstick_us"][1]) / med["yardstick_us"], 3)
                model_bytes = candidates * (8 + 2 * WIDTH) + n * 8
                summary["verify_GBps"] = round(model_bytes / med["verify_us"] / 1e3, 1)
                summary["hash_GBps"] = round(n * (WIDTH + 8) / med["hash_s_us"] / 1e3, 1)
                emit(summary)
                for p in (d_ms, d_mr, d_ks, d_kr):
                    held.remove(p)
                    c.dev_free(p)
        finally:
            for p in held:
                c.dev_free(p)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
