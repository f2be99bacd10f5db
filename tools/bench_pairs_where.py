#!/usr/bin/env python3
"""Times hj_pairs_where_dev over the inner pairs of the radix join against hj_pairs_verify_dev on the same maps: development tool.

    python tools/bench_pairs_where.py [--log2n 27] [--reps 5] [--out FILE]

|R| = |S| = n = 2^log2n, unique uint64 keys 1..n in two different random orders (generate_relation "pk"), everything
resident on the device before anything is timed. prj_build + prj_probe_pairs give the n inner pairs once; every call
measured reads those two maps.
  yardstick   pairs_verify with one 8-byte key column (the relations themselves): the existing kernel of the same shape and
              byte model, in the same process, alternating with the calls measured; keeps every pair
  all         pairs_where, one 8-byte "<=" term on the same two columns: keeps every pair
  half        the same term against R's keys with the odd ones lowered by one: keeps the pairs with an even key
  four        four 4-byte terms on four pairs of uint32 columns (<=, >=, ==, <=): keeps every pair
each with both mark planes and with none; the time is the call's own device time (verify_info / where_info). Then the
composition, as join_on chains it on one stream with nothing in between, by the host clock around the synchronised stream:
  join_on         key_hash(R), prj_build, key_hash(S), prj_probe_pairs, pairs_verify(planes), mark_rows
  join_on_where   the same with pairs_verify(no planes, pairs kept), pairs_where(one 8-byte term, planes), mark_rows
After one warm-up of every shape, `reps` alternating rounds; one JSON line per round, then a summary: median (min..max) per
call, its ratio to the yardstick of the same planes, the yardstick's own spread, and bytes/s under the byte model of
profiles/pairs_where.md (8 B of maps + two elements per term per pair, 8 B per kept pair)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import htm_hashjoin_amd as hj  # noqa: E402

UINT, LE, GE, EQ = hj.HJ_VAL_UINT, hj.HJ_CMP_LE, hj.HJ_CMP_GE, hj.HJ_CMP_EQ


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--reps", type=int, default=5)
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

        def put(arr):
            d = alloc(arr.nbytes)
            c.copy_h2d(d, np.ascontiguousarray(arr))
            return d

        def wall_us(fn):
            c.synchronize()
            t0 = time.perf_counter()
            fn()
            c.synchronize()
            return (time.perf_counter() - t0) * 1e6

        try:
            d_r, d_s = put(R), put(S)
            d_r_half = put(R - (R & np.uint64(1)))
            r32, s32 = R.astype(np.uint32), S.astype(np.uint32)
            four = [(put(s32 + np.uint32(k)), put(r32 + np.uint32(k)), 4, UINT, op) for k, op in enumerate((LE, GE, EQ, LE))]
            d_tr, d_ts = alloc(8 * n), alloc(8 * n)
            d_marks_s, d_marks_r, d_lone = alloc(4 * words), alloc(4 * words), alloc(4 * n)
            d_ms, d_mr, d_ks, d_kr, d_es, d_er = (alloc(4 * n) for _ in range(6))
            zeros = np.zeros(words, dtype=np.uint32)
            key = [(d_s, d_r, 8)]
            settings = {"all": ([(d_s, d_r, 8, UINT, LE)], n), "half": ([(d_s, d_r_half, 8, UINT, LE)], n // 2), "four": (four, n)}
            c.reserve("prj", n, n, keepRowIds=True)
            c.prj_build(d_r, n)
            c.prj_probe_pairs(d_s, n, d_ms, d_mr, n)
            assert c.pairs_info()[:2] == (n, n)
            # the candidates of the hashed join (a counting probe): the planes the chained sequences write, apart from the maps above
            c.key_hash(key, hj.HJ_KEY_SIDE_R, n, d_tr)
            c.key_hash(key, hj.HJ_KEY_SIDE_S, n, d_ts)
            c.prj_build(d_tr, n)
            c.prj_probe_pairs(d_ts, n, 0, 0, 0)
            candidates = c.pairs_info()[0]
            d_cs, d_cr = alloc(4 * candidates), alloc(4 * candidates)

            def clear():
                c.copy_h2d(d_marks_s, zeros)
                c.copy_h2d(d_marks_r, zeros)

            def verify_us(planes):
                clear()
                c.pairs_verify(d_ms, d_mr, n, 0, n, n, key, d_ks, d_kr, n, *((d_marks_s, d_marks_r) if planes else (0, 0)))
                kept, wrote, us, dropped = c.verify_info()
                assert (kept, wrote, dropped) == (n, n, 0), (kept, wrote, dropped)
                return us

            def where_us(name, planes):
                terms, expect = settings[name]
                clear()
                c.pairs_where(d_ms, d_mr, n, 0, n, n, terms, d_ks, d_kr, n, *((d_marks_s, d_marks_r) if planes else (0, 0)))
                kept, wrote, us, dropped = c.where_info()
                assert (kept, wrote, dropped) == (expect, expect, 0), (name, kept, wrote, dropped)
                return us

            def chained(where):
                """join_on's calls with nothing between them but the stream"""
                c.key_hash(key, hj.HJ_KEY_SIDE_R, n, d_tr)
                c.prj_build(d_tr, n)
                c.key_hash(key, hj.HJ_KEY_SIDE_S, n, d_ts)
                c.prj_probe_pairs(d_ts, n, d_cs, d_cr, candidates)
                if where:
                    c.pairs_verify(d_cs, d_cr, candidates, 0, n, n, key, d_es, d_er, n)
                    c.pairs_where(d_es, d_er, n, 0, n, n, settings["all"][0], d_ks, d_kr, n, d_marks_s, d_marks_r)
                else:
                    c.pairs_verify(d_cs, d_cr, candidates, 0, n, n, key, d_ks, d_kr, n, d_marks_s, d_marks_r)
                c.mark_rows(d_marks_s, n, 0, 0, d_lone, n)

            def one_round():
                row = {}
                for planes in (True, False):
                    tag = "planes" if planes else "plain"
                    row[f"verify_{tag}_us"] = verify_us(planes)
                    for name in settings:
                        row[f"where_{name}_{tag}_us"] = where_us(name, planes)
                for where in (False, True):
                    clear()
                    row["join_on_where_us" if where else "join_on_us"] = round(wall_us(lambda: chained(where)), 1)
                return row

            one_round()                                             # warm-up of every shape
            rounds = []
            for rep in range(a.reps):
                row = {"rep": rep, "n": n, "candidates": candidates, **one_round()}
                emit(row)
                rounds.append(row)
            keys = [k for k in rounds[0] if k.endswith("_us")]
            summary = {"summary": True, "n": n, "reps": a.reps}
            for k in keys:
                v = [r[k] for r in rounds]
                summary[k] = [round(statistics.median(v), 1), min(v), max(v)]
            for tag in ("planes", "plain"):
                y = summary[f"verify_{tag}_us"]
                summary[f"verify_{tag}_spread"] = round((y[2] - y[1]) / y[0], 3)
                for name, (terms, kept) in settings.items():
                    med = summary[f"where_{name}_{tag}_us"][0]
                    summary[f"where_{name}_{tag}_over_verify"] = round(med / y[0], 3)
                    summary[f"where_{name}_{tag}_GBps"] = round((n * (8 + 2 * sum(t[2] for t in terms)) + 8 * kept) / med / 1e3, 1)
                summary[f"verify_{tag}_GBps"] = round(n * (8 + 16 + 8) / y[0] / 1e3, 1)
            summary["join_on_where_over_join_on"] = round(summary["join_on_where_us"][0] / summary["join_on_us"][0], 3)
            emit(summary)
        finally:
            for p in held:
                c.dev_free(p)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
