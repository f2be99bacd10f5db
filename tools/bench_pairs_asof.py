#!/usr/bin/env python3
"""Times hj_pairs_asof_dev over the inner pairs of the radix join against the five-call composition that gave the same
rows before it existed: development tool.

    python tools/bench_pairs_asof.py [--log2s 27] [--log2keys 24] [--versions 8] [--reps 5] [--out FILE]

R holds 2^log2keys keys x `versions` versions (row i: key i % keys + 1, a random int64 timestamp), S 2^log2s rows with a
random key of R and a random int64 timestamp, so every S row has `versions` candidate pairs; everything is resident on the
device before anything is timed. prj_build + prj_probe_pairs give the inner pairs once (S rows' pairs side by side, as the
probe writes them); every call measured reads those two maps.
  fused       pairs_asof, one 8-byte ">=" term, both mark planes: asof_info's device time of the whole call
  yardstick   the composition, built from entry points older than pairs_asof, in the same process, alternating with it:
                1. pairs_where(s_ts >= r_ts)              -> list A        (no planes)
                2. pairs_agg(MAX r_ts by S row) over A    -> plane best    (signed 64-bit)
                3. pairs_where(best[s] == r_ts[r]) over A -> list B        (no planes)
                4. pairs_agg(MIN r row by S row) over B   -> plane bestRow (the R row as a 64-bit value)
                5. pairs_where(bestRow[s] == row[r]) over B, both mark planes
              its time is the sum of the five calls' own *_info device times; the fills of its two accumulator planes are
              not counted (the fused call's two initialisations are)
After one warm-up of both, `reps` alternating rounds; one JSON line per round, then a summary: median (min..max) of either,
their ratio, the yardstick's own spread. Both must keep the same number of pairs, and on small inputs (log2s <= 22) the
same R row per S row.
Then the cost of a hot S row, on a synthetic list of 2^24 pairs (8 per S row of 2^21): the fused call on the list as it is,
with 2^16 consecutive pairs given to ONE S row (a run), and with 2^16 pairs at random places given to it (scattered)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import htm_hashjoin_amd as hj  # noqa: E402

INT, UINT, GE, EQ = hj.HJ_VAL_INT, hj.HJ_VAL_UINT, hj.HJ_CMP_GE, hj.HJ_CMP_EQ
I64_MIN, U64_MAX = np.int64(-(1 << 63)), np.uint64((1 << 64) - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2s", type=int, default=27)
    ap.add_argument("--log2keys", type=int, default=24)
    ap.add_argument("--versions", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n_s, keys = 1 << a.log2s, 1 << a.log2keys
    n_r, n_pairs = keys * a.versions, n_s * a.versions
    sink = open(a.out, "w") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    rng = np.random.default_rng(2718)
    R = (np.arange(n_r, dtype=np.uint64) % np.uint64(keys)) + np.uint64(1)
    S = rng.integers(1, keys + 1, n_s).astype(np.uint64)
    r_ts, s_ts = rng.integers(0, 1 << 40, n_r), rng.integers(0, 1 << 40, n_s)
    with hj.HashJoinContext(0) as c:
        held = []

        def alloc(nbytes):
            held.append(c.dev_alloc(max(int(nbytes), 16)))
            return held[-1]

        def put(arr):
            d = alloc(arr.nbytes)
            c.copy_h2d(d, np.ascontiguousarray(arr))
            return d

        def fill(d, value, n, dtype, chunk=1 << 24):
            block = np.full(min(n, chunk), value, dtype=dtype)
            for lo in range(0, n, chunk):
                c.copy_h2d(d + lo * block.itemsize, block[:min(chunk, n - lo)])

        try:
            d_r, d_s = put(R), put(S)
            d_rts, d_sts = put(r_ts), put(s_ts)
            d_row = put(np.arange(n_r, dtype=np.uint64))             # the R row as a value: steps 4 and 5 of the composition
            c.reserve("prj", n_r, n_s, keepRowIds=True)
            c.prj_build(d_r, n_r)
            d_ms, d_mr = alloc(4 * n_pairs), alloc(4 * n_pairs)
            c.prj_probe_pairs(d_s, n_s, d_ms, d_mr, n_pairs)
            assert c.pairs_info()[:2] == (n_pairs, n_pairs), c.pairs_info()
            sw, rw = (n_s + 31) // 32, (n_r + 31) // 32
            d_marks_s, d_marks_r = alloc(4 * sw), alloc(4 * rw)
            d_bv, d_br = alloc(8 * n_s), alloc(4 * n_s)              # the fused call's planes
            d_best, d_best_row = alloc(8 * n_s), alloc(8 * n_s)      # the composition's
            d_as, d_ar = alloc(4 * n_pairs), alloc(4 * n_pairs)      # list A: every pair may pass
            d_bs, d_brr = alloc(4 * n_pairs), alloc(4 * n_pairs)     # list B
            d_ks, d_kr = alloc(4 * n_s), alloc(4 * n_s)              # the result: one pair per S row at most

            def clear():
                fill(d_marks_s, 0, sw, np.uint32)
                fill(d_marks_r, 0, rw, np.uint32)

            def fused():
                clear()
                c.pairs_asof(d_ms, d_mr, n_pairs, 0, n_s, n_r, (d_sts, d_rts, 8, INT, GE), d_bv, d_br, d_ks, d_kr, n_s, d_marks_s, d_marks_r)
                kept, wrote, us, dropped = c.asof_info()
                assert wrote == kept and dropped == 0, (kept, wrote, dropped)
                return us, kept

            def composed():
                clear()
                fill(d_best, I64_MIN, n_s, np.int64)
                fill(d_best_row, U64_MAX, n_s, np.uint64)
                parts = []
                c.pairs_where(d_ms, d_mr, n_pairs, 0, n_s, n_r, [(d_sts, d_rts, 8, INT, GE)], d_as, d_ar, n_pairs)
                n_a, _, us, _ = c.where_info()
                parts.append(us)
                c.pairs_agg(d_as, d_ar, n_a, 0, n_s, 0, n_r, [(d_rts, 0, d_best, hj.HJ_AGG_MAX, 8, hj.HJ_AGG_SIGNED)])
                parts.append(c.pairs_agg_info()[2])
                c.pairs_where(d_as, d_ar, n_a, 0, n_s, n_r, [(d_best, d_rts, 8, INT, EQ)], d_bs, d_brr, n_pairs)
                n_b, _, us, _ = c.where_info()
                parts.append(us)
                c.pairs_agg(d_bs, d_brr, n_b, 0, n_s, 0, n_r, [(d_row, 0, d_best_row, hj.HJ_AGG_MIN, 8, 0)])
                parts.append(c.pairs_agg_info()[2])
                c.pairs_where(d_bs, d_brr, n_b, 0, n_s, n_r, [(d_best_row, d_row, 8, UINT, EQ)], d_ks, d_kr, n_s, d_marks_s, d_marks_r)
                kept, wrote, us, dropped = c.where_info()
                parts.append(us)
                assert wrote == kept and dropped == 0, (kept, wrote, dropped)
                return sum(parts), kept, parts, (n_a, n_b)

            def one_round():
                f_us, f_kept = fused()
                y_us, y_kept, parts, lists = composed()
                assert f_kept == y_kept, (f_kept, y_kept)
                return {"asof_us": f_us, "composition_us": y_us, "composition_parts_us": parts, "kept": f_kept, "list_a": lists[0], "list_b": lists[1]}

            one_round()                                             # warm-up of both
            if a.log2s <= 22:                                       # the same R row per S row (the composition's is a 64-bit word)
                mine, theirs = np.empty(n_s, dtype=np.uint32), np.empty(n_s, dtype=np.uint64)
                fused()
                c.copy_d2h(mine, d_br)
                composed()
                c.copy_d2h(theirs, d_best_row)
                assert np.array_equal(mine, theirs.astype(np.uint32)), "the fused call and the composition keep different rows"
            rounds = []
            for rep in range(a.reps):
                row = {"rep": rep, "n_s": n_s, "n_r": n_r, "pairs": n_pairs, **one_round()}
                emit(row)
                rounds.append(row)
            summary = {"summary": True, "n_s": n_s, "n_r": n_r, "pairs": n_pairs, "kept": rounds[0]["kept"], "reps": a.reps}
            for k in ("asof_us", "composition_us"):
                v = [r[k] for r in rounds]
                summary[k] = [statistics.median(v), min(v), max(v)]
            y = summary["composition_us"]
            summary["composition_spread"] = round((y[2] - y[1]) / y[0], 3)
            summary["asof_over_composition"] = round(summary["asof_us"][0] / y[0], 3)
            # bytes under the model of profiles/pairs_asof.md: per pass and pair 8 B of maps; passes 1 and 2 two 8-byte elements
            # and one plane access (8 B, 4 B) each; pass 3 one 4-byte read; 8 B per kept pair
            model = n_pairs * (3 * 8 + 2 * 16 + 8 + 4 + 4) + 8 * summary["kept"]
            summary["asof_model_GBps"] = round(model / summary["asof_us"][0] / 1e3, 1)
            emit(summary)

            # ---- a hot S row: 2^16 of the pairs belong to one S row
            h_s, h_pairs, hot = 1 << 21, 1 << 24, 1 << 16
            if n_s >= h_s and n_r >= h_pairs // 8:
                base_s = np.repeat(np.arange(h_s, dtype=np.uint32), 8)
                base_r = rng.integers(0, n_r, h_pairs).astype(np.uint32)
                lists = {"even": base_s, "run": base_s.copy(), "scattered": base_s.copy()}
                lists["run"][4096:4096 + hot] = 7
                lists["scattered"][rng.choice(h_pairs, hot, replace=False)] = 7
                d_hr, d_hs = put(base_r), alloc(4 * h_pairs)
                hot_row = {"hot_row": True, "pairs": h_pairs, "s_rows": h_s, "hot_pairs": hot}
                for name, m in lists.items():
                    c.copy_h2d(d_hs, m)
                    times = []
                    for _ in range(a.reps + 1):
                        c.pairs_asof(d_hs, d_hr, h_pairs, 0, h_s, n_r, (d_sts, d_rts, 8, INT, GE), d_bv, d_br, d_ks, d_kr, h_s)
                        times.append(c.asof_info()[2])
                    v = times[1:]
                    hot_row[f"{name}_us"] = [statistics.median(v), min(v), max(v)]
                emit(hot_row)
        finally:
            for p in held:
                c.dev_free(p)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
