#!/usr/bin/env python3
"""Prices key_hash2 / pairs_verify2 on key columns in the Arrow layout (validity planes, variable-length elements) against
the same kernels on plain columns: development tool.

    python tools/bench_join_on_columns.py [--log2n 27] [--var-log2n 27] [--reps 5] [--nulls 0.1] [--out FILE]

|R| = |S| = n = 2^log2n, unique uint64 keys 1..n in two different random orders (generate_relation "pk"), everything
resident on the device before anything is timed; no map visits the host. The candidates are those of the full join word:
key_hash(R), prj_build, key_hash(S), prj_probe_pairs, once per leg. There is one hash kernel and one verify kernel; the v1
names (key_hash / pairs_verify on hj_key_col) run their narrow instances (kVar false, kForm 0).
  plain      one non-nullable 8-byte column through the v1 names: the timing of those names, to be compared across two
             builds (profiles/join_on_columns.md, (e)), and the yardstick of the next leg. (Up to the commit that removed
             the first kernel pair this leg timed that pair against the narrow instances in one process: section (a).)
  nullable   the same column with validity planes on both sides, a share --nulls of the bits clear, through key_hash2 /
             pairs_verify2 (kForm 1), alternating with the v1 names on the same elements (kForm 0; they know no NULL: they
             keep every candidate), whose own spread over the rounds is the noise
             (byte model: the plain one plus n / 8 B of plane for the hash and one 4 B validity word per side and
             candidate for the verify step; the pairs written are put at n though fewer are kept: an upper bound)
  varlen     one variable-length column, 2^var-log2n rows: the element of key k is its 8 little-endian bytes repeated to
             8 + k % 17 bytes (8 .. 24, mean 16), so both sides agree and every kept pair is compared to its last byte;
             against the byte model -- hash: 8 B of offsets, the bytes and the 8 B tuple per row; verify: 8 B of maps, 16 B
             of offsets and both elements per candidate, 8 B per kept pair
Per round the S-side hash is timed with the host clock around the synchronised call (the hash has no *_info) and the
verify step by verify_info's device time. One JSON line per round, one summary line per leg: median (min..max) and the
spread (max - min) / median of every timing, the model bandwidth of the leg's last variant and, with two variants, the
ratio of the medians."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import htm_hashjoin_amd as hj  # noqa: E402


def varlen_of(keys, chunk=1 << 22):
    """(offsets, bytes) of the column whose element for key k is k's 8 bytes repeated to 8 + k % 17 bytes"""
    lens = (8 + keys % np.uint64(17)).astype(np.int64)
    off = np.zeros(keys.size + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    data = np.empty(int(off[-1]) + 3 & ~3, dtype=np.uint8)
    reach = np.arange(24)
    for lo in range(0, keys.size, chunk):
        k = keys[lo:lo + chunk]
        tiled = np.tile(k.view(np.uint8).reshape(k.size, 8), 3)
        data[off[lo]:off[lo + k.size]] = tiled[reach[None, :] < lens[lo:lo + chunk, None]]
    return off.astype(np.uint32), data


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--var-log2n", type=int, default=27)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nulls", type=float, default=0.1)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sink = open(a.out, "w") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    with hj.HashJoinContext(0) as c:
        held = []

        def alloc(nbytes):
            held.append(c.dev_alloc(max(int(nbytes), 4)))
            return held[-1]

        def put(a_):
            d = alloc(a_.nbytes)
            c.copy_h2d(d, a_)
            return d

        def free(*ptrs):
            for p in ptrs:
                held.remove(p)
                c.dev_free(p)

        def wall_us(fn):
            c.synchronize()
            t0 = time.perf_counter()
            fn()
            c.synchronize()
            return (time.perf_counter() - t0) * 1e6

        def leg(name, n, hash_s, verify, bytes_hash, bytes_verify, extra):
            """hash_s / verify: {variant: call}, "v1" (the yardstick, where there are two) and / or "new"; verify returns
            (kept, dropped). Alternating rounds."""
            for which in hash_s:
                hash_s[which](), verify[which]()                       # warm-up of every shape
            rounds = []
            for rep in range(a.reps):
                row = {"leg": name, "rep": rep, "n": n}
                for which in hash_s:
                    row[f"hash_{which}_us"] = round(wall_us(hash_s[which]), 1)
                    row[f"kept_{which}"], row[f"dropped_{which}"] = verify[which]()
                    row[f"verify_{which}_us"] = float(c.verify_info()[2])
                emit(row)
                rounds.append(row)
            summary = dict({"leg": name, "summary": True, "n": n, "reps": a.reps}, **extra)
            for k in (k for k in rounds[0] if k.endswith("_us")):
                v = [r[k] for r in rounds]
                summary[k] = [round(statistics.median(v), 1), min(v), max(v)]
                summary[k[:-3] + "_spread"] = round((max(v) - min(v)) / statistics.median(v), 3)
            last = list(hash_s)[-1]
            for step, model in (("hash", bytes_hash), ("verify", bytes_verify)):
                summary[f"{step}_{last}_GBps"] = round(model / summary[f"{step}_{last}_us"][0] / 1e3, 1)
                if len(hash_s) == 2:
                    summary[f"{step}_new_over_v1"] = round(summary[f"{step}_new_us"][0] / summary[f"{step}_v1_us"][0], 3)
            summary.update({k: rounds[-1][k] for k in rounds[-1] if k.startswith(("kept_", "dropped_"))})
            emit(summary)

        try:
            n = 1 << a.log2n
            words = (n + 31) // 32
            R = hj.generate_relation("pk", n, seed=12345)
            S = hj.generate_relation("pk", n, seed=54321)
            d_r, d_s, d_tr, d_ts = put(R), put(S), alloc(8 * n), alloc(8 * n)
            plain = [(d_s, d_r, 8)]
            c.reserve("prj", n, n, keepRowIds=True)
            c.key_hash(plain, hj.HJ_KEY_SIDE_R, n, d_tr)
            c.key_hash(plain, hj.HJ_KEY_SIDE_S, n, d_ts)
            c.prj_build(d_tr, n)
            c.prj_probe_pairs(d_ts, n, 0, 0, 0)
            cand = c.pairs_info()[0]
            d_ms, d_mr, d_ks, d_kr = (alloc(4 * cand) for _ in range(4))
            c.prj_probe_pairs(d_ts, n, d_ms, d_mr, cand)
            assert c.pairs_info()[:2] == (cand, cand)
            d_marks_s, d_marks_r = alloc(4 * words), alloc(4 * words)
            zeros = np.zeros(words, dtype=np.uint32)

            def verifier(fn, cols, pairs, rows):
                def run():
                    c.copy_h2d(d_marks_s, zeros[:(rows + 31) // 32])
                    c.copy_h2d(d_marks_r, zeros[:(rows + 31) // 32])
                    fn(d_ms, d_mr, pairs, 0, rows, rows, cols, d_ks, d_kr, pairs, d_marks_s, d_marks_r)
                    kept, _, _, dropped = c.verify_info()
                    return kept, dropped
                return run

            v1_hash = lambda: c.key_hash(plain, hj.HJ_KEY_SIDE_S, n, d_ts)        # noqa: E731
            v1 = verifier(c.pairs_verify, plain, cand, n)
            leg("plain", n, {"v1": v1_hash}, {"v1": v1}, n * 16, cand * 24 + n * 8, {"candidates": cand})

            rng = np.random.default_rng(7)
            planes = []
            for _ in "sr":      # a share --nulls of the bits clear, 2^24 rows at a time
                bits = np.concatenate([np.packbits(rng.random(min(1 << 24, n - lo)) >= a.nulls, bitorder="little")
                                       for lo in range(0, n, 1 << 24)])
                planes.append(np.resize(bits, 4 * words).view(np.uint32))
            d_vs, d_vr = put(planes[0]), put(planes[1])
            nullable = [(d_s, d_r, 8, 0, 0, d_vs, d_vr, 0)]
            leg("nullable", n, {"v1": v1_hash, "new": lambda: c.key_hash2(nullable, hj.HJ_KEY_SIDE_S, n, d_ts)},
                {"v1": v1, "new": verifier(c.pairs_verify2, nullable, cand, n)}, n * 16 + n // 8, cand * 32 + n * 8,
                {"candidates": cand, "nulls": a.nulls})
            free(d_vs, d_vr, d_ms, d_mr, d_ks, d_kr)

            m = 1 << a.var_log2n
            assert m <= n
            columns = []
            for rel in (S[:m], R[:m]):          # not the same key sets below n: the candidates are what the join finds
                off, data = varlen_of(rel)
                columns.append((put(data), put(off), int(off[-1])))
                del off, data
            (d_bs, d_os, bytes_s), (d_br, d_or, bytes_r) = columns
            varlen = [(d_bs, d_br, 0, d_os, d_or, 0, 0, 0)]
            c.key_hash2(varlen, hj.HJ_KEY_SIDE_R, m, d_tr)
            c.key_hash2(varlen, hj.HJ_KEY_SIDE_S, m, d_ts)
            c.prj_build(d_tr, m)
            c.prj_probe_pairs(d_ts, m, 0, 0, 0)
            cand = c.pairs_info()[0]
            d_ms, d_mr, d_ks, d_kr = (alloc(4 * cand) for _ in range(4))
            c.prj_probe_pairs(d_ts, m, d_ms, d_mr, cand)
            assert c.pairs_info()[:2] == (cand, cand)
            run = verifier(c.pairs_verify2, varlen, cand, m)
            kept = run()[0]
            mean = bytes_s / m
            leg("varlen", m, {"new": lambda: c.key_hash2(varlen, hj.HJ_KEY_SIDE_S, m, d_ts)}, {"new": run},
                m * 16 + bytes_s, cand * 24 + int(cand * 2 * mean) + kept * 8,
                {"candidates": cand, "bytes_s": bytes_s, "bytes_r": bytes_r, "mean_len": round(mean, 2)})
        finally:
            for p in held:
                c.dev_free(p)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
