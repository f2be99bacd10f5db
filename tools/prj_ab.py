#!/usr/bin/env python3
"""Two builds of the library side by side on the same device buffers, in one process: the radix join of another checkout
(--parent DIR: its htm-hashjoin_amd/ with a built lib/) against this one. Development tool, C ABI only, no torch.

    python tools/prj_ab.py --parent ../parent oneshot [--log2n 30 | --n 20000000] [--dist local_shuffle:1024] [--radix-bits 0]
    python tools/prj_ab.py --parent ../parent skew [--log2r 28] [--slices 12]         # tools/skew_config5.py --algos prj
    python tools/prj_ab.py --parent ../parent pairs [--log2n 27] [--s sorted,uniform,zipf]   # tools/prj_pairs_bench.py
    python tools/prj_ab.py --parent ../parent results [--log2n 27]

oneshot / skew / pairs: one warm-up launch per build, then `--reps` launches of each, alternating parent, change, parent, ...
Per figure one JSON line: every repetition, the medians, spread = max - min of the PARENT's repetitions, and
pass = (change median - parent median <= spread).
results: hj_prj_join_dev, hj_prj_build_dev + hj_prj_probe_dev and hj_prj_probe_pairs_dev of both builds on local_shuffle:1024
R with sorted, uniform and Zipf(0.9) S; the integers must be equal.
The exit status is 1 when results differ between the builds; a timing that does not pass is reported, not an error."""
import argparse
import importlib.util
import json
import os
import statistics
import sys

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_pkg(name, root):
    d = os.path.join(root, "htm-hashjoin_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def report(figure, reps, **extra):
    p, c = reps["parent"], reps["change"]
    spread = max(p) - min(p)
    row = {"figure": figure, **extra, "parent": [round(x, 1) for x in p], "change": [round(x, 1) for x in c],
           "parent_median": round(statistics.median(p), 1), "change_median": round(statistics.median(c), 1),
           "parent_spread": round(spread, 1)}
    row["pass"] = row["change_median"] - row["parent_median"] <= row["parent_spread"]
    print(json.dumps(row), flush=True)


def s_relation(c, hj, name, n, dS, theta=0.9):
    if name == "sorted":
        c.copy_h2d(dS, np.arange(1, n + 1, dtype=np.uint64))
    elif name == "uniform":
        c.copy_h2d(dS, np.random.default_rng(54321).integers(1, n + 1, size=n, dtype=np.uint64))
    else:
        c.zipf_open(n, theta, 54321)
        c.zipf_next(n, dS)
        c.zipf_close()
    c.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="checkout of the commit to compare against, built")
    ap.add_argument("--reps", type=int, default=6)
    sub = ap.add_subparsers(dest="what", required=True)
    o = sub.add_parser("oneshot")
    o.add_argument("--log2n", type=int, default=30)
    o.add_argument("--n", type=int, default=0)
    o.add_argument("--dist", default="local_shuffle:1024")
    o.add_argument("--radix-bits", type=int, default=0)
    k = sub.add_parser("skew")
    k.add_argument("--log2r", type=int, default=28)
    k.add_argument("--slices", type=int, default=12)
    k.add_argument("--radix-bits", type=int, default=0)
    p = sub.add_parser("pairs")
    p.add_argument("--log2n", type=int, default=27)
    p.add_argument("--s", default="sorted,uniform,zipf")
    r = sub.add_parser("results")
    r.add_argument("--log2n", type=int, default=27)
    a = ap.parse_args()

    libs = {"parent": load_pkg("hj_parent", os.path.abspath(a.parent)), "change": load_pkg("hj_change", HERE)}
    hj = libs["change"]
    ok = True
    with libs["parent"].HashJoinContext(0) as cp, libs["change"].HashJoinContext(0) as cc:
        ctx = {"parent": cp, "change": cc}
        order = ("parent", "change")

        if a.what == "oneshot":
            n = a.n or (1 << a.log2n)
            dist, w = a.dist.split(":")
            dR, dS = cc.dev_alloc(n * 8), cc.dev_alloc(n * 8)
            cc.copy_h2d(dS, np.arange(1, n + 1, dtype=np.uint64))
            cc.copy_h2d(dR, hj.generate_data(dist, n, n, int(w)))
            cc.synchronize()
            rows = {w_: [] for w_ in order}
            for w_ in order:
                ctx[w_].reserve("prj", n, n, radixBits=a.radix_bits)
            for rep in range(a.reps + 1):
                for w_ in order:
                    ctx[w_].prj_join(dR, n, dS, n)
                    rows[w_].append(ctx[w_].fetch())
            same = all(rows["parent"][i][f] == rows["change"][i][f] for i in range(a.reps + 1) for f in ("totalMatches", "prjChecksum", "prjPath"))
            last = rows["change"][-1]
            for fig in ("join_us", "total_us"):
                report(fig, {w_: [x[fig] for x in rows[w_][1:]] for w_ in order}, n=n, dist=a.dist, radixBits=last["radixBits"],
                             prjPath=last["prjPath"], matches=last["totalMatches"], results_equal=same)
            ok &= same

        elif a.what == "skew":
            n = 1 << a.log2r
            dR, dS = cc.dev_alloc(n * 8), cc.dev_alloc(n * 8)
            cc.copy_h2d(dR, hj.generate_data("local_shuffle", n, n, 1024))
            cc.synchronize()
            for w_ in order:
                ctx[w_].reserve("prj", n, n, radixBits=a.radix_bits)
                ctx[w_].prj_build(dR, n)
                ctx[w_].fetch()
            cc.zipf_open(n, 0.9, 0)
            rows = {w_: [] for w_ in order}
            prev = {w_: 0 for w_ in order}
            same = True
            for sl in range(a.slices + 1):
                cc.zipf_next(n, dS)
                cc.synchronize()
                got = {}
                for w_ in (order if sl % 2 == 0 else order[::-1]):
                    ctx[w_].prj_probe(dS, n)
                    res = ctx[w_].fetch()
                    rows[w_].append(res)
                    got[w_] = res["totalMatches"] - prev[w_]
                    prev[w_] = res["totalMatches"]
                same &= got["parent"] == got["change"] == n
            cc.zipf_close()
            info = cc.prj_resident_info()
            for fig in ("join_us", "probe_us"):
                report("resident probe " + fig + " per slice", {w_: [x[fig] for x in rows[w_][1:]] for w_ in order}, rSize=n,
                             slices=a.slices, items=info["items"], splitPartitions=info["splitPartitions"], results_equal=same)
            ok &= same

        elif a.what == "pairs":
            n = 1 << a.log2n
            dR, dS = cc.dev_alloc(n * 8), cc.dev_alloc(n * 8)
            dOutS, dOutR = cc.dev_alloc(4 * n + 16), cc.dev_alloc(4 * n + 16)
            cc.copy_h2d(dR, hj.generate_data("shuffle", n, n))
            for sname in a.s.split(","):
                s_relation(cc, hj, sname, n, dS)
                for w_ in order:
                    ctx[w_].reserve("prj", n, n, keepRowIds=True)
                    ctx[w_].prj_build(dR, n)
                    ctx[w_].fetch()
                us = {w_: [] for w_ in order}
                join = {w_: [] for w_ in order}
                for rep in range(a.reps + 1):
                    for w_ in order:
                        ctx[w_].prj_probe_pairs(dS, n, dOutS, dOutR, n)
                        found, written, t, _ = ctx[w_].pairs_info()
                        assert found == written == n, (w_, found, written)
                        us[w_].append(t); join[w_].append(ctx[w_].fetch()["join_us"])
                report("pairs_us", {w_: us[w_][1:] for w_ in order}, S=sname, log2n=a.log2n)
                report("pairs_join_us", {w_: join[w_][1:] for w_ in order}, S=sname, log2n=a.log2n)

        else:
            n = 1 << a.log2n
            dR, dS = cc.dev_alloc(n * 8), cc.dev_alloc(n * 8)
            cc.copy_h2d(dR, hj.generate_data("local_shuffle", n, n, 1024))
            for sname in ("sorted", "uniform", "zipf"):
                s_relation(cc, hj, sname, n, dS)
                vals = {}
                for w_ in order:
                    c = ctx[w_]
                    c.reserve("prj", n, n)
                    c.prj_join(dR, n, dS, n)
                    one = c.fetch()
                    c.reserve("prj", n, n)
                    c.prj_build(dR, n)
                    c.prj_probe(dS, n)
                    res = c.fetch()
                    c.reserve("prj", n, n, keepRowIds=True)
                    c.prj_build(dR, n)
                    c.prj_probe_pairs(dS, n, 0, 0, 0)                  # capacity 0: the pairs are counted only
                    found = c.pairs_info()[0]
                    vals[w_] = {"join_totalMatches": one["totalMatches"], "join_prjChecksum": one["prjChecksum"],
                                "build_probe_matches": res["totalMatches"], "build_prjChecksum": res["prjChecksum"], "pairs": found}
                same = vals["parent"] == vals["change"]
                print(json.dumps({"figure": "results", "S": sname, "log2n": a.log2n, "equal": same, **{w_: vals[w_] for w_ in order}}), flush=True)
                ok &= same
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
