#!/usr/bin/env python3
"""Times the aggregating joins against what a user composes without them, on the same device and the same data: development tool.

    python tools/bench_join_aggregate.py [--log2n 27] [--shape fk|zipf] [--cols 1 4] [--radix-bits 0] [--reps 7] [--out FILE]

One context created with hj_create_on_stream on torch's current stream; every buffer is a torch tensor whose data_ptr()
goes to the C ABI. R = the keys 1..n in random order (n = 2^log2n), built once with its row ids. S, one slice of n tuples:
  fk      a foreign key: n uniform draws from 1..n
  zipf    n draws from 1..n with P(k) ~ 1 / rank(k)^theta (--theta, default 1.0), the ranks scattered over the keys -- drawn with
          torch by inverse CDF, not by the library's generator: the shape of BASELINE config 5, not its exact tuples
Values: one int64 column per aggregate, drawn below 2^40 so that the baseline's sums cannot overflow where ours wrap.
Per (shape, cols) one JSON line, the median with minimum and maximum over `reps` launches after one warm-up launch, each
launch between two events on the stream:
  fused_us      hj_prj_agg_begin + hj_prj_probe_agg_dev + hj_prj_agg_rows_dev: the first `cols` of SUM, MIN, MAX, COUNT
  baseline_us   the composition on the parent commit: the outputs zeroed, hj_prj_probe_join_dev(INNER) into two planes,
                hj_gather_dev of the value columns through the S plane, then by the R plane torch.index_add_ (SUM, COUNT) and
                torch.scatter_reduce_ (amin, amax, include_self with the identities)
  pairs_agg_us  hj_pairs_agg_dev over those two planes (the values read through the S plane by the call itself)
  index_add_us  the gather and the torch reductions alone, on the same planes
  equal         the three results agree element for element, checked before anything is timed
  fused_model_GBps  the byte model of profiles/join_aggregate.md over fused_us"""
import argparse
import json
import os
import statistics
import sys

import torch  # first: it ships its own HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import htm_hashjoin_amd as hj  # noqa: E402
from htm_hashjoin_amd import _lib  # noqa: E402

I64_MAX, I64_MIN = (1 << 63) - 1, -(1 << 63)
OPS = [(_lib.HJ_AGG_SUM, 8, _lib.HJ_AGG_SIGNED), (_lib.HJ_AGG_MIN, 8, _lib.HJ_AGG_SIGNED), (_lib.HJ_AGG_MAX, 8, _lib.HJ_AGG_SIGNED),
       (_lib.HJ_AGG_COUNT, 0, 0)]
IDENTITY = [0, I64_MAX, I64_MIN, 0]


def timed(fn, reps):
    """-> microseconds of reps launches of fn after one warm-up launch, each between two events on the current stream"""
    out = []
    for k in range(reps + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        if k:
            out.append(t0.elapsed_time(t1) * 1000.0)
    return out


def stats(prefix, us):
    return {prefix + "_us": round(statistics.median(us), 1), prefix + "_us_min": round(min(us), 1), prefix + "_us_max": round(max(us), 1)}


def zipf_keys(n, theta, dev, g):
    w = torch.arange(1, n + 1, dtype=torch.float64, device=dev).pow_(-theta)
    cdf = torch.cumsum(w, 0)
    cdf /= cdf[-1].clone()
    ranks = torch.searchsorted(cdf, torch.rand(n, dtype=torch.float64, device=dev, generator=g)).clamp_(max=n - 1)
    return torch.randperm(n, device=dev, generator=g)[ranks] + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--shape", choices=("fk", "zipf"), default="fk")
    ap.add_argument("--theta", type=float, default=1.0)
    ap.add_argument("--cols", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--radix-bits", type=int, default=0, help="hj_params.radixBits of the resident R (0: automatic)")
    ap.add_argument("--tag", default="", help="copied into every row")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = 1 << a.log2n
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    sink = open(a.out, "a") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    with hj.HashJoinContext(0, stream=torch.cuda.current_stream().cuda_stream) as c:
        R = torch.randperm(n, device=dev, generator=g) + 1                 # int64 whose value is the key: the tuple layout
        S = zipf_keys(n, a.theta, dev, g) if a.shape == "zipf" else torch.randint(1, n + 1, (n,), dtype=torch.int64, device=dev, generator=g)
        vals = [torch.randint(-(1 << 40), 1 << 40, (n,), dtype=torch.int64, device=dev, generator=g) for _ in range(3)]
        c.reserve("prj", n, n, radixBits=a.radix_bits, keepRowIds=True)
        c.prj_build(R.data_ptr(), n)
        map_s, map_r = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        fused = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4)]
        base = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4)]
        pagg = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4)]
        gathered = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3)]
        ones = torch.ones(n, dtype=torch.int64, device=dev)
        for n_cols in a.cols:
            specs = OPS[:n_cols]
            srcs = [(vals[k].data_ptr() if specs[k][1] else 0, 0) for k in range(n_cols)]
            n_vals = min(n_cols, 3)

            def run_fused():
                c.prj_agg_begin(specs)
                c.prj_probe_agg(S.data_ptr(), n, srcs)
                c.prj_agg_rows([fused[k].data_ptr() for k in range(n_cols)])

            def probe():
                c.prj_probe_pairs(S.data_ptr(), n, map_s.data_ptr(), map_r.data_ptr(), n)

            def reduce_torch():
                c.gather(map_s.data_ptr(), n, n, [(vals[k].data_ptr(), gathered[k].data_ptr(), 8, 0) for k in range(n_vals)])
                for k in range(n_cols):
                    base[k].fill_(IDENTITY[k])
                base[0].index_add_(0, map_r, gathered[0])
                if n_cols > 1:
                    base[1].scatter_reduce_(0, map_r.to(torch.int64), gathered[1], "amin", include_self=True)
                if n_cols > 2:
                    base[2].scatter_reduce_(0, map_r.to(torch.int64), gathered[2], "amax", include_self=True)
                if n_cols > 3:
                    base[3].index_add_(0, map_r, ones)

            def run_baseline():
                probe()
                reduce_torch()

            def run_pairs_agg():
                for k in range(n_cols):
                    pagg[k].fill_(IDENTITY[k])
                c.pairs_agg(map_r.data_ptr(), map_s.data_ptr(), n, 0, n, 0, n,
                            [(srcs[k][0], 0, pagg[k].data_ptr()) + specs[k] for k in range(n_cols)])

            run_fused()
            run_baseline()
            found = c.pairs_info()[0]
            assert found == n, found                                       # R holds every key once: one pair per S tuple
            run_pairs_agg()
            c.synchronize()
            equal = all(torch.equal(fused[k], base[k]) and torch.equal(pagg[k], base[k]) for k in range(n_cols))
            row = {"shape": a.shape, "log2n": a.log2n, "cols": n_cols, "radix_bits": a.radix_bits, "reps": a.reps, "equal": bool(equal)}
            if a.tag:
                row["tag"] = a.tag
            if a.shape == "zipf":
                row["theta"] = a.theta
                row["hottest_row"] = int(torch.bincount(map_r.to(torch.int64)).max())
            us = timed(run_fused, a.reps)
            row.update(stats("fused", us))
            row["last_probe_agg_info_us"] = c.prj_agg_info()["us"]
            # per S tuple: 16 B through the stamping histogram and through each of the two scatters, 8 B read by the join, 8 B per
            # value column; per R tuple: 8 B read by the join, and per plane 8 B initialised, 16 B updated, 16 B through the rows call
            row["fused_model_GBps"] = round(((48 + 8 + 8 * n_vals) + (8 + 40 * (n_cols + 1))) * n / statistics.median(us) / 1e3, 1)
            bas = timed(run_baseline, a.reps)
            row.update(stats("baseline", bas))
            row["ratio"] = round(statistics.median(us) / statistics.median(bas), 3)
            probe()
            pa = timed(run_pairs_agg, a.reps)
            row.update(stats("pairs_agg", pa))
            row["last_pairs_agg_info_us"] = c.pairs_agg_info()[2]
            ia = timed(reduce_torch, a.reps)
            row.update(stats("index_add", ia))
            row["pairs_agg_ratio"] = round(statistics.median(pa) / statistics.median(ia), 3)
            emit(row)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
