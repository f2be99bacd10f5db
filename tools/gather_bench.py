#!/usr/bin/env python3
"""Times hj_gather_dev against torch.index_select on the same device, the same maps and the same columns: development tool.

    python tools/gather_bench.py [--log2n 27] [--reps 7] [--out FILE]

One context created with hj_create_on_stream on torch's current stream; every buffer is a torch tensor whose data_ptr()
goes to the C ABI. |R| = |S| = n = 2^log2n output rows from an n-row source.
Maps, all written by the engine on the device and never copied to the host:
  ascending   hj_r_rows_dev(HJ_R_UNMATCHED) after a build that no probe has marked: every R row, ascending
  s_sorted    the S plane of hj_probe_join_dev(INNER) over a sorted S
  r_random    the R plane of the same probe; R is a random permutation (generate_relation "pk"), so the plane is one too
NULL share 0.5: the same map with every second entry replaced by HJ_NO_ROW (index_select cannot take it: no baseline).
Columns: 1 and 4 columns of 4, 8 and 16 bytes (index_select: int32, int64, complex128; one call per column).
Per configuration one JSON line: the median, minimum and maximum over `reps` launches after one warm-up launch, each
launch between two events on the stream, for the gather (gather_us*) and for index_select (select_us*); gather_GBps =
(4 B of map + 2 x width per column: read and written) x n / the median, the algorithmic bytes, not the lines fetched; ratio
= gather median / index_select median; equal = the two outputs are the same bytes (checked once per configuration)."""
import argparse
import json
import os
import statistics
import sys

import torch  # first: it ships its own HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import htm_hashjoin_amd as hj  # noqa: E402
from htm_hashjoin_amd import _lib  # noqa: E402

SELECT_DTYPE = {4: torch.int32, 8: torch.int64, 16: torch.complex128}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = 1 << a.log2n
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    sink = open(a.out, "w") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    with hj.HashJoinContext(0, stream=torch.cuda.current_stream().cuda_stream) as c:
        # ---- the maps, from the engine ----
        R = torch.from_numpy(hj.generate_relation("pk", n).view("int64")).to(dev)
        S = torch.arange(1, n + 1, dtype=torch.int64, device=dev)
        maps = {k: torch.empty(n, dtype=torch.int32, device=dev) for k in ("ascending", "s_sorted", "r_random")}
        c.reserve("htm", n, n, keepRowIds=True, trackRMatches=True)
        c.build(R.data_ptr(), n)
        c.r_rows(_lib.HJ_R_UNMATCHED, maps["ascending"].data_ptr(), n)
        assert c.r_rows_info()[:2] == (n, n)
        c.probe_pairs(S.data_ptr(), n, maps["s_sorted"].data_ptr(), maps["r_random"].data_ptr(), n)
        assert c.pairs_info()[:2] == (n, n)
        c.fetch()
        del R, S
        # ---- the columns: four sources and four outputs of 16 bytes an element, narrower columns are their front ----
        g = torch.Generator(device=dev)
        g.manual_seed(1)
        srcs = [torch.randint(0, 1 << 62, (2 * n,), dtype=torch.int64, device=dev, generator=g) for _ in range(4)]
        dsts = [torch.empty(2 * n, dtype=torch.int64, device=dev) for _ in range(4)]
        check = torch.empty(2 * n, dtype=torch.int64, device=dev)
        for name, base in maps.items():
            for null_share in (0.0, 0.5):
                m = base
                if null_share:
                    m = base.clone()
                    m[::2] = -1                                 # HJ_NO_ROW
                for width in (4, 8, 16):
                    for n_cols in (1, 4):
                        cols = [(srcs[k].data_ptr(), dsts[k].data_ptr(), width, 0) for k in range(n_cols)]
                        us = timed(lambda: c.gather(m.data_ptr(), n, n, cols), a.reps)
                        info = c.gather_info()
                        assert info[0] == n and info[3] == 0 and info[1] == (n // 2 if null_share else 0), info
                        med = statistics.median(us)
                        row = {"map": name, "null_share": null_share, "width": width, "cols": n_cols, "log2n": a.log2n, "reps": a.reps}
                        row.update(stats("gather", us))
                        row["gather_GBps"] = round((4.0 + 2.0 * width * n_cols) * n / med / 1e3, 1)
                        row["last_gather_info_us"] = info[2]
                        if not null_share:
                            dt = SELECT_DTYPE[width]
                            words = n * width // 8
                            views = [(srcs[k][:words].view(dt), check[:words].view(dt) if k == 0 else dsts[k][:words].view(dt))
                                     for k in range(n_cols)]
                            idx = m                             # int32: the uint32 map as it lies, its entries are below 2^31

                            def select():
                                for src, dst in views:
                                    torch.index_select(src, 0, idx, out=dst)

                            sel = timed(select, a.reps)
                            row.update(stats("select", sel))
                            row["ratio"] = round(med / statistics.median(sel), 3)
                            c.gather(m.data_ptr(), n, n, cols[:1])  # column 0 again: index_select wrote the others' outputs
                            c.synchronize()
                            row["equal"] = bool(torch.equal(dsts[0][:words], check[:words]))
                        emit(row)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
