#!/usr/bin/env python3
"""Cost of counting in key-range passes: bench.py's C2 workload (or --shards N concatenated C4 rank
shards) at P = 1, 2, 4, 8 on one GPU.  Per P: the count step time (count_run + the wait for its
counters), the per-kernel times of a profiled run, the bytes the run requested next to
hga_count_estimate's figure, the pass statistics, and the conservation identity at min 1
(sum of counts == instances).  One JSON line per P on stdout.

    python tools/count_pass_cost.py [--steps 10] [--passes 1,2,4,8] [--shards 0] [--budget BYTES]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hybrid-genome-assembler_amd")]

import numpy as np  # noqa: E402

import bench  # noqa: E402
import hga  # noqa: E402

KERNELS = ("kc_init", "kc_bin1", "kc_layout", "kc_rebin", "kc_split3", "kc_count")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--passes", default="1,2,4,8")
    ap.add_argument("--shards", type=int, default=0, help="count this many C4 rank shards (bench.make_c4_shard) instead of C2")
    ap.add_argument("--budget", type=int, default=0, help="with --passes 0: the budget that chooses P")
    ap.add_argument("--check", action="store_true", help="also check sum(counts) == instances at min 1")
    args = ap.parse_args()
    if args.shards:
        files = [[], []]
        for r in range(args.shards):
            r4a, r4b = bench.make_c4_shard(r)
            files[0].append(r4a.seq)
            files[1].append(r4b.seq)
        label = f"{args.shards} C4 rank shards"
    else:
        _, _, ra, rb = bench.make_c2(0)
        files = [[ra.seq], [rb.seq]]
        label = "C2"
    with hga.Ctx(int(os.environ.get("HGA_DEVICE", "0"))) as ctx:
        ctx.count_begin(bench.K, 2)
        for f, parts in enumerate(files):
            for s in parts:
                ctx.count_add(f, s)
        del files
        for P in [int(x) for x in args.passes.split(",")]:
            ctx.count_set_passes(P, args.budget)
            est = ctx.count_estimate(2, P)
            for _ in range(2):   # warm-up: allocations
                ctx.count_run(2)
                ctx.count_stats()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ctx.count_run(2)
                st = ctx.count_stats()
            ms = (time.perf_counter() - t0) / args.steps * 1e3
            ctx.profile(True)
            ctx.profile_reset()
            for _ in range(args.steps):
                ctx.count_run(2)
                ctx.count_stats()
            kern = {}
            for name in KERNELS:
                t, n = ctx.profile_get(name)
                if n:
                    kern[name] = round(t / args.steps, 4)
            ctx.profile(False)
            ps = ctx.count_pass_stats()
            out = {"workload": label, "passes_asked": P, "passes": ps.passes, "ms_per_count": round(ms, 3),
                   "kernels_ms_per_count": kern, "kernels_sum_ms": round(sum(kern.values()), 4),
                   "work_bytes": ps.work_bytes, "estimate_bytes": est, "instances": st.instances,
                   "rows": st.distinct_rows, "max_pass_instances": ps.max_pass_instances,
                   "min_pass_instances": ps.min_pass_instances, "buckets": st.buckets}
            if args.check:
                ctx.count_run(1)
                st1 = ctx.count_stats()
                _, counts = ctx.rows()
                out["conservation"] = bool(int(counts.astype(np.uint64).sum()) == st1.instances)
                del counts
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
