#!/usr/bin/env python3
"""Cost of the SDK lookup in read batches: bench.py's C3 workload (Nanosim-like reads of the C2 genome pair,
the SDK set = the C2 count's [10, 25] export) one-shot (hga_lookup_set_reads + hga_lookup_run) and in batches
of 256 M, 64 M and 16 M bases (hga_lookup_begin / _add_reads / _finish).  Per setting: the wall time from the
first call to a synchronised end (median and range of --steps runs after a warm-up), the per-kernel times of
a profiled run, and for the batched settings the session's statistics (slot_bytes, result_bytes, regrowths,
host_waits) next to the bytes of the one-shot scan buffers.  --check compares the nine fetched arrays with the
one-shot run's.  One JSON line per setting on stdout.

    python tools/lookup_batch_cost.py [--steps 5] [--batches 256M,64M,16M] [--scale 1.0] [--check]
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

KERNELS = ("lk_pack", "lk_count", "lk_emit", "lk_rebase", "lk_post", "lk_sort", "lk_kci", "scan", "radix_upsweep",
           "radix_downsweep")
NAMES = ("hit_ptr", "hit_kid", "hit_pos", "sorted_kid", "first_ptr", "first_kid", "first_pos", "kci_ptr", "kci_read")


def parse_size(s):
    mult = {"K": 1 << 10, "M": 1 << 20, "G": 1 << 30}.get(s[-1].upper())
    return int(s[:-1]) * mult if mult else int(s)


def cut(offsets, size):
    """Read-index bounds of batches of whole reads: as many as fit in `size` bases, at least one."""
    bounds, i, n = [0], 0, len(offsets) - 1
    while i < n:
        j = int(np.searchsorted(offsets, offsets[i] + np.uint64(size), side="right")) - 1
        i = min(max(j, i + 1), n)
        bounds.append(i)
    return bounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batches", default="256M,64M,16M")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the C3 reads to use")
    ap.add_argument("--check", action="store_true", help="compare the nine fetched arrays with the one-shot run's")
    args = ap.parse_args()
    dev = int(os.environ.get("HGA_DEVICE", "0"))
    ga, gb, ra, rb = bench.make_c2(0)
    with hga.Ctx(dev) as cc:
        cc.count_begin(bench.K, 2)
        cc.count_add(0, ra.seq)
        cc.count_add(1, rb.seq)
        cc.count_run(2)
        sdk, _, _ = cc.select(bench.LOWER, bench.UPPER)
    del ra, rb
    bases, offsets = bench.make_c3(ga, gb, 0)
    if args.scale < 1.0:
        n = max(1, int((len(offsets) - 1) * args.scale))
        offsets = offsets[:n + 1]
        bases = bases[:int(offsets[-1])]
    view = memoryview(bases)
    n_reads, n_bases = len(offsets) - 1, int(offsets[-1])

    def one_shot(ctx):
        ctx.lookup_set_reads(bases, offsets, 1)
        ctx.lookup_run()
        ctx.sync()

    def batched(ctx, bounds):
        ctx.lookup_begin(1)
        for a, b in zip(bounds[:-1], bounds[1:]):
            lo, hi = int(offsets[a]), int(offsets[b])
            ctx.lookup_add_reads(bytes(view[lo:hi]), offsets[a:b + 1] - offsets[a])
        ctx.lookup_finish()
        ctx.sync()

    want = None
    settings = [("one-shot", None)] + [(s, parse_size(s)) for s in args.batches.split(",") if s]
    for label, size in settings:
        bounds = cut(offsets, size) if size else None
        run = (lambda c: batched(c, bounds)) if size else one_shot
        with hga.Ctx(dev) as ctx:   # a ctx per setting: its buffers are this setting's
            ctx.lookup_load(bench.K, sdk)
            run(ctx)   # warm-up: allocations (the hit arrays grow here; later runs find them large enough)
            first = ctx.lookup_batch_stats() if size else None
            times = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                run(ctx)
                times.append((time.perf_counter() - t0) * 1e3)
            ctx.profile(True)
            ctx.profile_reset()
            run(ctx)
            kern = {}
            for name in KERNELS:
                t, n = ctx.profile_get(name)
                if n:
                    kern[name] = [round(t, 4), n]
            ctx.profile(False)
            s = ctx.lookup_sizes()
            out = {"workload": "C3", "setting": label, "reads": n_reads, "bases": n_bases, "sdk": int(len(sdk)),
                   "hits": s.hits, "ms_median": round(float(np.median(times)), 3), "ms_min": round(min(times), 3),
                   "ms_max": round(max(times), 3), "kernels_ms_launches": kern,
                   "one_shot_scan_bytes": ctx.lookup_batch_estimate(n_bases, n_reads) // 2,
                   "note": "ms: set_reads + run (one-shot) or begin .. finish (batched), host copies of the batch "
                           "slices included, to a synchronised end; one_shot_scan_bytes: the one-shot scan buffers "
                           "of this read set, aligned as a slot"}
            if size:
                st = ctx.lookup_batch_stats()
                out.update(batch_bases=size, batches=st.batches, slot_bytes=st.slot_bytes, result_bytes=st.result_bytes,
                           regrowths=st.regrowths, regrowths_first_run=first.regrowths,
                           host_waits=st.host_waits,
                           estimate_bytes=ctx.lookup_batch_estimate(
                               max(int(offsets[b] - offsets[a]) for a, b in zip(bounds[:-1], bounds[1:])),
                               max(b - a for a, b in zip(bounds[:-1], bounds[1:]))))
            if args.check:
                got = ctx.lookup_fetch()
                if want is None:
                    want = got
                else:
                    out["equals_one_shot"] = bool(all(np.array_equal(got[n], want[n]) for n in NAMES))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
