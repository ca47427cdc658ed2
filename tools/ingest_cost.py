#!/usr/bin/env python3
"""Cost of getting a read file into the count: bench.py's C2 pair written as ART-like FASTQ (as the bench's
ingest leg writes it), then per run, alternating,
  host    jf_stream (the multi-threaded host reader) + count_add of its stream, and
  device  count_add_file of the file's raw bytes (parsed on the GPU),
each from the file's bytes in memory to the resident stream.  Per route: wall time, the bytes moved to the
device, and for the device route the per-kernel times of a profiled run with their bytes per second (read:
the raw bytes; written: the stream).  --cli also runs bin/jf_occurrences with and without --device-parse,
alternating, after one discarded warm run.  --check compares count_seq and the rows of both routes.
One JSON line per run on stdout.

    python tools/ingest_cost.py [--runs 5] [--cli 9] [--check]
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "hybrid-genome-assembler_amd")]

import numpy as np  # noqa: E402

import bench  # noqa: E402
import hga  # noqa: E402

KERNELS = ("ig_count", "ig_starts", "ig_lines", "ig_kept", "ig_scatter", "scan")
# bytes each parser kernel reads / writes, from (raw bytes, stream bytes, lines, tiles)
TRAFFIC = {
    "ig_count": lambda n, out, lines, tiles: (n, 8 * tiles),
    "ig_starts": lambda n, out, lines, tiles: (n + 8 * tiles, 4 * lines),
    "ig_lines": lambda n, out, lines, tiles: (12 * lines, 0),
    "ig_kept": lambda n, out, lines, tiles: (n + 8 * tiles, 16 * tiles),
    "ig_scatter": lambda n, out, lines, tiles: (n + 8 * tiles, out),
}


def host_route(ctx, paths):
    t0 = time.perf_counter()
    streams = [hga.jf_stream(p) for p in paths]
    t1 = time.perf_counter()
    ctx.count_begin(bench.K, len(paths))
    for f, s in enumerate(streams):
        ctx.count_add(f, s)
    t2 = time.perf_counter()
    return {"route": "host", "read_files_ms": round((t1 - t0) * 1e3, 2), "upload_ms": round((t2 - t1) * 1e3, 2),
            "total_ms": round((t2 - t0) * 1e3, 2), "bytes_to_device": sum(len(s) for s in streams)}


def device_route(ctx, raws, profile):
    ctx.count_begin(bench.K, len(raws))
    if profile:
        ctx.profile(True)
        ctx.profile_reset()
    t0 = time.perf_counter()
    infos = [ctx.count_add_file(f, r) for f, r in enumerate(raws)]
    dt = time.perf_counter() - t0
    out = {"route": "device", "total_ms": round(dt * 1e3, 2), "bytes_to_device": sum(len(r) for r in raws),
           "layouts": [i["layout"] for i in infos], "seq_bytes": sum(i["seq_bytes"] for i in infos),
           "lines": sum(i["lines"] for i in infos), "profiled": profile}
    if profile:
        n, seq, lines = out["bytes_to_device"], out["seq_bytes"], out["lines"]
        tiles = sum((len(r) + hga.ingest_tile() - 1) // hga.ingest_tile() for r in raws)
        kern = {}
        for name in KERNELS:
            ms, launches = ctx.profile_get(name)
            if not launches:
                continue
            kern[name] = {"ms": round(ms, 4), "launches": launches}
            if name in TRAFFIC:
                rd, wr = TRAFFIC[name](n, seq, lines, tiles)
                kern[name].update(read_bytes=rd, written_bytes=wr, GBps=round((rd + wr) / (ms * 1e-3) / 1e9, 1))
        out["kernels"] = kern
        out["kernels_sum_ms"] = round(sum(k["ms"] for k in kern.values()), 4)
        ctx.profile(False)
    return out


def cli_run(d, paths, extra):
    for p in paths:   # no dump caches: every run counts
        c = p + f"_{bench.K}-mers_sorted"
        if os.path.exists(c):
            os.unlink(c)
    cli = os.path.join(ROOT, "hybrid-genome-assembler_amd", "bin", "jf_occurrences")
    env = dict(os.environ, HGA_PLOT_CMD="cat > /dev/null", HGA_TIMING="1")
    t0 = time.perf_counter()
    r = subprocess.run([cli, *paths, "-k", str(bench.K), *extra], input=f"{bench.LOWER} {bench.UPPER} 1\n", text=True,
                       capture_output=True, cwd=d, env=env, timeout=600)
    dt = time.perf_counter() - t0
    phases = {}
    for line in r.stderr.splitlines():
        f = line.split()
        if len(f) == 3 and f[0] == "hga-timing":
            phases[f[1]] = float(f[2])
    return {"cli": "device-parse" if extra else "host", "rc": r.returncode, "wall_s": round(dt, 4), "phases_ms": phases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cli", type=int, default=0, help="also time the CLI this many times per route")
    ap.add_argument("--check", action="store_true", help="compare count_seq and the rows of the two routes")
    args = ap.parse_args()
    ga, gb, _, _ = bench.make_c2(0)
    d = tempfile.mkdtemp(prefix="hga_ingest_cost_")
    try:
        paths = [os.path.join(d, "mg1655.fq"), os.path.join(d, "uti89.fq")]
        for g, pth, seed, name in ((ga, paths[0], 1000, "A"), (gb, paths[1], 1001, "B")):
            hga.write_art_fastq(g, name, bench.COVERAGE * len(g) // bench.READ_LEN, bench.READ_LEN, seed, pth)
        raws = [open(p, "rb").read() for p in paths]
        print(json.dumps({"files": "C2 pair as ART-like FASTQ", "bytes": sum(len(r) for r in raws),
                          "tile": hga.ingest_tile()}), flush=True)
        with hga.Ctx(int(os.environ.get("HGA_DEVICE", "0"))) as ctx:
            host_route(ctx, paths)            # warm: page cache, allocations
            device_route(ctx, raws, False)
            for i in range(args.runs):
                for out in (host_route(ctx, paths), device_route(ctx, raws, False)):
                    out["run"] = i
                    print(json.dumps(out), flush=True)
            print(json.dumps(device_route(ctx, raws, True)), flush=True)
            if args.check:
                host_route(ctx, paths)
                seq_h = [ctx.count_seq(f) for f in range(2)]
                ctx.count_run(2)
                rows_h = ctx.rows()
                device_route(ctx, raws, False)
                seq_d = [ctx.count_seq(f) for f in range(2)]
                ctx.count_run(2)
                rows_d = ctx.rows()
                print(json.dumps({"check": {"count_seq_equal": seq_h == seq_d,
                                            "rows_equal": bool(np.array_equal(rows_h[0], rows_d[0]) and
                                                               np.array_equal(rows_h[1], rows_d[1])),
                                            "rows": int(len(rows_d[0]))}}), flush=True)
        if args.cli:
            cli_run(d, paths, [])   # discarded warm run
            for i in range(args.cli):
                for extra in ([], ["--device-parse"]):
                    out = cli_run(d, paths, extra)
                    out["run"] = i
                    print(json.dumps(out), flush=True)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
