"""bench.py's plain run and --dump-outputs: a plain run prints the headline line only (no leg that
needs --full), --steps sets the number of timed steps, and --dump-outputs writes the last timed step's
outputs as float .npy files (at most 64 MB, a fixed seeded sample of the per-row arrays), identical from
run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("roofline", "kernels_ms_per_step", "categorize", "ingest", "cpu_baseline", "scale_c4", "parity", "export")


class _Rank0:
    rank = 0


class _Ctx:
    """Stand-in for the device context: n merged rows of 2 files, every third row selected."""

    def __init__(self, n):
        self.keys = np.arange(n, dtype=np.uint64) * np.uint64(524287) + np.uint64(1 << 33)
        self.counts = np.stack([np.arange(n) % 40, np.arange(n) % 7], axis=1).astype(np.uint32)

    def rows(self):
        return self.keys, self.counts

    def select(self, lower, upper):
        sel = self.keys[::3]
        return sel, (np.arange(len(sel)) % 2).astype(np.uint8), int(len(sel) // 2)


def _dump(tmp_path, name, n):
    import bench
    ctx = _Ctx(n)
    hist = np.arange(21, dtype=np.int64).reshape(-1, 3)
    d = str(tmp_path / name)
    shapes = bench.dump_outputs(d, ctx, None, _Rank0(), {"spec_hist": hist}, len(ctx.keys[::3]), 5)
    out = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert {k: list(v.shape) for k, v in out.items()} == shapes
    return ctx, hist, out


def test_dump_outputs_small_is_whole(tmp_path):
    ctx, hist, out = _dump(tmp_path, "a", 1000)
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert np.array_equal(out["rows_keys"], ctx.keys.astype(np.float64))
    assert np.array_equal(out["rows_counts"], ctx.counts)
    assert np.array_equal(out["selected_keys"], ctx.keys[::3].astype(np.float64))
    assert np.array_equal(out["spec_hist"], hist)
    assert out["select_counts"].tolist() == [334.0, 5.0]
    assert out["totals"][:5].tolist() == [1000.0, 334.0, 167.0, float(ctx.counts[:, 0].sum()), float(ctx.counts[:, 1].sum())]


def test_dump_outputs_large_is_a_fixed_sample(tmp_path):
    import bench
    n = 3 * bench.DUMP_SAMPLE + 17
    ctx, _, a = _dump(tmp_path, "a", n)
    _, _, b = _dump(tmp_path, "b", n)
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    assert len(a["rows_keys"]) == bench.DUMP_SAMPLE and len(a["selected_keys"]) == bench.DUMP_SAMPLE
    idx = ((a["rows_keys"] - float(1 << 33)) / 524287).astype(np.int64)   # the sampled row numbers, ascending
    assert np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(a["rows_counts"], ctx.counts[idx])
    assert a["totals"][0] == n   # whole-array totals, not the sample's


@pytest.mark.gpu
def test_plain_run_headline_and_dump(tmp_path):
    runs = []
    for name in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs",
                            str(tmp_path / name)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        runs.append(json.loads(lines[0]))
    res = runs[0]
    assert res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1 and res["full"] is False
    assert res["unit"] == "k-mers/s" and res["higher_is_better"] is True and res["dtype"] == "u64"
    assert res["ms_per_step"] > 0
    # value = instances / (ms_per_step rounded to 1 us)
    assert res["value"] == pytest.approx(res["config"]["instances_per_gpu"] / (res["ms_per_step"] * 1e-3), rel=2e-3)
    assert not [k for k in FULL_ONLY if k in res]
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n in res["dumped"])
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64)
        assert np.array_equal(a, b), f   # same arguments: same inputs, same outputs
        total += a.nbytes
    assert total <= 64 << 20
    rows, n_sel, n_disc = np.load(tmp_path / "a" / "totals.npy")[:3]
    assert rows == res["config"]["distinct_rows"]
    assert [n_sel, n_disc] == [res["config"]["selected"], res["config"]["discriminative"]]
    assert np.load(tmp_path / "a" / "select_counts.npy").tolist() == [n_sel, n_disc]
