"""bench.py's command line: what a plain run does and reports, --full, and --dump-outputs.

CPU: argument parsing and the .npy writer (float32, exact, the 64 MB bound with its fixed seeded sample).
GPU: one plain run on a small stream; its result line, and the dumped decisions against the CPU oracle.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_parse_plain_and_full():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full and a.dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def test_dump_outputs_is_exact_float32(tmp_path):
    inv = np.array([-2, -1, 0, 9_999, 65_535, (1 << 24) - 1], dtype=np.int32)
    fl = np.array([0, 1, 255], dtype=np.uint8)
    bench.dump_outputs(str(tmp_path / "o"), {"a_inv": inv, "a_fl": fl}, 2)
    got = {f[:-4]: np.load(tmp_path / "o" / f) for f in sorted(os.listdir(tmp_path / "o"))}
    assert sorted(got) == ["a_fl", "a_inv"]
    assert got["a_inv"].dtype == np.float32 and got["a_fl"].dtype == np.float32
    assert np.array_equal(got["a_inv"].astype(np.int64), inv) and np.array_equal(got["a_fl"].astype(np.int64), fl)


def test_dump_outputs_bound_and_fixed_sample(tmp_path, monkeypatch):
    # a scaled-down bound: 3 arrays share 12,000 bytes, so each keeps at most 1,000 - 32 float32 values
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 12_000)
    big = np.arange(5_000, dtype=np.int32)
    small = np.arange(100, dtype=np.int32)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "big2": big[::-1].copy(), "small": small}, 3)
    x = {n: np.load(tmp_path / "x" / f"{n}.npy") for n in ("big", "big2", "small")}
    y = {n: np.load(tmp_path / "y" / f"{n}.npy") for n in ("big", "big2", "small")}
    assert all(np.array_equal(x[n], y[n]) for n in x)  # the same sample in every run
    assert np.array_equal(x["small"], small)
    assert len(x["big"]) == 1_000 - 32 and np.all(np.diff(x["big"]) > 0)  # sorted, distinct positions of arange
    assert np.array_equal(x["big2"], 4_999 - x["big"])  # the same positions for every array of that length
    total = sum(os.path.getsize(tmp_path / "x" / f) for f in os.listdir(tmp_path / "x"))
    assert total <= 12_000


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    import oracle as O
    from openwhisk_amd import cluster

    n = 20_000
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                          "--n-activations", str(n), "--dump-outputs", str(tmp_path / "o")],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "decisions/s" and d["higher_is_better"] is True and d["dtype"] == "int32"
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(n / (d["ms_per_step"] * 1e-3), rel=1e-9)
    # what only --full measures or checks is absent from a plain run
    assert all(d[k] is None for k in ("bit_exact", "roofline", "h2d_inclusive", "shim_path", "cpu_baseline"))
    w = cluster.shard_workload("headline", 0, 1, n_activations=n)
    st = O.state_for(w)
    o_inv, o_fl, o_rf = st.replay(w.stream)
    got = {k: np.load(tmp_path / "o" / f"shard0_{k}.npy") for k in ("out_invoker", "out_flags", "rel_flags", "permits")}
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["out_invoker"], o_inv) and np.array_equal(got["out_flags"], o_fl)
    assert np.array_equal(got["rel_flags"], o_rf[: len(got["rel_flags"])]) and len(got["rel_flags"]) == len(w.stream.rel_aid)
    assert np.array_equal(got["permits"], st.permits())
