"""bench.py end to end on a small generated mesh: a plain run prints the headline line and nothing that takes runs of its
own; --full adds the run in the other storage mode.  (The CPU baseline of --full is left out here: it times the host for
about 40 s by design.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SMALL = ["--tets", "6000", "--steps", "2", "--warmup", "1"]


def _bench(tmp_path, *args):
    tmpdir = tmp_path / "tmp"
    tmpdir.mkdir()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env["TMPDIR"] = str(tmpdir)
    res = subprocess.run([sys.executable, str(ROOT / "bench.py"), *SMALL, *args], cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    assert not [p.name for p in tmpdir.iterdir() if p.name.startswith("vaspfsi_bench_")], "generated mesh left behind"
    return json.loads(lines[0])


def test_a_plain_run_does_only_the_headline(tmp_path):
    out = _bench(tmp_path, "--dump-outputs", str(tmp_path / "dump"))
    assert out["unit"] == "Newton-iterations/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(out["newton_iterations"] / (2 * out["ms_per_step"] * 1e-3))
    assert out["roofline"]["kernel"] in out["kernels"]
    assert "cpu_baseline" not in out and not [k for k in out if k.endswith("_storage")]
    for name in ("displacement", "velocity", "pressure", "newton_history"):
        assert np.load(tmp_path / "dump" / f"{name}.npy").dtype == np.float64


def test_full_adds_the_other_storage_mode(tmp_path):
    out = _bench(tmp_path, "--full", "--no-cpu-baseline")
    assert out["dtype"] == "f64" and "cpu_baseline" not in out
    side = out["mixed_storage"]
    assert "error" not in side, side
    assert out["value_mixed_storage"] == side["value"] > 0 and out["ms_per_step_mixed_storage"] == side["ms_per_step"] > 0
    assert side["dtype"] != "f64"
