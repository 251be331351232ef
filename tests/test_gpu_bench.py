"""bench.py at a small shape on the GPU: a plain run prints the headline line only, `--dump-outputs` writes the last
timed step's loss and gradients, `--full` adds the secondary figures (per-kernel rooflines, the fp32 modes)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--bev", "28", "--batch", "1"]
SECONDARY = {"roofline", "roofline_hbm", "roofline_lds", "bf16x3_mode", "f32_mode", "cpu_baseline"}


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL, *args], capture_output=True, text=True,
                       timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_only_and_dumps_the_last_step(tmp_path):
    rec = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["unit"] == "samples/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "bf16" and rec["value"] > 0 and rec["ms_per_step"] > 0
    assert abs(rec["value"] * rec["ms_per_step"] - 1e3) < 20       # batch 1: samples/s = 1000 / ms_per_step
    assert not SECONDARY & set(rec)
    files = sorted(os.listdir(tmp_path))
    assert {"loss.npy", "grad.bev_embedding.weight.npy",
            "grad.layers.1.spatial_cross_attn.spatial_deform_attn.rpe_table.npy"} <= set(files)
    total = 0
    for f in files:
        a = np.load(tmp_path / f)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), f
        total += a.nbytes
    assert total <= 64 << 20
    assert np.abs(np.load(tmp_path / "grad.bev_embedding.weight.npy")).max() > 0


def test_runs_with_the_same_arguments_compute_the_same_outputs(tmp_path):
    """Every step starts from the seeded weights, so the last timed step has the same inputs in every run: its loss is
    identical bit for bit, its gradients differ only by the rounding of the backward's float atomics."""
    for run in ("a", "b"):
        _bench("--steps", "3", "--warmup", "2", "--dump-outputs", str(tmp_path / run))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(os.listdir(tmp_path / "b"))
    a = {f: np.load(tmp_path / "a" / f) for f in files}
    b = {f: np.load(tmp_path / "b" / f) for f in files}
    np.testing.assert_array_equal(a["loss.npy"], b["loss.npy"])
    # atomically reduced weight gradients (depthwise convolutions, rpe tables) cancel: their rounding is relative to the
    # size of the summed terms, seen up to ~1.5e-5 of the largest gradient entry at this shape
    scale = max(np.abs(v).max() for f, v in a.items() if f.startswith("grad."))
    for f in files:
        np.testing.assert_allclose(b[f], a[f], rtol=1e-3, atol=5e-4 * scale, err_msg=f)
        # and on each array's own scale, within the rounding of this bf16 path (no gradient that is pure noise)
        assert np.abs(b[f] - a[f]).max() <= 5e-3 * np.abs(a[f]).max(), f


def test_full_run_adds_the_secondary_figures():
    rec = _bench("--full", "--steps", "1", "--warmup", "1", "--f32-steps", "1", "--no-cpu-baseline")
    assert SECONDARY - {"cpu_baseline"} <= set(rec) and "cpu_baseline" not in rec
    assert rec["roofline"]["kernel"].startswith("bevr_attn") and rec["bf16x3_mode"]["value"] > 0
