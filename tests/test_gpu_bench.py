"""bench.py on one GPU: a plain run prints the headline record alone (no roofline, CPU baseline or side workloads: each of those needs runs of
its own); --full adds them after the same timed steps and changes neither the headline fields nor what --dump-outputs writes.  Small custom
shapes keep every run to seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "scaling", "config")
MEASURED_APART = ("roofline", "cpu_baseline", "workloads")


def _bench(*args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    shape = ("--batch", "2", "--seq-len", "256", "--nfe", "2", "--steps", "2", "--warmup", "1")
    plain = _bench(*shape, "--dump-outputs", str(tmp_path / "plain"))
    assert all(k in plain for k in HEADLINE) and not any(k in plain for k in MEASURED_APART)
    assert plain["metric"] == plain["unit"] == "mel-frames/s" and plain["higher_is_better"] is True and plain["dtype"] == "bf16"
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["value"] > 0
    assert plain["value"] == pytest.approx(2 * 256 / (plain["ms_per_step"] * 1e-3), rel=1e-3)  # frames per second of the timed steps
    full = _bench(*shape, "--full", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    assert all(k in full for k in HEADLINE) and "cpu_baseline" not in full and "workloads" not in full  # (a custom shape has no side workloads)
    assert {k["kernel"] for k in full["roofline"]["kernels"]} >= {"qkv", "attention", "attn_out", "ff1", "ff2"}
    assert full["roofline"]["achieved"] > 0
    # the same seeded weights and inputs, the same timed steps: the dumped mels agree bit for bit
    a, b = np.load(tmp_path / "plain" / "mel.npy"), np.load(tmp_path / "full" / "mel.npy")
    assert a.shape == (2, 256, 100) and np.isfinite(a).all() and np.array_equal(a, b)


def test_plain_vocoder_run_is_the_headline_and_full_adds_the_head_roofline():
    shape = ("--workload", "vocos", "--batch", "2", "--seq-len", "64", "--steps", "2", "--warmup", "1")
    plain = _bench(*shape)
    assert plain["metric"] == "vocoder mel-frames/s" and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert not any(k in plain for k in MEASURED_APART)
    full = _bench(*shape, "--full", "--no-cpu-baseline")
    assert full["roofline"]["bound"] == "hbm" and full["roofline"]["achieved"] > 0 and "cpu_baseline" not in full
