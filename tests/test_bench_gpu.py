"""GPU: a plain `bench.py` run does only what its headline needs; `--full` adds the measurements of their own after the timed
steps (roofline probes here) and leaves the timed steps and what they return untouched."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(args):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None), env.pop("RANK", None), env.pop("LOCAL_RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"] + args,
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_skips_the_extra_legs_and_full_keeps_its_timed_steps(tmp_path):
    plain = _bench(["--dump-outputs", str(tmp_path / "plain")])
    full = _bench(["--full", "--no-modes", "--no-other-configs", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    for j in (plain, full):
        assert all(k in j for k in HEADLINE) and j["value"] > 0 and j["steps"] == 3 and j["warmup"] == 1
        assert j["dtype"] == "bf16" and j["higher_is_better"] is True
    assert not {"parity_mode", "modes", "configs", "cpu_baseline"} & set(plain)
    rf = plain["roofline"]
    assert not {"moe_ffn_block", "dominant_kernel_alone", "launches_timed"} & set(rf)
    assert rf["what"].startswith("whole step") and rf["frac"] == rf["whole_step"]["frac"]
    rf = full["roofline"]
    assert {"moe_ffn_block", "dominant_kernel_alone", "launches_timed"} <= set(rf) and rf["launches_timed"] > 0
    # the legs of --full run after the timed steps: the last timed step's results are the same, bit for bit
    for name in ("sample", "pred_xstart"):
        a, b = np.load(tmp_path / "plain" / f"{name}.npy"), np.load(tmp_path / "full" / f"{name}.npy")
        assert a.shape == (32, 196, 263) and np.isfinite(a).all() and np.array_equal(a, b)
