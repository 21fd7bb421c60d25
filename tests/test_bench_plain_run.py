"""bench.py's plain command line on the GPU: `python bench.py --gpus 1 --steps N --warmup W` is the headline alone — set-up,
warm-up, the timed steps and the result line — and everything else the benchmark measures or checks waits for --full."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir))

# seconds a plain run may spend outside its warm-up and timed steps: whole process, start to exit
OVERHEAD_BOUND_S = 30.0


def test_full_is_an_option_and_off_by_default():
    usage = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], text=True, timeout=120)
    assert "--full" in usage and "--dump-outputs" in usage


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_lean():
    steps, warmup = 3, 1
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    t0 = time.perf_counter()
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                                   "--warmup", str(warmup)], env=env, text=True, timeout=600)
    wall = time.perf_counter() - t0
    r = json.loads(out.strip().splitlines()[-1])
    assert r["unit"] == "PBS/s" and r["higher_is_better"] is True and r["dtype"] == "f64 (u64 torus)"
    assert r["n_gpus"] == 1 and r["steps"] == steps and r["warmup"] == warmup
    assert r["value"] == pytest.approx(4096 * steps / (r["ms_per_step"] * steps * 1e-3), rel=1e-6)
    # what moved behind --full is not in the line
    assert "extra" not in r and "cpu_baseline" not in r
    assert "measured in this bench run" not in r["roofline"]["traffic_source"]
    overhead = wall - (steps + warmup) * r["ms_per_step"] * 1e-3
    print(f"plain run: {wall:.1f} s of wall time, {overhead:.1f} s outside its {steps + warmup} steps")
    assert overhead <= OVERHEAD_BOUND_S
