"""bench.py end to end on the GPU: a plain run (no --full) carries the headline keys and none of the --full legs, and two
runs with the same arguments dump the same outputs (--dump-outputs)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _bench(*args):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MSG_LIB_VARIANT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--resolution", "64", "--batch", "4", *args]
    run = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, run.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_dumps_reproducible_outputs(tmp_path):
    runs = [_bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for out in runs:
        assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
        assert out["unit"] == "img/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
        assert out["value"] > 0 and out["ms_per_step"] > 0
        assert out["losses"] and all(v == v and abs(v) != float("inf") for v in out["losses"].values())
        # the --full legs stay out of a plain run
        assert out["roofline"] is None and out["kernels"] == {} and out["clock_iterations"] == 0 and out["h2d"] is None
        assert not {"cpu_baseline", "value_fp32_path", "value_fp32_split_path", "value_dead_work_elided"} & set(out)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"generator_params.npy", "discriminator_params.npy", "generator_ema_params.npy",
            "loss_generator.npy", "loss_discriminator_real.npy"} <= set(names)
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        assert np.array_equal(a, b), n                       # seeded inputs, deterministic step: the same numbers
        total += a.nbytes
    assert total <= 64 * 2 ** 20
    # the dumped losses are the last step's: the ones the JSON line reports for the keys every step logs
    assert np.load(tmp_path / "a" / "loss_generator.npy").tolist() == [pytest.approx(runs[0]["losses"]["loss_generator"], abs=1e-5)]
