"""GPU: `bench.py --dump-outputs DIR` end to end -- the timed region runs exactly --steps steps, the line carries ms_per_step, a plain
run (no --full) leaves out every other leg, and DIR holds what the last timed train step handed its caller (forward outputs, loss
terms, updated parameters) as float32 .npy."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_dump_outputs_of_the_last_timed_step(tmp_path):
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2",
                        "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    # a plain run: nothing after the timed steps but the dump and the line -- every other leg needs --full
    for leg in ("without_cross_step_pipelining", "deterministic_mode", "fp32_mfma_gemms", "bf16x3_forward_operands", "full_row_layout",
                "configs", "dp_collectives", "check_dp", "roofline_mlp", "cpu_baseline"):
        assert line[leg] is None, leg
    arrays = line["dump_outputs"]["arrays"]
    assert {"seeds_xyz", "seeds_points", "votes_xyz", "votes_points", "proposals_xyz", "proposals_output", "losses", "grad"} <= set(arrays)
    total = 0
    for name, shape in arrays.items():
        a = np.load(str(out / (name + ".npy")))
        assert a.dtype == np.float32 and list(a.shape) == shape and np.isfinite(a).all(), name
        total += a.nbytes
    assert total <= 64 << 20
    assert arrays["proposals_output"][:2] == [2, 256] and arrays["losses"] == [12]
