"""bench.py's plain run: the contract line with exactly --steps timed steps, and --dump-outputs writing what the last timed step
computed -- the same arrays, to rounding, from two runs with the same arguments (the inputs are seeded)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
@pytest.mark.timeout(1300)
def test_plain_run_line_and_dumped_outputs(tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        line = _bench("--workload", "c2_b128", "--steps", "7", "--warmup", "2", "--dump-outputs", str(d))
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["steps"] == 7 and line["warmup"] == 2 and line["ms_per_step"] > 0
        assert line["metric"] == "dgn_layer_fwd_bwd_edges_per_sec" and line["unit"] == "edges/s" and line["dtype"] == "f32"
        assert abs(line["value"] * line["ms_per_step"] * 1e-3 - line["config"]["edges_per_gpu"]) <= 1e-3 * line["config"]["edges_per_gpu"]
        assert "extra" not in line and line["roofline"] is None and line["cpu_baseline"] is None
        files = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(str(d / "*.npy"))}
        assert {"out", "h.grad"} <= set(files) and any(k.endswith("weight.grad") for k in files)
        assert sum(a.nbytes for a in files.values()) < 64e6
        for k, a in files.items():
            assert a.dtype in (np.float32, np.float64), k
            assert np.isfinite(a).all(), k
        assert files["out"].shape[0] == line["config"]["nodes_per_gpu"]
        runs.append(files)
    assert set(runs[0]) == set(runs[1])
    for k in runs[0]:
        np.testing.assert_allclose(runs[0][k], runs[1][k], rtol=1e-4, atol=1e-5, err_msg=k)
