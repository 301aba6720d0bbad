"""The driver parses the LAST stdout line of bench.py; round 3's line grew to 32 KB and was recorded as `parsed: null`
(VERDICT r03 item 1).  The compact line must stay below 4 KB, parse, and carry the contract's fields."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_compact_line_of_the_largest_committed_record_is_small_and_complete():
    b = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r03_bench_default.json")))     # 32 KB, 19 extras
    assert len(json.dumps(full)) > 30000
    last_line = json.dumps(b.compact_line(full))
    assert len(last_line) < 4096
    rec = json.loads(last_line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in rec, key
    assert rec["config"]["workload"].startswith("c2")
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel"):
        assert key in rec["roofline"], key
    assert abs(rec["roofline"]["frac"] - rec["roofline"]["achieved"] / rec["roofline"]["peak"]) < 1e-4
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in rec["cpu_baseline"], key
    assert set(rec["extra"]) >= {"c1", "c3", "c4", "c5"}


def test_compact_line_sheds_fields_rather_than_overflow():
    b = _bench()
    full = json.load(open(os.path.join(ROOT, "profiles", "r03_bench_default.json")))
    full["extra"] = {f"leg{i}": dict(ms_per_step=1.0, value=2.0, roofline=dict(frac=0.5)) for i in range(400)}
    full["ranks"] = [dict(rank=i, nodes=1, edges=2, allreduce_ms=0.1) for i in range(8)]
    rec = b.compact_line(full)
    assert len(json.dumps(rec)) < 4096
    assert "roofline" in rec and "cpu_baseline" in rec and "value" in rec


def test_dump_outputs_sample_is_fixed_and_within_budget():
    """--dump-outputs: arrays over the budget come out as the same seeded row sample on every call (with their row indices), small
    arrays whole, non-float tensors left out, everything together within DUMP_BYTES (under 64 MB)."""
    import numpy as np
    import torch
    b = _bench()
    g = torch.Generator().manual_seed(0)
    named = {"out": torch.randn(300_000, 70, generator=g), "h.grad": torch.randn(300_000, 70, generator=g),
             "w.grad": torch.randn(70, 70, generator=g), "bn.num_batches_tracked": torch.tensor(3), "none.grad": None}
    a1, a2 = b.snapshot_outputs(named), b.snapshot_outputs(named)
    assert set(a1) == {"out", "out_rows", "h.grad", "h.grad_rows", "w.grad"}
    assert sum(a.nbytes for a in a1.values()) <= b.DUMP_BYTES < 64e6
    for k in a1:
        assert a1[k].dtype in (np.float32, np.float64), k
        np.testing.assert_array_equal(a1[k], a2[k])
    rows = a1["out_rows"].astype(np.int64)
    assert len(rows) > 10_000 and np.all(np.diff(rows) > 0)
    np.testing.assert_array_equal(a1["out"], named["out"].numpy()[rows])
    np.testing.assert_array_equal(a1["h.grad_rows"], a1["out_rows"])
    np.testing.assert_array_equal(a1["w.grad"], named["w.grad"].numpy())
    whole = b.snapshot_outputs({"out": named["out"][:1000]})
    assert set(whole) == {"out"} and whole["out"].shape == (1000, 70)
