"""bench.py's two modes: a plain run times the headline step and prints the contract fields only; `--full` adds the
correctness gate against the CPU oracle and the figures that take runs of their own (breakdown, roofline, prelude,
cpu_baseline), as every run did before."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("breakdown_ms", "roofline", "roofline_inv", "path_hbm", "prelude", "cpu_baseline")


def _bench(args, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          timeout=timeout, env=env, cwd=ROOT)


def test_full_is_an_option():
    r = _bench(["--help"], 120)
    assert r.returncode == 0 and "--full" in r.stdout


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_full_adds_gate_and_figures():
    import torch
    assert torch.cuda.is_available(), "this test needs the MI355X"
    args = ["--gpus", "1", "--workload", "cfg2", "--rows", "200000", "--steps", "3", "--warmup", "1", "--settle-steps", "0"]
    outs = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--skip-cpu-baseline"])):
        r = _bench(args + extra, 600)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        outs[mode] = json.loads(lines[0])
    plain, full = outs["plain"], outs["full"]
    for o in (plain, full):
        assert all(k in o for k in CONTRACT)
        assert o["value"] > 0 and o["ms_per_step"] > 0 and o["steps"] == 3 and o["higher_is_better"] is True
    assert plain["metric"] == full["metric"] and plain["unit"] == full["unit"] and plain["dtype"] == full["dtype"]
    assert not any(k in plain for k in FULL_ONLY)
    assert plain["oracle_gate"]["roundtrip_rel_err"] <= 1e-5
    assert all(k in full for k in FULL_ONLY)
    g = full["oracle_gate"]
    assert g["max_rel_err_T"] <= 2e-6 and g["q_beyond_coefficient_error_bound"] == 0 and g["order_RAGFT_equal"]
    assert full["breakdown_ms"]["fwd_quant_fused_ms"] > 0 and 0 < full["roofline"]["frac"] < 1
