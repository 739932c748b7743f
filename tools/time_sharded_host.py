"""Host cost of a sharded step: the Python time per call of ShardedRaht.step / local_step at world 1 when the local_ops
do nothing (stub plans and row calls that hand back preallocated tensors). Needs no GPU and no library: what it measures
is the driver's own bookkeeping between the launches, which is what a change to sharded.py can make slower.

  python tools/time_sharded_host.py [--against OTHER_SHARDED_PY] [--runs 9] [--calls 3000]
With --against, the other file is loaded beside this tree's sharded.py and the two are timed alternately, run by run.
Prints one JSON line: microseconds per call, median / min / max over the runs, per leg and per file."""
import argparse
import importlib.util
import json
import os
import sys
import time

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
N, D, ROOTS = 64, 59, 8


class StubPlan:
    def __init__(self, n):
        self.N = n
        self.root_rows = torch.arange(0, n, max(1, n // ROOTS), dtype=torch.int64)
        self.inv_order = torch.arange(n, dtype=torch.int64)
        self.order_RAGFT = self.inv_order
        self._f = {dt: torch.zeros((n, D), dtype=dt) for dt in (torch.float32, torch.float64)}
        self._q = torch.zeros((n, D), dtype=torch.int32)

    def set_row_map(self, row_map, n_matrix_rows):
        pass

    def forward(self, C, want_w=False, roots=None, out=None):
        return self._f[C.dtype] if out is None else out

    def inverse(self, T, roots=None, out=None):
        return self._f[T.dtype] if out is None else out

    def forward_quant(self, C, step, roots=None):
        return self._q

    def dequant_inverse(self, Q, step, roots=None):
        return self._f[torch.float32]


class StubOps:
    quant_dtype = torch.float32

    @staticmethod
    def make_plan(keys, nbits, top_level=None, leaf_weights=None):
        return StubPlan(int(keys.shape[0]))

    quant_rows = quant_rows_f64 = staticmethod(lambda X, step, pos, Q: Q)
    dequant_rows = dequant_rows_f64 = staticmethod(lambda Q, step, pos, out: out)
    rows_gather = rows_scatter = staticmethod(lambda src, pos, out: out)
    forward_quant_mixed = staticmethod(lambda plan, C, step, n_wide, roots=None, roots_wide=None: plan._q)
    dequant_inverse_mixed = staticmethod(lambda plan, Q, step, n_wide, roots=None, roots_wide=None: plan._f[torch.float32])


def legs(mod):
    keys = torch.arange(N, dtype=torch.int64) << 9                     # 15-bit keys, one row per 9-bit prefix node
    C = torch.zeros((N, D), dtype=torch.float32)
    out = {}
    for nw in (0, 3):
        sh = mod.ShardedRaht(keys, 15, prefix_bits=9, local_ops=StubOps, n_wide=nw)
        out[f"step_n_wide_{nw}"] = lambda sh=sh: sh.step(C, 0.01)
        out[f"local_step_n_wide_{nw}"] = lambda sh=sh: sh.local_step(C, 0.01)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", default=None, help="another sharded.py to time beside this tree's")
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--calls", type=int, default=3000)
    a = ap.parse_args()
    from raht_3dgs_codec_amd import sharded
    mods = {"this": sharded}
    if a.against:
        spec = importlib.util.spec_from_file_location("raht_3dgs_codec_amd._other_sharded", a.against)
        mods["other"] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mods["other"])
    fns = {who: legs(m) for who, m in mods.items()}
    us = {who: {leg: [] for leg in f} for who, f in fns.items()}
    for run in range(a.runs + 1):                                       # run 0 warms up and is dropped
        for leg in fns["this"]:
            for who in sorted(fns, reverse=run % 2 == 0):               # alternate who goes first
                fn = fns[who][leg]
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    fn()
                if run:
                    us[who][leg].append((time.perf_counter() - t0) / a.calls * 1e6)
    stat = lambda v: {"median": round(sorted(v)[len(v) // 2], 3), "min": round(min(v), 3), "max": round(max(v), 3)}   # noqa: E731
    print(json.dumps({"kind": "host microseconds per call, stub local_ops, world 1, no GPU", "runs": a.runs, "calls_per_run": a.calls,
                      "us_per_call": {who: {leg: stat(v) for leg, v in d.items()} for who, d in us.items()}}))


if __name__ == "__main__":
    main()
