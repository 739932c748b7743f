#!/usr/bin/env python3
"""Times the mixed-precision batch entries against their alternatives on frame sequences.

Two workloads, a full step (forward + quantize, dequantize + inverse) of every scene each:
  frames : --frames scenes of the reference's operating point (~1 M voxels x 59 channels, J = 10, synth.scene)
  cfg4   : the first --batch-scenes draws of BASELINE configs[3] (1-6 M x 59, J = 12)
Four legs per workload:
  a  mixed, one call per scene          (plan.forward_quant_mixed / dequant_inverse_mixed)
  b  mixed batch                        (ops.forward_quant_mixed_batch / dequant_inverse_mixed_batch)
  c  float32 batch                      (ops.forward_quant_batch / dequant_inverse_batch)
  d  float32, one call per scene        (plan.forward_quant / dequant_inverse)
One process; every leg is warmed before anything is timed; a repeat times --steps steps of one leg with a host clock that ends in
a device synchronise; the legs alternate inside every repeat (a b c d, a b c d, ...), so drift hits all of them alike. Reported
per leg: the median over the repeats, the smallest and the largest (the spread), and the ratios b/a, b/c of the medians.

    python tools/time_mixed_batch.py --out profiles/mixed_batch.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--frame-draws", type=int, default=1_000_000)
    ap.add_argument("--batch-scenes", type=int, default=4, help="cfg4 scenes (0: skip that workload)")
    ap.add_argument("--steps", type=int, default=10, help="steps per timed repeat")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps of every leg before the first repeat")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--quant-step", type=float, default=0.01)
    ap.add_argument("--n-wide", type=int, default=3)
    ap.add_argument("--only-leg", default="", help="run ONE leg of the frames workload, nothing timed (for a kernel trace): a, b, c or d")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.repeats < 5 and not a.only_leg:
        ap.error("--repeats must be at least 5 (median and spread)")

    import numpy as np
    import torch
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no CPU path"
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import ops, synth
    dev = torch.device("cuda:0")
    qs, nw = a.quant_step, a.n_wide

    def scenes(draws, J, D, seed0):
        plans, Cs = [], []
        for i, n in enumerate(draws):
            V, keys, C = synth.scene(n, J, D, seed0 + i)
            plans.append(R.RahtPlan.from_keys(torch.from_numpy(keys.view(np.int64)).to(dev), 3 * J))
            Cs.append(torch.from_numpy(C).to(dev))
        return plans, Cs

    def legs_of(plans, Cs):
        return {
            "a_mixed_one_call_per_scene": lambda: [p.dequant_inverse_mixed(p.forward_quant_mixed(c, qs, nw), qs, nw) for p, c in zip(plans, Cs)],
            "b_mixed_batch": lambda: ops.dequant_inverse_mixed_batch(plans, ops.forward_quant_mixed_batch(plans, Cs, qs, nw), qs, nw),
            "c_float32_batch": lambda: ops.dequant_inverse_batch(plans, ops.forward_quant_batch(plans, Cs, qs), qs),
            "d_float32_one_call_per_scene": lambda: [p.dequant_inverse(p.forward_quant(c, qs), qs) for p, c in zip(plans, Cs)],
        }

    def measure(name, plans, Cs):
        legs = legs_of(plans, Cs)
        # the batch is the looped call, bit for bit, at the sizes timed here
        Qb = ops.forward_quant_mixed_batch(plans, Cs, qs, nw)
        assert all(torch.equal(q, p.forward_quant_mixed(c, qs, nw)) for q, p, c in zip(Qb, plans, Cs)), "mixed batch != single-scene calls"
        del Qb
        for f in legs.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for _ in range(a.repeats):
            for k, f in legs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    f()
                torch.cuda.synchronize()
                ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        D = int(Cs[0].shape[1])
        res = {"scenes": [int(p.N) for p in plans], "rows_total": int(sum(p.N for p in plans)), "channels": D,
               "steps_per_repeat": a.steps, "repeats": a.repeats, "warmup_steps": a.warmup, "quant_step": qs, "n_wide": nw,
               "stages_of_scene_0": len(plans[0].mixed_stats(D, nw)["rows_per_stage"]),
               "launches_mixed_batch": {d: ops.mixed_batch_stats(plans, D, nw, inverse=(d == "inverse")) for d in ("forward", "inverse")},
               "ms_per_step": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                                   "all": [round(x, 4) for x in v]} for k, v in ms.items()}}
        med = {k: statistics.median(v) for k, v in ms.items()}
        res["b_over_a"] = round(med["b_mixed_batch"] / med["a_mixed_one_call_per_scene"], 4)
        res["b_over_c"] = round(med["b_mixed_batch"] / med["c_float32_batch"], 4)
        res["c_over_d"] = round(med["c_float32_batch"] / med["d_float32_one_call_per_scene"], 4)
        print(name, json.dumps(res["ms_per_step"]), "b/a", res["b_over_a"], "b/c", res["b_over_c"], flush=True)
        return res

    if a.only_leg:
        plans, Cs = scenes([a.frame_draws] * a.frames, 10, 59, 100)
        f = [v for k, v in legs_of(plans, Cs).items() if k.startswith(a.only_leg + "_")][0]
        for _ in range(a.warmup + a.steps):
            f()
        torch.cuda.synchronize()
        return
    out = {"tool": "tools/time_mixed_batch.py", "device": torch.cuda.get_device_name(0),
           "clock": "host perf_counter around --steps steps, device synchronised before and after; legs alternate inside every repeat"}
    plans, Cs = scenes([a.frame_draws] * a.frames, 10, 59, 100)
    out["frames"] = measure("frames", plans, Cs)
    del plans, Cs
    if a.batch_scenes > 0:
        n_draws, J, D, seed = synth.CONFIGS["cfg4"]
        plans, Cs = scenes(synth.CFG4_DRAWS[:a.batch_scenes], J, D, seed)
        out["cfg4"] = measure("cfg4", plans, Cs)
        del plans, Cs
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
