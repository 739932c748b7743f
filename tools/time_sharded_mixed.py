"""GPU timing of the mixed-precision sharded step (ShardedRaht(n_wide=3)) against the float32 one, in ONE process on ONE GPU.

Scenes:
  cfg5_shard8  the shard of rank 0 when cfg5 (50 M draws, J = 14, 59 channels) is cut for 8 ranks by balanced_prefix_cuts:
               ~6.25 M x 59, keys and attributes generated on the device from the cfg5 seed (as bench.py does for cfg5)
  cfg3_pb9     cfg3 (3 M draws, J = 12, 59 channels) as ONE shard with prefix_bits = 9
Legs, alternating float32 / mixed inside every round: local_step(C, 0.01) (truncated fused passes with their root buffers, no
exchange, no top tree) and step(C, 0.01) (the whole sharded step: a one-rank NCCL group with force_collectives=True, so the
all-gathers run through RCCL); collective_ms() over the timed steps covers every gather of a direction (mixed: the float
and the wide one).

  python tools/time_sharded_mixed.py [--scene cfg5_shard8|cfg3_pb9|all] [--rounds 5] [--reps 20] [--leg LEG]
--leg f32_local|mx_local|f32_step|mx_step runs that one leg only (for a rocprofv3 --kernel-trace --stats run). Prints one JSON line.
"""
import argparse
import json
import os
import socket
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def device_scene(n_draws, J, D, seed, world, rank, dev):
    """the cfg5 generation of bench.py (sorted unique 3J-bit keys, N(0,1) attributes in column blocks of 8 from one device
    generator), cut for `world` ranks; -> this rank's keys and attributes"""
    from raht_3dgs_codec_amd import sharded
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    kraw = torch.randint(0, 1 << (3 * J), (int(n_draws * 1.002),), device=dev, dtype=torch.int64, generator=g)
    kd_all = torch.unique(kraw)[:n_draws].contiguous()
    del kraw
    N = int(kd_all.shape[0])
    cuts = sharded.balanced_prefix_cuts(kd_all, 3 * J, world, prefix_bits=9)
    lo, hi = cuts[rank], cuts[rank + 1]
    kd = kd_all[lo:hi].contiguous()
    del kd_all
    Cd = torch.empty((hi - lo, D), dtype=torch.float32, device=dev)
    for c0 in range(0, D, 8):
        blk = torch.randn((N, min(8, D - c0)), device=dev, generator=g)
        Cd[:, c0:c0 + 8] = blk[lo:hi]
        del blk
    return kd, Cd


def scene(name, dev):
    import numpy as np
    from raht_3dgs_codec_amd import synth
    if name == "cfg5_shard8":
        n, J, D, seed = synth.CONFIGS["cfg5"]
        kd, Cd = device_scene(n, J, D, seed, 8, 0, dev)
        return kd, Cd, 3 * J
    n, J, D, seed = synth.CONFIGS["cfg3"]
    _, keys, C = synth.scene(n, J, D, seed)
    return torch.from_numpy(keys.view(np.int64)).to(dev), torch.from_numpy(C).to(dev), 3 * J


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="all", choices=["all", "cfg5_shard8", "cfg3_pb9"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", type=float, default=0.01)
    ap.add_argument("--leg", default=None, choices=["f32_local", "mx_local", "f32_step", "mx_step"])
    a = ap.parse_args()
    import torch.distributed as dist
    from raht_3dgs_codec_amd import sharded
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    out = {"kind": "sharded mixed (n_wide=3) vs float32 step, one process, one GPU", "step": a.step, "scenes": {}}
    names = ["cfg5_shard8", "cfg3_pb9"] if a.scene == "all" else [a.scene]
    for name in names:
        kd, Cd, nbits = scene(name, dev)
        sh = {"f32": sharded.ShardedRaht(kd, nbits, prefix_bits=9, force_collectives=True),
              "mx": sharded.ShardedRaht(kd, nbits, prefix_bits=9, force_collectives=True, n_wide=3)}
        legs = {f"{k}_local": (lambda s=s: s.local_step(Cd, a.step)) for k, s in sh.items()}
        legs.update({f"{k}_step": (lambda s=s: s.step(Cd, a.step)) for k, s in sh.items()})
        if a.leg:
            legs = {a.leg: legs[a.leg]}
        for fn in legs.values():                                   # warm-up: schedules, workspaces, buffers, communicators
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        res = {k: [] for k in legs}
        coll = {"f32": [], "mx": []}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                which = k.split("_")[0]
                if k.endswith("_step"):
                    sh[which].time_collectives(True)
                res[k].append(timed(fn, a.reps))
                if k.endswith("_step"):
                    coll[which].append(sh[which].collective_ms())
                    sh[which].time_collectives(False)
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        r = {"rows": int(kd.shape[0]), "n_roots": sh["f32"].n_roots, "ms_median": {k: round(v, 4) for k, v in med.items()},
             "ms_all": {k: [round(x, 4) for x in v] for k, v in res.items()}}
        for part in ("local", "step"):
            if f"f32_{part}" in med and f"mx_{part}" in med:
                r[f"{part}_ratio_mx_over_f32"] = round(med[f"mx_{part}"] / med[f"f32_{part}"], 4)
        for which, v in coll.items():
            if v:
                r[f"collective_ms_{which}"] = {"forward": round(sorted(x[0] for x in v)[len(v) // 2], 4),
                                               "inverse": round(sorted(x[1] for x in v)[len(v) // 2], 4)}
        if "collective_ms_f32" in r and "collective_ms_mx" in r:
            r["wide_gathers_add_us_per_step"] = round(1e3 * sum(r["collective_ms_mx"][d] - r["collective_ms_f32"][d]
                                                               for d in ("forward", "inverse")), 2)
        out["scenes"][name] = r
        del sh, legs, kd, Cd
        torch.cuda.empty_cache()
    torch.cuda.synchronize()
    dist.destroy_process_group()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
