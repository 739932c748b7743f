#!/usr/bin/env python3
"""The octree geometry stage (geometry.OctreeCoder, csrc/octree.hip) on the cfg2 and cfg3 key sets, stage by stage, and -- in the
same process -- its two neighbours: raht_plan_create_from_keys on the same keys and the attribute entropy coder's encode + decode
of one quantization step of the same frame at D = 56 (seg_len 2048, row-major, as encode_frame codes it).

Per stage: HIP events around enough back-to-back calls to fill `min_s` seconds, `reps` (>= 20) repetitions after a warm-up, the
median / min / max ms per call. Stages: counts, encode (occupancy stream), symbols (histogram + rank table + map), RLGR encode,
RLGR decode, bytes (rank -> byte), decode (stream -> keys); the RLGR stages and the two totals (counts -> streams on the device;
streams -> keys) for every seg_len of SEG_LENS; container bytes per mode and seg_len. Prints one JSON line (profiles/geometry.json).
   python tools/time_geometry.py [reps] [min_s] [cfg ...]
   python tools/time_geometry.py trace [cfg]     ONE encode + ONE decode of the section (mode 1, default seg_len), nothing else: the
                                                 run to put under `rocprofv3 --kernel-trace --stats` for launch counts"""
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raht_3dgs_codec_amd as R  # noqa: E402
from raht_3dgs_codec_amd import geometry, rlgr, synth  # noqa: E402

TRACE = len(sys.argv) > 1 and sys.argv[1] == "trace"
if TRACE:
    sys.argv[1:] = ["21", "0.05"] + sys.argv[2:3]
reps = max(20, int(sys.argv[1])) if len(sys.argv) > 1 else 21
min_s = float(sys.argv[2]) if len(sys.argv) > 2 else 0.05
cfgs = sys.argv[3:] or ["cfg2", "cfg3"]
SEG_LENS = (256, 512, 1024, 2048)
OC = geometry.OctreeCoder


def timed(fn):
    """-> ms per call: median / min / max over `reps` repetitions of as many back-to-back calls as fill min_s"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    n = max(1, math.ceil(min_s / max(time.perf_counter() - t, 1e-6)))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / n)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": reps, "calls_per_rep": n}


def scene(cfg):
    n, J, _, seed = synth.CONFIGS[cfg]
    keys = synth.sorted_unique_keys(n, J, seed)
    res = {"N": int(len(keys)), "J": J}
    kd = torch.from_numpy(keys.view(np.int64)).cuda()
    counts = OC.counts(kd, J)
    n_nodes = sum(counts[:-1])
    res["n_nodes"] = n_nodes
    occ = torch.empty(n_nodes, dtype=torch.uint8, device="cuda")
    sym = torch.empty((1, n_nodes), dtype=torch.int32, device="cuda")
    occ2 = torch.empty(n_nodes, dtype=torch.uint8, device="cuda")
    keys2 = torch.empty(len(keys), dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    OC.occupancy(kd, J, counts, out=occ)
    _, table = OC.symbols(occ, out=sym)
    st = res["stages"] = {}
    st["counts"] = timed(lambda: OC.counts(kd, J))
    st["encode"] = timed(lambda: OC.occupancy(kd, J, counts, out=occ))
    st["symbols"] = timed(lambda: OC.symbols(occ, out=sym))
    st["bytes"] = timed(lambda: OC.bytes_from_symbols(sym, table, bad, out=occ2))
    st["decode"] = timed(lambda: OC.keys_from_occupancy(occ, counts, J, bad, out=keys2))
    assert torch.equal(keys2, kd) and torch.equal(occ2, occ) and int(bad.item()) == 0
    st["counts_plus_encode"] = timed(lambda: (OC.counts(kd, J), OC.occupancy(kd, J, counts, out=occ)))
    res["bytes_raw"] = len(OC.encode(kd, J, entropy="raw"))
    res["seg_len"] = {}
    out = torch.empty((1, n_nodes), dtype=torch.int32, device="cuda")
    for S in SEG_LENS:
        sc = rlgr.SegmentedCoder(n_nodes, 1, S, 0, "cuda")
        r = res["seg_len"][str(S)] = {"lanes": sc.G}
        r["rlgr_encode"] = timed(lambda: sc.encode(sym))
        r["rlgr_decode"] = timed(lambda: sc.decode(out=out))
        assert torch.equal(out, sym) and int(sc.bad.item()) == 0

        def enc():
            c = OC.counts(kd, J)
            OC.occupancy(kd, J, c, out=occ)
            OC.symbols(occ, out=sym)
            sc.encode(sym)

        def dec():
            sc.decode(out=out)
            OC.bytes_from_symbols(out, table, bad, out=occ2)
            OC.keys_from_occupancy(occ2, counts, J, bad, out=keys2)

        r["geometry_encode"] = timed(enc)
        r["geometry_decode"] = timed(dec)
        assert torch.equal(keys2, kd) and int(bad.item()) == 0
        r["geometry_total_ms"] = round(r["geometry_encode"]["median_ms"] + r["geometry_decode"]["median_ms"], 4)
        r["bytes_rlgr"] = len(OC.encode(kd, J, seg_len=S))
        r["ratio_to_raw"] = round(r["bytes_rlgr"] / res["bytes_raw"], 4)
        del sc
    # the neighbours, same process, same keys
    plans = []

    def plan():
        plans.clear()                                     # (destroys the previous plan: its blocks go back to the cache)
        plans.append(R.RahtPlan.from_keys(kd, 3 * J))

    st["plan_create_from_keys"] = timed(plan)
    res["counts_plus_encode_over_plan"] = round(st["counts_plus_encode"]["median_ms"] / st["plan_create_from_keys"]["median_ms"], 3)
    D = 56
    C = torch.from_numpy(synth.gaussian_attributes(len(keys), D, synth.CONFIGS[cfg][3])).cuda()
    Q = plans[0].forward_quant(C, 0.01)
    ac = rlgr.SegmentedCoder(len(keys), D, 2048, 1, "cuda")
    Qo = torch.empty_like(Q)
    a = res["attribute_coder_D56_step0.01"] = {"lanes": ac.G}
    a["encode"] = timed(lambda: ac.encode(Q))
    a["decode"] = timed(lambda: ac.decode(out=Qo, row_major=True))
    assert torch.equal(Qo, Q)
    a["total_ms"] = round(a["encode"]["median_ms"] + a["decode"]["median_ms"], 4)
    S = str(geometry.DEFAULT_SEG_LEN)
    res["default_seg_len"] = geometry.DEFAULT_SEG_LEN
    res["geometry_total_over_attribute_step"] = round(res["seg_len"][S]["geometry_total_ms"] / a["total_ms"], 3)
    return res


def trace(cfg):
    n, J, _, seed = synth.CONFIGS[cfg]
    keys = synth.sorted_unique_keys(n, J, seed)
    kd = torch.from_numpy(keys.view(np.int64)).cuda()
    blob = OC.encode(kd, J)
    assert torch.equal(OC.decode(blob, "cuda"), kd)
    print(json.dumps({"cfg": cfg, "N": int(len(keys)), "section_bytes": len(blob)}))


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    if TRACE:
        return trace(cfgs[0] if sys.argv[3:] else "cfg3")
    out = {"what": "octree geometry stage, per stage and against its neighbours (tools/time_geometry.py)", "reps": reps, "min_s": min_s,
           "device": torch.cuda.get_device_name(0)}
    for cfg in cfgs:
        out[cfg] = scene(cfg)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
