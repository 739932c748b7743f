#!/usr/bin/env python3
"""One depth-2 cell of the cfg3-shaped frame (59 columns, xyz wide) through bitstream.decode_region_bytes, with and without the keys
of an earlier call, against decode_frame_bytes on the same blob, at seg_len 2048 and 512; in one process, alternating, wall times
that end in a device synchronise (median and spread). Also: the region decoder's stages one by one (each a wall time ending in a
synchronise), the share of the segments and of the bytes the region needs, and both decoders' errors on the region's rows against
each other. Writes one JSON file.
   python tools/time_region.py [out.json] [reps] [draws]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raht_3dgs_codec_amd import bitstream, ops, synth  # noqa: E402
from raht_3dgs_codec_amd.geometry import OctreeCoder  # noqa: E402
from raht_3dgs_codec_amd.rlgr import SegmentedCoder  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "region.json")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
draws = int(sys.argv[3]) if len(sys.argv) > 3 else synth.CONFIGS["cfg3"][0]
DEPTH, STEP, N_WIDE = 2, 0.01, 3
assert torch.cuda.is_available(), "a measurement needs the GPU"

_, J, D, seed = synth.CONFIGS["cfg3"]
V, keys, C = synth.scene(draws, J, D, seed)
N = len(keys)
# the occupied depth-2 cell of median population
cell, count = np.unique(keys >> np.uint64(3 * (J - DEPTH)), return_counts=True)
pick = int(np.argsort(count, kind="stable")[len(count) // 2])
c0 = int(cell[pick])


def sync():
    torch.cuda.synchronize()


def timed(fns, warm=2):
    """fns: {name: callable}; alternates them inside every repetition -> {name: {median_ms, min_ms, max_ms}}"""
    for _ in range(warm):
        for f in fns.values():
            f()
            sync()
    ts = {n: [] for n in fns}
    for _ in range(reps):
        for n, f in fns.items():
            sync()
            t = time.perf_counter()
            f()
            sync()
            ts[n].append((time.perf_counter() - t) * 1e3)
    return {n: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "reps": len(v)} for n, v in ts.items()}


result = {"N": N, "J": J, "D": D, "n_wide": N_WIDE, "step": STEP, "depth": DEPTH, "cell": c0, "cell_voxels": int(count[pick]),
          "occupied_cells": len(cell), "reps": reps, "device": torch.cuda.get_device_name(0), "seg_len": {}}
for S in (2048, 512):
    blob = bitstream.encode_frame_bytes(V, C, J, STEP, "cuda", n_wide=N_WIDE, seg_len=S)
    Vw, Cw = bitstream.decode_frame_bytes(blob, "cuda")
    Vr, Cr, info = bitstream.decode_region_bytes(blob, DEPTH, (c0, c0 + 1), "cuda")
    a, b = info["rows"]
    assert b - a == int(count[pick]) and torch.equal(Vr, Vw[a:b])
    kd = info["keys"]
    diff = (Cr.double() - Cw[a:b].double()).abs().max(dim=0).values
    scale = Cw[a:b].abs().max(dim=0).values.double()
    whole = timed({"decode_frame_bytes": lambda: bitstream.decode_frame_bytes(blob, "cuda"),
                   "decode_region_bytes": lambda: bitstream.decode_region_bytes(blob, DEPTH, (c0, c0 + 1), "cuda"),
                   "decode_region_bytes_cached_keys": lambda: bitstream.decode_region_bytes(blob, DEPTH, (c0, c0 + 1), "cuda", keys=kd)})
    # the stages of the region decoder, and the whole-frame decoder's for comparison
    h = bitstream.parse_frame(blob)
    (go, gl), (ao, al) = h["geometry"], h["attributes"]
    att, tl = blob[ao: ao + al], 3 * (J - DEPTH)
    n_d = OctreeCoder.parse(blob[go: go + gl])["counts"][DEPTH]
    ck, cf = ops.region_cells(kd, 3 * J, tl, n_d)
    n_top, runs = bitstream.region_runs(ops.region_layout(kd, 3 * J, a, b).tolist(), J, DEPTH, 1)
    ids, compact = bitstream.region_segments(n_top, runs, S)
    sc = SegmentedCoder.from_container_segments(att, ids, "cuda")[0]
    sc_all = SegmentedCoder.from_container(att, "cuda")
    Qc, Qall = sc.decode(row_major=True), sc_all.decode(row_major=True)
    top = ops.RahtPlan.from_keys(ck, 3 * DEPTH, leaf_weights=cf[1:] - cf[:-1])
    plan = ops.RahtPlan.from_keys(kd[a:b], 3 * J, top_level=tl)
    full = ops.RahtPlan.from_keys(kd, 3 * J)
    Qr = ops.region_assemble(Qc, [(compact(r), d, n) for r, d, n in runs], b - a)
    j0 = int(torch.searchsorted(ck, torch.tensor([c0], device="cuda")).item())
    roots = top.dequant_inverse(Qc[:n_top], STEP)[j0: j0 + 1].contiguous()
    wide = top.dequant_inverse(Qc[:n_top, :N_WIDE], STEP, dtype=torch.float64)[j0: j0 + 1].contiguous()
    stages = timed({
        "geometry_decode": lambda: OctreeCoder.decode(blob[go: go + gl], "cuda"),
        "region_cells": lambda: ops.region_cells(kd, 3 * J, tl, n_d),
        "region_layout_and_read_back": lambda: ops.region_layout(kd, 3 * J, a, b).tolist(),
        "select_and_upload_segments": lambda: SegmentedCoder.from_container_segments(att, ids, "cuda"),
        "entropy_decode_selected": lambda: sc.decode(row_major=True),
        "top_plan_build": lambda: ops.RahtPlan.from_keys(ck, 3 * DEPTH, leaf_weights=cf[1:] - cf[:-1]),
        "top_inverse_float32_and_float64": lambda: (top.dequant_inverse(Qc[:n_top], STEP), top.dequant_inverse(Qc[:n_top, :N_WIDE], STEP, dtype=torch.float64)),
        "region_plan_build": lambda: ops.RahtPlan.from_keys(kd[a:b], 3 * J, top_level=tl),
        "region_assemble": lambda: ops.region_assemble(Qc, [(compact(r), d, n) for r, d, n in runs], b - a),
        "region_inverse_mixed": lambda: plan.dequant_inverse_mixed(Qr, STEP, N_WIDE, roots=roots, roots_wide=wide),
        "demorton_region": lambda: ops.demorton(kd[a:b], J),
        "whole_upload_container": lambda: SegmentedCoder.from_container(att, "cuda"),
        "whole_entropy_decode": lambda: sc_all.decode(row_major=True),
        "whole_plan_build": lambda: ops.RahtPlan.from_keys(kd, 3 * J),
        "whole_inverse_mixed": lambda: full.dequant_inverse_mixed(Qall, STEP, N_WIDE),
    })
    frame = {"blob_bytes": len(blob), "rows": [a, b], "segments_decoded": info["segments_decoded"], "segments_total": info["segments_total"],
             "segment_share": round(info["segments_decoded"] / info["segments_total"], 4), "bytes_needed": info["bytes_needed"],
             "byte_share": round(info["bytes_needed"] / len(blob), 4), "byte_ranges": len(info["byte_ranges"]), "calls": whole, "stages": stages,
             "region_vs_whole_max_abs_diff_over_column_max": float((diff / scale).max().item()),
             "bit_identical_share": float((Cr.view(torch.int32) == Cw[a:b].view(torch.int32)).double().mean().item())}
    result["seg_len"][str(S)] = frame
    print(S, json.dumps(frame))
    del Qc, Qall, sc, sc_all, top, plan, full, Qr

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", out_path)
