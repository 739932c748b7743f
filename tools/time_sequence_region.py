#!/usr/bin/env python3
"""One depth-2 cell of the LAST frame of a motion-compensated sequence (tools/time_motion.py's: 8 frames of about 1 M voxels x 56
columns, J = 10, moving by (1, 0, -1) a frame, gop 8, motion 1, blocks of 16 voxels a side) through
bitstream.decode_sequence_region, cold and with the keys of an earlier call, against decode_sequence_bytes(blob, [7]) on the same
blob, at seg_len 2048 and 512; in one process, alternating, two warm-ups, wall times that end in a device synchronise (median, min,
max). Also: the bytes the call needs against the bytes of the 8 frames, the needed set along the chain, and the three entry
points under the call alone, on the intra frame's needed set (layout, assemble) and on the last frame's region (needs). Writes one
JSON file.   python tools/time_sequence_region.py [out.json] [reps] [draws]"""
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

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "sequence_region.json")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
draws = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
J, D, STEP, K_FRAMES, NOISE, M, T, DEPTH = 10, 56, 0.01, 8, 2e-3, 4, (1, 0, -1), 2
assert torch.cuda.is_available(), "a measurement needs the GPU"


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


V0, _, C0 = synth.scene(draws, J, 59, 100)
keep = np.all((V0 >= K_FRAMES) & (V0 < (1 << J) - K_FRAMES), axis=1)     # nothing leaves the cube in 8 frames
V0, A0 = V0[keep], np.ascontiguousarray(C0[keep, 3:])
rng = np.random.default_rng(7)
frames = []
for t in range(K_FRAMES):
    Vt = V0 + t * np.asarray(T, np.int64)
    At = A0 + (NOISE * rng.standard_normal(A0.shape)).astype(np.float32) if t else A0
    o = np.argsort(synth.morton_keys(Vt, J), kind="stable")
    frames.append((torch.from_numpy(Vt[o]).cuda(), torch.from_numpy(np.ascontiguousarray(At[o])).cuda()))
last = K_FRAMES - 1
keys_last = synth.morton_keys(frames[last][0].cpu().numpy(), J)
cell, count = np.unique(keys_last >> np.uint64(3 * (J - DEPTH)), return_counts=True)
pick = int(np.argsort(count, kind="stable")[len(count) // 2])           # the occupied depth-2 cell of median population
c0 = int(cell[pick])

result = {"J": J, "D": D, "block_log2": M, "step": STEP, "frames": K_FRAMES, "translation": T, "depth": DEPTH, "cell": c0,
          "cell_voxels": int(count[pick]), "occupied_cells": len(cell), "voxels": [int(A.shape[0]) for _, A in frames], "reps": reps,
          "device": torch.cuda.get_device_name(0), "seg_len": {}}
for S in (2048, 512):
    blob = bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", seg_len=S, gop=K_FRAMES, inter="auto", motion=1, block_log2=M)
    off = bitstream.parse_sequence(blob)
    kinds = "".join("M" if mo is not None else k for k, mo in zip(bitstream.sequence_kinds(blob), bitstream.sequence_motion(blob)))
    (Vw, Cw), = bitstream.decode_sequence_bytes(blob, [last])
    Vr, Cr, info = bitstream.decode_sequence_region(blob, last, DEPTH, (c0, c0 + 1))
    a, b = int(np.searchsorted(keys_last >> np.uint64(3 * (J - DEPTH)), np.uint64(c0))), int(np.searchsorted(keys_last >> np.uint64(3 * (J - DEPTH)), np.uint64(c0 + 1)))
    assert torch.equal(Vr, Vw[a:b]) and torch.equal(Cr.view(torch.int32), Cw[a:b].view(torch.int32))            # bit for bit
    kd = info["keys"]
    calls = timed({"decode_sequence_bytes_last_frame": lambda: bitstream.decode_sequence_bytes(blob, [last]),
                   "decode_sequence_region": lambda: bitstream.decode_sequence_region(blob, last, DEPTH, (c0, c0 + 1)),
                   "decode_sequence_region_cached_keys": lambda: bitstream.decode_sequence_region(blob, last, DEPTH, (c0, c0 + 1), keys=kd)})
    chain = info["chain"]
    per_frame = [{"frame": f, "kind": kinds[f], "ranges": len(info["frames"][f]["ranges"]),
                  "cells": sum(c1 - c for c, c1 in info["frames"][f]["ranges"]), "rows": info["frames"][f]["rows"],
                  "row_share": round(info["frames"][f]["rows"] / result["voxels"][f], 4),
                  "segments_decoded": info["frames"][f]["segments_decoded"], "segments_total": info["frames"][f]["segments_total"],
                  "bytes_needed": info["frames"][f]["bytes_needed"], "frame_bytes": off[f + 1] - off[f]} for f in chain]
    # the three entry points alone: layout and assemble on the intra frame's needed set, needs on the last frame's region
    f0 = chain[0]
    fb = bitstream.sequence_frame(blob, f0)
    h = bitstream.parse_frame(fb)
    (go, gl), (ao, al) = h["geometry"], h["attributes"]
    tl = 3 * (J - DEPTH)
    ck, cf = ops.region_cells(kd[f0], 3 * J, tl, OctreeCoder.parse(fb[go: go + gl])["counts"][DEPTH])
    S0 = info["frames"][f0]["ranges"]
    j = torch.searchsorted(ck, torch.tensor([c for r in S0 for c in r], dtype=torch.int64, device="cuda"))
    bounds = cf[j]
    rows = bounds.tolist()
    n_roots, n = int((j[1::2] - j[0::2]).sum()), sum(rows[1::2]) - sum(rows[0::2])
    n_top, runs = bitstream.region_runs_set(ops.region_layout_set(kd[f0], 3 * J, bounds).tolist(), J, DEPTH, n_roots)
    ids, compact = bitstream.region_segments(n_top, runs, S)
    sc = SegmentedCoder.from_container_segments(fb[ao: ao + al], ids, "cuda")[0]
    Qc = sc.decode(row_major=True)
    inner_last = bitstream._parse_wrapper(bitstream.sequence_frame(blob, last))[3] if kinds[last] != "I" else bitstream.sequence_frame(blob, last)
    table = [(compact(r), d, c) for r, d, c in runs]
    table_dev = torch.tensor(table, dtype=torch.int64, device="cuda")
    kr = kd[last][a:b].contiguous()
    mo = bitstream.sequence_motion(blob)[last]
    entry = {"region_layout_set_and_read_back": lambda: ops.region_layout_set(kd[f0], 3 * J, bounds).tolist(),
             "region_layout_one_range_and_read_back": lambda: ops.region_layout(kd[f0], 3 * J, rows[0], rows[1]).tolist(),
             "region_assemble_set_host_table": lambda: ops.region_assemble_set(Qc, table, n),
             "region_assemble_set_device_table": lambda: ops.region_assemble_set(Qc, table_dev, n),
             "region_needs_no_field": lambda: ops.region_needs(kr, J, tl, 0),
             # where a chain frame's time goes: the set decoder on the intra frame's needed set and on the last frame's one cell, keys cached,
             # and the two stages of it that do not shrink with the region (tools/time_region.py has the others)
             "decode_cells_bytes_intra_frame_cached_keys": lambda: bitstream.decode_cells_bytes(fb, DEPTH, S0, keys=kd[f0]),
             "decode_cells_bytes_last_frame_cached_keys": lambda: bitstream.decode_cells_bytes(inner_last, DEPTH, [(c0, c0 + 1)], keys=kd[last]),
             "select_and_upload_segments_intra_frame": lambda: SegmentedCoder.from_container_segments(fb[ao: ao + al], ids, "cuda"),
             "entropy_decode_selected_intra_frame": lambda: sc.decode(row_major=True)}
    if mo is not None:
        bf, mv = bitstream._region_motion(ops.motion_blocks(kd[last], J, mo[0], len(mo[1])), torch.from_numpy(mo[1].copy()).cuda(), [(a, b)], "cuda")
        entry["region_needs_under_the_field"] = lambda: ops.region_needs(kr, J, tl, 0, bf, mv, mo[0])
        entry["motion_blocks_whole_frame"] = lambda: ops.motion_blocks(kd[last], J, mo[0], len(mo[1]))
    frame = {"kinds": kinds, "sequence_bytes": len(blob), "chain": chain, "bytes_needed": info["bytes_needed"],
             "byte_share_of_the_sequence": round(info["bytes_needed"] / len(blob), 4), "rows": [a, b], "calls": calls, "chain_frames": per_frame,
             "intra_frame_ranges": len(S0), "intra_frame_runs": len(runs), "intra_frame_rows": n, "entry_points": timed(entry)}
    result["seg_len"][str(S)] = frame
    print(S, json.dumps(frame))
    del Qc, Vw, Cw, Vr, Cr, kd, info

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", out_path)
