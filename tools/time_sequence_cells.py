#!/usr/bin/env python3
"""Regions of B frames through bitstream.decode_sequence_cells, on the shapes of tools/time_sequence_region.py: about
1 M voxels x 56 columns, J = 10, seg_len 2048.
  * the 8 correlated frames of tools/time_bidir.py at bframes = 1 (gop 8, inter "always"): one depth-2 cell of a B frame;
  * the wipe of tools/time_block_modes.py under block modes (gop 3, blocks of 16 voxels a side): one depth-2 cell on either side of
    the cut.
For each region, in one process, alternating, two warm-ups, wall times that end in a device synchronise (median, min, max):
decode_sequence_cells cold and with the keys of an earlier call against decode_sequence_bytes(blob, [i]) on the same blob; the
bytes the call needs against the bytes of the sequence; the needed set per frame of the closure; and ops.region_needs_bi on the
region's keys against the two ops.region_needs calls it replaces -- under the frame's own blocks (no field: the modes alone, or
nothing), and under two synthetic fields of radius 1 over the region's blocks. Writes one JSON file.
   python tools/time_sequence_cells.py [out.json] [reps] [draws]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raht_3dgs_codec_amd import bitstream, ops, synth  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "sequence_cells.json")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
draws = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
J, D, STEP, S, K, M, DEPTH = 10, 56, 0.01, 2048, 8, 4, 2
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


def median_cell(keys, where=None):
    """the occupied depth-2 cell of median population (among the cells ``where`` accepts) -> (cell, voxels)"""
    cell, count = np.unique(keys >> np.uint64(3 * (J - DEPTH)), return_counts=True)
    if where is not None:
        keep = np.array([where(int(c)) for c in cell])
        cell, count = cell[keep], count[keep]
    pick = int(np.argsort(count, kind="stable")[len(count) // 2])
    return int(cell[pick]), int(count[pick])


def region(blob, i, keys_i, c0, voxels):
    """one depth-2 cell of frame i -> the record of its measurements"""
    off = bitstream.parse_sequence(blob)
    kinds = bitstream.sequence_kinds(blob)
    ranges = [(c0, c0 + 1)]
    (Vw, Cw), = bitstream.decode_sequence_bytes(blob, [i])
    Vr, Cr, info = bitstream.decode_sequence_cells(blob, i, DEPTH, ranges)
    cells = keys_i >> np.uint64(3 * (J - DEPTH))
    a, b = int(np.searchsorted(cells, np.uint64(c0))), int(np.searchsorted(cells, np.uint64(c0 + 1)))
    assert torch.equal(Vr, Vw[a:b]) and torch.equal(Cr.view(torch.int32), Cw[a:b].view(torch.int32))            # bit for bit
    kd = info["keys"]
    calls = timed({"decode_sequence_bytes_this_frame": lambda: bitstream.decode_sequence_bytes(blob, [i]),
                   "decode_sequence_cells": lambda: bitstream.decode_sequence_cells(blob, i, DEPTH, ranges),
                   "decode_sequence_cells_cached_keys": lambda: bitstream.decode_sequence_cells(blob, i, DEPTH, ranges, keys=kd)})
    chain = info["chain"]
    voxels_of = {f: len(keys_i) for f in chain}                              # (both scenes keep their voxels from frame to frame)
    per_frame = [{"frame": f, "kind": kinds[f], "ranges": len(info["frames"][f]["ranges"]),
                  "cells": sum(c1 - c for c, c1 in info["frames"][f]["ranges"]), "rows": info["frames"][f]["rows"],
                  "row_share": round(info["frames"][f]["rows"] / voxels_of[f], 4),
                  "segments_decoded": info["frames"][f]["segments_decoded"], "segments_total": info["frames"][f]["segments_total"],
                  "bytes_needed": info["frames"][f]["bytes_needed"], "frame_bytes": off[f + 1] - off[f]} for f in chain]
    whole = sum(off[f + 1] - off[f] for f in chain)                          # what decode_sequence_bytes(blob, [i]) reads
    # the entry point against the two calls it replaces, on the region's keys
    tl = 3 * (J - DEPTH)
    kr = kd[i][a:b].contiguous()
    modes = bitstream.sequence_modes(blob)[i]
    n_blocks = int(np.unique(keys_i >> np.uint64(3 * M)).shape[0])
    bf, (md,) = bitstream._region_blocks(ops.motion_blocks(kd[i], J, M, n_blocks), [(a, b)], "cuda",
                                         None if modes is None else torch.from_numpy(modes.copy()).cuda())
    nb = int(bf.shape[0]) - 1
    g = torch.Generator().manual_seed(5)
    f0, f1 = (torch.randint(-1, 2, (nb, 3), generator=g).to(torch.int8).cuda() for _ in range(2))
    entry = {"region_needs_bi_no_field": lambda: ops.region_needs_bi(kr, J, tl, 0),
             "two_region_needs_no_field": lambda: (ops.region_needs(kr, J, tl, 0), ops.region_needs(kr, J, tl, 0)),
             "region_needs_bi_two_fields": lambda: ops.region_needs_bi(kr, J, tl, 0, bf, f0, f1, None, M),
             "two_region_needs_two_fields": lambda: (ops.region_needs(kr, J, tl, 0, bf, f0, M), ops.region_needs(kr, J, tl, 0, bf, f1, M))}
    if md is not None:                                                       # (the old entry point knows no mode: it asks both references for everything)
        entry["region_needs_bi_modes"] = lambda: ops.region_needs_bi(kr, J, tl, 0, bf, None, None, md, M)
        entry["region_needs_bi_two_fields_and_modes"] = lambda: ops.region_needs_bi(kr, J, tl, 0, bf, f0, f1, md, M)
    got, want = entry["region_needs_bi_two_fields"](), entry["two_region_needs_two_fields"]()
    assert all(torch.equal(x, y) for x, y in zip(got, want))
    return {"frame": i, "cell": c0, "cell_voxels": voxels, "rows": [a, b], "region_blocks": nb, "chain": chain, "bytes_needed": info["bytes_needed"],
            "bytes_of_the_closure": whole, "sequence_bytes": len(blob), "byte_share_of_the_sequence": round(info["bytes_needed"] / len(blob), 4),
            "byte_share_of_the_closure": round(info["bytes_needed"] / whole, 4), "calls": calls,
            "cells_over_whole_frame": round(calls["decode_sequence_cells"]["median_ms"] / calls["decode_sequence_bytes_this_frame"]["median_ms"], 3),
            "cached_keys_over_whole_frame": round(calls["decode_sequence_cells_cached_keys"]["median_ms"]
                                                  / calls["decode_sequence_bytes_this_frame"]["median_ms"], 3),
            "chain_frames": per_frame, "entry_points": timed(entry)}


result = {"J": J, "D": D, "step": STEP, "seg_len": S, "block_log2": M, "depth": DEPTH, "reps": reps, "device": torch.cuda.get_device_name(0)}
V0, k0, C0 = synth.scene(draws, J, 59, 100)
A0 = np.ascontiguousarray(C0[:, 3:])
Vd = torch.from_numpy(V0).cuda()

# ---- the 8 correlated frames of tools/time_bidir.py at bframes = 1 ---------------------------------------------------------------------
rng = np.random.default_rng(7)
frames = [(Vd, torch.from_numpy(A0 + (2e-3 * rng.standard_normal(A0.shape)).astype(np.float32)).cuda()) for _ in range(K)]
blob = bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", seg_len=S, gop=K, inter="always", bframes=1)
kinds = bitstream.sequence_kinds(blob)
i = max(f for f, k in enumerate(kinds) if k == "B")                      # the B frame with the longest way back to the intra frame
c0, voxels = median_cell(k0)
result["correlated"] = {"kinds": "".join(kinds), "refs": [list(r) for r in bitstream.sequence_refs(blob)], "voxels": int(k0.shape[0]),
                        "regions": {"a_cell_of_a_b_frame": region(blob, i, k0, c0, voxels)}}
print(json.dumps(result["correlated"]))
del frames, blob

# ---- the wipe of tools/time_block_modes.py under block modes ---------------------------------------------------------------------------
rng = np.random.default_rng(7)
Ap = np.roll(A0, len(A0) // 2, axis=0)
left = V0[:, 0] < (1 << (J - 1))
Xh = (np.where(left[:, None], A0, Ap) + 1e-3 * rng.standard_normal(A0.shape)).astype(np.float32)
frames = [(Vd, torch.from_numpy(a).cuda()) for a in (A0, Xh, Ap)]
blob = bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", seg_len=S, gop=3, bframes=1, block_log2=M, inter="always", block_modes=True)
kinds = bitstream.sequence_kinds(blob)
modes = bitstream.sequence_modes(blob)[1]
half = 8 ** DEPTH // 2                                                  # x is the key's top bit: the cells below `half` are x < 2^(J-1)
sides = {"a_cell_left_of_the_cut": median_cell(k0, lambda c: c < half), "a_cell_right_of_the_cut": median_cell(k0, lambda c: c >= half)}
result["wipe"] = {"kinds": "".join(kinds), "refs": [list(r) for r in bitstream.sequence_refs(blob)], "voxels": int(k0.shape[0]),
                  "modes_chosen": None if modes is None else np.bincount(modes, minlength=4).tolist(),
                  "regions": {n: region(blob, 1, k0, c, v) for n, (c, v) in sides.items()}}
print(json.dumps(result["wipe"]))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", out_path)
