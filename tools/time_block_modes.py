#!/usr/bin/env python3
"""Block modes of a B frame on the shapes of tools/time_bidir.py: about 1 M voxels x 56 columns, J = 10, blocks of
16^3 voxels, on a WIPE -- anchor 0 carries A, anchor 1 a row rotation of A on the same voxels, the frame between them A where
x < 2^(J-1) and the rotation elsewhere plus 1e-3 noise. In one process, alternating; HIP events around back-to-back calls: median
[min, max] after warm-ups.
  * raht_mode_search (ops.mode_search) against
      - the torch composition it replaces: two ops.predict, the hit masks, the mean, four cost passes (|X - P| w summed per row by
        torch, capped, 2^-10 fixed point, index_add_ per block) and argmin -- torch's row sums are not in the definition's order, so
        the number of blocks in which it chooses the same mode is recorded, and the largest relative difference of the tables;
      - raht_predict_bi (X - P into a matrix) in the same run: the floor, since the search reads the same bytes of X and of both
        references (and writes none);
  * raht_predict_bi_modes under the chosen modes against raht_predict_bi;
  * whole encode_sequence_bytes / decode_sequence_bytes calls on the three frames (gop = 3, bframes = 1, inter "always" and
    "auto"), with and without block_modes: the B frame's bytes, the sequence's bytes, encode and decode times.
Writes one JSON file.   python tools/time_block_modes.py [out.json] [reps] [draws]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raht_3dgs_codec_amd import bitstream, ops, synth  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "block_modes.json")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
draws = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
J, D, STEP, S, M, NOISE = 10, 56, 0.01, 2048, 4, 1e-3
assert torch.cuda.is_available(), "a measurement needs the GPU"


def timed(fns, warm=2, inner=1, n=None):
    """fns: {name: callable}; alternates them inside every repetition; inner: back-to-back calls between the two events
    -> {name: {median_ms, ...}} per call"""
    for _ in range(warm):
        for f in fns.values():
            f()
            torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(n or reps):
        for k, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(inner):
                f()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) / inner)
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v),
                "calls_per_rep": inner} for k, v in ts.items()}


result = {"J": J, "D": D, "step": STEP, "seg_len": S, "block_log2": M, "noise": NOISE, "reps": reps, "device": torch.cuda.get_device_name(0)}

# ---- the wipe ---------------------------------------------------------------------------------------------------------------------------
V0, k0, C0 = synth.scene(draws, J, 59, 100)
A = np.ascontiguousarray(C0[:, 3:])
rng = np.random.default_rng(7)
Ap = np.roll(A, len(A) // 2, axis=0)
left = V0[:, 0] < (1 << (J - 1))
Xh = (np.where(left[:, None], A, Ap) + NOISE * rng.standard_normal(A.shape)).astype(np.float32)
keys = torch.from_numpy(k0.view(np.int64)).cuda()
N = int(keys.shape[0])
X = torch.from_numpy(Xh).cuda()
# the anchors as a decoder has them: half a step of quantization error
refs = [(keys, torch.from_numpy((a + 0.5 * STEP * rng.uniform(-1, 1, a.shape)).astype(np.float32)).cuda()) for a in (A, Ap)]
n_blocks = int(np.unique(k0 >> np.uint64(3 * M)).shape[0])
block_first = ops.motion_blocks(keys, J, M, n_blocks)
block_of = torch.repeat_interleave(torch.arange(n_blocks, device="cuda"), block_first[1:] - block_first[:-1])
wh = np.full(D, 1.0 / STEP, np.float32)                                  # the encoder's default weights: a cost counts steps
w = torch.from_numpy(wh).cuda()
frame = dict(J=J, block_log2=M, block_first=block_first)
out = torch.empty_like(X)


def composition():
    P = [ops.predict(keys, r, C) for r, C in refs]
    hit = []
    for r, _ in refs:
        idx = torch.searchsorted(r, keys).clamp_(max=int(r.shape[0]) - 1)
        hit.append(r[idx] == keys)
    Pb = torch.where((hit[0] & hit[1])[:, None], 0.5 * (P[0] + P[1]), torch.where(hit[0][:, None], P[0], P[1]))
    table = torch.zeros((n_blocks, 4), dtype=torch.int64, device="cuda")
    for k, Pk in enumerate((Pb, P[0], P[1], None)):
        c = ((X if Pk is None else X - Pk).abs() * w).sum(dim=1)
        q = torch.floor(torch.fmin(c, torch.full_like(c, 1048576.0)) * 1024.0).to(torch.int64)
        table[:, k].index_add_(0, block_of, q)
    return table.argmin(dim=1).to(torch.uint8), table


mode, best, table = ops.mode_search(keys, *refs, X, J, M, block_first, wh, want_table=True)
mode_c, table_c = composition()
side = left[block_first[:-1].cpu().numpy()]
on_side = int((mode.cpu().numpy() == np.where(side, 1, 2)).sum())       # (recorded, not asserted: this is a measurement)
same_as_composition = int((mode == mode_c).sum())
rel = float(((table - table_c).abs().double() / table.clamp(min=1).double()).max())
R_mean, R_modes = ops.predict_bi(keys, *refs, X=X), ops.predict_bi(keys, *refs, X=X, modes=mode, **frame)
resid = {"frame_wide_mean_steps": round(float(R_mean.abs().mean()) / STEP, 3), "block_modes_steps": round(float(R_modes.abs().mean()) / STEP, 3)}
del R_mean, R_modes, table_c
kern = timed({
    "raht_mode_search": lambda: ops.mode_search(keys, *refs, X, J, M, block_first, wh),
    "torch_composition": composition,
    "raht_predict_bi_subtract": lambda: ops.predict_bi(keys, *refs, X=X, out=out),
    "raht_predict_bi_modes_subtract": lambda: ops.predict_bi(keys, *refs, X=X, out=out, modes=mode, **frame),
}, inner=10)
read_bytes = 3 * N * D * 4 + 8 * 3 * N                                   # X and a row of each reference per row, the three key lists
for n, r in kern.items():
    r["GB_per_s_algorithmic"] = round((read_bytes + (N * D * 4 if "predict_bi" in n else 0)) / (r["median_ms"] * 1e-3) / 1e9, 1)
result["kernels"] = {"N": N, "n_blocks": n_blocks, "modes_chosen": np.bincount(mode.cpu().numpy(), minlength=4).tolist(),
                     "blocks_that_choose_their_side": on_side, "blocks_the_composition_chooses_alike": same_as_composition,
                     "composition_table_max_relative_difference": rel, "mean_abs_residual": resid, "times": kern,
                     "mode_search_over_predict_bi": round(kern["raht_mode_search"]["median_ms"] / kern["raht_predict_bi_subtract"]["median_ms"], 3),
                     "composition_over_mode_search": round(kern["torch_composition"]["median_ms"] / kern["raht_mode_search"]["median_ms"], 3),
                     "predict_bi_modes_over_predict_bi": round(kern["raht_predict_bi_modes_subtract"]["median_ms"]
                                                               / kern["raht_predict_bi_subtract"]["median_ms"], 3)}
print(json.dumps(result["kernels"]))
del X, out, refs, block_of

# ---- whole calls: anchor 0, the frame between, anchor 1 ---------------------------------------------------------------------------------
Vd = torch.from_numpy(V0).cuda()
frames = [(Vd, torch.from_numpy(a).cuda()) for a in (A, Xh, Ap)]
kw = dict(seg_len=S, gop=3, bframes=1, block_log2=M)
enc = {f"{inter}_{'block_modes' if bm else 'plain'}": (lambda inter=inter, bm=bm: bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", inter=inter,
                                                                                                                 block_modes=bm, **kw))
       for inter in ("always", "auto") for bm in (False, True)}
blobs = {n: f() for n, f in enc.items()}
sizes = {}
for n, b in blobs.items():
    off = bitstream.parse_sequence(b)
    modes = bitstream.sequence_modes(b)[1]
    sizes[n] = {"kinds": "".join(bitstream.sequence_kinds(b)), "frame_1_magic": bytes(bitstream.sequence_frame(b, 1)[:8]).decode(),
                "sequence_bytes": len(b), "frame_bytes": [off[i + 1] - off[i] for i in range(3)],
                "modes_chosen": None if modes is None else np.bincount(modes, minlength=4).tolist()}
for n in ("always_block_modes", "auto_block_modes"):                    # the closed loop holds at this size: within the quantizer's bound
    for (V, C), (V1, A1) in zip(bitstream.decode_sequence_bytes(blobs[n]), frames):
        assert torch.equal(V, V1) and float((C - A1).norm(dim=0).max()) <= (0.5 * STEP + 1e-4) * A1.shape[0] ** 0.5
dec = {n: (lambda b=b: bitstream.decode_sequence_bytes(b)) for n, b in blobs.items()}
result["sequence"] = {"voxels": N, "bytes": sizes,
                      "b_frame_bytes_ratio_always": round(sizes["always_block_modes"]["frame_bytes"][1] / sizes["always_plain"]["frame_bytes"][1], 4),
                      "sequence_bytes_ratio_always": round(sizes["always_block_modes"]["sequence_bytes"] / sizes["always_plain"]["sequence_bytes"], 4),
                      "encode_sequence_bytes": timed(enc, warm=1, n=3), "decode_sequence_bytes": timed(dec, warm=1, n=3)}
print(json.dumps(result["sequence"]))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", out_path)
