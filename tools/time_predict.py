#!/usr/bin/env python3
"""Inter-frame prediction on a sequence of the reference's shape: 8 frames of about 1 M voxels x 56 columns, J = 10. Frame t is frame
0's voxels with attributes perturbed by small seeded noise, so that prediction pays; a second run takes 8 independent frames, where
it cannot. In one process, alternating, wall times that end in a device synchronise: median [min, max] after warm-ups.
  * raht_predict (ops.predict) for up = 0 and 1, both directions (X - P into a fresh matrix, X + P in place), against the torch
    composition X -/+ where(hit, C_ref[idx], 0) from searchsorted (up = 0; its gather is the co-located row) and against a plain
    torch copy of the same 3 N D 4 bytes; GB/s are the algorithmic bytes 3 N D 4 + 8 (N + N') over the median
  * whole encode_sequence_bytes / decode_sequence_bytes calls with gop = 8 (inter "auto" and "always") against gop = 1
  * bytes per frame, I against P
Writes one JSON file.   python tools/time_predict.py [out.json] [reps] [draws]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raht_3dgs_codec_amd import bitstream, ops, synth  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "predict.json")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
draws = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
J, D, STEP, S, K, NOISE = 10, 56, 0.01, 2048, 8, 2e-3
assert torch.cuda.is_available(), "a measurement needs the GPU"


def sync():
    torch.cuda.synchronize()


def timed(fns, warm=2, inner=1):
    """fns: {name: callable}; alternates them inside every repetition; inner: calls per timed window -> {name: {median_ms, ...}}"""
    for _ in range(warm):
        for f in fns.values():
            f()
            sync()
    ts = {n: [] for n in fns}
    for _ in range(reps):
        for n, f in fns.items():
            sync()
            t = time.perf_counter()
            for _ in range(inner):
                f()
            sync()
            ts[n].append((time.perf_counter() - t) * 1e3 / inner)
    return {n: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v),
                "calls_per_rep": inner} for n, v in ts.items()}


result = {"J": J, "D": D, "step": STEP, "seg_len": S, "frames": K, "noise": NOISE, "reps": reps, "device": torch.cuda.get_device_name(0)}

# ---- the predictor alone: frame 0 against a reference that holds 7 of its 8 voxels and another scene's (misses, N' != N) ---------
V0, k0, C0 = synth.scene(draws, J, 59, 100)
A0 = np.ascontiguousarray(C0[:, 3:])
keys = torch.from_numpy(k0.view(np.int64)).cuda()
ref_keys = torch.from_numpy(np.union1d(np.delete(k0, np.s_[::8]), synth.sorted_unique_keys(draws // 8, J, 101)).view(np.int64)).cuda()
N, Nr = int(keys.shape[0]), int(ref_keys.shape[0])
g = torch.Generator(device="cuda").manual_seed(1)
X = torch.from_numpy(A0).cuda()
C_ref = torch.randn((Nr, D), generator=g, device="cuda")
algo_bytes = 3 * N * D * 4 + 8 * (N + Nr)
out, Xio = torch.empty_like(X), X.clone()
src3, dst3 = torch.empty(3 * N * D // 2, device="cuda"), torch.empty(3 * N * D // 2, device="cuda")      # a copy moves its bytes twice


def torch_predict(sub):
    idx = torch.searchsorted(ref_keys, keys).clamp_(max=Nr - 1)
    hit = ref_keys[idx] == keys
    P = torch.where(hit[:, None], C_ref[idx], 0.0)
    return X - P if sub else X + P


P0, n0 = ops.predict(keys, ref_keys, C_ref, up=0, want_matched=True)
idx = torch.searchsorted(ref_keys, keys).clamp_(max=Nr - 1)
hit = ref_keys[idx] == keys
assert int(n0.item()) == int(hit.sum().item()) and torch.equal(P0, torch.where(hit[:, None], C_ref[idx], 0.0))
assert torch.equal(ops.predict(keys, ref_keys, C_ref, X=X, up=0), torch_predict(True))
assert torch.equal(ops.predict(keys, ref_keys, C_ref, X=X, up=0, add=True), torch_predict(False))
del P0, idx, hit
n1 = int(ops.predict(keys, ref_keys, C_ref, up=1, want_matched=True)[1].item())
kern = timed({
    "raht_predict_up0_subtract": lambda: ops.predict(keys, ref_keys, C_ref, X=X, up=0, out=out),
    "raht_predict_up0_add_in_place": lambda: ops.predict(keys, ref_keys, C_ref, X=Xio, up=0, add=True, out=Xio),
    "raht_predict_up1_subtract": lambda: ops.predict(keys, ref_keys, C_ref, X=X, up=1, out=out),
    "raht_predict_up1_add_in_place": lambda: ops.predict(keys, ref_keys, C_ref, X=Xio, up=1, add=True, out=Xio),
    "torch_composition_up0_subtract": lambda: torch_predict(True),
    "torch_composition_up0_add": lambda: torch_predict(False),
    "torch_copy_same_bytes": lambda: dst3.copy_(src3),
}, inner=10)
for n, r in kern.items():
    r["GB_per_s_algorithmic"] = round(algo_bytes / (r["median_ms"] * 1e-3) / 1e9, 1)
result["predictor"] = {"N": N, "N_ref": Nr, "matched_up0": int(n0.item()), "matched_up1": n1, "algorithmic_bytes_up0": algo_bytes,
                       "times": kern}
print(json.dumps(result["predictor"]))
del X, C_ref, out, Xio, src3, dst3, keys, ref_keys

# ---- whole calls ----------------------------------------------------------------------------------------------------------------
rng = np.random.default_rng(7)
Vd = torch.from_numpy(V0).cuda()
runs = {"correlated": [(Vd, torch.from_numpy(A0 + (NOISE * rng.standard_normal(A0.shape)).astype(np.float32)).cuda()) for _ in range(K)],
        "independent": [(torch.from_numpy(V).cuda(), torch.from_numpy(np.ascontiguousarray(C[:, 3:])).cuda())
                        for V, _, C in (synth.scene(draws, J, 59, 200 + i) for i in range(K))]}
result["sequences"] = {}
for name, frames in runs.items():
    enc = {f"gop{gop}_{inter}": (lambda gop=gop, inter=inter: bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", seg_len=S, gop=gop, inter=inter))
           for gop, inter in ((1, "auto"), (K, "auto"), (K, "always"))}
    blobs = {n: f() for n, f in enc.items()}
    sizes = {}
    for n, b in blobs.items():
        off = bitstream.parse_sequence(b)
        kinds = bitstream.sequence_kinds(b)
        per = [off[i + 1] - off[i] for i in range(K)]
        sizes[n] = {"kinds": "".join(kinds), "sequence_bytes": len(b), "frame_bytes": per,
                    "mean_I_bytes": round(statistics.mean(x for x, k in zip(per, kinds) if k == "I")),
                    "mean_P_bytes": round(statistics.mean(x for x, k in zip(per, kinds) if k == "P")) if "P" in kinds else None}
    # the closed loop holds at this size too: every frame within the quantizer's bound of its input (an orthonormal transform, every
    # coefficient off by half a step at most: a column's error has norm <= step / 2 sqrt(N), float32 rounding far below)
    for n in (f"gop{K}_always",):
        for (V, C), (V1, A) in zip(bitstream.decode_sequence_bytes(blobs[n]), frames):
            assert torch.equal(V, V1) and float((C - A).norm(dim=0).max()) <= (0.5 * STEP + 1e-4) * A.shape[0] ** 0.5
    dec = {n: (lambda b=b: bitstream.decode_sequence_bytes(b)) for n, b in blobs.items()}
    result["sequences"][name] = {"voxels": [int(A.shape[0]) for _, A in frames], "bytes": sizes,
                                 "encode_sequence_bytes": timed(enc, warm=1), "decode_sequence_bytes": timed(dec, warm=1)}
    print(name, json.dumps(result["sequences"][name]))
    del blobs, dec, enc

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", out_path)
