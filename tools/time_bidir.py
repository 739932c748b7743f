#!/usr/bin/env python3
"""The two-reference predictor and B frames on the shapes of tools/time_predict.py / tools/time_motion.py: about 1 M voxels x 56
columns, J = 10. In one process, alternating, wall times that end in a device synchronise: median [min, max] after warm-ups.
  * raht_predict_bi (ops.predict_bi) at up = 0, X - P into a fresh matrix and X + P in place, without and with two motion fields
    (blocks of 16^3 voxels; all-zero vectors: the block lookups and key shifts on the traffic of the call without fields; random
    vectors of [-1, 1]^3: most rows then miss, and the references' rows are not read), against
      - the composition it replaces: two ops.predict(X=None), the hit masks from searchsorted, where, add, multiply, subtract,
      - a plain torch copy of the same 4 N D 4 algorithmic bytes (X, Y and one row of each reference per row),
      - ops.predict against reference 0 alone;
    GB/s are the algorithmic bytes 4 N D 4 + 8 (N + N0' + N1') over the median (3 N D 4 + 8 (N + N0') for ops.predict)
  * whole encode_sequence_bytes / decode_sequence_bytes calls on 8 correlated frames, gop = 8, bframes 0, 1 and 3 (inter "auto" and
    "always"): bytes per I / P / B frame, encode and decode times
Writes one JSON file.   python tools/time_bidir.py [out.json] [reps] [draws]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raht_3dgs_codec_amd import bitstream, ops, synth  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "bidir.json")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
draws = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
J, D, STEP, S, K, NOISE, M = 10, 56, 0.01, 2048, 8, 2e-3, 4
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


result = {"J": J, "D": D, "step": STEP, "seg_len": S, "frames": K, "noise": NOISE, "block_log2": M, "reps": reps,
          "device": torch.cuda.get_device_name(0)}

# ---- the predictor alone: frame 0 against two references that each hold 7 of its 8 voxels and another scene's -----------------------
V0, k0, C0 = synth.scene(draws, J, 59, 100)
A0 = np.ascontiguousarray(C0[:, 3:])
keys = torch.from_numpy(k0.view(np.int64)).cuda()
rk = [torch.from_numpy(np.union1d(np.delete(k0, np.s_[o::8]), synth.sorted_unique_keys(draws // 8, J, 101 + o)).view(np.int64)).cuda()
      for o in (0, 3)]
N, Nr = int(keys.shape[0]), [int(r.shape[0]) for r in rk]
g = torch.Generator(device="cuda").manual_seed(1)
X = torch.from_numpy(A0).cuda()
Cr = [torch.randn((n, D), generator=g, device="cuda") for n in Nr]
refs = [(rk[0], Cr[0]), (rk[1], Cr[1])]
n_blocks = int(np.unique(k0 >> np.uint64(3 * M)).shape[0])
block_first = ops.motion_blocks(keys, J, M, n_blocks)
mv = [torch.randint(-1, 2, (n_blocks, 3), generator=g, device="cuda").to(torch.int8) for _ in range(2)]
field = dict(J=J, block_log2=M, block_first=block_first, mv0=mv[0], mv1=mv[1])
algo_bytes = 4 * N * D * 4 + 8 * (N + sum(Nr))
algo_bytes_one = 3 * N * D * 4 + 8 * (N + Nr[0])
out, Xio = torch.empty_like(X), X.clone()
src4, dst4 = torch.empty(2 * N * D, device="cuda"), torch.empty(2 * N * D, device="cuda")      # a copy moves its bytes twice


def composition(sub):
    P = [ops.predict(keys, r, C) for r, C in refs]
    hit = []
    for r, n in zip(rk, Nr):
        idx = torch.searchsorted(r, keys).clamp_(max=n - 1)
        hit.append(r[idx] == keys)
    Pb = torch.where((hit[0] & hit[1])[:, None], 0.5 * (P[0] + P[1]), torch.where(hit[0][:, None], P[0], P[1]))
    return X - Pb if sub else X + Pb


Pb, nm = ops.predict_bi(keys, *refs, want_matched=True)
assert torch.equal(ops.predict_bi(keys, *refs, X=X), composition(True)) and torch.equal(ops.predict_bi(keys, *refs, X=X, add=True), composition(False))
zero = dict(field, mv0=torch.zeros_like(mv[0]), mv1=torch.zeros_like(mv[1]))
assert torch.equal(ops.predict_bi(keys, *refs, **zero), Pb)
nm_field = ops.predict_bi(keys, *refs, want_matched=True, **field)[1]
del Pb
kern = timed({
    "raht_predict_bi_subtract": lambda: ops.predict_bi(keys, *refs, X=X, out=out),
    "raht_predict_bi_add_in_place": lambda: ops.predict_bi(keys, *refs, X=Xio, add=True, out=Xio),
    "raht_predict_bi_zero_fields_subtract": lambda: ops.predict_bi(keys, *refs, X=X, out=out, **zero),
    "raht_predict_bi_fields_subtract": lambda: ops.predict_bi(keys, *refs, X=X, out=out, **field),
    "raht_predict_bi_fields_add_in_place": lambda: ops.predict_bi(keys, *refs, X=Xio, add=True, out=Xio, **field),
    "composition_subtract": lambda: composition(True),
    "composition_add": lambda: composition(False),
    "torch_copy_same_bytes": lambda: dst4.copy_(src4),
    "raht_predict_one_reference_subtract": lambda: ops.predict(keys, *refs[0], X=X, out=out),
}, inner=10)
for n, r in kern.items():
    r["GB_per_s_algorithmic"] = round((algo_bytes_one if "one_reference" in n else algo_bytes) / (r["median_ms"] * 1e-3) / 1e9, 1)
result["predictor"] = {"N": N, "N_ref": Nr, "n_blocks": n_blocks, "matched_ref0_ref1_both": nm.tolist(),
                       "matched_under_fields": nm_field.tolist(), "algorithmic_bytes": algo_bytes,
                       "algorithmic_bytes_one_reference": algo_bytes_one, "times": kern}
print(json.dumps(result["predictor"]))
del X, Cr, refs, out, Xio, src4, dst4, keys, rk, mv, field, zero, block_first

# ---- whole calls --------------------------------------------------------------------------------------------------------------------
rng = np.random.default_rng(7)
Vd = torch.from_numpy(V0).cuda()
frames = [(Vd, torch.from_numpy(A0 + (NOISE * rng.standard_normal(A0.shape)).astype(np.float32)).cuda()) for _ in range(K)]
enc = {f"bframes{b}_{inter}": (lambda b=b, inter=inter: bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", seg_len=S, gop=K, inter=inter,
                                                                                        bframes=b))
       for b in (0, 1, 3) for inter in ("auto", "always")}
blobs = {n: f() for n, f in enc.items()}
sizes = {}
for n, b in blobs.items():
    off = bitstream.parse_sequence(b)
    kinds = bitstream.sequence_kinds(b)
    per = [off[i + 1] - off[i] for i in range(K)]
    sizes[n] = {"kinds": "".join(kinds), "refs": [list(r) for r in bitstream.sequence_refs(b)], "sequence_bytes": len(b), "frame_bytes": per}
    for k in "IPB":
        sizes[n][f"mean_{k}_bytes"] = round(statistics.mean(x for x, kk in zip(per, kinds) if kk == k)) if k in kinds else None
# the closed loop holds at this size too: every frame within the quantizer's bound of its input (time_predict.py has the reasoning)
for n in ("bframes1_always", "bframes3_always"):
    for (V, C), (V1, A) in zip(bitstream.decode_sequence_bytes(blobs[n]), frames):
        assert torch.equal(V, V1) and float((C - A).norm(dim=0).max()) <= (0.5 * STEP + 1e-4) * A.shape[0] ** 0.5
dec = {n: (lambda b=b: bitstream.decode_sequence_bytes(b)) for n, b in blobs.items()}
anchors = [i for i, k in enumerate(bitstream.sequence_kinds(blobs["bframes1_always"])) if k != "B"]
dec["bframes1_always_anchors_only"] = lambda: bitstream.decode_sequence_bytes(blobs["bframes1_always"], frames=anchors)
result["sequences"] = {"correlated": {"voxels": [int(A.shape[0]) for _, A in frames], "bytes": sizes,
                                      "encode_sequence_bytes": timed(enc, warm=1), "decode_sequence_bytes": timed(dec, warm=1)}}
print(json.dumps(result["sequences"]))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", out_path)
assert kern["raht_predict_bi_subtract"]["median_ms"] < kern["composition_subtract"]["median_ms"], "the fused kernel must beat the composition"
