#!/usr/bin/env python3
"""Motion compensation on a sequence of the reference's shape: about 1 M voxels x 56 columns, J = 10, blocks of 16 voxels a side. The
current frame is the reference frame translated by (1, 0, -1) with small seeded noise on the attributes. In one process, alternating,
wall times that end in a device synchronise: median [min, max] after warm-ups (the protocol of tools/time_predict.py).
  * raht_motion_search (ops.motion_search) for radius 1 and 2, all 56 columns weighted and 4 columns weighted, against a torch
    composition of the same definition (per candidate: shifted keys, searchsorted, gather, weighted abs-sum, scatter_add) and against
    ONE full read of X and C_ref (a torch copy that moves the same bytes): how far the K-fold work is from the single-pass floor
  * raht_predict_mc against raht_predict on the same matrices; with --parent-lib, raht_predict of that build of the library (the
    parent commit's) twice and of this build once in the same alternation, all three through the same bare ctypes call: this build's
    raht_predict against the parent's own run-to-run spread
  * whole encode_sequence_bytes / decode_sequence_bytes calls on 8 translated frames, motion 0, 1 and 2: kinds, bytes, milliseconds
Writes one JSON file.   python tools/time_motion.py [out.json] [reps] [draws] [--parent-lib path/to/libraht_hip.so]"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raht_3dgs_codec_amd import bitstream, ops, synth  # noqa: E402

argv = list(sys.argv[1:])
parent_lib = None
if "--parent-lib" in argv:
    i = argv.index("--parent-lib")
    parent_lib = argv[i + 1]
    del argv[i: i + 2]
out_path = argv[0] if len(argv) > 0 else os.path.join("profiles", "motion.json")
reps = int(argv[1]) if len(argv) > 1 else 5
draws = int(argv[2]) if len(argv) > 2 else 1_000_000
J, D, STEP, S, K_FRAMES, NOISE, M, T = 10, 56, 0.01, 2048, 8, 2e-3, 4, (1, 0, -1)
assert torch.cuda.is_available(), "a measurement needs the GPU"


def sync():
    torch.cuda.synchronize()


def timed(fns, warm=2, inner=1, n=None):
    """fns: {name: callable}; alternates them inside every repetition; inner: calls per timed window -> {name: {median_ms, ...}}"""
    for _ in range(warm):
        for f in fns.values():
            f()
            sync()
    ts = {k: [] for k in fns}
    for _ in range(n or reps):
        for k, f in fns.items():
            sync()
            t = time.perf_counter()
            for _ in range(inner):
                f()
            sync()
            ts[k].append((time.perf_counter() - t) * 1e3 / inner)
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v),
                "calls_per_rep": inner} for k, v in ts.items()}


def translated(V, A, t, rng):
    """frame 0 moved by t voxels, re-sorted, attributes plus noise -> (V, A) numpy"""
    Vt = V + np.asarray(t, np.int64)
    At = A + (NOISE * rng.standard_normal(A.shape)).astype(np.float32)
    o = np.argsort(synth.morton_keys(Vt, J), kind="stable")
    return Vt[o], np.ascontiguousarray(At[o])


result = {"J": J, "D": D, "block_log2": M, "step": STEP, "seg_len": S, "frames": K_FRAMES, "noise": NOISE, "translation": T, "reps": reps,
          "device": torch.cuda.get_device_name(0)}

V0, _, C0 = synth.scene(draws, J, 59, 100)
keep = np.all((V0 >= K_FRAMES) & (V0 < (1 << J) - K_FRAMES), axis=1)     # nothing leaves the cube in 8 frames
V0, A0 = V0[keep], np.ascontiguousarray(C0[keep, 3:])
rng = np.random.default_rng(7)
V1, A1 = translated(V0, A0, T, rng)
ref_keys = ops.get_morton_code(torch.from_numpy(V0).cuda(), J)
keys = ops.get_morton_code(torch.from_numpy(V1).cuda(), J)
C_ref, X = torch.from_numpy(A0).cuda(), torch.from_numpy(A1).cuda()
N, Nr = int(keys.shape[0]), int(ref_keys.shape[0])
n_blocks = int(torch.unique(keys >> (3 * M)).shape[0])
block_first = ops.motion_blocks(keys, J, M, n_blocks)
block_of = torch.searchsorted(block_first, torch.arange(N, device="cuda"), right=True) - 1
Vcur = ops.demorton(keys, J)
read_bytes = (N + Nr) * D * 4
src, dst = torch.empty(read_bytes // 8, device="cuda"), torch.empty(read_bytes // 8, device="cuda")       # a copy moves its bytes twice


def torch_search(cand, w):
    """the definition with torch operators, up = 0 (the sum over columns in torch's order) -> (best_k, table)"""
    table = torch.zeros((n_blocks, len(cand)), dtype=torch.int64, device="cuda")
    for k, v in enumerate(cand.tolist()):
        W = Vcur + torch.tensor(v, device="cuda")
        ok = ((W >= 0) & (W < (1 << J))).all(dim=1)
        k2 = ops.get_morton_code(W.clamp(0, (1 << J) - 1), J)
        idx = torch.searchsorted(ref_keys, k2).clamp_(max=Nr - 1)
        hit = ok & (ref_keys[idx] == k2)
        P = torch.where(hit[:, None], C_ref[idx], 0.0)
        c = ((X - P).abs() * w).sum(dim=1)
        q = torch.floor(torch.clamp(c, max=1048576.0) * 1024.0).to(torch.int64)
        table[:, k].scatter_add_(0, block_of, q)
    return table.argmin(dim=1), table


result["search"] = {"N": N, "N_ref": Nr, "n_blocks": n_blocks, "full_read_bytes": read_bytes, "cases": {}}
weightings = {"all_56_columns": np.full(D, 1.0 / STEP, np.float32), "4_columns": np.where(np.arange(D) < 4, 1.0 / STEP, 0.0).astype(np.float32)}
for radius in (1, 2):
    cand = ops.motion_candidates(radius)
    for wname, w in weightings.items():
        wd = torch.from_numpy(w).cuda()
        mv, cost = ops.motion_search(keys, ref_keys, C_ref, X, J, M, block_first, cand, w)
        bk, _ = torch_search(cand, wd)
        agree = float((torch.from_numpy(cand).cuda()[bk].to(torch.int8) == mv).all(dim=1).float().mean().item())
        found = float((mv.cpu() == torch.tensor([-t for t in T], dtype=torch.int8)).all(dim=1).float().mean().item())
        nw = int((w != 0).sum())
        # what the definition has to touch: per candidate the keys' search and nw columns of the matched reference rows; once, nw columns of X
        algo = len(cand) * (N * nw * 4 + 8 * N) + N * nw * 4 + 8 * (N + Nr)
        times = timed({"raht_motion_search": lambda: ops.motion_search(keys, ref_keys, C_ref, X, J, M, block_first, cand, w),
                       "torch_composition": lambda: torch_search(cand, wd),
                       "torch_copy_full_read_bytes": lambda: dst.copy_(src)})
        ms = times["raht_motion_search"]["median_ms"]
        case = {"K": int(len(cand)), "weighted_columns": nw, "algorithmic_bytes": algo, "times": times,
                "GB_per_s_algorithmic": round(algo / (ms * 1e-3) / 1e9, 1),
                "speedup_over_torch": round(times["torch_composition"]["median_ms"] / ms, 2),
                "times_one_full_read": round(ms / times["torch_copy_full_read_bytes"]["median_ms"], 1),
                "blocks_agreeing_with_torch": round(agree, 5), "blocks_that_found_the_translation": round(found, 5)}
        result["search"]["cases"][f"radius{radius}_{wname}"] = case
        print(f"radius{radius}_{wname}", json.dumps(case))

# ---- the predictor under a field against the predictor, and against the parent's build ---------------------------------------------
mv, _ = ops.motion_search(keys, ref_keys, C_ref, X, J, M, block_first, ops.motion_candidates(1), weightings["all_56_columns"])
zero = torch.zeros_like(mv)
out, Xio = torch.empty_like(X), X.clone()
assert torch.equal(ops.predict_mc(keys, ref_keys, C_ref, zero, block_first, J, M, X=X), ops.predict(keys, ref_keys, C_ref, X=X))
fns = {"raht_predict_up0_subtract": lambda: ops.predict(keys, ref_keys, C_ref, X=X, up=0, out=out),
       "raht_predict_mc_up0_subtract": lambda: ops.predict_mc(keys, ref_keys, C_ref, mv, block_first, J, M, X=X, up=0, out=out),
       "raht_predict_mc_zero_field_up0_subtract": lambda: ops.predict_mc(keys, ref_keys, C_ref, zero, block_first, J, M, X=X, up=0, out=out),
       "raht_predict_up1_add_in_place": lambda: ops.predict(keys, ref_keys, C_ref, X=Xio, up=1, add=True, out=Xio),
       "raht_predict_mc_up1_add_in_place": lambda: ops.predict_mc(keys, ref_keys, C_ref, mv, block_first, J, M, X=Xio, up=1, add=True, out=Xio)}
if parent_lib:                                                           # both builds through the same bare ctypes call: the same host path
    from raht_3dgs_codec_amd import _lib
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    PL = ctypes.CDLL(os.path.abspath(parent_lib))
    PL.raht_predict.argtypes = [vp, i64, vp, i64, i32, vp, i64, vp, i64, i32, i32, vp, i64, vp, vp]

    def bare(L):
        def call():
            rc = L.raht_predict(keys.data_ptr(), N, ref_keys.data_ptr(), Nr, 0, C_ref.data_ptr(), D, X.data_ptr(), D, D, 0, out.data_ptr(), D, None,
                                vp(torch.cuda.current_stream().cuda_stream))
            assert rc == 0
        return call

    bare(PL)()
    assert torch.equal(out, ops.predict(keys, ref_keys, C_ref, X=X))   # the parent's bits
    fns["bare_call_parent_raht_predict_up0_subtract_a"] = bare(PL)
    fns["bare_call_this_build_raht_predict_up0_subtract"] = bare(_lib.lib())
    fns["bare_call_parent_raht_predict_up0_subtract_b"] = bare(PL)
pred = timed(fns, inner=10)
for r in pred.values():
    r["GB_per_s_algorithmic"] = round((3 * N * D * 4 + 8 * (N + Nr)) / (r["median_ms"] * 1e-3) / 1e9, 1)
result["predictor"] = {"N": N, "N_ref": Nr, "parent_lib": bool(parent_lib), "times": pred}
print(json.dumps(result["predictor"]))
del out, Xio, src, dst, X, C_ref, Vcur

# ---- whole calls on 8 translated frames -----------------------------------------------------------------------------------------------
frames, Vt, At = [], V0, A0
for t in range(K_FRAMES):
    frames.append((torch.from_numpy(Vt).cuda(), torch.from_numpy(At).cuda()))
    Vt, At = translated(V0, A0, tuple((t + 1) * x for x in T), rng)
enc = {f"motion{mo}": (lambda mo=mo: bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", seg_len=S, gop=K_FRAMES, inter="auto", motion=mo,
                                                                      block_log2=M)) for mo in (0, 1, 2)}
blobs = {k: f() for k, f in enc.items()}
sizes = {}
for k, b in blobs.items():
    off = bitstream.parse_sequence(b)
    kinds = bitstream.sequence_kinds(b)
    compensated = [mo is not None for mo in bitstream.sequence_motion(b)]
    per = [off[i + 1] - off[i] for i in range(K_FRAMES)]
    sizes[k] = {"kinds": "".join("M" if c else kd for kd, c in zip(kinds, compensated)), "sequence_bytes": len(b), "frame_bytes": per,
                "mean_I_bytes": round(statistics.mean(x for x, kd in zip(per, kinds) if kd == "I")),
                "mean_P_bytes": round(statistics.mean(x for x, kd, c in zip(per, kinds, compensated) if kd == "P" and not c))
                if any(kd == "P" and not c for kd, c in zip(kinds, compensated)) else None,
                "mean_M_bytes": round(statistics.mean(x for x, c in zip(per, compensated) if c)) if any(compensated) else None}
for (V, C), (V1, A) in zip(bitstream.decode_sequence_bytes(blobs["motion1"]), frames):     # the closed loop holds at this size too
    assert torch.equal(V, V1) and float((C - A).norm(dim=0).max()) <= (0.5 * STEP + 1e-4) * A.shape[0] ** 0.5
dec = {k: (lambda b=b: bitstream.decode_sequence_bytes(b)) for k, b in blobs.items()}
result["sequences"] = {"voxels": [int(A.shape[0]) for _, A in frames], "bytes": sizes,
                       "encode_sequence_bytes": timed(enc, warm=1, n=min(reps, 3)), "decode_sequence_bytes": timed(dec, warm=1, n=min(reps, 3))}
print(json.dumps(result["sequences"]))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", out_path)
