#!/usr/bin/env python3
"""Predicted geometry (geometry.OctreeCoder with ref_keys, csrc/octree_inter.hip) next to the intra coder, in one
process, on three sequences of 8 frames of ~1 M voxels at J = 10: static (frame 0's voxels, attributes plus seeded noise), moving
(frame 0 translated by one voxel in x per frame) and unrelated (8 scenes).

  sections   frame 1 against frame 0: the device stage alone (occupancy / residual stream; keys back from either), HIP events
             around back-to-back calls; the whole section call (OctreeCoder.encode / decode: device stages, RLGR, the host's
             copies and synchronisations), host clock around calls that end synchronised; section bytes both ways. The two coders
             alternate inside every repetition. What prediction adds to a stage is the search (oct_pred_xor_kernel): the level
             walks are the same launches.
  sequences  encode_sequence_bytes / decode_sequence_bytes at D = 56, gop = 8, inter="auto": geometry_inter "off" against "auto"
             (which codes the geometry of every candidate frame twice) -- bytes, how every frame's geometry went, ms per call.
Every time is a device measurement. Writes one JSON file.   python tools/time_geometry_inter.py [out.json] [reps] [draws]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raht_3dgs_codec_amd import bitstream, geometry, synth  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "geometry_inter.json")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
draws = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
J, D, STEP, S, K, NOISE = 10, 56, 0.01, 2048, 8, 2e-3
OC = geometry.OctreeCoder
assert torch.cuda.is_available(), "a measurement needs the GPU"


def timed(fns, warm=2, inner=1, events=False, n=None):
    """fns: {name: callable}, alternated inside every repetition -> {name: {median_ms, min_ms, max_ms, reps, calls_per_rep}}.
    events: HIP events around the `inner` calls (enqueue-only stages); otherwise the host clock between synchronisations"""
    for _ in range(warm):
        for f in fns.values():
            f()
            torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(n or reps):
        for k, f in fns.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            e0.record()
            for _ in range(inner):
                f()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / inner if events else (time.perf_counter() - t) * 1e3 / inner)
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v),
                "calls_per_rep": inner} for k, v in ts.items()}


def ratio(t, a, b):
    return round(t[a]["median_ms"] / t[b]["median_ms"], 3)


def sections(keys, ref):
    """frame `keys` against `ref` (numpy uint64): stages, whole calls, bytes"""
    kd, rd = (torch.from_numpy(x.view(np.int64)).cuda() for x in (keys, ref))
    counts = OC.counts(kd, J)
    n_nodes = sum(counts[:-1])
    occ, res = (torch.empty(n_nodes, dtype=torch.uint8, device="cuda") for _ in range(2))
    k0, k1 = (torch.empty(len(keys), dtype=torch.int64, device="cuda") for _ in range(2))
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    OC.occupancy(kd, J, counts, out=occ)
    OC.residual(kd, J, counts, rd, out=res)
    st = timed({"intra_occupancy": lambda: OC.occupancy(kd, J, counts, out=occ),
                "predicted_residual": lambda: OC.residual(kd, J, counts, rd, out=res),
                "intra_keys_from_occupancy": lambda: OC.keys_from_occupancy(occ, counts, J, bad, out=k0),
                "predicted_keys_from_residual": lambda: OC.keys_from_residual(res, counts, J, rd, bad, out=k1)}, inner=20, events=True)
    assert torch.equal(k0, kd) and torch.equal(k1, kd) and int(bad.item()) == 0
    blobs = {"intra": OC.encode(kd, J), "predicted": OC.encode(kd, J, ref_keys=rd)}
    assert torch.equal(OC.decode(blobs["predicted"], "cuda", ref_keys=rd), kd)
    calls = timed({"intra_encode": lambda: OC.encode(kd, J), "predicted_encode": lambda: OC.encode(kd, J, ref_keys=rd),
                   "intra_decode": lambda: OC.decode(blobs["intra"], "cuda"),
                   "predicted_decode": lambda: OC.decode(blobs["predicted"], "cuda", ref_keys=rd)}, inner=3)
    return {"N": int(len(keys)), "N_ref": int(len(ref)), "n_nodes": int(n_nodes), "zero_residuals": int((res == 0).sum().item()),
            "section_bytes": {k: len(b) for k, b in blobs.items()},
            "bits_per_voxel": {k: round(8 * len(b) / len(keys), 3) for k, b in blobs.items()},
            "device_stage": st, "section_call": calls,
            "predicted_over_intra": {"device_stage_encode": ratio(st, "predicted_residual", "intra_occupancy"),
                                     "device_stage_decode": ratio(st, "predicted_keys_from_residual", "intra_keys_from_occupancy"),
                                     "section_encode": ratio(calls, "predicted_encode", "intra_encode"),
                                     "section_decode": ratio(calls, "predicted_decode", "intra_decode")}}


def sequence(frames):
    enc = {g: (lambda g=g: bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", seg_len=S, gop=K, inter="auto", geometry_inter=g))
           for g in ("off", "auto")}
    blobs = {g: f() for g, f in enc.items()}
    # the same voxels either way, and the same bits where the geometry's cost has not changed which frames are predicted
    want, same = bitstream.decode_sequence_bytes(blobs["off"]), bitstream.sequence_kinds(blobs["off"]) == bitstream.sequence_kinds(blobs["auto"])
    for (V, C), (V1, C1) in zip(bitstream.decode_sequence_bytes(blobs["auto"]), want):
        assert torch.equal(V, V1) and (not same or torch.equal(C.view(torch.int32), C1.view(torch.int32)))
    del want
    sizes = {}
    for g, b in blobs.items():
        off = bitstream.parse_sequence(b)
        geo = []
        for i in range(K):
            fb = bitstream.sequence_frame(b, i, off)
            w = bitstream._parse_wrapper(fb)
            geo.append(bitstream.parse_frame(fb if w is None else w[3])["geometry"][1])
        sizes[g] = {"kinds": "".join(bitstream.sequence_kinds(b)), "geometry": [x[0] for x in bitstream.sequence_geometry(b)],
                    "sequence_bytes": len(b), "frame_bytes": [off[i + 1] - off[i] for i in range(K)], "geometry_section_bytes": geo}
    dec = {g: (lambda b=b: bitstream.decode_sequence_bytes(b)) for g, b in blobs.items()}
    te, td = timed(enc, warm=1, n=min(reps, 3)), timed(dec, warm=1, n=min(reps, 3))
    return {"voxels": [int(A.shape[0]) for _, A in frames], "bytes": sizes, "encode_sequence_bytes": te, "decode_sequence_bytes": td,
            "auto_over_off": {"bytes": round(sizes["auto"]["sequence_bytes"] / sizes["off"]["sequence_bytes"], 4),
                              "encode": ratio(te, "auto", "off"), "decode": ratio(td, "auto", "off")}}


def main():
    result = {"what": "predicted octree geometry against the intra coder (tools/time_geometry_inter.py); every time measured on the device",
              "J": J, "D": D, "step": STEP, "seg_len": S, "geometry_seg_len": geometry.DEFAULT_SEG_LEN, "frames": K, "draws": draws,
              "reps": reps, "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(7)
    V0, k0, C0 = synth.scene(draws, J, 59, 100)
    A0 = np.ascontiguousarray(C0[:, 3:])

    def noisy():
        return torch.from_numpy(A0 + (NOISE * rng.standard_normal(A0.shape)).astype(np.float32)).cuda()

    keep = V0[:, 0] < (1 << J) - (K - 1)
    moving = []
    for t in range(K):
        Vt = V0[keep] + np.array([t, 0, 0], np.int64)
        o = np.argsort(synth.morton_keys(Vt, J), kind="stable")
        moving.append((Vt[o], A0[keep][o]))
    others = [synth.scene(draws, J, 59, 200 + i) for i in range(2)]
    pairs = {"static": (k0, k0), "moving": (synth.morton_keys(moving[1][0], J), synth.morton_keys(moving[0][0], J)),
             "unrelated": (others[1][1], others[0][1])}
    result["sections"] = {}
    for name, (k, r) in pairs.items():
        result["sections"][name] = sections(k, r)
        print(name, json.dumps(result["sections"][name]), flush=True)
    Vd = torch.from_numpy(V0).cuda()
    runs = {"static": lambda: [(Vd, noisy()) for _ in range(K)],
            "moving": lambda: [(torch.from_numpy(V).cuda(), torch.from_numpy(A).cuda()) for V, A in moving],
            "unrelated": lambda: [(torch.from_numpy(V).cuda(), torch.from_numpy(np.ascontiguousarray(C[:, 3:])).cuda())
                                  for V, _, C in others + [synth.scene(draws, J, 59, 202 + i) for i in range(K - 2)]]}
    result["sequences"] = {}
    for name, make in runs.items():
        result["sequences"][name] = sequence(make())
        print(name, json.dumps(result["sequences"][name]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
