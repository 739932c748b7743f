#!/usr/bin/env python3
"""A sequence of 8 frames of the reference's shape (J = 10, about 1 M voxels each, a different count in every frame) through
bitstream.encode_sequence_bytes / decode_sequence_bytes against a loop of encode_frame_bytes / decode_frame_bytes, once x 56 columns
(n_wide = 0) and once x 59 (n_wide = 3); the entropy stage alone (SegmentedCoder.encode_ragged / decode_ragged against one call per
frame on the same integers); and the stages of both directions one by one, the geometry and the host assembly among them. In one
process, alternating, wall times that end in a device synchronise: median [min, max] after warm-ups. Writes one JSON file.
   python tools/time_sequence.py [out.json] [reps] [draws] [batch_parent.json batch_this.json]
The last two: the one-line outputs of tools/time_rlgr_batch.py on the parent commit and on this one (same box), copied into the
record under "same_shape_batch"."""
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

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "sequence.json")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
draws = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
J, STEP, S, K = 10, 0.01, 2048, 8
SHARE = (1.0, 0.9, 1.1, 0.95, 1.05, 0.85, 1.15, 1.0)                   # of `draws`, per frame
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


# the frames once, x 59 (xyz first); the 56-column run takes their other columns
scenes = [synth.scene(int(draws * SHARE[i]), J, 59, 100 + i) for i in range(K)]
result = {"J": J, "step": STEP, "seg_len": S, "frames": K, "voxels": [int(s[0].shape[0]) for s in scenes], "reps": reps,
          "device": torch.cuda.get_device_name(0), "runs": {}}

for D, n_wide in ((56, 0), (59, 3)):
    frames = [(torch.from_numpy(V).cuda(), torch.from_numpy(np.ascontiguousarray(C[:, 59 - D:])).cuda()) for V, _, C in scenes]
    enc_seq = lambda: bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", n_wide=n_wide, seg_len=S)                     # noqa: E731
    enc_loop = lambda: [bitstream.encode_frame_bytes(V, A, J, STEP, "cuda", n_wide=n_wide, seg_len=S) for V, A in frames]    # noqa: E731
    seq, alone = enc_seq(), enc_loop()
    assert [bytes(bitstream.sequence_frame(seq, i)) for i in range(K)] == alone
    got = bitstream.decode_sequence_bytes(seq)
    for (V, C), b in zip(got, alone):
        V1, C1 = bitstream.decode_frame_bytes(b, "cuda")
        assert torch.equal(V, V1) and torch.equal(C, C1)
    del got
    whole = timed({"encode_sequence_bytes": enc_seq, "loop_encode_frame_bytes": enc_loop,
                   "decode_sequence_bytes": lambda: bitstream.decode_sequence_bytes(seq),
                   "loop_decode_frame_bytes": lambda: [bitstream.decode_frame_bytes(b, "cuda") for b in alone]})

    # ---- the stages, on the same frames
    keys = [ops.get_morton_code(V, J) for V, _ in frames]
    plans = [ops.RahtPlan.from_keys(k, 3 * J) for k in keys]
    As = [A for _, A in frames]
    fq1 = (lambda p, A: p.forward_quant_mixed(A, STEP, n_wide)) if n_wide else (lambda p, A: p.forward_quant(A, STEP))
    fqb = (lambda: ops.forward_quant_mixed_batch(plans, As, STEP, n_wide)) if n_wide else (lambda: ops.forward_quant_batch(plans, As, STEP))
    Qs = fqb()
    coders = [SegmentedCoder(A.shape[0], D, S, 1, "cuda") for A in As]
    SegmentedCoder.encode_ragged(coders, Qs)
    ragged = [c.container() for c in coders]
    for c, Q in zip(coders, Qs):
        c.encode(Q)
    assert [c.container() for c in coders] == ragged
    geos = [OctreeCoder.encode(k, J) for k in keys]
    blobs = [b"".join(bitstream._frame_parts(J, A.shape[0], D, n_wide, [STEP], None, None, g, [a])) for A, g, a in zip(As, geos, ragged)]
    outs = [torch.empty((A.shape[0], D), dtype=torch.int32, device="cuda") for A in As]
    iq1 = (lambda p, Q: p.dequant_inverse_mixed(Q, STEP, n_wide)) if n_wide else (lambda p, Q: p.dequant_inverse(Q, STEP))
    iqb = (lambda: ops.dequant_inverse_mixed_batch(plans, Qs, STEP, n_wide)) if n_wide else (lambda: ops.dequant_inverse_batch(plans, Qs, STEP))
    heads = [bitstream.parse_frame(b) for b in blobs]
    stages = timed({
        "entropy_encode_ragged": lambda: SegmentedCoder.encode_ragged(coders, Qs),
        "entropy_encode_one_call_per_frame": lambda: [c.encode(Q) for c, Q in zip(coders, Qs)],
        "entropy_decode_ragged": lambda: SegmentedCoder.decode_ragged(coders, outs=outs),
        "entropy_decode_one_call_per_frame": lambda: [c.decode(out=o) for c, o in zip(coders, outs)],
        "transform_forward_batch": fqb,
        "transform_forward_one_call_per_frame": lambda: [fq1(p, A) for p, A in zip(plans, As)],
        "transform_inverse_batch": iqb,
        "transform_inverse_one_call_per_frame": lambda: [iq1(p, Q) for p, Q in zip(plans, Qs)],
        "morton_keys": lambda: [ops.get_morton_code(V, J) for V, _ in frames],
        "geometry_encode": lambda: [OctreeCoder.encode(k, J) for k in keys],
        "geometry_decode": lambda: [OctreeCoder.decode(b[h["geometry"][0]: sum(h["geometry"])], "cuda") for b, h in zip(blobs, heads)],
        "plan_build": lambda: [ops.RahtPlan.from_keys(k, 3 * J) for k in keys],
        "demorton": lambda: [ops.demorton(k, J) for k in keys],
        "coder_objects": lambda: [SegmentedCoder(A.shape[0], D, S, 1, "cuda") for A in As],
        "containers_to_host": lambda: [(h, l.tobytes(), p.tobytes()) for h, l, p in (c.container_parts() for c in coders)],
        "containers_to_host_joined": lambda: [c.container() for c in coders],
        "host_assembly": lambda: bitstream._pack_parts([bitstream._frame_parts(J, A.shape[0], D, n_wide, [STEP], None, None, g, [a])
                                                        for A, g, a in zip(As, geos, ragged)]),
        "host_parse": lambda: [bitstream.parse_frame(bitstream.sequence_frame(seq, i)) for i in range(K)],
        "containers_to_device": lambda: [SegmentedCoder.from_container(b[h["attributes"][0]: sum(h["attributes"])], "cuda") for b, h in zip(blobs, heads)],
    })
    for o, Q in zip(outs, Qs):
        assert torch.equal(o, Q)
    run = {"D": D, "n_wide": n_wide, "sequence_bytes": len(seq), "segments_per_frame": [c.G for c in coders], "calls": whole, "stages": stages}
    result["runs"][f"{D}_columns"] = run
    print(D, json.dumps(run))
    del frames, keys, plans, As, Qs, coders, outs, blobs, geos, ragged, seq, alone

if len(sys.argv) > 5:
    result["same_shape_batch"] = {"what": "tools/time_rlgr_batch.py, nine steps of a 3 M x 56 frame, same box, parent commit and this one",
                                  "parent": [json.loads(ln) for ln in open(sys.argv[4]) if ln.startswith("{")],
                                  "this": [json.loads(ln) for ln in open(sys.argv[5]) if ln.startswith("{")]}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", out_path)
