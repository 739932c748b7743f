#!/usr/bin/env python3
"""The segmented RLGR coder with 32-bit against 64-bit segment offsets (rlgr.SegmentedCoder(wide=False / True)) on the quantized
coefficients of a 3 M x 56 frame -- one frame, and its nine steps in one set of launches -- and the 64-bit path alone on a
6 M x 56 frame (which the 32-bit tables refuse), one frame and three steps. Row-major integers in and out, as encode_frame codes
them. HIP events around enough back-to-back calls to fill `min_s` seconds, `reps` repetitions, the two widths alternating on the
same data; every shape is warmed up first. Prints one JSON line: per case the median / min / max ms per frame, and for the 3 M
frame the difference of the medians next to the 32-bit path's own spread (max - min) in this run.
   python tools/time_rlgr_wide.py [reps] [min_s]"""
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
from raht_3dgs_codec_amd import rlgr, synth  # noqa: E402

reps = max(7, int(sys.argv[1])) if len(sys.argv) > 1 else 7
min_s = float(sys.argv[2]) if len(sys.argv) > 2 else 0.2
S = 2048
SC = rlgr.SegmentedCoder


def quantized(n_draws, seed, steps):
    V, keys, Ch = synth.scene(n_draws, 12, 56, seed)
    p = R.RahtPlan.from_keys(torch.from_numpy(keys.view(np.int64)).cuda(), 36)
    return p.forward_quant_multi(torch.from_numpy(Ch).cuda(), steps)          # (N, 56) row-major each


def calls_for(fn):
    """warm the shape up, then: how many back-to-back calls fill min_s"""
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return max(1, math.ceil(min_s / max(time.perf_counter() - t, 1e-6)))


def alternate(variants, frames):
    """variants: {name: fn}. -> {name: ms per frame of every repetition}; one repetition of each variant in turn"""
    n = {name: calls_for(fn) for name, fn in variants.items()}
    out = {name: [] for name in variants}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        for name, fn in variants.items():
            e0.record()
            for _ in range(n[name]):
                fn()
            e1.record()
            e1.synchronize()
            out[name].append(e0.elapsed_time(e1) / n[name] / frames)
    return out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def case(Qs, widths, batched):
    """encode + decode of the frames Qs, one call per frame (batched=False: the first frame only) or one set of launches for all"""
    N, D = Qs[0].shape
    k = len(Qs) if batched else 1
    coders = {w: [SC(N, D, S, wide=(w == "wide")) for _ in range(k)] for w in widths}
    outs = [torch.empty((N, D), dtype=torch.int32, device="cuda") for _ in range(k)]
    if batched:
        enc = {w: (lambda cs=cs: SC.encode_batch(cs, Qs)) for w, cs in coders.items()}
        dec = {w: (lambda cs=cs: SC.decode_batch(cs, outs=outs)) for w, cs in coders.items()}
    else:
        enc = {w: (lambda cs=cs: cs[0].encode(Qs[0])) for w, cs in coders.items()}
        dec = {w: (lambda cs=cs: cs[0].decode(out=outs[0])) for w, cs in coders.items()}
    e = alternate(enc, k)
    d = alternate(dec, k)
    for w, cs in coders.items():                                     # what was timed is right: every width decodes to the input
        (SC.decode_batch(cs, outs=outs) if batched else cs[0].decode(out=outs[0]))
        assert all(torch.equal(o, q) for o, q in zip(outs, Qs)) and int(cs[0].bad.item()) == 0, w
    if len(widths) == 2:
        assert all(a.total == b.total and torch.equal(a.out[: a.total], b.out[: b.total]) for a, b in zip(coders["narrow"], coders["wide"]))
    res = {"frames_per_call": k, "symbols_per_frame": N * D, "segments_per_frame": coders[widths[0]][0].G,
           "payload_bytes": [c.total for c in coders[widths[0]]]}
    for w in widths:
        res[w] = {"encode": summary(e[w]), "decode": summary(d[w])}
    if len(widths) == 2:
        for what, t in (("encode", e), ("decode", d)):
            diff = statistics.median(t["wide"]) - statistics.median(t["narrow"])
            spread = max(t["narrow"]) - min(t["narrow"])
            res[what + "_wide_minus_narrow"] = {"median_diff_ms": round(diff, 4), "narrow_spread_ms": round(spread, 4),
                                                "inside_narrow_spread": bool(abs(diff) <= spread)}
    else:
        per100m = 1e8 / (N * D)
        res["wide"]["encode"]["ms_per_100M_symbols"] = round(res["wide"]["encode"]["median_ms"] * per100m, 4)
        res["wide"]["decode"]["ms_per_100M_symbols"] = round(res["wide"]["decode"]["median_ms"] * per100m, 4)
    return res


result = {"seg_len": S, "reps": reps, "min_seconds_per_repetition": min_s, "timer": "HIP events", "layout": "row-major in and out",
          "device": torch.cuda.get_device_name(0)}
steps9 = [0.01, 0.04, 0.08, 0.12, 0.16, 0.20, 0.24, 0.32, 0.64]
Qs = quantized(3_000_000, 2, steps9)
result["3M_x_56_one_frame"] = case(Qs[:1], ("narrow", "wide"), False)
result["3M_x_56_nine_steps_batched"] = case(Qs, ("narrow", "wide"), True)
n3 = result["3M_x_56_one_frame"]["narrow"]
result["3M_x_56_one_frame"]["narrow_ms_per_100M_symbols"] = {k: round(n3[k]["median_ms"] * 1e8 / result["3M_x_56_one_frame"]["symbols_per_frame"], 4)
                                                           for k in ("encode", "decode")}
del Qs
torch.cuda.empty_cache()
Qs = quantized(6_000_000, 11, [0.05, 0.1, 0.2])
assert SC(Qs[0].shape[0], 56, S).wide, "the 6 M frame is meant to be one the 32-bit tables refuse"
result["6M_x_56_one_frame"] = case(Qs[:1], ("wide",), False)
result["6M_x_56_three_steps_batched"] = case(Qs, ("wide",), True)
print(json.dumps(result))
