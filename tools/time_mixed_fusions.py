#!/usr/bin/env python3
"""The two driver-loop fusions in mixed precision on the cfg3 scene (synth.CONFIGS["cfg3"]: 3 M x 59, n_wide = 3), each next to
the unfused sequence it replaces, and the float32 pairs beside them for comparison:
  forward  nine raht_fwd_quant_mixed calls          vs ONE raht_fwd_quant_mixed_multi with the nine steps
           nine raht_fwd_quant calls                vs ONE raht_fwd_quant_multi                                    (float32)
  inverse  raht_dequant_inv_mixed + raht_sqdiff_columns vs raht_dequant_inv_mixed_sqdiff with / without C_rec
           raht_dequant_inv + raht_sqdiff_columns   vs raht_dequant_inv_sqdiff with / without C_rec               (float32)
Device events around `reps` calls, after a warm-up; the legs of a pair alternate over `rounds` rounds and the median round is
reported. One JSON line per process: run it in several fresh processes (each under its own time limit) and compare."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raht_3dgs_codec_amd as R  # noqa: E402
from raht_3dgs_codec_amd import _lib, ops, synth  # noqa: E402

STEPS = [0.01 * s for s in (1, 4, 8, 12, 16, 20, 24, 32, 64)]        # python/encode_3dgs.py:28 colorStep, scaled


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / reps


def ab(legs, reps, rounds, warm):
    """legs: name -> callable; alternating rounds, median ms per call of each"""
    for fn in legs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in legs}
    for r in range(rounds):
        names = list(legs) if r % 2 == 0 else list(legs)[::-1]
        for k in names:
            got[k].append(timed(legs[k], reps))
    return {k: round(float(np.median(v)), 4) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warm", type=int, default=3)
    a = ap.parse_args()
    L = _lib.lib()
    n, J, D, seed = synth.CONFIGS["cfg3"]
    nw = 3
    V, keys, Ch = synth.scene(n, J, D, seed)
    Cd = torch.from_numpy(Ch).cuda()
    p = R.RahtPlan.from_keys(torch.from_numpy(keys.view(np.int64)).cuda(), 3 * J)
    N = int(Cd.shape[0])
    st = p.mixed_stats(D, nw)
    assert st["tile_rows"] > 0, "cfg3 must take the mixed tile kernels"
    s = ops._stream()
    vp = C.c_void_p
    k = len(STEPS)
    Qs = [torch.empty((N, D), dtype=torch.int32, device="cuda") for _ in range(k)]
    qptr = (vp * k)(*[q.data_ptr() for q in Qs])
    d1 = [(C.c_double * 1)(x) for x in STEPS]
    f1 = [(C.c_float * 1)(x) for x in STEPS]
    dk = (C.c_double * k)(*STEPS)
    fk = (C.c_float * k)(*STEPS)
    c = vp(Cd.data_ptr())
    rec = torch.empty_like(Cd)
    ssd = torch.empty(D, dtype=torch.float64, device="cuda")
    r_, q0, sq_ = vp(rec.data_ptr()), vp(Qs[0].data_ptr()), vp(ssd.data_ptr())

    def mx_single():
        for i in range(k):
            _lib.check(L.raht_fwd_quant_mixed(p._h, c, D, D, d1[i], 1, nw, vp(Qs[i].data_ptr()), D, s))

    def mx_multi():
        _lib.check(L.raht_fwd_quant_mixed_multi(p._h, c, D, D, dk, k, nw, qptr, D, s))

    def f32_single():
        for i in range(k):
            _lib.check(L.raht_fwd_quant(p._h, c, D, D, f1[i], 1, vp(Qs[i].data_ptr()), D, s))

    def f32_multi():
        _lib.check(L.raht_fwd_quant_multi(p._h, c, D, D, fk, k, qptr, D, s))

    fwd = ab({"mixed_nine_calls": mx_single, "mixed_multi": mx_multi, "f32_nine_calls": f32_single, "f32_multi": f32_multi},
             a.reps, a.rounds, a.warm)
    # the inverse legs decode the mixed forward's integers at the step a frame's PSNR columns are usually taken at
    step = 0.04
    mx_multi()
    _lib.check(L.raht_fwd_quant_mixed(p._h, c, D, D, d1[1], 1, nw, q0, D, s))
    d, f = (C.c_double * 1)(step), (C.c_float * 1)(step)

    def mx_two():
        _lib.check(L.raht_dequant_inv_mixed(p._h, q0, D, D, d, 1, nw, r_, D, s))
        _lib.check(L.raht_sqdiff_columns(c, D, r_, D, N, D, 0, sq_, s))

    def mx_fused():
        _lib.check(L.raht_dequant_inv_mixed_sqdiff(p._h, q0, D, D, d, 1, nw, c, D, r_, D, sq_, s))

    def mx_fused_norec():
        _lib.check(L.raht_dequant_inv_mixed_sqdiff(p._h, q0, D, D, d, 1, nw, c, D, None, D, sq_, s))

    def f32_two():
        _lib.check(L.raht_dequant_inv(p._h, q0, D, D, f, 1, r_, D, s))
        _lib.check(L.raht_sqdiff_columns(c, D, r_, D, N, D, 0, sq_, s))

    def f32_fused():
        _lib.check(L.raht_dequant_inv_sqdiff(p._h, q0, D, D, f, 1, c, D, r_, D, sq_, s))

    def f32_fused_norec():
        _lib.check(L.raht_dequant_inv_sqdiff(p._h, q0, D, D, f, 1, c, D, None, D, sq_, s))

    inv = ab({"mixed_inv_plus_sqdiff": mx_two, "mixed_fused": mx_fused, "mixed_fused_no_rec": mx_fused_norec,
              "f32_inv_plus_sqdiff": f32_two, "f32_fused": f32_fused, "f32_fused_no_rec": f32_fused_norec},
             a.reps * 3, a.rounds, a.warm)
    print(json.dumps({"scene": "cfg3", "rows": N, "channels": D, "n_wide": nw, "tile_rows": st["tile_rows"], "steps": k,
                      "forward_ms": fwd, "inverse_ms": inv,
                      "gain_multi_mixed": round(fwd["mixed_nine_calls"] / fwd["mixed_multi"], 3),
                      "gain_multi_f32": round(fwd["f32_nine_calls"] / fwd["f32_multi"], 3),
                      "gain_sqdiff_mixed": round(inv["mixed_inv_plus_sqdiff"] / inv["mixed_fused"], 3),
                      "gain_sqdiff_mixed_no_rec": round(inv["mixed_inv_plus_sqdiff"] / inv["mixed_fused_no_rec"], 3),
                      "gain_sqdiff_f32": round(inv["f32_inv_plus_sqdiff"] / inv["f32_fused"], 3),
                      "gain_sqdiff_f32_no_rec": round(inv["f32_inv_plus_sqdiff"] / inv["f32_fused_no_rec"], 3)}))


if __name__ == "__main__":
    main()
