#!/usr/bin/env python3
"""The rate-distortion curve of a cfg3 frame at the nine quantization steps of the driver loop: RahtPlan.rate_curve (one forward
transform, one read of the coefficients, nothing quantized or coded) against the existing route to the same nine sizes
(forward_quant_multi + SegmentedCoder.encode_batch), in one process, alternating. Median and spread of wall times that end in a
device synchronise ("parts": whole Python calls, with their allocations, the padded sums and the copy of the sizes to the host);
the C entry point alone between device events, tables allocated beforehand ("kernel_events": the copy of the step table and the
kernels, nothing else), at k = 1, 2, 4, 8 in one pass, as k passes of one step and, for k = 8, as two passes of four; peak device
memory of both routes; and the coefficient-domain squared error against the attribute-domain sums of dequant_inverse_sqdiff.
Writes one JSON file.
   python tools/time_rate_curve.py [out.json] [reps] [draws]"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import raht_3dgs_codec_amd as R  # noqa: E402
from raht_3dgs_codec_amd import _lib, ops, rlgr, synth  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "rate_curve.json")
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 9
draws = int(sys.argv[3]) if len(sys.argv) > 3 else synth.CONFIGS["cfg3"][0]
S = 2048
steps = [0.01, 0.04, 0.08, 0.12, 0.16, 0.20, 0.24, 0.32, 0.64]
k = len(steps)
SC = rlgr.SegmentedCoder
assert torch.cuda.is_available(), "a measurement needs the GPU"

_, J, _, seed = synth.CONFIGS["cfg3"]
V, keys, C59 = synth.scene(draws, J, 59, seed)
plan = R.RahtPlan.from_keys(torch.from_numpy(keys.view(np.int64)).cuda(), 3 * J)
N = plan.N
C59d = torch.from_numpy(C59).cuda()
C56d = C59d[:, 3:].contiguous()


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


def timed_events(fns, warm=2):
    """as timed, but between two device events on the current stream: what the device spends, without the host's share"""
    for _ in range(warm):
        for f in fns.values():
            f()
    sync()
    ts = {n: [] for n in fns}
    for _ in range(reps):
        for n, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ts[n].append(e0.elapsed_time(e1))
    return {n: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "reps": len(v)} for n, v in ts.items()}


def entry_point(Tq, sts, seg_bytes, seg_sse):
    """raht_rlgr_seg_rate itself on a float32 matrix and scalar steps, into tables the caller holds"""
    st = (ctypes.c_float * len(sts))(*sts)
    _lib.check(_lib.lib().raht_rlgr_seg_rate(ctypes.c_void_p(Tq.data_ptr()), _lib.RAHT_F32, Tq.stride(0), Tq.shape[0], Tq.shape[1], st, len(sts), 1, S, 1,
                                             ctypes.c_void_p(seg_bytes.data_ptr()), ctypes.c_void_p(seg_sse.data_ptr()) if seg_sse is not None else None,
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


def used_bytes():
    sync()
    torch.cuda.empty_cache()
    free, total = torch.cuda.mem_get_info()
    return total - free


def memory_of(f):
    """peak bytes of torch tensors during f above what was held before, and what the library's own pools grew by (they only grow)"""
    before = used_bytes()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    r = f()
    sync()
    peak = torch.cuda.max_memory_allocated() - base
    del r
    return {"torch_peak_bytes": int(peak), "library_pool_growth_bytes": int(max(0, used_bytes() - before))}


def route_b(Cd, n_wide):
    Qs = plan.forward_quant_mixed_multi(Cd, steps, n_wide) if n_wide else plan.forward_quant_multi(Cd, steps)
    coders = [SC(N, Cd.shape[1], S) for _ in steps]
    SC.encode_batch(coders, Qs)
    return [c.size_bytes for c in coders], Qs


result = {"N": N, "seg_len": S, "steps": steps, "reps": reps, "device": torch.cuda.get_device_name(0), "frames": {}}
for name, Cd, n_wide in (("cfg3_56_columns", C56d, 0), ("cfg3_59_columns_n_wide_3", C59d, 3)):
    D = Cd.shape[1]
    # (d) memory first, while the pools are as small as they will be: the new route, then the old one
    mem_a = memory_of(lambda: plan.rate_curve(Cd, steps, n_wide, S))
    mem_b = memory_of(lambda: route_b(Cd, n_wide))
    rc = plan.rate_curve(Cd, steps, n_wide, S)
    sizes_b, Qs = route_b(Cd, n_wide)
    assert [int(x) for x in rc["bytes"]] == sizes_b, (rc["bytes"], sizes_b)
    # (e) coefficient-domain error against the attribute-domain sums of the decoder
    ratio = []
    for j, st in enumerate(steps):
        ssd = (plan.dequant_inverse_mixed_sqdiff(Qs[j], st, Cd, n_wide, want_rec=False) if n_wide else plan.dequant_inverse_sqdiff(Qs[j], st, Cd, want_rec=False))[1]
        ratio.append(float(rc["sse"][j].sum() / ssd.sum().item()))
    del Qs
    # (a) against (b), alternating; (b) with its coders and matrices allocated inside, as a caller who wants sizes would
    ab = timed({"a_rate_curve": lambda: plan.rate_curve(Cd, steps, n_wide, S), "b_quant_multi_encode_batch": lambda: route_b(Cd, n_wide)})
    frame = {"D": D, "n_wide": n_wide, "container_bytes": sizes_b, "a_vs_b": ab, "memory": {"a_rate_curve": mem_a, "b_quant_multi_encode_batch": mem_b},
             "sse_over_attribute_sqdiff": ratio}
    if not n_wide:
        T = plan.forward(Cd, want_w=False)
        Tq = torch.empty_like(T)
        order = plan.order_RAGFT

        def fwd_gather():
            plan.forward(Cd, want_w=False, out=T)
            ops.rows_gather(T, order, Tq)

        fwd_gather()
        parts = {"forward_and_gather": fwd_gather, "rate_kernel_9_steps": lambda: SC.rate(Tq, steps, S), "rate_kernel_9_steps_no_sse": lambda: SC.rate(Tq, steps, S, want_sse=False)}
        # (c) what the interleaved chains buy: kk steps in one pass against kk passes of one step
        for kk in (1, 2, 4, 8):
            parts[f"rate_kernel_k{kk}_one_pass"] = lambda kk=kk: SC.rate(Tq, steps[:kk], S)
            if kk > 1:
                parts[f"rate_kernel_k{kk}_as_single_passes"] = lambda kk=kk: [SC.rate(Tq, [s], S) for s in steps[:kk]]
        Qm = plan.forward_quant_multi(Cd, steps)
        coders = [SC(N, D, S) for _ in steps]
        parts["forward_quant_multi"] = lambda: plan.forward_quant_multi(Cd, steps)
        parts["encode_batch_preallocated"] = lambda: SC.encode_batch(coders, Qm)
        frame["parts"] = timed(parts)
        del Qm, coders
        # the same comparison on the device's clock: the entry point alone, its tables allocated once
        G = D * ((N + S - 1) // S)
        sb = torch.empty((k, G), dtype=torch.int32, device="cuda")
        se = torch.empty((k, G), dtype=torch.float64, device="cuda")
        kern = {}
        for tag, e in (("", se), ("_no_sse", None)):
            kern[f"k9{tag}"] = lambda e=e: entry_point(Tq, steps, sb, e)
            for kk in (1, 2, 4, 8):
                kern[f"k{kk}_one_pass{tag}"] = lambda kk=kk, e=e: entry_point(Tq, steps[:kk], sb, e)
                if kk > 1:
                    kern[f"k{kk}_as_single_passes{tag}"] = lambda kk=kk, e=e: [entry_point(Tq, [s], sb, e) for s in steps[:kk]]
            kern[f"k8_as_two_passes_of_4{tag}"] = lambda e=e: [entry_point(Tq, steps[j:j + 4], sb, e) for j in (0, 4)]
        frame["kernel_events"] = timed_events(kern)
        ref = rlgr.SegmentedCoder.rate(Tq, steps, S)[1]
        entry_point(Tq, steps, sb, se)
        assert torch.equal(sb, ref)
        del T, Tq, sb, se, ref
    result["frames"][name] = frame
    print(name, json.dumps(frame))

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", out_path)
