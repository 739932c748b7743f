"""raht_plan_set_stage0_events across the entry points of the two tile engines (csrc/transform.hip, csrc/transform_mx.hip): the
caller's event pair is recorded around the stage-0 launch of EVERY transform of the plan -- a tile stage (scene A, a schedule of
several stages) or the single top stage of a one-launch tree (scene B) -- and recording changes no result.

Bars: hipEventElapsedTime succeeds with 0 < ms < 5 (the bound of test_gpu_parity.py::test_stage0_events_bracket_the_dominant_kernel:
these launches take tens of microseconds), and every output is bit-identical to the same call without events.
"""
import ctypes as C

import numpy as np
import pytest

from .test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

D, NW = 59, 3
STEP = 0.01
STEPS3 = [0.01, 0.02, 0.05]
TOP_ROWS_DEFAULT = 1536              # csrc/schedule.hip pick_tail_geometry: a stage of at most this many entries is a top stage
SCENES = {"A": (20000, 10), "B": (300, 6)}


@pytest.fixture(scope="module")
def rt():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    _lib.lib()
    return R


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")
    vp = C.c_void_p
    h.hipEventCreate.argtypes = [C.POINTER(vp)]
    h.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), vp, vp]
    h.hipEventDestroy.argtypes = [vp]
    return h


@pytest.fixture(scope="module")
def scenes(rt):
    """name -> plan, attributes and the inputs of the inverse-direction entries (computed once, without events)"""
    from raht_3dgs_codec_amd import ops, synth
    out = {}
    for name, (draws, J) in SCENES.items():
        V, keys, Cn = synth.scene(draws, J, D, seed=41)
        p = rt.RahtPlan.from_keys(_dev(keys.view(np.int64)), 3 * J)
        Cm = _dev(Cn)
        s = dict(p=p, C=Cm, C64=Cm.double())
        s["T"] = p.forward(s["C"], want_w=False)
        s["T64"] = p.forward(s["C64"], want_w=False)
        s["Q"] = p.forward_quant(s["C"], STEP)
        s["Qm"] = p.forward_quant_mixed(s["C"], STEP, NW)
        f32, f64, mx = p.stage_stats(4, D), p.stage_stats(8, D), p.mixed_stats(D, NW)
        for st in (f32, f64):
            assert st["valid"]
        assert mx["tile_rows"] >= 64
        rows = [f32["rows_per_stage"], f64["rows_per_stage"], mx["rows_per_stage"]]
        if name == "A":
            assert all(len(r) >= 2 for r in rows), rows
        else:
            # exactly one stage, a top stage. Mixed: asserted directly, the grouping counts one top launch and no tile launch.
            # float32 / float64: INFERRED from one stage of N <= 1536 rows, schedule.hip's default limit of a top stage (no entry
            # point reports is_top; should that default ever drop below N, this assertion keeps passing and means less)
            assert p.N <= TOP_ROWS_DEFAULT and all(r == [p.N] for r in rows), rows
            assert ops.mixed_batch_stats([p], D, NW) == {"tile_launches": 0, "top_launches": 1, "single_scene_calls": 0}
        out[name] = s
    return out


def _sq(res):
    rec, ssd = res
    return (ssd,) if rec is None else (rec, ssd)


ENTRIES = {
    "forward_f32": lambda s: (s["p"].forward(s["C"], want_w=False),),
    "forward_f64": lambda s: (s["p"].forward(s["C64"], want_w=False),),
    "inverse_f32": lambda s: (s["p"].inverse(s["T"]),),
    "inverse_f64": lambda s: (s["p"].inverse(s["T64"]),),
    "forward_quant_f32": lambda s: (s["p"].forward_quant(s["C"], STEP),),
    "forward_quant_f64": lambda s: (s["p"].forward_quant(s["C64"], STEP),),
    "dequant_inverse_f32": lambda s: (s["p"].dequant_inverse(s["Q"], STEP),),
    "dequant_inverse_f64": lambda s: (s["p"].dequant_inverse(s["Q"], STEP, dtype=s["C64"].dtype),),
    "forward_quant_multi": lambda s: tuple(s["p"].forward_quant_multi(s["C"], STEPS3)),
    "dequant_inverse_sqdiff_rec": lambda s: _sq(s["p"].dequant_inverse_sqdiff(s["Q"], STEP, s["C"], want_rec=True)),
    "dequant_inverse_sqdiff_norec": lambda s: _sq(s["p"].dequant_inverse_sqdiff(s["Q"], STEP, s["C"], want_rec=False)),
    "forward_quant_mixed": lambda s: (s["p"].forward_quant_mixed(s["C"], STEP, NW),),
    "dequant_inverse_mixed": lambda s: (s["p"].dequant_inverse_mixed(s["Qm"], STEP, NW),),
    "forward_quant_mixed_multi": lambda s: tuple(s["p"].forward_quant_mixed_multi(s["C"], STEPS3, NW)),
    "dequant_inverse_mixed_sqdiff": lambda s: _sq(s["p"].dequant_inverse_mixed_sqdiff(s["Qm"], STEP, s["C"], NW)),
}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_stage0_events_are_recorded_and_change_nothing(rt, hip, scenes, scene, entry):
    import torch
    from raht_3dgs_codec_amd import _lib
    s = scenes[scene]
    call = ENTRIES[entry]
    ref = call(s)
    L = _lib.lib()
    a, b = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(a)) == 0 and hip.hipEventCreate(C.byref(b)) == 0
    try:
        _lib.check(L.raht_plan_set_stage0_events(s["p"]._h, a, b))
        try:
            got = call(s)
        finally:
            _lib.check(L.raht_plan_set_stage0_events(s["p"]._h, None, None))
        torch.cuda.synchronize()
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), a, b) == 0, "the events were not recorded"
        assert 0.0 < ms.value < 5.0, ms.value
        assert len(got) == len(ref)
        for x, y in zip(got, ref):
            assert torch.equal(x, y)
    finally:
        hip.hipEventDestroy(a); hip.hipEventDestroy(b)
