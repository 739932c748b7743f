"""CPU-only checks of the mixed-precision batch entries at the C-ABI boundary (raht_fwd_quant_mixed_batch,
raht_dequant_inv_mixed_batch, raht_mixed_batch_stats): all three are exported and bound, and every argument rule that can be
judged without looking at a plan is refused with RAHT_ERR_INVALID, before any plan is dereferenced and before any HIP call, with
an error string that names the function. No compute calls: the "plans" are addresses that must never be read."""
import ctypes
import os

import pytest

INVALID = -1
NAMES = ("raht_fwd_quant_mixed_batch", "raht_dequant_inv_mixed_batch", "raht_mixed_batch_stats")


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def test_the_three_symbols_are_exported_and_bound(L):
    from raht_3dgs_codec_amd import _lib
    for name in NAMES:
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert len(L.raht_fwd_quant_mixed_batch.argtypes) == 11
    assert len(L.raht_dequant_inv_mixed_batch.argtypes) == 11
    assert len(L.raht_mixed_batch_stats.argtypes) == 8


def _vp(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _i64(*vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def _dbl(*vals):
    return (ctypes.c_double * len(vals))(*vals)


# never dereferenced: every case below is refused before a plan or a matrix is looked at
PLANS = (16, 32, 48)
MATS_A = (1024, 2048, 3072)
MATS_B = (4096, 5120, 6144)


def _cases():
    """name -> keyword overrides of one valid-looking call (3 scenes, D = 59, a scalar step, n_wide = 3)"""
    return {
        "NULL plans": dict(plans=None),
        "NULL input array": dict(a=None),
        "NULL output array": dict(b=None),
        "NULL input strides": dict(lda=None),
        "NULL output strides": dict(ldb=None),
        "NULL steps": dict(steps=None),
        "n = 0": dict(n=0),
        "n < 0": dict(n=-3),
        "NULL plans[1]": dict(plans=_vp(16, None, 48)),
        "NULL input matrix [2]": dict(a=_vp(1024, 2048, None)),
        "NULL output matrix [0]": dict(b=_vp(None, 5120, 6144)),
        "the same plan twice": dict(plans=_vp(16, 32, 16)),
        "n_wide = 0": dict(n_wide=0),
        "n_wide = 5": dict(n_wide=5),
        "n_wide > D": dict(D=2, n_wide=3, lda=_i64(2, 2, 2), ldb=_i64(2, 2, 2)),
        "D = 0": dict(D=0),
        "n_steps = 2": dict(steps=_dbl(0.01, 0.02), n_steps=2),
        "n_steps = 0": dict(n_steps=0),
        "n_steps = D - 1": dict(steps=_dbl(*([0.01] * 58)), n_steps=58),
        "step = 0": dict(steps=_dbl(0.0)),
        "step < 0": dict(steps=_dbl(-0.01)),
        "step NaN": dict(steps=_dbl(float("nan"))),
        "a per-channel step <= 0": dict(steps=_dbl(*([0.01] * 40 + [0.0] + [0.01] * 18)), n_steps=59),
        "a step that is 0 as float32": dict(steps=_dbl(1e-60)),
        "input stride [1] < D": dict(lda=_i64(59, 58, 59)),
        "output stride [2] < D": dict(ldb=_i64(59, 64, 12)),
    }


def _call(fn, n=3, plans=_vp(*PLANS), a=_vp(*MATS_A), lda=_i64(59, 64, 59), D=59, steps=_dbl(0.01), n_steps=1, n_wide=3,
          b=_vp(*MATS_B), ldb=_i64(59, 59, 80)):
    return fn(n, plans, a, lda, D, steps, n_steps, n_wide, b, ldb, None)


@pytest.mark.parametrize("name", NAMES[:2])
def test_argument_validation_before_any_plan_is_read(L, name):
    fn = getattr(L, name)
    for what, kw in _cases().items():
        rc = _call(fn, **kw)
        assert rc == INVALID, (name, what, rc)
        assert name.encode() in L.raht_last_error(), (name, what, L.raht_last_error())


@pytest.mark.parametrize("name", NAMES[:2])
def test_the_scene_is_named_where_it_applies(L, name):
    fn = getattr(L, name)
    for kw, scene in ((dict(plans=_vp(16, None, 48)), b"scene 1"), (dict(lda=_i64(59, 59, 3)), b"scene 2"),
                      (dict(b=_vp(None, 5120, 6144)), b"scene 0"), (dict(plans=_vp(16, 32, 16)), b"2")):
        assert _call(fn, **kw) == INVALID
        assert scene in L.raht_last_error(), L.raht_last_error()


def test_stats_argument_validation(L):
    t, u, v = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)

    def call(n=3, plans=_vp(*PLANS), D=59, n_wide=3, t=ctypes.byref(t), u=ctypes.byref(u), v=ctypes.byref(v)):
        return L.raht_mixed_batch_stats(n, plans, D, n_wide, 0, t, u, v)

    cases = {
        "NULL plans": dict(plans=None), "n = 0": dict(n=0), "n < 0": dict(n=-1), "NULL plans[1]": dict(plans=_vp(16, None, 48)),
        "the same plan twice": dict(plans=_vp(16, 16, 48)), "n_wide = 0": dict(n_wide=0), "n_wide = 5": dict(n_wide=5),
        "D = 0": dict(D=0), "NULL tile_launches": dict(t=None), "NULL top_launches": dict(u=None),
        "NULL single_scene_calls": dict(v=None),
    }
    for what, kw in cases.items():
        assert call(**kw) == INVALID, what
        assert b"raht_mixed_batch_stats" in L.raht_last_error(), (what, L.raht_last_error())
