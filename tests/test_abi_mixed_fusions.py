"""CPU-only checks of the two mixed-precision driver-loop fusions at the C-ABI boundary (raht_fwd_quant_mixed_multi,
raht_dequant_inv_mixed_sqdiff): both are exported, and a bad argument is refused with RAHT_ERR_INVALID, before any HIP call,
with an error string that names the function. No compute calls."""
import ctypes
import os

import pytest

INVALID = -1


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def test_both_symbols_are_exported(L):
    from raht_3dgs_codec_amd import _lib
    for name in ("raht_fwd_quant_mixed_multi", "raht_dequant_inv_mixed_sqdiff"):
        assert hasattr(L, name), name
        assert name in _lib.EXPORTS, name


def _multi(L, plan, C, steps, k, Q):
    return L.raht_fwd_quant_mixed_multi(plan, C, 59, 59, steps, k, 3, Q, 59, None)


def test_multi_argument_validation(L):
    dummy = ctypes.c_void_p(16)          # never dereferenced: every case below is refused before the plan is looked at
    steps = (ctypes.c_double * 3)(0.01, 0.02, 0.04)
    Q = (ctypes.c_void_p * 3)(32, 48, 64)
    cases = {
        "NULL plan": (None, dummy, steps, 3, Q),
        "k = 0": (dummy, dummy, steps, 0, Q),
        "k < 0": (dummy, dummy, steps, -2, Q),
        "NULL C": (dummy, None, steps, 3, Q),
        "NULL steps": (dummy, dummy, None, 3, Q),
        "NULL Q array": (dummy, dummy, steps, 3, None),
        "NULL Q[1]": (dummy, dummy, steps, 3, (ctypes.c_void_p * 3)(32, None, 64)),
        "Q[0] == Q[2]": (dummy, dummy, steps, 3, (ctypes.c_void_p * 3)(32, 48, 32)),
    }
    for what, args in cases.items():
        rc = _multi(L, *args)
        assert rc == INVALID, what
        assert b"raht_fwd_quant_mixed_multi" in L.raht_last_error(), (what, L.raht_last_error())


def test_sqdiff_argument_validation(L):
    dummy = ctypes.c_void_p(16)
    steps = (ctypes.c_double * 1)(0.01)

    def call(plan=dummy, Q=dummy, ref=dummy, rec=dummy, sq=dummy, D=59, ldref=59, ldc=59):
        return L.raht_dequant_inv_mixed_sqdiff(plan, Q, 59, D, steps, 1, 3, ref, ldref, rec, ldc, sq, None)

    cases = {
        "NULL plan": dict(plan=None),
        "NULL Q": dict(Q=None),
        "NULL C_ref": dict(ref=None),
        "NULL sqdiff": dict(sq=None),
        "NULL C_ref, no C_rec": dict(ref=None, rec=None),
        "D = 0": dict(D=0),
        "ld_ref < D": dict(ldref=58),
        "ldc < D": dict(ldc=40),
    }
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == INVALID, what
        assert b"raht_dequant_inv_mixed_sqdiff" in L.raht_last_error(), (what, L.raht_last_error())
