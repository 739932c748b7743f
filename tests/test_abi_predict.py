"""CPU-only checks of raht_predict at the C-ABI boundary: exported, bound, and every argument rule refused with RAHT_ERR_INVALID
and the function's name before any HIP call -- the "device pointers" below are addresses that must never be read."""
import os

import pytest

INVALID = -1
K, RK, CR, X, Y, NM = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000       # never dereferenced


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def test_the_symbol_is_exported_and_bound(L):
    from raht_3dgs_codec_amd import _lib
    assert "raht_predict" in _lib.EXPORTS and hasattr(L, "raht_predict")
    assert len(L.raht_predict.argtypes) == 15
    assert L.raht_version() == 300                                       # a new entry point, no new ABI version


def test_argument_validation(L):
    def call(keys=K, N=1000, ref=RK, N_ref=900, shift=3, C_ref=CR, ld_ref=8, x=X, ldx=8, D=8, add=0, y=Y, ldy=8, nm=NM):
        return L.raht_predict(keys, N, ref, N_ref, shift, C_ref, ld_ref, x, ldx, D, add, y, ldy, nm, None)

    cases = {"NULL keys": dict(keys=None), "NULL ref_keys": dict(ref=None), "NULL C_ref": dict(C_ref=None), "NULL Y": dict(y=None),
             "N = 0": dict(N=0), "N < 0": dict(N=-3), "N = 2^31": dict(N=2 ** 31), "N_ref = 0": dict(N_ref=0), "N_ref < 0": dict(N_ref=-1),
             "N_ref = 2^31": dict(N_ref=2 ** 31), "shift = 1": dict(shift=1), "shift = -3": dict(shift=-3), "shift = 12": dict(shift=12),
             "shift = 4": dict(shift=4), "D = 0": dict(D=0), "D < 0": dict(D=-8), "ld_ref < D": dict(ld_ref=7), "ldx < D": dict(ldx=7),
             "ldy < D": dict(ldy=7), "add = 2": dict(add=2), "add = -1": dict(add=-1),
             "NULL X, NULL Y": dict(x=None, y=None), "NULL X, add = 2": dict(x=None, add=2)}
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == INVALID, (what, rc)
        assert b"raht_predict" in L.raht_last_error(), (what, L.raht_last_error())


def test_python_wrapper_refuses_host_tensors_and_bad_arguments():
    import torch
    from raht_3dgs_codec_amd import ops
    k = torch.arange(10, dtype=torch.int64)
    C = torch.zeros((10, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.predict(k, k, C)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.predict(k, k, C, X=C, add=True, out=C, want_matched=True)
