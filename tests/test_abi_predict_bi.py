"""CPU-only checks of raht_predict_bi at the C-ABI boundary: declared, exported, bound, and every argument rule refused with
RAHT_ERR_INVALID and the function's name before any HIP call -- the "device pointers" below are addresses that must never be read."""
import os

import pytest

INVALID = -1
K, BF, MV0, MV1, RK0, CR0, RK1, CR1, X, Y, NM = (0x10000 * i for i in range(1, 12))       # never dereferenced
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def test_the_symbol_is_declared_exported_and_bound(L):
    from raht_3dgs_codec_amd import _lib
    assert "int raht_predict_bi(" in open(os.path.join(ROOT, "include", "raht.h")).read()
    assert "raht_predict_bi" in _lib.EXPORTS and hasattr(L, "raht_predict_bi")
    assert len(L.raht_predict_bi.argtypes) == 25
    assert L.raht_version() == 300                                       # a new entry point, no new ABI version


def test_argument_validation(L):
    def call(keys=K, N=1000, J=6, m=0, bf=None, n_blocks=0, mv0=None, mv1=None, ref0=RK0, N0=900, C0=CR0, ld0=8, ref1=RK1, N1=1100, C1=CR1,
             ld1=8, shift=3, x=X, ldx=8, D=8, add=0, y=Y, ldy=8, nm=NM):
        return L.raht_predict_bi(keys, N, J, m, bf, n_blocks, mv0, mv1, ref0, N0, C0, ld0, ref1, N1, C1, ld1, shift, x, ldx, D, add, y, ldy,
                                 nm, None)

    field = dict(m=2, bf=BF, n_blocks=10)
    cases = {"NULL keys": dict(keys=None), "NULL ref0 keys": dict(ref0=None), "NULL ref1 keys": dict(ref1=None), "NULL C_ref0": dict(C0=None),
             "NULL C_ref1": dict(C1=None), "NULL Y": dict(y=None), "NULL X, NULL Y": dict(x=None, y=None),
             "N = 0": dict(N=0), "N < 0": dict(N=-3), "N = 2^31": dict(N=2 ** 31),
             "N_ref0 = 0": dict(N0=0), "N_ref0 < 0": dict(N0=-1), "N_ref0 = 2^31": dict(N0=2 ** 31),
             "N_ref1 = 0": dict(N1=0), "N_ref1 < 0": dict(N1=-1), "N_ref1 = 2^31": dict(N1=2 ** 31),
             "shift = 1": dict(shift=1), "shift = -3": dict(shift=-3), "shift = 12": dict(shift=12), "shift = 4": dict(shift=4),
             "D = 0": dict(D=0), "D < 0": dict(D=-8), "ld_ref0 < D": dict(ld0=7), "ld_ref1 < D": dict(ld1=7), "ldx < D": dict(ldx=7),
             "ldy < D": dict(ldy=7), "add = 2": dict(add=2), "add = -1": dict(add=-1), "NULL X, add = 2": dict(x=None, add=2),
             "mv0 without block_first": dict(mv0=MV0, m=2, n_blocks=10), "mv1 without block_first": dict(mv1=MV1, m=2, n_blocks=10),
             "both fields without block_first": dict(mv0=MV0, mv1=MV1, m=2, n_blocks=10),
             "mv0, block_log2 = 0": dict(field, mv0=MV0, m=0), "mv1, block_log2 = 0": dict(field, mv1=MV1, m=0),
             "mv0, block_log2 < 0": dict(field, mv0=MV0, m=-1), "mv1, block_log2 = J + 1": dict(field, mv1=MV1, m=7),
             "both fields, block_log2 = J + 1": dict(field, mv0=MV0, mv1=MV1, m=7),
             "mv0, J = 0": dict(field, mv0=MV0, J=0, m=1), "mv1, J = 22": dict(field, mv1=MV1, J=22),
             "mv0, n_blocks = 0": dict(field, mv0=MV0, n_blocks=0), "mv1, n_blocks > N": dict(field, mv1=MV1, n_blocks=1001)}
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == INVALID, (what, rc)
        assert b"raht_predict_bi:" in L.raht_last_error(), (what, L.raht_last_error())


def test_python_wrapper_refuses_host_tensors_and_bad_arguments():
    import torch
    from raht_3dgs_codec_amd import ops
    k = torch.arange(10, dtype=torch.int64)
    C = torch.zeros((10, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.predict_bi(k, (k, C), (k, C))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.predict_bi(k, (k, C), (k, C), X=C, add=True, out=C, want_matched=True)
    with pytest.raises(ValueError, match="pairs"):
        ops.predict_bi(k, k, C)
    with pytest.raises(ValueError, match="a motion field needs"):
        ops.predict_bi(k, (k, C), (k, C), mv0=torch.zeros((1, 3), dtype=torch.int8))
    with pytest.raises(ValueError, match="a motion field needs"):
        ops.predict_bi(k, (k, C), (k, C), mv1=torch.zeros((1, 3), dtype=torch.int8), J=4, block_log2=2)
