"""CPU-only checks of raht_mode_search and raht_predict_bi_modes at the C-ABI boundary: declared, exported, bound with the header's
argument list, and every argument rule refused with RAHT_ERR_INVALID and the function's name before any HIP call -- the "device
pointers" below are addresses that must never be read."""
import ctypes
import os
import re

import pytest

INVALID = -1
K, BF, MV0, MV1, RK0, CR0, RK1, CR1, X, Y, NM, MD, W, BC, TB = (0x10000 * i for i in range(1, 16))      # never dereferenced
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"int": ctypes.c_int32, "int64_t": ctypes.c_int64, "raht_stream_t": ctypes.c_void_p}


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def _prototype(name):
    """the header's argument list of ``name`` as ctypes types: every pointer is a void pointer to the binding"""
    src = open(os.path.join(ROOT, "include", "raht.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    args = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src).group(1)
    out = []
    for a in args.split(","):
        a = a.strip()
        out.append(ctypes.c_void_p if "*" in a else CTYPE[a.replace("const ", "").split()[0]])
    return out


@pytest.mark.parametrize("name,n_args", [("raht_mode_search", 25), ("raht_predict_bi_modes", 26)])
def test_the_symbols_are_declared_exported_and_bound_as_declared(L, name, n_args):
    from raht_3dgs_codec_amd import _lib
    assert name in _lib.EXPORTS and hasattr(L, name)
    want = _prototype(name)
    assert len(want) == n_args and list(getattr(L, name).argtypes) == want
    assert L.raht_version() == 300                                       # new entry points, no new ABI version


def test_the_existing_two_reference_entry_point_keeps_its_signature(L):
    assert list(L.raht_predict_bi.argtypes) == _prototype("raht_predict_bi") and len(L.raht_predict_bi.argtypes) == 25


def _cases():
    return {"NULL keys": dict(keys=None), "NULL ref0 keys": dict(ref0=None), "NULL ref1 keys": dict(ref1=None), "NULL C_ref0": dict(C0=None),
            "NULL C_ref1": dict(C1=None), "N = 0": dict(N=0), "N < 0": dict(N=-3), "N = 2^31": dict(N=2 ** 31),
            "N_ref0 = 0": dict(N0=0), "N_ref0 = 2^31": dict(N0=2 ** 31), "N_ref1 = 0": dict(N1=0), "N_ref1 < 0": dict(N1=-1),
            "N_ref1 = 2^31": dict(N1=2 ** 31), "shift = 1": dict(shift=1), "shift = -3": dict(shift=-3), "shift = 12": dict(shift=12),
            "D = 0": dict(D=0), "D < 0": dict(D=-8), "ld_ref0 < D": dict(ld0=7), "ld_ref1 < D": dict(ld1=7), "ldx < D": dict(ldx=7),
            "NULL block_first": dict(bf=None), "NULL block_first under fields": dict(bf=None, mv0=MV0, mv1=MV1),
            "block_log2 = 0": dict(m=0), "block_log2 < 0": dict(m=-1), "block_log2 = J + 1": dict(m=7), "J = 0": dict(J=0, m=1),
            "J = 22": dict(J=22), "n_blocks = 0": dict(n_blocks=0), "n_blocks > N": dict(n_blocks=1001), "NULL mode": dict(mode=None)}


def test_mode_search_argument_validation(L):
    def call(keys=K, N=1000, J=6, m=2, bf=BF, n_blocks=10, mv0=None, mv1=None, ref0=RK0, N0=900, C0=CR0, ld0=8, ref1=RK1, N1=1100, C1=CR1,
             ld1=8, shift=3, x=X, ldx=8, D=8, w=W, mode=MD, best=BC, table=TB):
        return L.raht_mode_search(keys, N, J, m, bf, n_blocks, mv0, mv1, ref0, N0, C0, ld0, ref1, N1, C1, ld1, shift, x, ldx, D, w, mode, best,
                                  table, None)

    cases = dict(_cases(), **{"NULL X": dict(x=None), "NULL weights": dict(w=None)})
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == INVALID, (what, rc)
        assert b"raht_mode_search:" in L.raht_last_error(), (what, L.raht_last_error())


def test_predict_bi_modes_argument_validation(L):
    def call(keys=K, N=1000, J=6, m=2, bf=BF, n_blocks=10, mode=MD, mv0=None, mv1=None, ref0=RK0, N0=900, C0=CR0, ld0=8, ref1=RK1, N1=1100,
             C1=CR1, ld1=8, shift=3, x=X, ldx=8, D=8, add=0, y=Y, ldy=8, nm=NM):
        return L.raht_predict_bi_modes(keys, N, J, m, bf, n_blocks, mode, mv0, mv1, ref0, N0, C0, ld0, ref1, N1, C1, ld1, shift, x, ldx, D, add,
                                       y, ldy, nm, None)

    cases = dict(_cases(), **{"NULL Y": dict(y=None), "NULL X, NULL Y": dict(x=None, y=None), "ldy < D": dict(ldy=7), "add = 2": dict(add=2),
                              "add = -1": dict(add=-1), "NULL X, add = 2": dict(x=None, add=2)})
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == INVALID, (what, rc)
        assert b"raht_predict_bi_modes:" in L.raht_last_error(), (what, L.raht_last_error())


def test_python_wrappers_refuse_host_tensors_and_bad_arguments():
    import torch
    from raht_3dgs_codec_amd import ops
    k = torch.arange(10, dtype=torch.int64)
    C = torch.zeros((10, 3))
    bf = torch.tensor([0, 10])
    md = torch.zeros(1, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mode_search(k, (k, C), (k, C), C, 4, 2, bf, [1.0, 1.0, 1.0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.predict_bi(k, (k, C), (k, C), J=4, block_log2=2, block_first=bf, modes=md)
    with pytest.raises(ValueError, match="pairs"):
        ops.mode_search(k, k, C, C, 4, 2, bf, [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match="modes need"):
        ops.predict_bi(k, (k, C), (k, C), modes=md)
    with pytest.raises(ValueError, match="modes need"):
        ops.predict_bi(k, (k, C), (k, C), modes=md, J=4, block_log2=2)
