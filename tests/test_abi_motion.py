"""CPU-only checks of raht_motion_search and raht_predict_mc at the C-ABI boundary: exported, bound, and every argument rule refused
with RAHT_ERR_INVALID and the function's name before any HIP call -- the "device pointers" below are addresses that must never be
read."""
import os

import pytest

INVALID = -1
K, BF, RK, CR, X, Y, NM, W, CA, BK, BC, TB, MV = (0x10000 * i for i in range(1, 14))       # never dereferenced


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def test_the_symbols_are_exported_and_bound(L):
    from raht_3dgs_codec_amd import _lib
    for name, n_args in (("raht_motion_search", 21), ("raht_predict_mc", 20)):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == n_args
    assert L.raht_version() == 300                                       # new entry points, no new ABI version


FRAME = {"NULL keys": dict(keys=None), "NULL block_first": dict(bf=None), "NULL ref_keys": dict(ref=None), "NULL C_ref": dict(C_ref=None),
         "N = 0": dict(N=0), "N < 0": dict(N=-3), "N = 2^31": dict(N=2 ** 31, nb=1), "N_ref = 0": dict(N_ref=0), "N_ref < 0": dict(N_ref=-1),
         "N_ref = 2^31": dict(N_ref=2 ** 31), "J = 0": dict(J=0, m=0), "J = 22": dict(J=22), "J < 0": dict(J=-1),
         "block_log2 = 0": dict(m=0), "block_log2 < 0": dict(m=-2), "block_log2 = J + 1": dict(m=7), "n_blocks = 0": dict(nb=0),
         "n_blocks < 0": dict(nb=-1), "n_blocks = N + 1": dict(nb=1001), "shift = 1": dict(shift=1), "shift = -3": dict(shift=-3),
         "shift = 12": dict(shift=12), "shift = 4": dict(shift=4), "D = 0": dict(D=0), "D < 0": dict(D=-8), "ld_ref < D": dict(ld_ref=7),
         "ldx < D": dict(ldx=7)}


def _refused(L, name, call, cases):
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == INVALID, (name, what, rc)
        assert name.encode() in L.raht_last_error(), (what, L.raht_last_error())


def test_motion_search_argument_validation(L):
    def call(keys=K, N=1000, J=6, m=3, bf=BF, nb=40, ref=RK, N_ref=900, shift=3, C_ref=CR, ld_ref=8, x=X, ldx=8, D=8, w=W, cand=CA, k=27,
             best_k=BK, best_cost=BC, table=TB):
        return L.raht_motion_search(keys, N, J, m, bf, nb, ref, N_ref, shift, C_ref, ld_ref, x, ldx, D, w, cand, k, best_k, best_cost, table,
                                    None)

    cases = dict(FRAME)
    cases.update({"NULL X": dict(x=None), "NULL weights": dict(w=None), "NULL candidates": dict(cand=None), "NULL best_k": dict(best_k=None),
                  "K = 0": dict(k=0), "K < 0": dict(k=-27), "K = 513": dict(k=513),
                  "NULL table, K = 0": dict(table=None, best_cost=None, k=0)})
    _refused(L, "raht_motion_search", call, cases)


def test_predict_mc_argument_validation(L):
    def call(keys=K, N=1000, J=6, m=3, bf=BF, nb=40, mv=MV, ref=RK, N_ref=900, shift=3, C_ref=CR, ld_ref=8, x=X, ldx=8, D=8, add=0, y=Y,
             ldy=8, nm=NM):
        return L.raht_predict_mc(keys, N, J, m, bf, nb, mv, ref, N_ref, shift, C_ref, ld_ref, x, ldx, D, add, y, ldy, nm, None)

    cases = dict(FRAME)
    cases.update({"NULL mv": dict(mv=None), "NULL Y": dict(y=None), "ldy < D": dict(ldy=7), "add = 2": dict(add=2), "add = -1": dict(add=-1),
                  "NULL X, NULL Y": dict(x=None, y=None), "NULL X, add = 2": dict(x=None, add=2)})
    _refused(L, "raht_predict_mc", call, cases)


def test_python_wrappers_refuse_host_tensors_and_bad_arguments():
    import numpy as np
    import torch
    from raht_3dgs_codec_amd import ops
    k = torch.arange(10, dtype=torch.int64)
    C = torch.zeros((10, 3))
    bf = torch.tensor([0, 10])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.motion_blocks(k, 4, 2, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.motion_search(k, k, C, C, 4, 2, bf, ops.motion_candidates(1), np.ones(3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.predict_mc(k, k, C, torch.zeros((1, 3), dtype=torch.int8), bf, 4, 2, X=C, add=True, out=C, want_matched=True)
