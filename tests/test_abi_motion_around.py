"""CPU-only checks of raht_motion_search_around at the C-ABI boundary: declared, exported and bound with the header's argument
list, and every argument rule refused with RAHT_ERR_INVALID and the function's name before any HIP call -- the "device pointers"
below are addresses that must never be read."""
import os
import re

import pytest

INVALID = -1
K, BF, RK, CR, X, W, CA, BK, BC, TB, MV, BA = (0x10000 * i for i in range(1, 13))          # never dereferenced
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def _declared_args(name):
    """the parameter declarations of ``name`` in include/raht.h"""
    src = open(os.path.join(ROOT, "include", "raht.h")).read()
    m = re.search(r"\bint %s\(([^;]*?)\);" % name, src)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_the_header_the_library_and_the_binding_agree(L):
    import ctypes as C
    from raht_3dgs_codec_amd import _lib
    name = "raht_motion_search_around"
    assert name in _lib.EXPORTS and hasattr(L, name)
    args, parent = _declared_args(name), _declared_args("raht_motion_search")
    assert len(args) == 23 and len(getattr(L, name).argtypes) == 23
    # raht_motion_search's arguments plus base (in front of the candidates) and mv (behind best_cost)
    assert [a for a in args if a not in ("const int8_t *base", "int8_t *mv")] == parent
    assert args.index("const int8_t *base") == 15 and args.index("int8_t *mv") == 20
    kinds = {"*": C.c_void_p, "int64_t": C.c_int64, "int": C.c_int, "raht_stream_t": C.c_void_p}
    for decl, bound in zip(args, getattr(L, name).argtypes):
        want = kinds["*"] if "*" in decl else kinds[decl.rsplit(" ", 1)[0]]
        assert bound is want, (decl, bound)
    assert L.raht_version() == 300                                       # a new entry point, no new ABI version


def test_motion_search_around_argument_validation(L):
    def call(keys=K, N=1000, J=6, m=3, bf=BF, nb=40, ref=RK, N_ref=900, shift=3, C_ref=CR, ld_ref=8, x=X, ldx=8, D=8, w=W, base=BA, cand=CA,
             k=27, best_k=BK, best_cost=BC, mv=MV, table=TB):
        return L.raht_motion_search_around(keys, N, J, m, bf, nb, ref, N_ref, shift, C_ref, ld_ref, x, ldx, D, w, base, cand, k, best_k,
                                           best_cost, mv, table, None)

    cases = {"NULL keys": dict(keys=None), "NULL block_first": dict(bf=None), "NULL ref_keys": dict(ref=None), "NULL C_ref": dict(C_ref=None),
             "N = 0": dict(N=0), "N < 0": dict(N=-3), "N = 2^31": dict(N=2 ** 31, nb=1), "N_ref = 0": dict(N_ref=0), "N_ref < 0": dict(N_ref=-1),
             "N_ref = 2^31": dict(N_ref=2 ** 31), "J = 0": dict(J=0, m=0), "J = 22": dict(J=22), "J < 0": dict(J=-1),
             "block_log2 = 0": dict(m=0), "block_log2 < 0": dict(m=-2), "block_log2 = J + 1": dict(m=7), "n_blocks = 0": dict(nb=0),
             "n_blocks < 0": dict(nb=-1), "n_blocks = N + 1": dict(nb=1001), "shift = 1": dict(shift=1), "shift = -3": dict(shift=-3),
             "shift = 12": dict(shift=12), "shift = 4": dict(shift=4), "D = 0": dict(D=0), "D < 0": dict(D=-8), "ld_ref < D": dict(ld_ref=7),
             "ldx < D": dict(ldx=7), "NULL X": dict(x=None), "NULL weights": dict(w=None), "NULL candidates": dict(cand=None),
             "NULL best_k": dict(best_k=None), "K = 0": dict(k=0), "K < 0": dict(k=-27), "K = 513": dict(k=513),
             "NULL table, K = 0": dict(table=None, best_cost=None, k=0), "NULL base": dict(base=None), "NULL mv": dict(mv=None),
             "NULL base and mv": dict(base=None, mv=None), "NULL mv, K = 0": dict(mv=None, k=0)}
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == INVALID, (what, rc)
        assert b"raht_motion_search_around" in L.raht_last_error(), (what, L.raht_last_error())


def test_python_wrappers_refuse_host_tensors_and_bad_levels():
    import numpy as np
    import torch
    from raht_3dgs_codec_amd import ops
    k = torch.arange(10, dtype=torch.int64)
    C = torch.zeros((10, 3))
    bf = torch.tensor([0, 10])
    base = torch.zeros((1, 3), dtype=torch.int8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.motion_search_around(k, k, C, C, 4, 2, bf, base, ops.motion_candidates(1), np.ones(3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.motion_pyramid(k, C, 4, 1, [1, 1, 2, 5, 10])
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.motion_search_hier(k, k, C, C, 4, 2, bf, 1, 1, np.ones(3))
    for J, m, levels in ((4, 2, 2), (4, 4, 4), (4, 3, -1), (2, 2, 2), (3, 4, 3)):          # L > m - 1, L > 3, L < 0, J - L < 1 (twice)
        with pytest.raises(ValueError, match="levels"):
            ops.motion_search_hier(k, k, C, C, J, m, bf, levels, 1, np.ones(3))
    with pytest.raises(ValueError, match="radius"):
        ops.motion_search_hier(k, k, C, C, 4, 2, bf, 1, 4, np.ones(3))
