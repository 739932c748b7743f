"""CPU-only checks of the voxelizer's six entry points at the C-ABI boundary (csrc/voxelize.hip): exported and bound with their
arities, and every argument rule refused with RAHT_ERR_INVALID before any HIP call -- the "device pointers" below are addresses
that must never be read, and there is no GPU to launch on.

Every refusal carries the CALLED function's name in raht_last_error(). That part was new with the voxelizer's consolidation: before
it, raht_voxelize_all / _plan / _merge reported the rules they share with raht_voxelize under that name, so the name checks of
those three fail on older libraries. So do two rules that older libraries reached only behind their first device allocation (same
code on a GPU, out of device memory without one): a width of 0 or NaN given by the caller, and the residuals of a narrow cloud
without sort_idx."""
import ctypes
import os

import pytest

INVALID = -1
NAMES = {"raht_voxel_keys": 8, "raht_voxelize": 17, "raht_voxelize_all": 19, "raht_voxelize_plan": 16, "raht_voxelize_merge": 18,
         "raht_voxelize_residuals": 12}
A, B, Cc, Dd, E, F, G = (0x10000 * k for k in range(1, 8))          # never dereferenced


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def _f3(*v):
    return (ctypes.c_float * 3)(*v)


def _refused(L, name, rc, what):
    assert rc == INVALID, (name, what, rc)
    assert name.encode() + b":" in L.raht_last_error(), (name, what, L.raht_last_error())


def test_the_six_symbols_are_exported_and_bound(L):
    from raht_3dgs_codec_amd import _lib
    for name, arity in NAMES.items():
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == arity, name


def test_voxel_keys_argument_validation(L):
    def call(PC=A, ldpc=3, N=100, vmin=_f3(0, 0, 0), width=1.0, J=10, keys=B):
        return L.raht_voxel_keys(PC, ldpc, N, vmin, width, J, keys, None)

    for what, kw in {"NULL PC": dict(PC=None), "NULL keys": dict(keys=None), "NULL vmin": dict(vmin=None), "N < 0": dict(N=-1),
                     "J = 0": dict(J=0), "J = 22": dict(J=22), "ldpc < 3": dict(ldpc=2), "width = 0": dict(width=0.0),
                     "width < 0": dict(width=-1.0), "width NaN": dict(width=float("nan"))}.items():
        _refused(L, "raht_voxel_keys", call(**kw), what)
    assert call(N=0) == 0 and call(N=0, PC=None, keys=None) == 0          # an empty rank of a sharded cloud: nothing to do


# the rules the four voxelizing calls share; ``d`` is color_dim for raht_voxelize_merge (row width 11 + color_dim)
def _shared_cases(width_of_d):
    return {"NULL PC": dict(PC=None), "NULL n_vox": dict(n_vox=None), "N = 0": dict(N=0), "N < 0": dict(N=-5), "N = 2^31": dict(N=2 ** 31),
            "J = 0": dict(J=0), "J = 22": dict(J=22), "d < 0": dict(d=-1), "ldpc < row width": dict(ldpc=width_of_d(6) - 1),
            "width = 0": dict(width=0.0), "width = 0, vmin given": dict(width=0.0, vmin=_f3(0, 0, 0)), "width NaN": dict(width=float("nan"))}


def test_voxelize_argument_validation(L):
    nv = ctypes.c_int64()

    def call(PC=A, ldpc=9, N=100, d=6, vmin=None, width=-1.0, J=10, n_vox=ctypes.byref(nv)):
        return L.raht_voxelize(PC, ldpc, N, d, vmin, width, J, B, Cc, Dd, E, None, n_vox, None, None, None, None)

    for what, kw in _shared_cases(lambda d: 3 + d).items():
        _refused(L, "raht_voxelize", call(**kw), what)


def test_voxelize_all_argument_validation(L):
    nv = ctypes.c_int64()

    def call(PC=A, ldpc=9, N=100, d=6, vmin=None, width=-1.0, J=10, sort_idx=Cc, PCvox=E, PCsorted=F, DeltaPC=G, n_vox=ctypes.byref(nv)):
        return L.raht_voxelize_all(PC, ldpc, N, d, vmin, width, J, B, sort_idx, Dd, PCvox, None, PCsorted, DeltaPC, n_vox, None, None, None, None)

    cases = _shared_cases(lambda d: 3 + d)
    cases.update({"DeltaPC without PCvox": dict(PCvox=None), "position-only residuals without sort_idx": dict(PCvox=None, d=0, ldpc=3, sort_idx=None),
                  "residuals of a narrow cloud without sort_idx": dict(d=4, ldpc=7, sort_idx=None),
                  "sorted points of a narrow cloud without sort_idx": dict(d=2, ldpc=5, sort_idx=None, DeltaPC=None),
                  "sorted points with neither PCvox nor sort_idx": dict(PCvox=None, DeltaPC=None, sort_idx=None)})
    for what, kw in cases.items():
        _refused(L, "raht_voxelize_all", call(**kw), what)


def test_voxelize_plan_argument_validation(L):
    nv = ctypes.c_int64()
    h = ctypes.c_void_p(0x1234)

    def call(PC=A, ldpc=9, N=100, d=6, vmin=None, width=-1.0, J=10, vkeys=B, n_vox=ctypes.byref(nv), plan=ctypes.byref(h)):
        return L.raht_voxelize_plan(PC, ldpc, N, d, vmin, width, J, vkeys, Cc, Dd, n_vox, None, None, None, None, plan)

    cases = _shared_cases(lambda d: 3 + d)
    del cases["NULL n_vox"]                                              # optional here: the plan knows its size
    cases.update({"NULL voxel_keys": dict(vkeys=None), "NULL plan": dict(plan=None)})
    for what, kw in cases.items():
        h.value = 0x1234
        _refused(L, "raht_voxelize_plan", call(**kw), what)
        assert what == "NULL plan" or what == "NULL voxel_keys" or h.value is None, what          # *plan is NULL on failure


def test_voxelize_merge_argument_validation(L):
    nv = ctypes.c_int64()

    def call(PC=A, ldpc=17, N=100, d=6, wbo=1, vmin=None, width=-1.0, J=10, Gvox=E, n_vox=ctypes.byref(nv)):
        return L.raht_voxelize_merge(PC, ldpc, N, d, wbo, vmin, width, J, B, Cc, Dd, Gvox, F, n_vox, None, None, None, None)

    cases = _shared_cases(lambda cd: 11 + cd)
    cases.update({"color_dim < 0": dict(d=-1), "color_dim = -8": dict(d=-8, ldpc=3), "NULL Gvox": dict(Gvox=None)})
    for what, kw in cases.items():
        _refused(L, "raht_voxelize_merge", call(**kw), what)


def test_voxelize_residuals_argument_validation(L):
    def call(PC=A, ldpc=9, N=100, d=6, keys=B, sort_idx=Cc, PCvox=Dd, vmin=_f3(0, 0, 0), vs=0.25, PCsorted=E, DeltaPC=F):
        return L.raht_voxelize_residuals(PC, ldpc, N, d, keys, sort_idx, PCvox, vmin, vs, PCsorted, DeltaPC, None)

    for what, kw in {"NULL PC": dict(PC=None), "NULL keys_sorted": dict(keys=None), "NULL sort_idx": dict(sort_idx=None),
                     "NULL vmin": dict(vmin=None), "NULL DeltaPC": dict(DeltaPC=None), "NULL PCvox with attributes": dict(PCvox=None),
                     "N = 0": dict(N=0), "N = 2^31": dict(N=2 ** 31), "d < 0": dict(d=-1), "ldpc < 3 + d": dict(ldpc=8),
                     "voxel_size = 0": dict(vs=0.0), "voxel_size NaN": dict(vs=float("nan"))}.items():
        _refused(L, "raht_voxelize_residuals", call(**kw), what)
