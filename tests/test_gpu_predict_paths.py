"""The forms of raht_predict / raht_predict_mc that tests/test_gpu_predict.py never reaches, against the same definition
(tests/numpy_predict.py, tests/numpy_motion.py), bit for bit in all three modes -- P alone, X - P, X + P in place -- with the
count of matched rows:
  - rows of 1, 2, 7 and 8 floats: chunks of 16 bytes that hold four rows, two rows, straddle at most two rows, lie in one row
  - every mix of padded and contiguous C_ref, X and out: the flat path over a padded reference in all three modes (there only P
    alone runs it), the element path with one of X / out contiguous
  - contiguous matrices whose base is 4-byte but not 16-byte aligned (rows 1 .. of a larger matrix) under the 16-byte moves
  - cells that hold all 8^up reference rows: runs that end on the search window's end and on N_ref, 512 sequential additions
  - a reference of one row
Each case runs the co-located predictor and the compensated one, under a zero field and under a random field."""
import numpy as np
import pytest

from . import numpy_motion as MM
from . import numpy_predict as M
from .test_gpu_predict import _attrs

pytestmark = pytest.mark.gpu

FILL = 7.0


def _mat(a, padded=False, offset=False):
    """a float32 matrix on the device -> (the view the call takes, the allocation it lies in): padded = three more columns per row
    (row stride D + 3); offset = rows 1 .. of a contiguous (n + 1, D) matrix (row stride D, base D floats behind the allocation's).
    Whatever is not the matrix holds FILL."""
    import torch
    a = np.ascontiguousarray(a, np.float32)
    n, D = a.shape
    base = torch.full((n + int(offset), D + (3 if padded else 0)), FILL, dtype=torch.float32, device="cuda")
    view = base[int(offset):, :D]
    view.copy_(torch.from_numpy(a).cuda())
    assert view.stride(0) == D + (3 if padded else 0) and view.data_ptr() == base.data_ptr() + 4 * int(offset) * base.stride(0)
    return view, base


def _untouched(view, base, a, what):
    """the matrix holds a, bit for bit, and everything beside it in its allocation still holds FILL"""
    import torch
    assert np.array_equal(view.cpu().numpy().view(np.int32), np.ascontiguousarray(a, np.float32).view(np.int32)), what
    n, D = view.shape
    rest = torch.ones_like(base, dtype=torch.bool)
    rest[base.shape[0] - n:, :D] = False
    assert bool((base[rest] == FILL).all()), (what, "written beside the matrix")


def _keys(k):
    import torch
    return torch.from_numpy(np.ascontiguousarray(k).view(np.int64)).cuda()


def _fields(keys, J, m, seed):
    """a zero field and a random one within +-2 (hits, misses and rows that leave the cube)"""
    nb = len(MM.blocks(keys, m)[1]) - 1
    return [np.zeros((nb, 3), np.int8), np.random.default_rng(seed).integers(-2, 3, size=(nb, 3)).astype(np.int8)]


def _check(keys, ref_keys, C_ref, X, up, J, pads=(False, False, False), offset=False, what=""):
    """all three modes of raht_predict, and of raht_predict_mc under two fields, against the model. pads = (C_ref, X, out) padded;
    offset: every matrix lies one row behind its allocation's base -> the models' (lo, hi) runs"""
    import torch
    from raht_3dgs_codec_amd import ops
    k, r = _keys(keys), _keys(ref_keys)
    m = min(2, J)
    bf = ops.motion_blocks(k, J, m, len(MM.blocks(keys, m)[1]) - 1)
    calls = [("predict", M.predict(keys, ref_keys, C_ref, up), lambda **kw: ops.predict(k, r, kw.pop("C"), up=up, **kw))]
    for i, mv in enumerate(_fields(keys, J, m, len(keys))):
        mvd = torch.from_numpy(mv).cuda()
        calls.append((f"predict_mc, field {i}", MM.predict_mc(keys, ref_keys, C_ref, J, m, mv, up),
                      lambda mvd=mvd, **kw: ops.predict_mc(k, r, kw.pop("C"), mvd, bf, J, m, up=up, **kw)))
    assert np.array_equal(calls[0][1][0].view(np.int32), calls[1][1][0].view(np.int32))       # the model: a zero field is the predictor
    for name, (P, n), call in calls:
        tag = (what, name, up, pads, offset)
        Cr, Cb = _mat(C_ref, pads[0], offset)
        # P alone, into an output of the chosen form
        out, ob = _mat(np.zeros_like(X), pads[2], offset)
        res, nm = call(C=Cr, out=out, want_matched=True)
        assert res.data_ptr() == out.data_ptr() and int(nm.item()) == n, tag
        _untouched(out, ob, P, tag + ("P",))
        # X - P
        Xd, Xb = _mat(X, pads[1], offset)
        out, ob = _mat(np.zeros_like(X), pads[2], offset)
        res, nm = call(C=Cr, X=Xd, out=out, want_matched=True)
        assert res.data_ptr() == out.data_ptr() and int(nm.item()) == n, tag
        _untouched(out, ob, M.apply(X, P), tag + ("X - P",))
        _untouched(Xd, Xb, X, tag + ("X is read only",))
        # X + P in place, in X's form
        res, nm = call(C=Cr, X=Xd, add=True, out=Xd, want_matched=True)
        assert res.data_ptr() == Xd.data_ptr() and int(nm.item()) == n, tag
        _untouched(Xd, Xb, M.apply(X, P, add=True), tag + ("X + P in place",))
        _untouched(Cr, Cb, C_ref, tag + ("the reference is read only",))
    return M.runs(keys, ref_keys, up)


def _scene(n, J, seed):
    """n keys of depth J and a reference of another draw, N_ref != N, whose octant 6 is empty and whose octant 5 holds one voxel:
    empty runs, runs of one row and (from up = 1 on) of many rows at every up"""
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.choice(8 ** J, size=n, replace=False)).astype(np.uint64)
    ref = np.sort(rng.choice(8 ** J, size=max(1, (3 * n) // 4), replace=False)).astype(np.uint64)
    octant = ref >> np.uint64(3 * J - 3)
    ref = np.union1d(ref[(octant != 5) & (octant != 6)], np.array([5 * 8 ** (J - 1) + 11], np.uint64))
    return keys, ref


@pytest.mark.parametrize("up", [0, 1, 3])
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 769])
@pytest.mark.parametrize("D", [1, 2, 7, 8])
def test_narrow_and_aligned_rows(D, n, up):
    J = 4                                                                # 4096 voxels: 769 keys fill a fifth of them
    keys, ref = _scene(n, J, 100 + n)
    lo, hi = _check(keys, ref, _attrs(len(ref), D, 6), _attrs(n, D, 5), up, J, what=f"D = {D}, n = {n}")
    if n >= 255:                                                         # empty, single-row and multi-row runs are mixed
        assert (hi == lo).any() and (hi - lo == 1).any()
        assert up == 0 or (hi - lo > 1).any()


@pytest.mark.parametrize("pads", [(c, x, o) for c in (False, True) for x in (False, True) for o in (False, True)])
@pytest.mark.parametrize("D", [1, 5, 59, 64])
def test_every_mix_of_padded_and_contiguous_matrices(D, pads):
    """flat (X and out contiguous) over a padded reference; the element path with only X or only out padded; in place with X
    padded (the in-place mode takes X's form, whatever out's is). Pad columns keep their fill value: _untouched."""
    J, n = 4, 600                                                        # more than two tiles of rows
    keys, ref = _scene(n, J, 7)
    for up in (0, 2):
        lo, hi = _check(keys, ref, _attrs(len(ref), D, 6), _attrs(n, D, 5), up, J, pads, what=f"D = {D}")
        assert (hi == lo).any() and (hi > lo).any()


@pytest.mark.parametrize("D", [1, 3, 59])
def test_bases_that_are_not_16_byte_aligned(D):
    """C_ref, X and out are rows 1 .. of contiguous (n + 1, D) matrices: the base is 4 D bytes behind a 16-byte boundary, the row
    stride stays D, so the moves are the flat path's 16-byte nontemporal ones. Row 0 of the allocation is unchanged: _untouched."""
    J, n = 4, 600
    keys, ref = _scene(n, J, 8)
    probe, base = _mat(np.zeros((2, D), np.float32), offset=True)
    assert base.data_ptr() % 16 == 0 and probe.data_ptr() % 16 == (4 * D) % 16 != 0 and probe.data_ptr() % 4 == 0
    assert probe.is_contiguous()
    for up in (0, 1):
        lo, hi = _check(keys, ref, _attrs(len(ref), D, 6), _attrs(n, D, 5), up, J, offset=True, what=f"D = {D}, rows 1 ..")
        assert (hi == lo).any() and (hi > lo).any()


@pytest.mark.parametrize("up", [1, 2, 3])
@pytest.mark.parametrize("D", [5, 8])
def test_every_key_of_depth_3_as_reference(D, up):
    """N_ref = 512 = every key of depth 3, the frame 300 of them: every cell is full. up = 3: ONE run of 512 rows, which ends on
    the search window's end and on N_ref at once"""
    J = 3
    ref = np.arange(8 ** J, dtype=np.uint64)
    keys = np.sort(np.random.default_rng(9).choice(8 ** J, size=300, replace=False)).astype(np.uint64)
    lo, hi = _check(keys, ref, _attrs(len(ref), D, 6), _attrs(len(keys), D, 5), up, J, what="full cells")
    assert ((hi - lo) == 8 ** up).all() and (hi == len(ref)).any()


@pytest.mark.parametrize("D", [5, 8])
def test_full_first_and_last_cells_among_thinned_ones(D):
    """depth 4, up = 2: the first and the last cell of 64 voxels are full, the others keep every fifth voxel or none"""
    J, up = 4, 2
    rng = np.random.default_rng(10)
    every = np.arange(8 ** J, dtype=np.uint64)
    cell = every >> np.uint64(6)
    keep = (cell == 0) | (cell == 63) | ((cell % 3 != 1) & (rng.random(len(every)) < 0.2))
    ref = every[keep]
    keys = np.sort(rng.choice(8 ** J, size=700, replace=False)).astype(np.uint64)
    lo, hi = _check(keys, ref, _attrs(len(ref), D, 6), _attrs(len(keys), D, 5), up, J, what="full cells at either end")
    n = hi - lo
    assert (n == 64).any() and ((n == 64) & (hi == len(ref))).any() and ((n == 64) & (lo == 0)).any()
    assert (n == 0).any() and ((n > 0) & (n < 64)).any()


@pytest.mark.parametrize("up", [0, 3])
@pytest.mark.parametrize("D", [5, 59])
def test_a_reference_of_one_row(D, up):
    J, n = 4, 257
    keys, _ = _scene(n, J, 11)
    ref = keys[100:101].copy()
    lo, hi = _check(keys, ref, _attrs(1, D, 6), _attrs(n, D, 5), up, J, what="N_ref = 1")
    assert int((hi > lo).sum()) == (1 if up == 0 else int((keys >> np.uint64(9) == ref[0] >> np.uint64(9)).sum())) and (hi == lo).any()
