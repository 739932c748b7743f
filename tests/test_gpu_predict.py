"""ops.predict / raht_predict against the definition (tests/numpy_predict.py), bit for bit, in all three modes -- P alone, X - P, and
X + P in place -- with the count of matched rows. Shapes: the smallest at which the kernel can go wrong -- one row, rows of 59
floats (16-byte chunks straddle them), padded rows (the element-wise path), frames that end inside a workgroup's block of rows and
one row behind it, more blocks than one, runs that are empty, of one row and of many."""
import numpy as np
import pytest

from . import numpy_predict as M

pytestmark = pytest.mark.gpu

TILE = 256                                                               # rows a workgroup resolves per step (csrc/predict.hip: PR_TILE_ROWS)


def _attrs(n, D, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, D)).astype(np.float32)
    A[::7, 0] = -0.0                                                     # -0 - 0 = -0, -0 + 0 = +0: the operation is performed, not skipped
    return A


def _check(keys, ref_keys, C_ref, X, up, pad=0, what=""):
    """all three modes of one case against the model; pad: extra columns in every matrix (row stride D + pad)"""
    import torch
    from raht_3dgs_codec_amd import ops

    def dev(a):
        a = np.ascontiguousarray(a)
        if pad and a.ndim == 2:
            wide = torch.full((a.shape[0], a.shape[1] + pad), 7.0, dtype=torch.float32, device="cuda")
            wide[:, :a.shape[1]] = torch.from_numpy(a).cuda()
            return wide[:, :a.shape[1]]
        return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()

    P, n = M.predict(keys, ref_keys, C_ref, up)
    k, r, Cr = dev(keys), dev(ref_keys), dev(C_ref)
    assert (Cr.stride(0) == C_ref.shape[1] + pad)
    got, nm = ops.predict(k, r, Cr, up=up, want_matched=True)
    assert got.dtype == torch.float32 and nm.dtype == torch.int64
    assert int(nm.item()) == n, (what, up)
    assert torch.equal(got.cpu().view(torch.int32), torch.from_numpy(P).view(torch.int32)), (what, up, "P")
    out = dev(np.zeros_like(X))
    res = ops.predict(k, r, Cr, X=dev(X), up=up, out=out)
    assert res.data_ptr() == out.data_ptr()
    assert torch.equal(out.cpu().view(torch.int32), torch.from_numpy(M.apply(X, P)).view(torch.int32)), (what, up, "X - P")
    Xd = dev(X)
    _, nm = ops.predict(k, r, Cr, X=Xd, up=up, add=True, out=Xd, want_matched=True)                # in place
    assert int(nm.item()) == n
    assert torch.equal(Xd.cpu().view(torch.int32), torch.from_numpy(M.apply(X, P, add=True)).view(torch.int32)), (what, up, "X + P")
    if pad:                                                              # nothing was written beside the rows
        assert bool((Xd._base[:, -pad:] == 7.0).all()) and bool((out._base[:, -pad:] == 7.0).all())
    assert torch.equal(Cr.cpu().view(torch.int32), torch.from_numpy(np.ascontiguousarray(C_ref)).view(torch.int32))       # the reference is read only


@pytest.mark.parametrize("up", [0, 1, 2, 3])
def test_one_row_against_one_row(up):
    C, X = _attrs(1, 5, 1), _attrs(1, 5, 2)
    one = np.array([0o1234], np.uint64)
    _check(one, one, C, X, up, what="hit")
    _check(one, np.array([0o7234], np.uint64), C, X, up, what="miss")   # another cell at every up <= 3
    _check(one, np.array([0o1235], np.uint64), C, X, up, what="the neighbour: a hit from up = 1 on")


@pytest.mark.parametrize("up", [0, 1, 2, 3])
@pytest.mark.parametrize("n,J,D,pad", [(257, 3, 4, 0), (3000, 6, 5, 0), (3000, 6, 59, 0), (3000, 6, 5, 3), (3000, 6, 59, 3)])
def test_scenes_against_thinned_and_shifted_references(n, J, D, pad, up):
    from raht_3dgs_codec_amd import synth
    if J == 3:                                                           # exactly n of the 512 keys of depth 3, and n - 57 others
        rng = np.random.default_rng(10)
        keys, ref = (np.sort(rng.choice(8 ** J, size=m, replace=False)).astype(np.uint64) for m in (n, n - 57))
    else:
        keys = synth.sorted_unique_keys(n, J, 11)
        ref = synth.sorted_unique_keys(n, J, 12)                         # another scene: hits and misses mixed, N_ref != N
    X, C = _attrs(len(keys), D, 5), _attrs(len(ref), D, 6)
    _check(keys, ref, C, X, up, pad, "another scene")
    _check(keys, keys, X, X, up, pad, "itself")
    _check(keys, ref[::3], C[::3], X, up, pad, "every third key: empty cells and runs of one")


@pytest.mark.parametrize("up", [0, 3])
def test_current_keys_entirely_below_and_above_the_reference(up):
    from raht_3dgs_codec_amd import synth
    keys = synth.sorted_unique_keys(3000, 6, 13)
    h = len(keys) // 2
    cut = (keys[h] >> np.uint64(9)) << np.uint64(9)                      # split on a cell boundary of up = 3: no cell on both sides
    low, high = keys[keys < cut], keys[keys >= cut]
    assert len(low) > TILE and len(high) > TILE
    A = _attrs(len(keys), 5, 7)
    _check(low, high, A[len(low):], A[:len(low)], up, what="below")
    _check(high, low, A[:len(low)], A[len(low):], up, what="above")


@pytest.mark.parametrize("n,D", [(n, D) for D in (3, 59) for n in (TILE - 1, TILE, TILE + 1, 3 * TILE, 3 * TILE + 1)] + [(2049 * TILE + 1, 3)])
def test_frames_that_end_inside_and_just_behind_a_block_of_rows(n, D):
    """N no multiple of the rows a workgroup resolves, one row more than a multiple (a last tile of one row: its D elements are no
    multiple of four), and more tiles than the capped grid has workgroups (the grid-stride loop's second round)."""
    rng = np.random.default_rng(n)
    keys = np.sort(rng.choice(8 * n, size=n, replace=False)).astype(np.uint64)
    ref = np.sort(rng.choice(8 * n, size=n, replace=False)).astype(np.uint64)
    _check(keys, ref, _attrs(n, D, 8), _attrs(n, D, 9), 1, what=f"n = {n}")
