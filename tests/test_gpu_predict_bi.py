"""ops.predict_bi / raht_predict_bi against the definition (tests/numpy_predict_bi.py), bit for bit, in all three modes -- P alone,
X - P, and X + P in place -- with the three counts of matched rows. Shapes: the smallest at which the kernel can go wrong -- one
row in each of the four hit combinations, rows of 59 floats (16-byte chunks straddle them), padded rows (the element-wise path),
frames that end inside a workgroup's block of rows and one row behind it, more blocks than the grid has workgroups, motion fields
on either reference and on both with vectors that leave the cube. Values are in the normal float32 range."""
import numpy as np
import pytest

from . import numpy_motion as MM
from . import numpy_predict as M1
from . import numpy_predict_bi as M

pytestmark = pytest.mark.gpu

TILE = 256                                                               # rows a workgroup resolves per step (PR_TILE_ROWS)


def _attrs(n, D, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, D)).astype(np.float32)
    A[::7, 0] = -0.0                                                     # -0 - 0 = -0, -0 + 0 = +0: the operation is performed, not skipped
    return A


def _dev(a, pad=0):
    import torch
    a = np.ascontiguousarray(a)
    if pad and a.ndim == 2 and a.dtype == np.float32:
        wide = torch.full((a.shape[0], a.shape[1] + pad), 7.0, dtype=torch.float32, device="cuda")
        wide[:, :a.shape[1]] = torch.from_numpy(a).cuda()
        return wide[:, :a.shape[1]]
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _bits(t):
    import torch
    return (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))).cpu().contiguous().view(torch.int32)


def _check(keys, ref0, ref1, X, up, pad=0, what="", J=None, block_log2=0, mv0=None, mv1=None, combos=None):
    """all three modes of one case against the model; pad: extra columns in every matrix (row stride D + pad); combos: the hit
    combinations (reference 0, reference 1) that must occur -> the model's P"""
    import torch
    from raht_3dgs_codec_amd import ops
    P, n, h0, h1 = M.predict(keys, ref0, ref1, up, J, block_log2, mv0, mv1)
    for c in combos or ():
        assert ((h0 == c[0]) & (h1 == c[1])).any(), (what, up, c)
    k, r0, r1 = _dev(keys), (_dev(ref0[0]), _dev(ref0[1], pad)), (_dev(ref1[0]), _dev(ref1[1], pad))
    kw = dict(up=up)
    if mv0 is not None or mv1 is not None:
        bf = _dev(MM.blocks(keys, block_log2)[1])
        kw.update(J=J, block_log2=block_log2, block_first=bf, mv0=None if mv0 is None else _dev(mv0), mv1=None if mv1 is None else _dev(mv1))
    assert r0[1].stride(0) == ref0[1].shape[1] + pad and r1[1].stride(0) == ref1[1].shape[1] + pad
    got, nm = ops.predict_bi(k, r0, r1, want_matched=True, **kw)
    assert got.dtype == torch.float32 and nm.dtype == torch.int64 and tuple(nm.shape) == (3,)
    assert tuple(nm.tolist()) == n, (what, up)
    assert torch.equal(_bits(got), _bits(P)), (what, up, "P")
    out = _dev(np.zeros_like(X), pad)
    res = ops.predict_bi(k, r0, r1, X=_dev(X, pad), out=out, **kw)
    assert res.data_ptr() == out.data_ptr()
    assert torch.equal(_bits(out), _bits(M.apply(X, P))), (what, up, "X - P")
    Xd = _dev(X, pad)
    _, nm = ops.predict_bi(k, r0, r1, X=Xd, add=True, out=Xd, want_matched=True, **kw)             # in place
    assert tuple(nm.tolist()) == n
    assert torch.equal(_bits(Xd), _bits(M.apply(X, P, add=True))), (what, up, "X + P")
    if pad:                                                              # nothing was written beside the rows
        assert bool((Xd._base[:, -pad:] == 7.0).all()) and bool((out._base[:, -pad:] == 7.0).all())
    for r, ref in ((r0, ref0), (r1, ref1)):                              # the references are read only
        assert torch.equal(_bits(r[1]), _bits(ref[1]))
    return P


@pytest.mark.parametrize("up", [0, 1, 2, 3])
def test_one_row_against_one_row(up):
    X, C0, C1 = _attrs(1, 5, 1), _attrs(1, 5, 2), _attrs(1, 5, 3)
    one, far = np.array([0o1234], np.uint64), np.array([0o7234], np.uint64)           # far: another cell at every up <= 3
    for k0, k1, combo in ((one, one, (True, True)), (one, far, (True, False)), (far, one, (False, True)), (far, far, (False, False))):
        _check(one, (k0, C0), (k1, C1), X, up, what=str(combo), combos=[combo])


@pytest.mark.parametrize("up", [0, 1, 2, 3])
@pytest.mark.parametrize("n,J,D,pad", [(257, 3, 4, 0), (3000, 6, 5, 0), (3000, 6, 59, 0), (3000, 6, 5, 3), (3000, 6, 59, 3)])
def test_scenes_against_a_thinned_and_another_reference(n, J, D, pad, up):
    from raht_3dgs_codec_amd import synth
    if J == 3:                                                           # exactly n of the 512 keys of depth 3, and n - 57 others
        rng = np.random.default_rng(10)
        keys, other = (np.sort(rng.choice(8 ** J, size=m, replace=False)).astype(np.uint64) for m in (n, n - 57))
        combos = None
    else:
        keys, other = synth.sorted_unique_keys(n, J, 11), synth.sorted_unique_keys(n, J, 12)
        combos = [(a, b) for a in (True, False) for b in (True, False) if up < 2 or (a or b)]     # (few cells at up >= 2: none empty in both)
    X, C = _attrs(len(keys), D, 5), _attrs(len(other), D, 6)
    thin = (keys[::3], X[::3] + np.float32(0.25))
    _check(keys, thin, (other, C), X, up, pad, "every third key, another scene", combos=combos)
    _check(keys, (other, C), thin, X, up, pad, "the references exchanged")
    if J == 6:                                                           # some run is longer than one row from up = 1 on
        lo, hi = M1.runs(keys, other, up)
        assert (int((hi - lo).max()) > 1) == (up > 0)


@pytest.mark.parametrize("n,D", [(n, D) for D in (3, 59) for n in (TILE - 1, TILE, TILE + 1, 3 * TILE + 1)] + [(2049 * TILE + 1, 1)])
def test_frames_that_end_inside_and_just_behind_a_block_of_rows(n, D):
    """N no multiple of the rows a workgroup resolves, one row more than a multiple (a last tile of one row: its D elements are no
    multiple of four), and more tiles than the capped grid has workgroups (the grid-stride loop's second round; D = 1: a 16-byte
    chunk covers four rows)."""
    J = 7 if n > 4 * TILE else 4
    rng = np.random.default_rng(n)
    keys, k0, k1 = (np.sort(rng.choice(8 ** J, size=m, replace=False)).astype(np.uint64) for m in (n, n - 3, n // 2))
    _check(keys, (k0, _attrs(len(k0), D, 8)), (k1, _attrs(len(k1), D, 9)), _attrs(n, D, 10), 1, what=f"n = {n}",
           combos=[(True, True), (True, False), (False, True)])


@pytest.mark.parametrize("D,pad", [(5, 0), (59, 0), (5, 3)])
@pytest.mark.parametrize("fields", ["mv0", "mv1", "both"])
def test_motion_fields(fields, D, pad):
    """random vectors of [-3, 3]^3 per block of 4^3 voxels: some push voxels out of the cube; a field on one reference leaves the
    other unshifted; all-zero fields are no fields"""
    from raht_3dgs_codec_amd import synth
    J, m = 6, 2
    keys, other = synth.sorted_unique_keys(3000, J, 11), synth.sorted_unique_keys(3000, J, 12)
    X, C = _attrs(len(keys), D, 5), _attrs(len(other), D, 6)
    thin = (keys[::3], X[::3] + np.float32(0.25))
    n_blocks = len(MM.blocks(keys, m)[1]) - 1
    rng = np.random.default_rng(3)
    mv0, mv1 = (rng.integers(-3, 4, (n_blocks, 3)).astype(np.int8) for _ in range(2))
    use0, use1 = (mv0 if fields != "mv1" else None), (mv1 if fields != "mv0" else None)
    out_of_cube = [not MM.shifted(keys, J, mv.astype(np.int64)[MM.blocks(keys, m)[0]])[0].all() for mv in (mv0, mv1)]
    assert all(out_of_cube)
    for up in (0, 1):
        _check(keys, thin, (other, C), X, up, pad, fields, J, m, use0, use1, combos=[(a, b) for a in (True, False) for b in (True, False)])
    zero = np.zeros_like(mv0)
    Pz = _check(keys, thin, (other, C), X, 1, pad, "zero fields", J, m, None if use0 is None else zero, None if use1 is None else zero)
    assert np.array_equal(Pz.view(np.int32), M.predict(keys, thin, (other, C), 1)[0].view(np.int32))


@pytest.mark.parametrize("up", [0, 2])
def test_one_sided_rows_and_identical_references_have_the_one_reference_kernels_bits(up):
    import torch
    from raht_3dgs_codec_amd import ops, synth
    J, m, D = 6, 2, 59
    keys, other = synth.sorted_unique_keys(3000, J, 11), synth.sorted_unique_keys(3000, J, 12)
    X, C = _attrs(len(keys), D, 5), _attrs(len(other), D, 6)
    k, Xd = _dev(keys), _dev(X)
    r0, r1 = (_dev(keys[::3]), _dev(X[::3] + np.float32(0.25))), (_dev(other), _dev(C))
    bf = _dev(MM.blocks(keys, m)[1])
    rng = np.random.default_rng(4)
    mv0, mv1 = (torch.from_numpy(rng.integers(-3, 4, (len(bf) - 1, 3)).astype(np.int8)).cuda() for _ in range(2))
    # identical references: predict's bits, in every mode
    for kw in (dict(), dict(X=Xd), dict(X=Xd, add=True)):
        assert torch.equal(_bits(ops.predict_bi(k, r1, r1, up=up, **kw)), _bits(ops.predict(k, *r1, up=up, **kw)))
    # a row with a run in one reference only: that reference's one-reference bits, without and with fields
    got, nm = ops.predict_bi(k, r0, r1, X=Xd, up=up, want_matched=True)
    one = [ops.predict(k, *r, X=Xd, up=up) for r in (r0, r1)]
    runs = [M1.runs(keys, rk, up) for rk in (keys[::3], other)]
    hit = [torch.from_numpy(hi > lo).cuda() for lo, hi in runs]
    assert tuple(nm.tolist()) == (int(hit[0].sum()), int(hit[1].sum()), int((hit[0] & hit[1]).sum()))
    for a, b in ((0, 1), (1, 0)):
        rows = hit[a] & ~hit[b]
        assert bool(rows.any()) and torch.equal(_bits(got[rows]), _bits(one[a][rows]))
    got = ops.predict_bi(k, r0, r1, X=Xd, up=up, J=J, block_log2=m, block_first=bf, mv0=mv0, mv1=mv1)
    one = [ops.predict_mc(k, *r, mv, bf, J, m, X=Xd, up=up) for r, mv in ((r0, mv0), (r1, mv1))]
    _, n, h0, h1 = M.predict(keys, (keys[::3], X[::3]), (other, C), up, J, m, mv0.cpu().numpy(), mv1.cpu().numpy())
    hit = [torch.from_numpy(h).cuda() for h in (h0, h1)]
    for a, b in ((0, 1), (1, 0)):
        rows = hit[a] & ~hit[b]
        assert bool(rows.any()) and torch.equal(_bits(got[rows]), _bits(one[a][rows]))
