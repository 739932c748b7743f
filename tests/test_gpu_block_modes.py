"""ops.mode_search / raht_mode_search and ops.predict_bi(..., modes) / raht_predict_bi_modes against the definition
(tests/numpy_block_modes.py), bit for bit: the whole cost table, the modes, the best cost, and the predictor's three uses -- P alone,
X - P, X + P in place -- under a mode array. Shapes: the smallest at which the kernels can go wrong -- rows of 1, 5, 59 and 244
floats (244: the search reads X through the cache instead of LDS), blocks of one row, blocks longer than a wave and than a tile,
one block for the frame, frames that end inside a tile, more tiles than the capped grid has workgroups, references of other sizes
and of one voxel, fields whose vectors leave the cube, weights that are zero, and values that are not finite."""
import numpy as np
import pytest

from . import numpy_block_modes as M
from . import numpy_motion as MM

pytestmark = pytest.mark.gpu

J, TILE, CAP = 6, 256, 1 << 30                                           # CAP: the fixed-point cost of a row at the cap 2^20
_SCENE = {}


def _attrs(n, D, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, D)).astype(np.float32)
    A[::7, 0] = -0.0
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


def _eq(got, want, nan_ok=False):
    """the same bits; nan_ok: a NaN for a NaN, whatever its sign and payload (inf - inf has no one bit pattern across machines)"""
    import torch
    g, w = _bits(got), _bits(want)
    if nan_ok:
        gn, wn = torch.isnan(g.view(torch.float32)), torch.isnan(w.view(torch.float32))
        return torch.equal(gn, wn) and torch.equal(g[~gn], w[~wn])
    return torch.equal(g, w)


def _scene(D):
    """the frame (keys, X), a thinned reference near X and another scene of another size: computed once, left unchanged"""
    from raht_3dgs_codec_amd import synth
    if D not in _SCENE:
        keys, other = synth.sorted_unique_keys(3000, J, 11), synth.sorted_unique_keys(2500, J, 12)
        assert len(keys) % TILE and len(keys) != len(other)
        X = _attrs(len(keys), D, 5)
        _SCENE[D] = (keys, X, (keys[::3], X[::3] + np.float32(0.25)), (other, _attrs(len(other), D, 6)))
    return _SCENE[D]


def _fields(keys, m, seed=3):
    """random vectors of [-3, 3]^3 per block: some push voxels out of the cube"""
    b, first = MM.blocks(keys, m)
    rng = np.random.default_rng(seed)
    mv0, mv1 = (rng.integers(-3, 4, (len(first) - 1, 3)).astype(np.int8) for _ in range(2))
    if m <= 2:                                                           # (many small blocks: some lie at the cube's faces)
        assert all(not MM.shifted(keys, J, mv.astype(np.int64)[b])[0].all() for mv in (mv0, mv1))
    return mv0, mv1


def _check(keys, ref0, ref1, X, m, w, up=0, pad=0, mv0=None, mv1=None, what="", modes=None, J=J, nan_ok=False):
    """the search and, under a mode array, the predictor's three uses of one case against the model; pad: extra columns in every
    matrix (row stride D + pad); nan_ok: the predictor's NaNs are compared as NaNs (the costs are integers either way) -> the model's
    (table, mode, best_cost)"""
    import torch
    from raht_3dgs_codec_amd import ops
    T, mode, best = M.search(keys, ref0, ref1, X, J, m, w, up, mv0, mv1)
    n_blocks = len(T)
    k, r0, r1 = _dev(keys), (_dev(ref0[0]), _dev(ref0[1], pad)), (_dev(ref1[0]), _dev(ref1[1], pad))
    bf = _dev(MM.blocks(keys, m)[1])
    kw = dict(up=up, mv0=None if mv0 is None else _dev(mv0), mv1=None if mv1 is None else _dev(mv1))
    Xd = _dev(X, pad)
    got_mode, got_best, got_T = ops.mode_search(k, r0, r1, Xd, J, m, bf, w, want_table=True, **kw)
    assert got_mode.dtype == torch.uint8 and got_best.dtype == torch.int64 and got_T.dtype == torch.int64
    assert tuple(got_T.shape) == (n_blocks, 4) and tuple(got_mode.shape) == (n_blocks,) == tuple(got_best.shape)
    assert np.array_equal(got_T.cpu().numpy(), T), (what, np.flatnonzero((got_T.cpu().numpy() != T).any(axis=1))[:8])
    assert np.array_equal(got_mode.cpu().numpy(), mode) and np.array_equal(got_best.cpu().numpy(), best), what
    again = ops.mode_search(k, r0, r1, Xd, J, m, bf, w, **kw)            # the table in the library's scratch
    assert len(again) == 2 and torch.equal(again[0], got_mode) and torch.equal(again[1], got_best)
    assert _eq(Xd, X)                                                    # the search reads only
    # the predictor under modes: the search's own, and every mode somewhere
    for md in ([mode] if modes is None else modes) + [np.random.default_rng(m).integers(0, 4, n_blocks).astype(np.uint8)]:
        P = M.predict(keys, ref0, ref1, md, J, m, up, mv0, mv1)
        n = M.used_runs(keys, ref0, ref1, md, J, m, up, mv0, mv1)
        pk = dict(kw, J=J, block_log2=m, block_first=bf, modes=_dev(md))
        got, nm = ops.predict_bi(k, r0, r1, want_matched=True, **pk)
        assert tuple(nm.tolist()) == n, what
        assert _eq(got, P, nan_ok), (what, "P")
        out = _dev(np.zeros_like(X), pad)
        res = ops.predict_bi(k, r0, r1, X=Xd, out=out, **pk)
        assert res.data_ptr() == out.data_ptr() and _eq(out, M.apply(X, P), nan_ok), (what, "X - P")
        Xi = _dev(X, pad)
        ops.predict_bi(k, r0, r1, X=Xi, add=True, out=Xi, **pk)          # in place
        assert _eq(Xi, M.apply(X, P, add=True), nan_ok), (what, "X + P")
        if pad:                                                          # nothing was written beside the rows
            assert bool((Xi._base[:, -pad:] == 7.0).all()) and bool((out._base[:, -pad:] == 7.0).all())
    for r, ref in ((r0, ref0), (r1, ref1)):                              # the references are read only
        assert _eq(r[1], ref[1])
    return T, mode, best


@pytest.mark.parametrize("fields", [False, True])
@pytest.mark.parametrize("up", [0, 2])
@pytest.mark.parametrize("m", [1, 2, 4, 6])
@pytest.mark.parametrize("D", [1, 5, 59, 244])
def test_the_search_and_the_predictor_against_the_model(D, m, up, fields):
    from raht_3dgs_codec_amd import _lib
    assert (_lib.lib().raht_debug_motion_tile(D) == 0) == (D == 244)     # 244: the first width that is not staged in LDS
    keys, X, thin, other = _scene(D)
    rows = np.diff(MM.blocks(keys, m)[1])
    assert {1: rows.min() == 1, 2: rows.max() > 8, 4: rows.max() > 64, 6: len(rows) == 1 and rows[0] > TILE}[m]
    w = np.random.default_rng(D).uniform(0.5, 100.0, D).astype(np.float32)
    mv0, mv1 = _fields(keys, m) if fields else (None, None)
    T, mode, _ = _check(keys, thin, other, X, m, w, up, 0, mv0, mv1, what=f"D={D} m={m} up={up} fields={fields}")
    assert m == 6 or len(set(mode.tolist())) >= 2                        # (the choice is not the same everywhere)


@pytest.mark.parametrize("D,pad", [(5, 3), (59, 3), (244, 4)])
def test_views_and_column_slices(D, pad):
    keys, X, thin, other = _scene(D)
    mv0, mv1 = _fields(keys, 2)
    w = np.full(D, 100.0, np.float32)
    _check(keys, thin, other, X, 2, w, 1, pad, what="padded rows")
    _check(keys, other, thin, X, 2, w, 0, pad, mv0, mv1, what="padded rows, fields, the references exchanged")


@pytest.mark.parametrize("n,D", [(TILE - 1, 5), (TILE + 1, 59), (3 * TILE + 1, 5), (2049 * TILE + 1, 1)])
def test_frames_that_end_inside_a_tile_and_more_tiles_than_workgroups(n, D):
    """N no multiple of the tile, one row behind a multiple, and more tiles than the capped grid has workgroups (the grid-stride
    loop's second round): the block sums do not depend on where the tiles cut the blocks"""
    Jn = 7 if n > 4 * TILE else 4
    rng = np.random.default_rng(n)
    keys, k0, k1 = (np.sort(rng.choice(8 ** Jn, size=s, replace=False)).astype(np.uint64) for s in (n, n - 3, n // 2))
    w = np.full(D, 10.0, np.float32)
    _check(keys, (k0, _attrs(len(k0), D, 8)), (k1, _attrs(len(k1), D, 9)), _attrs(n, D, 10), 2, w, 1, what=f"n = {n}", J=Jn)


def test_a_reference_of_one_voxel():
    keys, X, thin, other = _scene(5)
    one = (keys[1000:1001], X[1000:1001].copy())
    w = np.full(5, 100.0, np.float32)
    for up in (0, 2):
        T, mode, _ = _check(keys, one, other, X, 2, w, up, what="reference 0 has one voxel")
        _check(keys, thin, one, X, 2, w, up, what="reference 1 has one voxel")
    assert (T[:, 0] != T[:, 2]).any()                                    # (the voxel is somebody's match)


def test_weights_that_are_zero():
    keys, X, thin, other = _scene(59)
    w = np.random.default_rng(1).uniform(0.5, 100.0, 59).astype(np.float32)
    w[[0, 7, 8, 58]] = 0.0
    Xn = X.copy()
    Xn[:, 7] = np.nan                                                    # a column of weight 0 is left out: its values are never seen
    T, _, _ = _check(keys, thin, other, Xn, 2, w, 0, what="some weights 0")
    assert T.max() < CAP
    T, mode, best = _check(keys, thin, other, X, 2, np.zeros(59, np.float32), 0, what="all weights 0",
                           modes=[np.full(len(T), k, np.uint8) for k in range(4)])
    assert not T.any() and not mode.any() and not best.any()


@pytest.mark.parametrize("D", [5, 244])
def test_values_that_are_not_finite_take_the_capped_cost(D):
    keys, X, thin, other = _scene(D)
    other = (keys[::2], _attrs(len(keys[::2]), D, 7))                     # (every row of either reference is some row's match)
    X, C0, C1 = X.copy(), thin[1].copy(), other[1].copy()
    X[5, 1 % D], X[9, 0], X[11, 2 % D] = np.nan, np.inf, -np.inf
    C0[3, 0], C0[40, 1 % D] = np.nan, np.inf
    C1[4, 1 % D], C1[8, 1 % D], C1[60, 0] = np.inf, -np.inf, np.nan
    w = np.full(D, 100.0, np.float32)
    with np.errstate(all="ignore"):
        for up in (0, 2):
            T, _, _ = _check(keys, (thin[0], C0), (other[0], C1), X, 6, w, up, what="NaN and inf", nan_ok=True)
            q = [MM.row_cost(X, P, w) for P in M.predictions(keys, (thin[0], C0), (other[0], C1), up)]
            assert all(int(c[r]) == CAP for c in q for r in (5, 9, 11))  # a row of X that is not finite: the cap under every mode
            assert (q[1] == CAP).sum() > 3 and (q[2] == CAP).sum() > 3   # ... and rows whose reference is not finite
            assert int(T[0, 3]) == sum(int(c) for c in q[3])


def test_uniform_modes_are_the_plain_predictors():
    import torch
    from raht_3dgs_codec_amd import ops
    keys, X, thin, other = _scene(59)
    m = 2
    k, Xd, r0, r1 = _dev(keys), _dev(X), tuple(_dev(a) for a in thin), tuple(_dev(a) for a in other)
    bf = _dev(MM.blocks(keys, m)[1])
    n_blocks = len(bf) - 1
    mv0, mv1 = (_dev(f) for f in _fields(keys, m))
    full = [torch.full((n_blocks,), v, dtype=torch.uint8, device="cuda") for v in range(4)]
    fr = dict(J=J, block_log2=m, block_first=bf)
    for up in (0, 2):
        for use in (dict(), dict(X=Xd), dict(X=Xd.clone(), add=True)):
            for fields in (dict(), dict(mv0=mv0, mv1=mv1)):
                got = [ops.predict_bi(k, r0, r1, up=up, modes=md, **fr, **fields, **use) for md in full]
                assert torch.equal(_bits(got[0]), _bits(ops.predict_bi(k, r0, r1, up=up, **(dict(fr, **fields) if fields else {}), **use)))
                if fields:
                    one = [ops.predict_mc(k, *r, mv, bf, J, m, up=up, **use) for r, mv in ((r0, mv0), (r1, mv1))]
                else:
                    one = [ops.predict(k, *r, up=up, **use) for r in (r0, r1)]
                assert torch.equal(_bits(got[1]), _bits(one[0])) and torch.equal(_bits(got[2]), _bits(one[1]))
                want = torch.zeros_like(Xd) if not use else (Xd + 0.0 if use.get("add") else Xd)
                assert torch.equal(_bits(got[3]), _bits(want))
    assert torch.equal(ops.predict_bi(k, r0, r1, X=Xd, modes=full[3], **fr), Xd)      # all modes 3: X comes back unchanged
    five = torch.full((n_blocks,), 5, dtype=torch.uint8, device="cuda")                # a value above 3 predicts as 3
    assert torch.equal(_bits(ops.predict_bi(k, r0, r1, X=Xd, modes=five, **fr)), _bits(Xd))


def test_identical_references_choose_mode_0():
    import torch
    from raht_3dgs_codec_amd import ops
    keys, X, thin, other = _scene(5)
    k, bf = _dev(keys), _dev(MM.blocks(keys, 2)[1])
    # another scene twice: the mean of a prediction with itself is that prediction, so the first three columns are equal and no
    # block prefers one reference -- where the scene predicts worse than nothing, mode 3 wins
    r = tuple(_dev(a) for a in other)
    mode, best, T = ops.mode_search(k, r, r, _dev(X), J, 2, bf, np.ones(5, np.float32), up=1, want_table=True)
    assert bool((T[:, 0] == T[:, 1]).all()) and bool((T[:, 0] == T[:, 2]).all())
    assert set(mode.tolist()) == {0, 3} and bool((best == torch.minimum(T[:, 0], T[:, 3])).all())
    # the frame itself a hundredth off, twice: mode 0 everywhere
    r = (k, _dev(X + np.float32(0.01)))
    mode, best, T = ops.mode_search(k, r, r, _dev(X), J, 2, bf, np.ones(5, np.float32), want_table=True)
    assert not bool(mode.any()) and bool((T[:, 0] == T[:, 1]).all()) and bool((T[:, 0] == T[:, 2]).all()) and bool((best == T[:, 0]).all())


def test_host_refusals():
    import torch
    from raht_3dgs_codec_amd import ops
    keys, X, thin, other = _scene(5)
    k, Xd, r0, r1 = _dev(keys), _dev(X), tuple(_dev(a) for a in thin), tuple(_dev(a) for a in other)
    bf = _dev(MM.blocks(keys, 2)[1])
    n_blocks = len(bf) - 1
    w = np.ones(5, np.float32)
    mv = torch.zeros((n_blocks, 3), dtype=torch.int8, device="cuda")
    md = torch.zeros(n_blocks, dtype=torch.uint8, device="cuda")
    search = {"weights of another length": dict(weights=np.ones(6, np.float32)), "a negative weight": dict(weights=-w),
              "a weight that is not finite": dict(weights=w * np.inf), "block_log2 = 0": dict(block_log2=0),
              "block_log2 = J + 1": dict(block_log2=J + 1), "J = 22": dict(J=22), "block_first too long": dict(block_first=torch.arange(len(k) + 2).cuda()),
              "block_first of another dtype": dict(block_first=bf.int()), "X of another dtype": dict(X=Xd.double()),
              "X of another length": dict(X=Xd[:-1]), "keys of another dtype": dict(keys=k.int()), "up = 4": dict(up=4),
              "a field of another shape": dict(mv0=mv[:-1]), "a field of another dtype": dict(mv1=mv.int()),
              "references of another D": dict(ref1=(r1[0], r1[1][:, :4])), "a reference that is no pair": dict(ref0=r0[0])}
    for what, kw in search.items():
        a = dict(keys=k, ref0=r0, ref1=r1, X=Xd, J=J, block_log2=2, block_first=bf, weights=w)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.mode_search(**a)
            pytest.fail(what)
    for what, kw in {"X on the host": dict(X=Xd.cpu()), "block_first on the host": dict(block_first=bf.cpu()), "a field on the host": dict(mv0=mv.cpu())}.items():
        a = dict(keys=k, ref0=r0, ref1=r1, X=Xd, J=J, block_log2=2, block_first=bf, weights=w)
        a.update(kw)
        with pytest.raises(RuntimeError, match="no CPU path"):
            ops.mode_search(**a)
            pytest.fail(what)
    fr = dict(J=J, block_log2=2, block_first=bf)
    for what, kw in {"modes of another length": dict(modes=md[:-1]), "modes of another dtype": dict(modes=md.to(torch.int8)),
                     "modes without the blocks": dict(modes=md, block_first=None), "block_log2 = J + 1": dict(modes=md, block_log2=J + 1),
                     "block_log2 = 0": dict(modes=md, block_log2=0)}.items():
        with pytest.raises(ValueError):
            ops.predict_bi(k, r0, r1, X=Xd, **dict(fr, **kw))
            pytest.fail(what)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.predict_bi(k, r0, r1, X=Xd, modes=md.cpu(), **fr)
