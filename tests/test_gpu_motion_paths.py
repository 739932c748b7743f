"""The forms of raht_motion_search / raht_predict_mc that tests/test_gpu_motion.py never reaches, against the same definition
(tests/numpy_motion.py) with the same comparisons: the table, the chosen candidate and its cost as integers, the compensated
prediction bit for bit in all three modes. Every test asserts that its input reaches the form it names: the tile from
raht_debug_motion_tile, the largest block against that tile, hits and misses mixed, more than one chosen vector.
  - the tiles of 192, 128 and 64 rows and the unstaged kernel (D = 60 .. 300), with blocks that span tiles and frames that end
    one row before, on and one row behind a tile of THAT size
  - the second round of a workgroup (more than 2048 tiles), at 256 and at 64 rows per tile
  - up = 2, 3 (runs of up to 64 / 512 reference rows per row and candidate), all weights zero, K = 1, K = 512 with duplicates
  - depth 21: 63-bit keys at both corners of the cube, vectors of +-127"""
import numpy as np
import pytest

from . import numpy_motion as MM
from . import numpy_predict as M
from .test_gpu_motion import _attrs, _check_predict, _check_search, _moved_reference, _n_blocks, _weights

pytestmark = pytest.mark.gpu

MAX_GRID = 2048                                                          # csrc/motion.hip: MS_MAX_GRID
WIDE = [60, 79, 80, 121, 122, 243, 244, 300]                             # both sides of every switch but 59 | 60's lower one, and beyond
TILE_OF = {60: 192, 79: 192, 80: 128, 121: 128, 122: 64, 243: 64, 244: 0, 300: 0}
PADDED = [79, 121, 243, 300]                                             # one D per form, with padded rows as well
_CACHE = {}


def _tile(D, want):
    """rows per workgroup step at D, asserted to be the form the test means: want = rows of the staged tile, 0 = unstaged"""
    from raht_3dgs_codec_amd import _lib
    t = _lib.lib().raht_debug_motion_tile(D)
    assert t == want, (D, t, want)
    return t if t else 256


def _matched_share(keys, ref, J, m, mv, up):
    ok, k2 = MM.shifted(keys, J, np.asarray(mv, np.int64)[MM.blocks(keys, m)[0]])
    lo, hi = M.runs(k2, ref, up)
    return float((ok & (hi > lo)).mean())


def _scene(D):
    """(keys, X, ref keys, C_ref) of the scene cases: computed once per D and left unchanged"""
    from raht_3dgs_codec_amd import synth
    if D not in _CACHE:
        keys = synth.sorted_unique_keys(900, 6, 21)
        X = _attrs(len(keys), D, 5)
        _CACHE[D] = (keys, X) + _moved_reference(keys, X, 6, 22)
    return _CACHE[D]


@pytest.mark.parametrize("up", [0, 1])
@pytest.mark.parametrize("D,pad", [(D, 0) for D in WIDE] + [(D, 3) for D in PADDED])
def test_scenes_at_every_tile_size(D, pad, up):
    J, m = 6, 2
    _tile(D, TILE_OF[D])
    keys, X, ref, C = _scene(D)
    assert 700 < len(keys) <= 900
    w = _weights(D)
    assert not w[1::3].any() and w[0::3].all() and w[2::3].all()         # every third column has weight 0
    mv, _ = _check_search(keys, ref, C, X, J, m, MM.candidates(1), w, up, pad, f"D = {D}")
    assert len(np.unique(mv, axis=0)) > 1
    if up == 0:
        assert (mv == (-1, 1, 0)).all(axis=1).mean() > 0.5               # found where it is
    assert 0.0 < _matched_share(keys, ref, J, m, mv, up) < 1.0
    _check_predict(keys, ref, C, X, J, m, mv, up, pad, f"D = {D}: the field that was found")


@pytest.mark.parametrize("J,m,dense", [(6, 6, False), (6, 4, True)])
@pytest.mark.parametrize("D", WIDE)
def test_blocks_that_span_tiles_of_every_size(D, J, m, dense):
    """one block for the whole frame, and a corner so dense that one block of 16^3 cells holds more rows than two tiles"""
    from raht_3dgs_codec_amd import synth
    T = _tile(D, TILE_OF[D])
    keys = synth.sorted_unique_keys(1500, J, 13)
    if dense:
        rng = np.random.default_rng(14)
        keys = np.unique(np.concatenate([keys, MM.morton(rng.integers(0, 12, size=(1500, 3)), J)]))
    _, first = MM.blocks(keys, m)
    assert int(np.diff(first).max()) > 2 * T
    X = _attrs(len(keys), D, 5)
    ref, C = _moved_reference(keys, X, J, 15, t=(0, 1, -1))
    mv, _ = _check_search(keys, ref, C, X, J, m, MM.candidates(1), _weights(D), 0, what=f"D = {D}: large blocks")
    assert 0.0 < _matched_share(keys, ref, J, m, mv, 0) < 1.0
    _check_predict(keys, ref, C, X, J, m, mv, 0, what=f"D = {D}: large blocks")


@pytest.mark.parametrize("off", [-1, 0, 1])
@pytest.mark.parametrize("D", WIDE)
def test_frames_that_end_inside_on_and_just_behind_a_tile_of_every_size(D, off):
    J, m = 4, 2
    n = _tile(D, TILE_OF[D]) + off
    rng = np.random.default_rng(n)
    keys = np.sort(rng.choice(8 ** J, size=n, replace=False)).astype(np.uint64)
    X = _attrs(n, D, 8)
    ref, C = _moved_reference(keys, X, J, 16, t=(0, 0, 1))
    mv, _ = _check_search(keys, ref, C, X, J, m, MM.candidates(1), _weights(D), 1, what=f"D = {D}, n = {n}")
    assert len(np.unique(mv, axis=0)) > 1 and 0.0 < _matched_share(keys, ref, J, m, mv, 1) < 1.0
    _check_predict(keys, ref, C, X, J, m, mv, 1, what=f"D = {D}, n = {n}")


@pytest.mark.parametrize("D,T,J,m", [(3, 256, 8, 3), (122, 64, 7, 2)])
def test_more_tiles_than_the_capped_grid_has_workgroups(D, T, J, m):
    """2049 tiles and one row: workgroup 0 walks a second tile and a third of one row, through the barrier that guards the staged
    rows and both sets of block slots. At D = 122 all but five columns have weight 0: the tile is chosen from D alone."""
    assert _tile(D, T) == T
    n = (MAX_GRID + 1) * T + 1
    assert (n + T - 1) // T > MAX_GRID + 1 and 8 * n <= 8 ** J
    rng = np.random.default_rng(n)
    keys, ref = (np.sort(rng.choice(8 * n, size=n, replace=False)).astype(np.uint64) for _ in range(2))
    first = MM.blocks(keys, m)[1]
    ends = np.arange(T, n, T)                                            # a tile ends in front of these rows
    assert len(first) - 1 > 2000 and int((~np.isin(ends, first)).sum()) > 1000      # thousands of blocks, and of blocks cut by a tile's end
    X, C = _attrs(n, D, 8), _attrs(n, D, 9)
    w = np.zeros(D, np.float32)
    w[[0, D // 2, D - 1]] = (1.0, 0.5, 3.0)
    if D > 3:
        w[[7, 64]] = (2.0, 0.25)
    cand = np.array([[0, 0, 0], [0, 0, 1]], np.int32)
    mv, cost = _check_search(keys, ref, C, X, J, m, cand, w, 0, what=f"n = {n}")
    assert len(np.unique(mv, axis=0)) == 2 and cost.all()
    for v in cand:
        assert 0.0 < _matched_share(keys, ref, J, J, [v], 0) < 1.0


@pytest.mark.parametrize("up", [2, 3])
def test_runs_of_many_reference_rows_in_the_search(up):
    from raht_3dgs_codec_amd import synth
    J, m, D = 6, 2, 5
    keys = synth.sorted_unique_keys(3000, J, 11)
    X = _attrs(len(keys), D, 5)
    ref, C = _moved_reference(keys, X, J, 12)
    more = synth.sorted_unique_keys(12000, J, 11)                        # the frame's own blobs, four times the draws: crowded cells
    ref, at = np.unique(np.concatenate([ref, more]), return_index=True)
    C = np.ascontiguousarray(np.concatenate([C, _attrs(len(more), D, 13)])[at])
    lo, hi = M.runs(keys, ref, up)
    assert 8 ** (up - 1) < int((hi - lo).max()) <= 8 ** up               # runs that no smaller up can hold
    mv, _ = _check_search(keys, ref, C, X, J, m, MM.candidates(1), _weights(D), up, what=f"up = {up}")
    assert len(np.unique(mv, axis=0)) > 1
    _check_predict(keys, ref, C, X, J, m, mv, up, what=f"up = {up}")


@pytest.mark.parametrize("D,T", [(5, 256), (122, 64), (244, 0)])
def test_all_weights_zero(D, T):
    """nw == 0: the kernel returns before its loop; the table stays what the memset left, every block picks k = 0 at cost 0"""
    from raht_3dgs_codec_amd import synth
    J, m = 6, 2
    _tile(D, T)
    keys = synth.sorted_unique_keys(900, J, 21)
    X = _attrs(len(keys), D, 5)
    ref, C = _moved_reference(keys, X, J, 22)
    table, best_k, best_cost = MM.search(keys, ref, C, X, J, m, MM.candidates(1), np.zeros(D, np.float32))
    assert not table.any() and not best_k.any() and not best_cost.any()
    mv, cost = _check_search(keys, ref, C, X, J, m, MM.candidates(1), np.zeros(D, np.float32), 0, what="no weight")
    assert not mv.any() and not cost.any()
    rev = np.ascontiguousarray(MM.candidates(1)[::-1])                   # k = 0 is then (1, 1, 1)
    mv, cost = _check_search(keys, ref, C, X, J, m, rev, np.zeros(D, np.float32), 1, what="no weight, reversed")
    assert (mv == 1).all() and not cost.any()


def test_one_candidate():
    from raht_3dgs_codec_amd import synth
    J, m, D = 6, 2, 5
    keys = synth.sorted_unique_keys(900, J, 21)
    X = _attrs(len(keys), D, 5)
    ref, C = _moved_reference(keys, X, J, 22)
    for v in ([-1, 1, 0], [3, 0, -2]):
        cand = np.array([v], np.int32)
        mv, cost = _check_search(keys, ref, C, X, J, m, cand, _weights(D), 0, what=f"K = 1: {v}")
        assert (mv == v).all() and cost.any()
        _check_predict(keys, ref, C, X, J, m, mv, 0, what=f"K = 1: {v}")
    assert 0.0 < _matched_share(keys, ref, J, m, np.repeat([[-1, 1, 0]], _n_blocks(keys, m), axis=0), 0) < 1.0


def test_512_candidates_with_duplicates():
    """random vectors within +-127, (0, 0, 0) at k = 256, the vectors of k = 20 .. 29 once more at k = 300 .. 309. The reference
    holds every block's rows moved by one of the vectors 20 .. 29 with the frame's own attributes: cost 0 at that k AND at its
    duplicate, and the smaller index must win."""
    J, m, D = 9, 2, 3
    rng = np.random.default_rng(23)
    cand = rng.integers(-127, 128, size=(512, 3)).astype(np.int32)
    cand[256] = 0
    cand[300:310] = cand[20:30]
    assert np.abs(cand).max() == 127
    V = np.unique(rng.integers(248, 264, size=(300, 3)), axis=0)         # the middle of the cube: no vector leaves it
    keys = MM.morton(V, J)
    o = np.argsort(keys)
    keys, V = keys[o], V[o]
    X = _attrs(len(keys), D, 24)
    b, first = MM.blocks(keys, m)
    j = 20 + b % 10
    W = V + cand[j]
    assert W.min() >= 0 and W.max() < (1 << J)
    rk, at = np.unique(MM.morton(W, J), return_index=True)
    C = np.ascontiguousarray(X[at])
    assert 250 < len(keys) <= 300 and len(first) - 1 > 20
    table, best_k, best_cost = MM.search(keys, rk, C, X, J, m, cand, np.ones(D, np.float32))
    tied = table[np.arange(len(table)), best_k] == table[np.arange(len(table)), best_k + 280]
    assert ((best_k >= 20) & (best_k < 30)).all() and tied.all() and not best_cost.any()     # the model: every block has its tie
    assert len(np.unique(best_k)) > 1 and (table[:, 256] > 0).all()
    mv, cost = _check_search(keys, rk, C, X, J, m, cand, np.ones(D, np.float32), 0, what="K = 512")
    assert np.array_equal(mv, cand[best_k].astype(np.int8)) and not cost.any()
    _check_predict(keys, rk, C, X, J, m, mv, 0, what="K = 512")


def _corners():
    """a frame and a reference of depth 21 in the 24-wide corners of the cube, at 0 and at 2^21 - 24: about 700 rows at either
    end. The reference holds part of the frame moved by (0, -1, 1), part of it moved by the long vectors that stay inside the
    cube -- (127, 126, 5) from the low corner, (-127, -126, -5) from the high one -- and voxels of its own."""
    if "corners" not in _CACHE:
        J, D = 21, 5
        rng = np.random.default_rng(25)
        top = (1 << J) - 24
        V = np.concatenate([np.unique(rng.integers(0, 24, size=(720, 3)), axis=0), top + np.unique(rng.integers(0, 24, size=(720, 3)), axis=0)])
        keys = MM.morton(V, J)
        o = np.argsort(keys)
        keys, V = keys[o], V[o]
        X = _attrs(len(keys), D, 26)
        low = V[:, 0] < 24
        near = V + np.where(low[:, None], (0, -1, 1), (1, 0, -1))
        ok = np.all((near >= 0) & (near < (1 << J)), axis=1) & (rng.random(len(V)) < 0.6)
        far = V + np.where(low[:, None], (127, 126, 5), (-127, -126, -5))
        pick = rng.random(len(V)) < 0.3
        own = np.concatenate([rng.integers(0, 24, size=(150, 3)), top + rng.integers(0, 24, size=(150, 3))])
        W = np.concatenate([near[ok], far[pick], own])
        C = np.concatenate([X[ok], X[pick], _attrs(len(own), D, 27)])
        C = (C + 0.05 * rng.standard_normal(C.shape)).astype(np.float32)
        # one slab of cells of up = 3 stays empty in either corner (x < 8; z in the high corner's first 8): rows without a match
        # at every up, while the voxels beside 2^21 - 1 stay
        keep = (W[:, 0] >= 8) & ~((W[:, 2] >= top) & (W[:, 2] < top + 8))
        rk, at = np.unique(MM.morton(W[keep], J), return_index=True)
        C = C[keep]
        _CACHE["corners"] = (keys, X, rk, np.ascontiguousarray(C[at]))
    return _CACHE["corners"]


LONG = np.array([[0, 0, 0], [127, 126, 5], [127, -127, 5], [-127, -126, -5], [-127, 127, -5], [0, -1, 1], [127, 127, 127], [-127, -127, -127]],
                np.int32)


@pytest.mark.parametrize("cand", ["radius 1", "long"])
@pytest.mark.parametrize("up", [0, 3])
@pytest.mark.parametrize("m", [3, 21])
def test_depth_21(m, up, cand):
    J, D = 21, 5
    keys, X, ref, C = _corners()
    assert int(keys.max()) >> 62 == 1 and int(ref.max()) >> 62 == 1 and int(keys.min()) < 8 ** 5      # bit 62 is set; both corners
    assert 1300 < len(keys) <= 1440 and len(ref) > 1000
    cands = MM.candidates(1) if cand == "radius 1" else LONG
    mv, _ = _check_search(keys, ref, C, X, J, m, cands, _weights(D), up, what=f"J = 21, m = {m}, {cand}")
    # the model finds rows with a match and rows without: under vectors the search walks (one block may well choose a vector
    # that leaves the cube: at up = 3 a mean of many unrelated rows predicts worse than 0) ...
    assert sum(0.0 < _matched_share(keys, ref, J, J, [v], up) < 1.0 for v in cands) >= 3
    if m == 3:                                                           # ... and under the field that was found
        assert 0.0 < _matched_share(keys, ref, J, m, mv, up) < 1.0
        assert len(np.unique(mv, axis=0)) > 1
        if cand == "long" and up == 0:                                   # both long vectors that stay inside are chosen somewhere
            assert (mv == LONG[1]).all(axis=1).any() and (mv == LONG[3]).all(axis=1).any()
    _check_predict(keys, ref, C, X, J, m, mv, up, what=f"J = 21, m = {m}, {cand}")
    if cand == "long":                                                   # the predictor under every long vector, whatever was chosen
        for v in LONG[1:5]:
            _check_predict(keys, ref, C, X, J, m, np.repeat([v], _n_blocks(keys, m), axis=0), up, what=f"J = 21 under {v}")
