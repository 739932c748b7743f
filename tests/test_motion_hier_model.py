"""The numpy model of the hierarchical motion search (tests/numpy_motion_hier.py) against the model of the exhaustive search
(tests/numpy_motion.py) and against its own definition: no device."""
import numpy as np
import pytest

from . import numpy_motion as MM
from . import numpy_motion_hier as MH
from . import numpy_predict as P0


def _scene(J=5, n=500, D=4, seed=3, t=(1, -1, 0)):
    rng = np.random.default_rng(seed)
    V = np.unique(rng.integers(0, 1 << J, size=(n, 3)), axis=0)
    keys = np.sort(MM.morton(V, J))
    X = rng.normal(size=(len(keys), D)).astype(np.float32)
    W = MM.demorton(keys, J) + np.asarray(t)
    ok = np.all((W >= 0) & (W < (1 << J)), axis=1) & (rng.random(len(W)) < 0.8)
    rk, at = np.unique(MM.morton(W[ok], J), return_index=True)
    C = (X[ok][at] + 0.05 * rng.standard_normal((len(rk), D))).astype(np.float32)
    w = np.array([1.0, 0.0, 2.5, 0.5], np.float32)[:D]
    return keys, X, rk, C, w


def test_pyramid_levels_are_cell_means_in_row_order():
    keys, X, _, _, _ = _scene()
    for l, (k_l, C_l) in enumerate(MH.pyramid(keys, X, 3), start=1):
        cell = keys >> np.uint64(3 * l)
        assert np.array_equal(k_l, np.unique(cell)) and C_l.dtype == np.float32 and C_l.shape == (len(k_l), X.shape[1])
        for j in (0, len(k_l) // 2, len(k_l) - 1):                      # by hand: the sequential float32 sum, one division
            rows = X[cell == k_l[j]]
            s = rows[0].copy()
            for r in rows[1:]:
                s = s + r
            assert np.array_equal((s / np.float32(len(rows))).view(np.int32), C_l[j].view(np.int32))
    assert MH.pyramid(keys, X, 0) == []


@pytest.mark.parametrize("up", [0, 1])
def test_a_zero_base_is_the_search(up):
    keys, X, rk, C, w = _scene()
    J, m, cand = 5, 2, MM.candidates(1)
    table, best_k, best_cost = MM.search(keys, rk, C, X, J, m, cand, w, up)
    t2, k2, c2, mv = MH.search_around(keys, rk, C, X, J, m, np.zeros((len(table), 3), np.int8), cand, w, up)
    assert np.array_equal(t2, table) and np.array_equal(k2, best_k) and np.array_equal(c2, best_cost)
    assert np.array_equal(mv, cand[best_k].astype(np.int8)) and len(np.unique(mv, axis=0)) > 1


def test_a_constant_base_is_the_search_with_shifted_candidates():
    keys, X, rk, C, w = _scene()
    J, m, cand, v = 5, 2, MM.candidates(1), np.array([2, -1, 1])
    table, best_k, best_cost = MM.search(keys, rk, C, X, J, m, cand + v, w)
    t2, k2, c2, mv = MH.search_around(keys, rk, C, X, J, m, np.repeat([v], len(table), axis=0), cand, w)
    assert np.array_equal(t2, table) and np.array_equal(k2, best_k) and np.array_equal(c2, best_cost)
    assert np.array_equal(mv, (cand + v)[best_k].astype(np.int8))


@pytest.mark.parametrize("up", [0, 1])
def test_no_levels_is_the_search(up):
    keys, X, rk, C, w = _scene()
    for r in (1, 2):
        _, best_k, best_cost = MM.search(keys, rk, C, X, 5, 2, MM.candidates(r), w, up)
        mv, cost, per_level = MH.search_hier(keys, rk, C, X, 5, 2, 0, r, w, up)
        assert np.array_equal(mv, MM.candidates(r)[best_k].astype(np.int8)) and np.array_equal(cost, best_cost) and len(per_level) == 1


def test_invalid_pairs_and_blocks_without_a_valid_pair():
    keys, X, rk, C, w = _scene(J=8, n=300)
    J, m, cand = 8, 3, MM.candidates(1)
    b, first = MM.blocks(keys, m)
    n_blocks = len(first) - 1
    assert n_blocks >= 8
    base = np.zeros((n_blocks, 3), np.int8)
    base[0], base[1], base[2], base[3], base[4], base[5] = (126, 0, 0), (127, 0, 0), (-127, -127, 127), (-128, 0, 0), (-128, 127, -128), (0, -126, 0)
    # every int8 base has a valid pair among all of [-1, 1]^3 (-128 + 1 is a vector), so a block with none needs fewer candidates:
    # the 18 of them with dx <= 0 leave the blocks 3 and 4 without one
    table, best_k, best_cost, mv = MH.search_around(keys, rk, C, X, J, m, base, cand, w)
    v = base.astype(np.int64)[:, None, :] + cand.astype(np.int64)[None]
    valid = np.all(np.abs(v) <= 127, axis=2)
    assert valid[0].all() and valid[5].all() and valid[6:].all()         # +-126 + 1 is a vector
    assert valid[1].sum() == 18 and valid[2].sum() == 8                  # 127 + 1 is none
    assert valid[3].sum() == 9 and valid[4].sum() == 2                   # -128 + 1 alone
    assert np.array_equal(table == MH.INVALID, ~valid) and (best_k >= 0).all()
    half = np.ascontiguousarray(cand[cand[:, 0] <= 0])
    assert len(half) == 18
    t2, k2, c2, mv2 = MH.search_around(keys, rk, C, X, J, m, base, half, w)
    assert (t2[3:5] == MH.INVALID).all() and (k2[3:5] == -1).all() and (c2[3:5] == -1).all() and not mv2[3:5].any()
    assert (k2[:3] >= 0).all() and (k2[5:] >= 0).all() and np.array_equal(t2[0], table[0][cand[:, 0] <= 0])
    ok = valid.any(axis=1)
    assert (best_k[ok] >= 0).all() and valid[np.flatnonzero(ok), best_k[ok]].all()
    for blk in np.flatnonzero(ok):                                       # the smallest k among the valid pairs of smallest cost
        costs = np.where(valid[blk], table[blk], np.iinfo(np.int64).max)
        assert best_k[blk] == int(np.flatnonzero(costs == costs.min())[0]) and best_cost[blk] == costs.min()
        assert np.array_equal(mv[blk], v[blk, best_k[blk]])
    # a valid pair's cost is the exhaustive search's under that vector
    ref_table, _, _ = MM.search(keys, rk, C, X, J, m, np.array([[127, 0, 0], [-127, 1, 0]]), w)
    assert table[1, list(map(tuple, cand)).index((0, 0, 0))] == ref_table[1, 0]
    assert table[3, list(map(tuple, cand)).index((1, 1, 0))] == ref_table[3, 1]


def test_reach():
    assert [MH.reach(L, r) for L, r in ((0, 3), (1, 1), (2, 1), (2, 3), (3, 3))] == [3, 3, 7, 15, 31]
    # the bound is attained: voxels that are alone in their blocks, at x = 0 mod 16, moved along x. Every level's cell then holds
    # one row, the vector of level l is d >> l with cost 0 -- as long as d >> L <= r: the reach is found, one voxel more is not.
    J, m, D = 7, 4, 3
    rng = np.random.default_rng(5)
    V = 16 * np.array([(i, j, k) for i in range(1, 6) for j in range(1, 7) for k in (2, 5)]) + np.concatenate(
        [np.zeros((60, 1), np.int64), rng.integers(0, 16, size=(60, 2))], axis=1)
    A = rng.normal(size=(len(V), D)).astype(np.float32)
    k = MM.morton(V, J)
    o = np.argsort(k)
    keys, X = k[o], A[o]
    assert len(MM.blocks(keys, m)[1]) - 1 == len(keys)
    for L, r in ((1, 1), (2, 1), (2, 3), (3, 3)):
        for d, found in ((MH.reach(L, r), True), (MH.reach(L, r) + 1, False)):
            rk = MM.morton(V + (d, 0, 0), J)
            p = np.argsort(rk)
            mv, cost, per_level = MH.search_hier(keys, rk[p], A[p], X, J, m, L, r, np.ones(D, np.float32))
            assert np.abs(mv.astype(np.int64)).max() <= MH.reach(L, r) and len(per_level) == L + 1
            hit = (mv == (d, 0, 0)).all(axis=1)
            assert (hit.all() and not cost.any()) if found else (not hit.any() and cost.all()), (L, r, d)


def test_hierarchy_follows_a_translation_by_a_multiple_of_the_coarsest_cell():
    J, m, L, D, t = 7, 3, 2, 3, np.array([8, -4, 12])
    rng = np.random.default_rng(6)
    V = np.unique(rng.integers(16, 100, size=(1500, 3)), axis=0)
    A = rng.normal(size=(len(V), D)).astype(np.float32)
    k, rk = MM.morton(V, J), MM.morton(V + t, J)
    o, p = np.argsort(k), np.argsort(rk)
    mv, cost, per_level = MH.search_hier(k[o], rk[p], A[p], A[o], J, m, L, 3, np.ones(D, np.float32))
    assert (mv == t).all() and not cost.any()
    for l, v in enumerate(per_level):
        assert (v.astype(np.int64) * 2 ** l == t).all()
    _, best_k, _ = MM.search(k[o], rk[p], A[p], A[o], J, m, MM.candidates(3), np.ones(D, np.float32))
    assert not (MM.candidates(3)[best_k] == t).all(axis=1).any()        # out of the flat search's reach
