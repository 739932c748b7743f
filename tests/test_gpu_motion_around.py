"""ops.motion_search_around / raht_motion_search_around, ops.motion_pyramid and ops.motion_search_hier against the definition
(tests/numpy_motion_hier.py): the whole cost table, best_k, best_cost and mv as integers, bit for bit. Shapes: the smallest at which
the AROUND instantiations of the search kernel and the new select kernel can go wrong -- every tile size and the unstaged path,
frames that end one row before, on and one row behind a tile, a block that spans more than two tiles, blocks cut inside a wave, the
capped grid, bases that leave the cube, bases at the edge of int8 (invalid pairs, a block with no valid pair), K = 1 and K = 512,
no weight at all, depth 21 -- and the two identities that tie the new entry point to raht_motion_search."""
import numpy as np
import pytest

from . import numpy_motion as MM
from . import numpy_motion_hier as MH
from .test_gpu_motion import _attrs, _dev, _moved_reference, _n_blocks, _weights

pytestmark = pytest.mark.gpu

MAX_GRID = 2048                                                          # csrc/motion.hip: MS_MAX_GRID
TILE_OF = {1: 256, 5: 256, 59: 256, 79: 192, 121: 128, 243: 64, 244: 0}  # rows of the staged tile, 0: unstaged (256 rows a step)
WIDE = [59, 79, 121, 243, 244]
_CACHE = {}


def _tile(D):
    from raht_3dgs_codec_amd import _lib
    t = _lib.lib().raht_debug_motion_tile(D)
    assert t == TILE_OF[D], (D, t)
    return t if t else 256


def _check(keys, ref, C_ref, X, J, m, base, cand, w, up=0, pad=0, what=""):
    """one case against the model -> (table, best_k, best_cost, mv) of the model"""
    import torch
    from raht_3dgs_codec_amd import ops
    base = np.ascontiguousarray(base, np.int8)
    table, best_k, best_cost, mv = MH.search_around(keys, ref, C_ref, X, J, m, base, cand, w, up)
    k = _dev(keys)
    bf = ops.motion_blocks(k, J, m, _n_blocks(keys, m))
    Xd, bd = _dev(X, pad), torch.from_numpy(base).cuda()
    g_mv, g_cost, g_k, g_tab = ops.motion_search_around(k, _dev(ref), _dev(C_ref, pad), Xd, J, m, bf, bd, cand, w, up=up, want_table=True)
    assert g_mv.dtype == torch.int8 and g_cost.dtype == torch.int64 and g_k.dtype == torch.int32 and g_tab.dtype == torch.int64
    assert torch.equal(g_tab.cpu(), torch.from_numpy(table)), (what, "table")
    assert torch.equal(g_k.cpu(), torch.from_numpy(best_k)), (what, "best_k")
    assert torch.equal(g_cost.cpu(), torch.from_numpy(best_cost)), (what, "best_cost")
    assert torch.equal(g_mv.cpu(), torch.from_numpy(mv)), (what, "mv")
    mv2, cost2, k2 = ops.motion_search_around(k, _dev(ref), _dev(C_ref, pad), Xd, J, m, bf, bd, cand, w, up=up)      # the pool's table
    assert torch.equal(mv2, g_mv) and torch.equal(cost2, g_cost) and torch.equal(k2, g_k), (what, "without a table")
    assert np.array_equal(Xd.cpu().numpy().view(np.int32), np.ascontiguousarray(X).view(np.int32))       # X and base are read only
    assert np.array_equal(bd.cpu().numpy(), base)
    return table, best_k, best_cost, mv


def _scene(D):
    """(keys, X, ref keys, C_ref) of ~800 rows at J = 6: computed once per D and left unchanged"""
    from raht_3dgs_codec_amd import synth
    if D not in _CACHE:
        keys = synth.sorted_unique_keys(800, 6, 21)
        X = _attrs(len(keys), D, 5)
        _CACHE[D] = (keys, X) + _moved_reference(keys, X, 6, 22, t=(3, -2, 1))
    return _CACHE[D]


def _random_base(n_blocks, seed, r=3):
    return np.random.default_rng(seed).integers(-r, r + 1, size=(n_blocks, 3)).astype(np.int8)


@pytest.mark.parametrize("up", [0, 1])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("D", WIDE)
def test_scenes_at_every_tile_size_around_a_random_base(D, pad, up):
    J, m = 6, 2
    _tile(D)
    keys, X, ref, C = _scene(D)
    assert 600 < len(keys) <= 800
    w = _weights(D)
    assert not w[1::3].any() and w[0::3].all() and w[2::3].all()         # every third column has weight 0
    first = MM.blocks(keys, m)[1]
    assert (first[1:-1] % 64 != 0).sum() > 50                            # blocks cut inside a wave
    base = _random_base(len(first) - 1, 30)
    assert np.abs(base).max() == 3 and len(np.unique(base, axis=0)) > 100
    _, best_k, _, mv = _check(keys, ref, C, X, J, m, base, MM.candidates(1), w, up, pad, f"D = {D}")
    assert len(np.unique(best_k)) > 5 and (best_k >= 0).all()
    if up == 0:                                                          # the moved rows are found where the base lets them be
        near = np.abs(base.astype(np.int64) - (-3, 2, -1)).max(axis=1) <= 1
        assert near.sum() > 5 and (mv[near] == (-3, 2, -1)).all(axis=1).mean() > 0.5


@pytest.mark.parametrize("off", [-1, 0, 1])
@pytest.mark.parametrize("D", WIDE)
def test_frames_that_end_inside_on_and_just_behind_a_tile(D, off):
    J, m = 4, 2
    n = _tile(D) + off
    rng = np.random.default_rng(n)
    keys = np.sort(rng.choice(8 ** J, size=n, replace=False)).astype(np.uint64)
    X = _attrs(n, D, 8)
    ref, C = _moved_reference(keys, X, J, 16, t=(0, 0, 1))
    _, best_k, _, _ = _check(keys, ref, C, X, J, m, _random_base(_n_blocks(keys, m), 31, 2), MM.candidates(1), _weights(D), 1,
                             what=f"D = {D}, n = {n}")
    assert len(np.unique(best_k)) > 1


@pytest.mark.parametrize("J,m", [(6, 6), (6, 4)])
@pytest.mark.parametrize("D", WIDE)
def test_a_block_that_spans_more_than_two_tiles(D, J, m):
    """one block for the whole frame, and a corner so dense that one block of 16^3 cells holds more rows than two tiles"""
    from raht_3dgs_codec_amd import synth
    T = _tile(D)
    keys = synth.sorted_unique_keys(1500, J, 13)
    if m < J:
        keys = np.unique(np.concatenate([keys, MM.morton(np.random.default_rng(14).integers(0, 12, size=(1500, 3)), J)]))
    first = MM.blocks(keys, m)[1]
    assert int(np.diff(first).max()) > 2 * T
    X = _attrs(len(keys), D, 5)
    ref, C = _moved_reference(keys, X, J, 15, t=(0, 2, -2))
    base = np.repeat(np.array([[0, -1, 1]], np.int8), len(first) - 1, axis=0)
    _, _, _, mv = _check(keys, ref, C, X, J, m, base, MM.candidates(1), _weights(D), 0, what=f"D = {D}: large blocks")
    assert (mv[np.diff(first).argmax()] == (0, -2, 2)).all()


def test_more_tiles_than_the_capped_grid_has_workgroups():
    """2049 tiles and one row at D = 1: workgroup 0 walks a second tile and a third of one row, and reads its blocks' bases again"""
    D, J, m = 1, 8, 3
    T = _tile(D)
    n = (MAX_GRID + 1) * T + 1
    assert (n + T - 1) // T > MAX_GRID + 1 and 8 * n <= 8 ** J
    rng = np.random.default_rng(n)
    keys, ref = (np.sort(rng.choice(8 * n, size=n, replace=False)).astype(np.uint64) for _ in range(2))
    first = MM.blocks(keys, m)[1]
    assert len(first) - 1 > 2000 and int((~np.isin(np.arange(T, n, T), first)).sum()) > 1000      # blocks cut by a tile's end
    X, C = _attrs(n, D, 8), _attrs(n, D, 9)
    cand = np.array([[0, 0, 0], [0, 0, 1]], np.int32)
    _, best_k, best_cost, _ = _check(keys, ref, C, X, J, m, _random_base(len(first) - 1, 32, 1), cand, np.ones(1, np.float32), 0, what=f"n = {n}")
    assert len(np.unique(best_k)) == 2 and best_cost.all()


def test_a_base_that_throws_whole_blocks_out_of_the_cube():
    J, m, D = 6, 2, 5
    keys, X, ref, C = _scene(D)
    b, first = MM.blocks(keys, m)
    base = _random_base(len(first) - 1, 33)
    base[::3] = (100, 0, 0)                                              # 2^J = 64: every row of these blocks leaves the cube ...
    base[1::3, 1] = -66                                                  # ... and of these, under every candidate
    w = _weights(D)
    table, best_k, best_cost, mv = _check(keys, ref, C, X, J, m, base, MM.candidates(1), w, 0, what="out of the cube")
    alone = np.zeros((len(keys), D), np.float32)                         # the cost of a block without a match: its rows against 0
    q = np.zeros(len(first) - 1, np.int64)
    np.add.at(q, b, MM.row_cost(X, alone, w).astype(np.int64))
    assert (table[::3] == q[::3, None]).all() and (table[1::3] == q[1::3, None]).all() and q.all()
    assert not best_k[::3].any() and (mv[::3] == (100, 0, 0)).all()      # a tie of all 27: k = 0, and mv is the base itself


def test_bases_at_the_edge_of_int8():
    """+-126, +-127 and -128 under the candidates of radius 1: invalid pairs. Every int8 base has a valid pair among all 27
    (-128 + 1 is a vector), so the block with none is searched with the 18 candidates that have dx <= 0."""
    J, m, D = 8, 3, 5
    rng = np.random.default_rng(34)
    V = np.concatenate([rng.integers(0, 24, size=(300, 3)), 232 + rng.integers(0, 24, size=(300, 3))])
    keys = np.unique(MM.morton(V, J))
    X = _attrs(len(keys), D, 35)
    W = MM.demorton(keys, J)
    far = W + np.where(W[:, :1] < 128, (127, 126, -1), (-127, -126, 1))
    ok = np.all((far >= 0) & (far < 256), axis=1)
    ref, at = np.unique(MM.morton(far[ok], J), return_index=True)
    C = np.ascontiguousarray(X[ok][at])
    n_blocks = _n_blocks(keys, m)
    edge = np.array([(126, 126, 0), (127, 0, 0), (-127, -127, 127), (-128, 0, 0), (-128, 127, -128), (0, -126, 0), (-126, -126, 1), (127, 127, -127),
                     (126, 127, -1), (-127, -126, 1)], np.int8)
    base = edge[np.arange(n_blocks) % len(edge)]
    assert n_blocks > 3 * len(edge)
    cand = MM.candidates(1)
    table, best_k, best_cost, mv = _check(keys, ref, C, X, J, m, base, cand, _weights(D), 0, what="the edge of int8")
    n_valid = (table != MH.INVALID).sum(axis=1)
    assert sorted(set(n_valid.tolist())) == [2, 8, 9, 18, 27] and (best_k >= 0).all()
    assert (mv == (127, 126, -1)).all(axis=1).any() and (mv == (-127, -126, 1)).all(axis=1).any()        # the long vectors are found
    half = np.ascontiguousarray(cand[cand[:, 0] <= 0])
    table, best_k, best_cost, mv = _check(keys, ref, C, X, J, m, base, half, _weights(D), 1, what="a block with no valid pair")
    none = (base[:, 0] == -128)
    assert none.sum() >= 6 and (best_k[none] == -1).all() and (best_cost[none] == -1).all() and not mv[none].any()
    assert (table[none] == -1).all() and (best_k[~none] >= 0).all()


def test_one_candidate():
    J, m, D = 6, 2, 5
    keys, X, ref, C = _scene(D)
    base = _random_base(_n_blocks(keys, m), 36)
    for v in ([0, 0, 0], [-2, 1, 0]):
        _, best_k, best_cost, mv = _check(keys, ref, C, X, J, m, base, np.array([v], np.int32), _weights(D), 0, what=f"K = 1: {v}")
        assert not best_k.any() and best_cost.any() and np.array_equal(mv, base + np.array(v, np.int8))


def test_512_candidates_with_duplicates():
    """random candidates within +-100 around a base within +-27, the candidates of k = 20 .. 29 once more at k = 300 .. 309. The
    reference holds every block's rows moved by base + one of the candidates 20 .. 29 with the frame's own attributes: cost 0 at
    that k AND at its duplicate, and the smaller index must win."""
    J, m, D = 9, 2, 3
    rng = np.random.default_rng(23)
    cand = rng.integers(-100, 101, size=(512, 3)).astype(np.int32)
    cand[256] = 0
    cand[300:310] = cand[20:30]
    V = np.unique(rng.integers(248, 264, size=(300, 3)), axis=0)         # the middle of the cube: no vector leaves it
    keys = MM.morton(V, J)
    o = np.argsort(keys)
    keys, V = keys[o], V[o]
    X = _attrs(len(keys), D, 24)
    b, first = MM.blocks(keys, m)
    base = _random_base(len(first) - 1, 37, 27)
    W = V + base[b].astype(np.int64) + cand[20 + b % 10]
    assert W.min() >= 0 and W.max() < (1 << J) and np.abs(base[:, None, :].astype(np.int64) + cand[None]).max() <= 127
    rk, at = np.unique(MM.morton(W, J), return_index=True)
    table, best_k, best_cost, mv = _check(keys, rk, np.ascontiguousarray(X[at]), X, J, m, base, cand, np.ones(D, np.float32), 0, what="K = 512")
    rows = np.arange(len(table))
    assert ((best_k >= 20) & (best_k < 30)).all() and not best_cost.any() and not table[rows, best_k + 280].any()
    assert len(np.unique(best_k)) > 1 and (table[:, 256] > 0).all()


@pytest.mark.parametrize("D", [5, 243, 244])
def test_all_weights_zero(D):
    """the kernel returns before its loop: a valid pair costs 0, an invalid one is still marked, k = 0 wins where it is valid"""
    J, m = 6, 2
    _tile(D)
    keys, X, ref, C = _scene(D)
    base = _random_base(_n_blocks(keys, m), 38)
    base[::4] = (127, 0, 0)
    table, best_k, best_cost, mv = _check(keys, ref, C, X, J, m, base, MM.candidates(1), np.zeros(D, np.float32), 0, what="no weight")
    assert not best_k.any() and not best_cost.any() and np.array_equal(mv, base)
    assert ((table[::4] == -1).sum(axis=1) == 9).all() and not table[1::4].any()


def test_depth_21():
    """63-bit keys at both corners of the cube, bases of +-126 under radius 1: vectors of up to +-127"""
    from .test_gpu_motion_paths import _corners
    J, D = 21, 5
    keys, X, ref, C = _corners()
    assert int(keys.max()) >> 62 == 1 and int(ref.max()) >> 62 == 1 and int(keys.min()) < 8 ** 5
    for m in (3, 21):
        b, first = MM.blocks(keys, m)
        low = MM.demorton(keys[first[:-1]], J)[:, 0] < 24
        base = np.where(low[:, None], (126, 126, 4), (-126, -126, -4)).astype(np.int8)
        base[1::5] = (0, -1, 0)
        for up in (0, 3):
            _, best_k, _, mv = _check(keys, ref, C, X, J, m, base, MM.candidates(1), _weights(D), up, what=f"J = 21, m = {m}, up = {up}")
            if m == 3 and up == 0:                                       # both long vectors that stay inside are found somewhere
                assert (mv == (127, 126, 5)).all(axis=1).any() and (mv == (-127, -126, -5)).all(axis=1).any()
                assert (mv == (0, -1, 1)).all(axis=1).any()


@pytest.mark.parametrize("up", [0, 1])
@pytest.mark.parametrize("D,pad", [(59, 0), (59, 3), (243, 0), (244, 0)])
def test_identities_against_the_exhaustive_entry_point(D, pad, up):
    """as bits, product against product: a zero base gives raht_motion_search's table and selection; a constant base v gives the
    table of raht_motion_search with the candidates v + c"""
    import torch
    from raht_3dgs_codec_amd import ops
    J, m = 6, 2
    keys, X, ref, C = _scene(D)
    k, r, Cd, Xd = _dev(keys), _dev(ref), _dev(C, pad), _dev(X, pad)
    n_blocks = _n_blocks(keys, m)
    bf = ops.motion_blocks(k, J, m, n_blocks)
    cand, w = MM.candidates(1), _weights(D)
    mv0, cost0, tab0 = ops.motion_search(k, r, Cd, Xd, J, m, bf, cand, w, up=up, want_table=True)
    zero = torch.zeros((n_blocks, 3), dtype=torch.int8, device="cuda")
    mv1, cost1, k1, tab1 = ops.motion_search_around(k, r, Cd, Xd, J, m, bf, zero, cand, w, up=up, want_table=True)
    assert torch.equal(tab1, tab0) and torch.equal(cost1, cost0) and torch.equal(mv1, mv0)
    assert torch.equal(torch.from_numpy(cand).cuda().to(torch.int8)[k1.long()], mv0) and len(torch.unique(k1)) > 1
    v = np.array([-2, 3, -1])
    mv2, cost2, tab2 = ops.motion_search(k, r, Cd, Xd, J, m, bf, cand + v, w, up=up, want_table=True)
    const = torch.from_numpy(np.repeat([v], n_blocks, axis=0).astype(np.int8)).cuda()
    mv3, cost3, _, tab3 = ops.motion_search_around(k, r, Cd, Xd, J, m, bf, const, cand, w, up=up, want_table=True)
    assert torch.equal(tab3, tab2) and torch.equal(cost3, cost2) and torch.equal(mv3, mv2) and bool(tab3.any())


def _translated(J=7, D=5, n=3000, t=(2, -1, 3), seed=40, noise=0.05):
    """a frame and a reference that holds most of it moved by t, with noise, and voxels of its own"""
    if ("translated", J, D) not in _CACHE:
        from raht_3dgs_codec_amd import synth
        keys = synth.sorted_unique_keys(n, J, seed)
        X = _attrs(len(keys), D, seed + 1)
        _CACHE[("translated", J, D)] = (keys, X) + _moved_reference(keys, X, J, seed + 2, t=tuple(-c for c in t), keep=0.8, noise=noise)
    return _CACHE[("translated", J, D)]


@pytest.mark.parametrize("pad", [0, 3])
def test_the_pyramid(pad):
    import torch
    from raht_3dgs_codec_amd import ops
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    J = 7
    keys, X, _, _ = _translated()
    k = _dev(keys)
    counts = OctreeCoder.counts(k, J)
    for L in (1, 2, 3):
        want = MH.pyramid(keys, X, L)
        for cnt in (counts, None):
            got = ops.motion_pyramid(k, _dev(X, pad), J, L, cnt)
            assert len(got) == L
            for (gk, gC), (wk, wC) in zip(got, want):
                assert gk.dtype == torch.int64 and gC.dtype == torch.float32
                assert np.array_equal(gk.cpu().numpy(), wk.astype(np.int64)), (L, "keys")
                assert np.array_equal(gC.cpu().numpy().view(np.int32), wC.view(np.int32)), (L, "means")
    assert ops.motion_pyramid(k, _dev(X), J, 0) == []
    assert len(want[0][0]) < len(keys) and len(want[2][0]) < len(want[1][0]) < len(want[0][0])


@pytest.mark.parametrize("up", [0, 1])
@pytest.mark.parametrize("L", [0, 1, 2])
@pytest.mark.parametrize("D", [5, 59])
def test_the_hierarchy_level_by_level(D, L, up):
    import torch
    from raht_3dgs_codec_amd import ops
    J, m, r = 7, 3, 2
    keys, X, ref, C = _translated(D=D)
    w = _weights(D)
    mv, cost, per_level = MH.search_hier(keys, ref, C, X, J, m, L, r, w, up)
    k, rk, Cd, Xd = _dev(keys), _dev(ref), _dev(C), _dev(X)
    bf = ops.motion_blocks(k, J, m, _n_blocks(keys, m))
    g_mv, g_cost, info = ops.motion_search_hier(k, rk, Cd, Xd, J, m, bf, L, r, w, up=up)
    assert len(info["mv"]) == L + 1 and len(info["pyramid"]) == L and len(info["ref_pyramid"]) == L
    for l in range(L, -1, -1):                                           # from the top: the first level that differs is named
        assert np.array_equal(info["mv"][l].cpu().numpy(), per_level[l]), (L, up, "level", l)
    assert torch.equal(g_mv, info["mv"][0]) and g_mv.dtype == torch.int8
    assert np.array_equal(g_cost.cpu().numpy(), cost)
    for (gk, gC), (wk, wC) in zip(info["ref_pyramid"], MH.pyramid(ref, C, L)):
        assert np.array_equal(gk.cpu().numpy(), wk.astype(np.int64)) and np.array_equal(gC.cpu().numpy().view(np.int32), wC.view(np.int32))
    if L:                                                                # the reference's pyramid handed back in: the same result
        again = ops.motion_search_hier(k, rk, Cd, Xd, J, m, bf, L, r, w, up=up, ref_pyramid=info["ref_pyramid"])
        assert torch.equal(again[0], g_mv) and torch.equal(again[1], g_cost) and again[2]["ref_pyramid"] is info["ref_pyramid"]
    assert len(np.unique(mv, axis=0)) > 1
    found = (mv == (2, -1, 3)).all(axis=1)                               # z = 3 lies beyond radius 2 and within 2 * 2 + 1
    assert not found.any() if L == 0 else found.any()
    if L == 1 and up == 0:
        assert found.mean() > 0.5
