"""raht_region_needs_bi on the GPU against the numpy model (tests/numpy_region_bi.py), on the shapes of
test_gpu_region_set.test_needs_equals_the_model: the cells of both references of a B frame from one pass over the keys, under two
motion fields and the block modes, and the five equalities with raht_region_needs."""
import numpy as np
import pytest

from . import numpy_motion as MM
from . import numpy_region_bi as NB
from .test_gpu_region_set import _dev

pytestmark = pytest.mark.gpu


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _blocks(keys, m, rng, radius=3, modes=4):
    bf = MM.blocks(keys, m)[1]
    n = len(bf) - 1
    return (bf, rng.integers(-radius, radius + 1, size=(n, 3)).astype(np.int8), rng.integers(-radius, radius + 1, size=(n, 3)).astype(np.int8),
            rng.integers(0, modes, size=n).astype(np.uint8))


def _case(keys, J, depth, up, bf=None, mv0=None, mv1=None, mode=None, m=0, **kw):
    import torch
    from raht_3dgs_codec_amd import ops
    tl = 3 * (J - depth)
    want = NB.needs_bi(keys, J, tl, up, bf, mv0, mv1, mode)
    got = ops.region_needs_bi(_dev(keys), J, tl, up, _t(bf), _t(mv0), _t(mv1), _t(mode), m, **kw)
    for g, w in zip(got, want):
        assert g.dtype == torch.int64 and np.array_equal(g.cpu().numpy().view(np.uint64), w), (J, depth, up, m)
    return want


def _every_subset(keys, J, depth, up, bf, mv0, mv1, mode, m):
    """the fields and the modes, each given or not"""
    for a, b, c in ((mv0, mv1, mode), (mv0, None, None), (None, mv1, None), (None, None, mode), (mv0, mv1, None), (None, mv1, mode)):
        want = _case(keys, J, depth, up, bf, a, b, c, m)
    return want


def test_one_row_that_leaves_the_cube_in_one_reference():
    one = MM.morton(np.array([[3, 0, 7]]), 3)
    bf = np.array([0, 1], np.int64)
    stay, leave = np.array([[1, 0, -2]], np.int8), np.array([[0, -1, 0]], np.int8)
    for mv0, mv1, n0, n1 in ((stay, leave, 1, 0), (leave, stay, 0, 1), (leave, leave, 0, 0), (stay, stay, 1, 1), (None, leave, 1, 0)):
        for mode, use in ((None, (1, 1)), (0, (1, 1)), (1, (1, 0)), (2, (0, 1)), (3, (0, 0))):
            want = _case(one, 3, 2, 0, bf, mv0, mv1, None if mode is None else np.array([mode], np.uint8), 1)
            assert (len(want[0]), len(want[1])) == (n0 * use[0], n1 * use[1])


def test_257_keys_at_J_3():
    rng = np.random.default_rng(14)
    keys = np.sort(rng.choice(512, 257, replace=False)).astype(np.uint64)           # more than one workgroup step
    for depth, up in ((1, 0), (2, 0), (2, 1), (2, 2), (1, 3)):
        _case(keys, 3, depth, up)
        for m in (1, 2, 3):
            _every_subset(keys, 3, depth, up, *_blocks(keys, m, rng), m)


def test_3000_draws_at_J_6():
    from raht_3dgs_codec_amd import synth
    rng = np.random.default_rng(15)
    keys = synth.sorted_unique_keys(3000, 6, 61)
    for m in (2, 4, 6):
        blocks = _blocks(keys, m, rng)
        for depth, up in ((1, 0), (2, 1), (5, 0), (5, 3), (4, 3)):
            want = _every_subset(keys, 6, depth, up, *blocks, m)
            assert m == 6 or depth == 1 or (len(want[0]) > 1 and len(want[1]) > 1)
    _case(keys, 6, 5, 0)


def test_vectors_of_127_at_the_corners_of_the_cube_at_J_21():
    top = 2 ** 21 - 1
    V = np.array([[0, 0, 0], [0, 0, 1], [100, 200, 50], [top - 1, top, top], [top, top, top]], np.int64)
    keys = np.sort(MM.morton(V, 21))
    bf = MM.blocks(keys, 1)[1]
    assert len(bf) - 1 == 3
    for vec in ((127, 127, 127), (-127, -127, -127), (127, -127, 0)):
        mv0 = np.tile(np.array(vec, np.int8), (3, 1))
        mv0[1] = -mv0[1]
        mv1 = -mv0
        for mode in (None, np.array([0, 1, 2], np.uint8), np.array([2, 0, 1], np.uint8)):
            for depth, up in ((1, 0), (20, 0), (20, 3), (13, 2)):
                _case(keys, 21, depth, up, bf, mv0, mv1, mode, 1)


def test_the_five_equalities_with_region_needs():
    import torch
    from raht_3dgs_codec_amd import ops, synth
    rng = np.random.default_rng(16)
    keys = synth.sorted_unique_keys(3000, 6, 61)
    kd = _dev(keys)
    for m in (2, 4):
        bf, mv0, mv1, _ = _blocks(keys, m, rng)
        n = len(bf) - 1
        bfd, f0, f1 = _t(bf), _t(mv0), _t(mv1)
        all_ = lambda v: torch.full((n,), v, dtype=torch.uint8, device="cuda")
        for depth, up in ((1, 0), (2, 1), (5, 0), (5, 3), (4, 3)):
            tl = 3 * (6 - depth)
            one0, one1, none = ops.region_needs(kd, 6, tl, up, bfd, f0, m), ops.region_needs(kd, 6, tl, up, bfd, f1, m), ops.region_needs(kd, 6, tl, up)
            empty = none[:0]
            for got, want in ((ops.region_needs_bi(kd, 6, tl, up, bfd, f0, f0, None, m), (one0, one0)),
                              (ops.region_needs_bi(kd, 6, tl, up), (none, none)),
                              (ops.region_needs_bi(kd, 6, tl, up, bfd, f0, f1, all_(1), m), (one0, empty)),
                              (ops.region_needs_bi(kd, 6, tl, up, bfd, f0, f1, all_(2), m), (empty, one1)),
                              (ops.region_needs_bi(kd, 6, tl, up, bfd, f0, f1, all_(3), m), (empty, empty)),
                              (ops.region_needs_bi(kd, 6, tl, up, bfd, f0, f1, None, m), (one0, one1)),
                              (ops.region_needs_bi(kd, 6, tl, up, bfd, None, None, all_(0), m), (none, none))):
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (m, depth, up)


def test_mode_bytes_above_3_behave_as_3():
    import torch
    from raht_3dgs_codec_amd import ops, synth
    rng = np.random.default_rng(17)
    keys = synth.sorted_unique_keys(3000, 6, 61)
    bf, mv0, mv1, mode = _blocks(keys, 2, rng)
    for byte in (4, 255):
        other = np.where(mode == 3, byte, mode).astype(np.uint8)
        assert (other == byte).any()
        want = _case(keys, 6, 2, 1, bf, mv0, mv1, mode, 2)
        got = ops.region_needs_bi(_dev(keys), 6, 12, 1, _t(bf), _t(mv0), _t(mv1), _t(other), 2)
        assert all(np.array_equal(g.cpu().numpy().view(np.uint64), w) for g, w in zip(got, want))
        got = ops.region_needs_bi(_dev(keys), 6, 12, 1, _t(bf), _t(mv0), _t(mv1), torch.full((len(mode),), byte, dtype=torch.uint8, device="cuda"), 2)
        assert got[0].numel() == 0 and got[1].numel() == 0


def test_a_capacity_of_the_larger_count_passes_and_one_less_is_refused():
    from raht_3dgs_codec_amd import ops, synth
    rng = np.random.default_rng(18)
    keys = synth.sorted_unique_keys(3000, 6, 61)
    bf, mv0, mv1, mode = _blocks(keys, 4, rng, modes=3)
    mode[: len(mode) // 2] = 1                                                # reference 0 has more cells than reference 1
    mirrored = np.where(mode == 1, 2, np.where(mode == 2, 1, mode)).astype(np.uint8)     # ... and the other way round
    for args in ((), (bf, mv0, mv1, mode, 4), (bf, mv1, mv0, mirrored, 4)):
        want = _case(keys, 6, 2, 0, *args)
        cap = max(len(want[0]), len(want[1]))
        assert not args or len(want[0]) != len(want[1])
        _case(keys, 6, 2, 0, *args, capacity=cap)
        with pytest.raises(ops.RahtError, match="RAHT_ERR_INVALID.*raht_region_needs_bi"):
            _case(keys, 6, 2, 0, *args, capacity=cap - 1)


def test_every_row_its_own_block():
    from raht_3dgs_codec_amd import synth
    rng = np.random.default_rng(19)
    keys = synth.sorted_unique_keys(3000, 6, 61)
    n = len(keys)
    bf = np.arange(n + 1, dtype=np.int64)
    mv0, mv1 = (rng.integers(-3, 4, size=(n, 3)).astype(np.int8) for _ in range(2))
    mode = rng.integers(0, 4, size=n).astype(np.uint8)
    for depth, up in ((2, 0), (5, 1), (4, 3)):
        _case(keys, 6, depth, up, bf, mv0, mv1, mode, 1)
