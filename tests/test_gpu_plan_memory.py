"""Who owns a plan's device memory (csrc/raht_common.h: DevBuf; csrc/schedule.hip): every block a plan, its schedules and their
workspaces take from the library's block cache goes back when the plan is destroyed or its construction fails part-way.
Counted with raht_debug_live_blocks() (blocks handed out and not yet given back), never with the free memory of the device:
other processes move that."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, NBITS = 30000, 30


@pytest.fixture(scope="module")
def rt():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    _lib.lib()
    return R


def _live():
    from raht_3dgs_codec_amd import _lib
    return int(_lib.lib().raht_debug_live_blocks())


def _keys(seed):
    rng = np.random.default_rng(seed)
    return np.unique(rng.integers(0, (1 << NBITS) - 1, size=N + 64, dtype=np.int64))[:N]


def test_a_plan_gives_back_every_block_it_took(rt):
    """One ordinary plan through everything that allocates or drops schedule memory: schedules of three geometries, tile
    programs, a workspace regrow, truncation and back (schedules dropped, roots recomputed), an abandoned schedule."""
    import torch
    gc.collect()
    base = _live()
    rng = np.random.default_rng(41)
    keys = torch.from_numpy(_keys(41)).cuda()
    C7 = torch.from_numpy(rng.normal(size=(N, 7)).astype(np.float32)).cuda()
    C59 = torch.from_numpy(rng.normal(size=(N, 59)).astype(np.float32)).cuda()
    p = rt.RahtPlan.from_keys(keys, NBITS)
    assert _live() > base
    T0 = p.forward(C7, want_w=False)
    p.forward(C7.double(), want_w=False)
    p.forward_quant_mixed(C59, 0.01, 3)                        # tile programs
    p.set_concurrent_directions(True)
    assert torch.equal(p.forward(C7, want_w=False), T0)       # workspaces re-made, one per direction
    p.set_engine("tile", 64, 64, 0, 64)                        # a second schedule
    assert (p.forward(C7, want_w=False) - T0).abs().max().item() <= 4e-6 * T0.abs().max().item()
    lvl = np.sort(p.arrays()[1][1:])
    p.set_top_level(int(lvl[len(lvl) // 2]))                   # schedules dropped, roots recomputed
    assert p.n_roots > 1
    p.set_top_level(64)
    assert p.n_roots == 1
    p.set_max_stages(1)                                        # the 64-row schedule cannot finish in one stage: level engine
    assert not p.stage_stats(4, 7)["valid"]
    assert (p.forward(C7, want_w=False) - T0).abs().max().item() <= 4e-6 * T0.abs().max().item()
    p.set_max_stages(24)
    p.set_engine("tile", 0, 0, 0, 0)
    assert torch.equal(p.forward(C7, want_w=False), T0)
    torch.cuda.synchronize()
    del p
    gc.collect()
    assert _live() == base


def test_the_exact_builder_gives_back_what_the_stopped_chain_took(rt):
    """The half_roots plan of test_schedule_chain_exits: stage 0 keeps more entries than the chain's buffer of stage 1 holds, the
    chain stops, its speculative blocks are dropped and the exact builder builds the schedule."""
    import torch
    from tests.numpy_ops import NumpyPlan
    gc.collect()
    base = _live()
    rng = np.random.default_rng(1)
    keys = np.unique(rng.integers(0, (1 << NBITS) - 1, size=N + 64, dtype=np.int64))[:N]
    lv = np.sort(np.asarray(NumpyPlan(torch.from_numpy(keys.copy()), NBITS).lvl)[1:])
    top = int(lv[len(lv) // 2])
    p = rt.RahtPlan.from_keys(torch.from_numpy(keys.copy()).cuda(), NBITS, top_level=top)
    assert 0.3 * N < p.n_roots < 0.7 * N
    assert p.stage_stats(4, 7)["valid"]
    Cd = torch.from_numpy(rng.normal(size=(N, 7))).cuda()
    roots = torch.empty((p.n_roots, 7), dtype=Cd.dtype, device="cuda")
    T = p.forward(Cd, want_w=False, roots=roots)
    assert (p.inverse(T, roots=roots) - Cd).abs().max().item() <= 1e-11 * Cd.abs().max().item()
    torch.cuda.synchronize()
    del p
    gc.collect()
    assert _live() == base


def test_constructions_that_fail_part_way_leave_nothing_behind(rt):
    import torch
    from raht_3dgs_codec_amd._lib import RahtError
    gc.collect()
    base = _live()
    keys = _keys(43)
    keys[[1000, 1001]] = keys[[1001, 1000]]
    with pytest.raises(RahtError, match="RAHT_ERR_UNSORTED"):
        rt.RahtPlan.from_keys(torch.from_numpy(keys).cuda(), NBITS)
    assert _live() == base
    J = 10
    V = np.random.default_rng(44).integers(0, 1 << J, size=(N, 3), dtype=np.int64)
    V[777, 1] = 1 << J
    with pytest.raises(RahtError, match="RAHT_ERR_BOUNDS"):
        rt.RahtPlan.from_coords(torch.from_numpy(V).cuda(), [0.0, 0.0, 0.0], float(1 << J), J)
    assert _live() == base
    small = rt.RahtPlan.from_keys(torch.from_numpy(_keys(45)[:100].copy()).cuda(), NBITS)
    m = torch.arange(100, dtype=torch.int64)
    m[17] = 128
    with pytest.raises(RahtError, match="RAHT_ERR_BOUNDS"):
        small.set_row_map(m.cuda(), 128)
    torch.cuda.synchronize()
    del small
    gc.collect()
    assert _live() == base


def test_a_cache_limit_of_zero_keeps_nothing(rt):
    """raht_set_cached_memory_limit(0): every block a dropped plan gives back goes to hipFree -- the live count is back where it
    started and the cache holds nothing that raht_release_cached_memory() could free; with the default limit the same plan
    leaves its blocks cached. Blocks are counted, never the device's free memory."""
    import torch
    from raht_3dgs_codec_amd import _lib
    L = _lib.lib()

    def build_and_drop():
        p = rt.RahtPlan.from_keys(torch.from_numpy(_keys(47)).cuda(), NBITS)
        p.forward(torch.zeros((N, 7), device="cuda"), want_w=False)        # a schedule and its workspaces
        torch.cuda.synchronize()
        del p
        gc.collect()

    gc.collect()
    _lib.check(L.raht_release_cached_memory())
    assert L.raht_debug_cached_blocks() == 0
    base = _live()
    try:
        _lib.check(L.raht_set_cached_memory_limit(0))
        build_and_drop()
        assert _live() == base
        assert L.raht_debug_cached_blocks() == 0
        assert L.raht_set_cached_memory_limit(-1) != 0                   # refused, the limit stays
        build_and_drop()
        assert L.raht_debug_cached_blocks() == 0
    finally:
        _lib.check(L.raht_set_cached_memory_limit(8 << 30))
    build_and_drop()
    assert _live() == base
    assert L.raht_debug_cached_blocks() > 0
    _lib.check(L.raht_release_cached_memory())
    assert L.raht_debug_cached_blocks() == 0
