"""The mixed-precision batch entries (raht_fwd_quant_mixed_batch, raht_dequant_inv_mixed_batch; ops.forward_quant_mixed_batch,
ops.dequant_inverse_mixed_batch) on the GPU: several 59-column scenes in one set of launches, every scene's output bit for bit
what the single-scene mixed call returns (tile_kernel_mx_batch / top_kernel_mx_batch run tile_body_mx / top_body_mx on the same
tiles), the reference's xyz integers on the golden frames, and -- through raht_mixed_batch_stats, a dry run of the grouping the
runner itself uses -- the launch counts that make it a batch rather than a loop."""
import numpy as np
import pytest

from .conftest import load_golden
from .test_gpu_mixed import _assert_only_ties
from .test_gpu_parity import _batch_scenes, _dev, _plan

pytestmark = pytest.mark.gpu

SIZE_LISTS = [
    [(40000, 10), (300, 6), (150000, 11), (5000, 9)],                       # 4 scenes of different depth
    [(20000 + 3000 * i, 10) for i in range(11)],                            # more scenes than one launch carries
    [(70000, 12)],                                                          # a batch of one
]


@pytest.fixture(scope="module")
def rt():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    _lib.lib()
    return R


def _widen(Cs, seed=7):
    """wide-range integers in the first four columns, like voxel coordinates (tests/test_gpu_mixed_fusions.py: _scene)"""
    import torch
    gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
    for C in Cs:
        C[:, :4] = torch.randint(0, 4096, (C.shape[0], 4), device="cuda", generator=gen).float()
    return Cs


def _per_channel(D):
    return [0.01 * (1 + (c % 5)) for c in range(D)]


def _check_against_single_calls(plans, Cs, steps, nw, what=""):
    """forward and inverse batch against one single-scene mixed call per scene, torch.equal; -> the batch's outputs"""
    import torch
    from raht_3dgs_codec_amd import ops
    Qb = ops.forward_quant_mixed_batch(plans, Cs, steps, nw)
    assert len(Qb) == len(plans)
    for i, (p, C, Q) in enumerate(zip(plans, Cs, Qb)):
        assert Q.dtype == torch.int32 and tuple(Q.shape) == tuple(C.shape)
        assert torch.equal(Q, p.forward_quant_mixed(C, steps, nw)), (what, "forward", i, nw)
    Cb = ops.dequant_inverse_mixed_batch(plans, Qb, steps, nw)
    for i, (p, Q, c) in enumerate(zip(plans, Qb, Cb)):
        assert c.dtype == torch.float32
        assert torch.equal(c, p.dequant_inverse_mixed(Q, steps, nw)), (what, "inverse", i, nw)
    return Qb, Cb


# 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [59, 14])
@pytest.mark.parametrize("sizes", SIZE_LISTS, ids=["4_depths", "11_scenes", "batch_of_one"])
def test_batch_equals_the_single_scene_mixed_calls_bit_for_bit(rt, D, sizes):
    plans, Cs = _batch_scenes(rt, sizes, D)
    _widen(Cs)
    for nw in (1, 3, 4):
        for steps in (0.02, _per_channel(D)):
            assert plans[0].mixed_stats(D, nw)["tile_rows"] >= 64            # the mixed tile kernels, not the two-pass path
            _check_against_single_calls(plans, Cs, steps, nw, (D, len(sizes)))


# 2 ---------------------------------------------------------------------------------------------------------------------------
def test_batch_returns_the_reference_integers(rt):
    """The two 59-column golden frames and a synthetic scene in one batch: on the golden frames the xyz integers are the
    reference's (bars of test_mixed_returns_the_reference_integers); the 14-column frame in a batch of one."""
    from raht_3dgs_codec_amd import ops
    gs = [load_golden("mx_n1500_j12_d59"), load_golden("mx_n2000_j10_d59")]
    plans = [_plan(rt, g) for g in gs]
    Cs = [_dev(g["C"]) for g in gs]
    sp, sC = _batch_scenes(rt, [(60000, 10)], 59, seed0=91)
    plans, Cs = plans + sp, Cs + sC
    keys = sorted(set(k for k in gs[0] if k.startswith("q_step")) & set(k for k in gs[1] if k.startswith("q_step")))
    assert keys
    for key in keys:
        step = float(key[len("q_step"):])
        Qb = ops.forward_quant_mixed_batch(plans, Cs, step, 3)
        for g, Q in zip(gs, Qb):
            N = g["C"].shape[0]
            pre = g["T"][g["order"]] / step + 0.5
            n_ties = _assert_only_ties(Q.cpu().numpy(), g[key], pre, 0, 3, lambda r, c: 1e-9 * max(1.0, abs(pre[r, c])))
            assert n_ties <= 0.05 * 3 * N
    g = load_golden("mx_n1000_j10_d14")
    p, C = _plan(rt, g), _dev(g["C"])
    for key in [k for k in g if k.startswith("q_step")]:
        step = float(key[len("q_step"):])
        (Q,) = ops.forward_quant_mixed_batch([p], [C], step, 3)
        pre = g["T"][g["order"]] / step + 0.5
        n_ties = _assert_only_ties(Q.cpu().numpy(), g[key], pre, 0, 3, lambda r, c: 1e-9 * max(1.0, abs(pre[r, c])))
        assert n_ties <= 0.05 * 3 * g["C"].shape[0]


# 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw", [1, 3, 4])
def test_batch_is_the_float32_batch_on_the_attribute_columns_and_the_float64_kernel_on_the_wide_ones(rt, nw):
    import torch
    from raht_3dgs_codec_amd import ops
    D = 59
    plans, Cs = _batch_scenes(rt, SIZE_LISTS[0], D, seed0=60)
    _widen(Cs, seed=8)
    for steps in (0.013, _per_channel(D)):
        Qb = ops.forward_quant_mixed_batch(plans, Cs, steps, nw)
        Q32 = ops.forward_quant_batch(plans, Cs, steps)                       # (float) step: the binding rounds to float32
        for p, C, Q, q32 in zip(plans, Cs, Qb, Q32):
            assert torch.equal(Q[:, nw:], q32[:, nw:])
            assert torch.equal(Q[:, :nw], p.forward_quant(C.double(), steps)[:, :nw])
        Cb = ops.dequant_inverse_mixed_batch(plans, Qb, steps, nw)
        C32 = ops.dequant_inverse_batch(plans, Qb, steps)
        for p, Q, c, c32 in zip(plans, Qb, Cb, C32):
            assert torch.equal(c[:, nw:], c32[:, nw:])
            assert torch.equal(c[:, :nw], p.dequant_inverse(Q, steps, dtype=torch.float64)[:, :nw].float())


# 4, 5 ------------------------------------------------------------------------------------------------------------------------
TRUNC = 4


def _mixed_company(rt, D, nw):
    """six scenes: 0, 2, 5 ordinary; 1 on the level engine; 3 with another tile geometry; 4 a truncated plan (root buffers)"""
    import torch
    from raht_3dgs_codec_amd import synth
    plans, Cs = _batch_scenes(rt, [(30000, 10), (30000, 10), (45000, 10), (30000, 10), (20000, 9)], D, seed0=70)
    plans[1].set_engine("level")
    plans[3].set_engine("tile", 64, 64, 0, 64)
    J = 9
    V, keys, C = synth.scene(90000, J, D, seed=53)
    plans.insert(TRUNC, rt.RahtPlan.from_keys(_dev(keys.view(np.int64)), 3 * J, top_level=3 * J - 9))
    Cs.insert(TRUNC, _dev(C))
    _widen(Cs, seed=9)
    # strided rows, another stride per scene (ld > D)
    strided = []
    for i, C in enumerate(Cs):
        big = torch.zeros((C.shape[0], D + 1 + 2 * i), dtype=torch.float32, device="cuda")
        big[:, :D] = C
        strided.append(big[:, :D])
    nr = plans[TRUNC].n_roots

    def bufs():
        return (torch.full((nr, D), 7.5, dtype=torch.float32, device="cuda"), torch.full((nr, nw), 7.5, dtype=torch.float64, device="cuda"))
    return plans, Cs, strided, bufs


def test_mixed_company_in_one_call(rt):
    import torch
    from raht_3dgs_codec_amd import ops
    D, nw, T = 59, 3, TRUNC
    plans, Cs, strided, bufs = _mixed_company(rt, D, nw)
    n = len(plans)
    for steps in (0.02, _per_channel(D)):
        (rb1, rw1), (rbn, rwn) = bufs(), bufs()
        ref = [p.forward_quant_mixed(C, steps, nw, **(dict(roots=rb1, roots_wide=rw1) if i == T else {}))
               for i, (p, C) in enumerate(zip(plans, Cs))]
        refC = [p.dequant_inverse_mixed(Q, steps, nw, **(dict(roots=rb1, roots_wide=rw1) if i == T else {}))
                for i, (p, Q) in enumerate(zip(plans, ref))]
        torch.cuda.synchronize()
        # what the call will do, from the grouping function itself: the level-engine scene and the truncated plan are
        # single-scene calls; the scene of another geometry is a launch of its own shape, not a single-scene call
        for inverse in (False, True):
            st = ops.mixed_batch_stats(plans, D, nw, inverse=inverse)
            print(f"mixed company, inverse={inverse}: {st}")
            assert st["single_scene_calls"] == 2, st
            own = ops.mixed_batch_stats([plans[3]], D, nw, inverse=inverse)
            assert own["single_scene_calls"] == 0 and own["tile_launches"] >= 1, own
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        roots = [None] * n
        wide = [None] * n
        roots[T], wide[T] = rbn, rwn
        with torch.cuda.stream(side):                                        # strided rows, a non-default stream
            Qb = ops.forward_quant_mixed_batch(plans, strided, steps, nw, roots=roots, roots_wide=wide)
            Cb = ops.dequant_inverse_mixed_batch(plans, Qb, steps, nw, roots=roots, roots_wide=wide)
        side.synchronize()
        # (a truncated plan leaves its roots' Q rows to the caller: compared are the other rows, and the root buffers)
        nonroot = torch.ones(Cs[T].shape[0], dtype=torch.bool, device="cuda")
        nonroot[plans[T].inv_order[plans[T].root_rows]] = False
        for i in range(n):
            if i == T:
                assert torch.equal(Qb[i][nonroot], ref[i][nonroot])
                assert torch.equal(rbn[:, nw:], rb1[:, nw:]) and torch.equal(rwn, rw1)
            else:
                assert torch.equal(Qb[i], ref[i]), i
                assert torch.equal(Cb[i], refC[i]), i
        # the inverse of the truncated plan reads its roots from the buffers: the same integers for both
        Cb_T = ops.dequant_inverse_mixed_batch(plans, ref, steps, nw, roots=roots, roots_wide=wide)
        torch.cuda.synchronize()
        for i in range(n):
            assert torch.equal(Cb_T[i], refC[i]), i
        # the root buffers are taken off the plan again after the call
        with pytest.raises(rt.RahtError):
            plans[T].forward_quant_mixed(Cs[T], 0.02, nw)


def test_every_scene_on_the_two_pass_path(rt):
    """D = 6, n_wide = 3 (D - n_wide < 4): no scene has a mixed tile schedule; the batch is n single-scene calls."""
    from raht_3dgs_codec_amd import ops
    D, nw = 6, 3
    plans, Cs = _batch_scenes(rt, [(30000, 10), (300, 6), (50000, 11)], D, seed0=80)
    _widen(Cs, seed=10)
    for inverse in (False, True):
        st = ops.mixed_batch_stats(plans, D, nw, inverse=inverse)
        assert st == {"tile_launches": 0, "top_launches": 0, "single_scene_calls": len(plans)}, st
    for steps in (0.02, _per_channel(D)):
        _check_against_single_calls(plans, Cs, steps, nw, "two-pass")


@pytest.mark.parametrize("n", [8, 11])
def test_it_is_really_batched(rt, n):
    """n distinct plans built from ONE key tensor (equal trees, equal schedules), different attributes: 8 scenes go out in as many
    launches as ONE scene has stages, 11 in twice as many; none takes the single-scene call. The outputs of the same batches are
    compared with the single calls, so the count and the results come from one call sequence."""
    import torch
    from raht_3dgs_codec_amd import ops, synth
    D, nw, J = 59, 3, 10
    V, keys, C0 = synth.scene(60000, J, D, seed=21)
    kd = _dev(keys.view(np.int64))
    plans = [rt.RahtPlan.from_keys(kd, 3 * J) for _ in range(n)]
    gen = torch.Generator(device="cuda"); gen.manual_seed(5)
    Cs = [_dev(C0) + (0.25 * i) * torch.randn(C0.shape, device="cuda", generator=gen) for i in range(n)]
    _widen(Cs, seed=11)
    K = len(plans[0].mixed_stats(D, nw)["rows_per_stage"])
    assert K >= 2
    launches = (n + 7) // 8
    for inverse in (False, True):
        st = ops.mixed_batch_stats(plans, D, nw, inverse=inverse)
        print(f"n={n} inverse={inverse} K={K}: {st}")
        assert st["tile_launches"] + st["top_launches"] == launches * K, (st, K)
        assert st["top_launches"] <= launches
        assert st["single_scene_calls"] == 0
    _check_against_single_calls(plans, Cs, 0.02, nw, "equal trees")
    _check_against_single_calls(plans, Cs, _per_channel(D), nw, "equal trees")


# 6 ---------------------------------------------------------------------------------------------------------------------------
def test_concurrent_directions(rt):
    """A forward batch on one stream next to an inverse batch of earlier integers on another: each direction uses its own
    workspaces of every plan; equal to the serial results."""
    import torch
    from raht_3dgs_codec_amd import ops
    D, nw = 59, 3
    plans, Cs = _batch_scenes(rt, [(300000, 12), (120000, 11), (200000, 12), (40000, 10)], D, seed0=30)
    _widen(Cs, seed=12)
    s0, s1 = 0.02, 0.05
    for p in plans:
        p.set_concurrent_directions(True)
    # both directions once serially: schedules, tile programs and both workspace sets exist before two streams share a plan
    Q0 = ops.forward_quant_mixed_batch(plans, Cs, s0, nw)
    C0 = ops.dequant_inverse_mixed_batch(plans, Q0, s0, nw)
    Q1 = ops.forward_quant_mixed_batch(plans, Cs, s1, nw)
    torch.cuda.synchronize()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(a):
        Q1c = ops.forward_quant_mixed_batch(plans, Cs, s1, nw)
    with torch.cuda.stream(b):
        C0c = ops.dequant_inverse_mixed_batch(plans, Q0, s0, nw)
    a.synchronize()
    b.synchronize()
    torch.cuda.synchronize()
    for i in range(len(plans)):
        assert torch.equal(Q1c[i], Q1[i]), i
        assert torch.equal(C0c[i], C0[i]), i
        assert torch.equal(Q0[i], plans[i].forward_quant_mixed(Cs[i], s0, nw)), i
        assert torch.equal(C0[i], plans[i].dequant_inverse_mixed(Q0[i], s0, nw)), i


# 7 ---------------------------------------------------------------------------------------------------------------------------
def test_larger_scenes(rt):
    """~1 M and ~3 M x 59: tile counts beyond one round of the chip."""
    plans, Cs = _batch_scenes(rt, [(1_000_000, 10), (3_000_000, 12)], 59, seed0=40)
    assert Cs[0].shape[0] > 500_000 and Cs[1].shape[0] > 2_000_000
    _check_against_single_calls(plans, Cs, 0.01, 3, "large")


# the wrappers' own rules -----------------------------------------------------------------------------------------------------
def test_wrapper_refusals(rt):
    import torch
    from raht_3dgs_codec_amd import ops
    D, nw = 59, 3
    plans, Cs = _batch_scenes(rt, [(5000, 9), (300, 6)], D, seed0=95)
    with pytest.raises(rt.RahtError) as e:
        ops.forward_quant_mixed_batch([plans[0], plans[0]], [Cs[0], Cs[0]], 0.02, nw)
    assert "raht_fwd_quant_mixed_batch" in str(e.value)
    with pytest.raises(rt.RahtError) as e:
        ops.dequant_inverse_mixed_batch(plans, [torch.zeros_like(C, dtype=torch.int32) for C in Cs], 0.02, 5)
    assert "raht_dequant_inv_mixed_batch" in str(e.value)
    with pytest.raises(ValueError):
        ops.forward_quant_mixed_batch(plans, Cs, 0.02, nw, roots=[None])
    # a row-mapped plan refuses the whole batch (as the single calls refuse it), before anything is launched
    tk = np.unique(np.random.default_rng(2).integers(0, 512, size=300)).astype(np.int64)
    top = rt.RahtPlan.from_keys(_dev(tk), 9)
    top.set_row_map(_dev(np.arange(tk.shape[0], dtype=np.int64) * 2), 2 * tk.shape[0])
    X = torch.zeros((top.N, D), dtype=torch.float32, device="cuda")
    with pytest.raises(rt.RahtError) as e:
        ops.forward_quant_mixed_batch([plans[0], top], [Cs[0], X], 0.02, nw)
    assert "scene 1" in str(e.value)
    with pytest.raises(rt.RahtError):
        ops.mixed_batch_stats([plans[0], top], D, nw)
