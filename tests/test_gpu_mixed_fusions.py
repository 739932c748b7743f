"""The driver-loop fusions in mixed precision (raht_fwd_quant_mixed_multi, raht_dequant_inv_mixed_sqdiff, csrc/transform_mx.hip):
one forward pass that writes one quantization per step, and an inverse whose stage 0 also sums the squared differences behind
the PSNR columns (python/encode_3dgs.py:28,199-217,274,298-310), with the wide columns carried in float64.

Bars:
  multi    Q[i] bit-identical to forward_quant_mixed(C, steps[i]) -- hence the reference's integers on the wide columns of the
           mx_* fixtures, except next to an exact rounding tie of the reference's own quotient
  sqdiff   C_rec bit-identical to dequant_inverse_mixed; the sums equal raht_sqdiff_columns(C_ref, C_rec) up to the order of the
           float64 additions (rtol 1e-12), and bit-identical with and without C_rec
"""
import numpy as np
import pytest

from .conftest import golden_names, load_golden
from .test_gpu_parity import _dev, _plan

pytestmark = pytest.mark.gpu

MX = golden_names(prefix="mx_")
GEOMS = [(0, 0, 0, 0), (64, 64, 0, 64), (128, 64, 0, 64), (64, 256, 0, 0), (192, 128, 0, 128)]
COLOR_STEPS = [0.01 * s for s in (1, 4, 8, 12, 16, 20, 24, 32, 64)]          # encode_3dgs.py:28 colorStep, scaled
STEP_LISTS = {
    "one": [0.37],
    "nine": COLOR_STEPS,
    "fourteen": [0.005 * (i + 1) for i in range(14)],                          # more than one chunk of MULTI_Q_MAX (12)
    "extremes": [1e-30, 3e30, 1.0],                                            # outside the fast float division's range, both ends
}


@pytest.fixture(scope="module")
def rt():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    _lib.lib()
    return R


def _scene(seed, N, nbits, D):
    import torch
    gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
    keys = torch.unique(torch.randint(0, 1 << nbits, (int(N * 1.3) + 8,), device="cuda", dtype=torch.int64, generator=gen))[:N].contiguous()
    C = torch.randn((int(keys.shape[0]), D), device="cuda", generator=gen)
    C[:, :4] = torch.randint(0, 4096, (C.shape[0], 4), device="cuda", generator=gen).float()     # wide-range, like voxel coordinates
    return keys, C


def _sqdiff_columns(A, B):
    """raht_sqdiff_columns(A, B) through the C ABI"""
    import torch
    from raht_3dgs_codec_amd import _lib, ops
    import ctypes
    N, D = A.shape
    out = torch.empty(D, dtype=torch.float64, device=A.device)
    _lib.check(_lib.lib().raht_sqdiff_columns(ctypes.c_void_p(A.data_ptr()), A.stride(0), ctypes.c_void_p(B.data_ptr()), B.stride(0),
                                              N, D, 0, ctypes.c_void_p(out.data_ptr()), ops._stream()))
    return out


def _check_multi(p, C, steps, nw, what, **roots):
    import torch
    Qs = p.forward_quant_mixed_multi(C, steps, nw, **roots)
    assert len(Qs) == len(steps)
    for s, Q in zip(steps, Qs):
        assert torch.equal(Q, p.forward_quant_mixed(C, s, nw, **roots)), (what, s)
    return Qs


def _check_sqdiff(p, Q, steps, C, nw, what, **roots):
    import torch
    Cr0 = p.dequant_inverse_mixed(Q, steps, nw, **roots)
    Cr, sq = p.dequant_inverse_mixed_sqdiff(Q, steps, C, nw, **roots)
    assert torch.equal(Cr, Cr0), what
    ref = _sqdiff_columns(C, Cr0)
    assert torch.allclose(sq, ref, rtol=1e-12, atol=0.0), (what, float(((sq - ref).abs() / ref.abs().clamp_min(1e-300)).max()))
    none, sq2 = p.dequant_inverse_mixed_sqdiff(Q, steps, C, nw, want_rec=False, **roots)
    assert none is None and torch.equal(sq2, sq), what
    return Cr, sq


@pytest.mark.parametrize("which", sorted(STEP_LISTS))
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("name", MX)
def test_multi_equals_the_single_mixed_calls(rt, name, geom, which):
    g = load_golden(name)
    p = _plan(rt, g, "tile", *geom)
    C = _dev(g["C"])
    N, D = g["C"].shape
    st = p.mixed_stats(D, 3)
    assert st["tile_rows"] >= 64 and st["rows_per_stage"][0] == N          # the mixed tile kernels run, not the fallback
    _check_multi(p, C, STEP_LISTS[which], 3, (name, geom, which))


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("name", MX)
def test_multi_returns_the_reference_integers(rt, name, geom):
    from .test_gpu_mixed import _assert_only_ties
    g = load_golden(name)
    p = _plan(rt, g, "tile", *geom)
    C = _dev(g["C"])
    N, D = g["C"].shape
    keys = [k for k in g if k.startswith("q_step")]
    steps = [float(k[len("q_step"):]) for k in keys]
    Qs = p.forward_quant_mixed_multi(C, steps, 3)
    for key, step, Q in zip(keys, steps, Qs):
        pre = g["T"][g["order"]] / step + 0.5
        n_ties = _assert_only_ties(Q.cpu().numpy(), g[key], pre, 0, 3, lambda r, c: 1e-9 * max(1.0, abs(pre[r, c])))
        assert n_ties <= 0.05 * 3 * N
        # the fused inverse from the reference's integers
        _check_sqdiff(p, _dev(g[key]), step, C, 3, (name, geom, step))


@pytest.mark.parametrize("seed", range(16))
def test_randomised_shapes(rt, seed):
    """N (one-launch trees to several tile stages), key width, n_wide, D, tile geometry, scalar and per-channel steps."""
    rng = np.random.default_rng(2000 + seed)
    N = int(rng.choice([1, 2, 3, 40, 700, 1536, 1537, 5000, 40000, 200000]))
    nbits = int(rng.choice([12, 21, 30, 36, 60])) if N < 4000 else int(rng.choice([21, 30, 36, 60]))
    nw = int(rng.integers(1, 5))
    D = int(rng.choice([nw + 4, nw + 5, 14, 32, 59, 60, 63, 64, 66]))
    D = max(D, nw + 4)
    keys, C = _scene(seed, N, nbits, D)
    p = rt.RahtPlan.from_keys(keys, nbits)
    geom = [(0, 0, 0, 0), (64, 64, 0, 64), (128, 64, 0, 0), (256, 128, 0, 256), (0, 64, 0, 64)][seed % 5]
    p.set_engine("tile", *geom)
    assert p.mixed_stats(D, nw)["tile_rows"] >= 64
    what = (N, nbits, D, nw, geom)
    Qs = _check_multi(p, C, [0.013, 0.05, 0.4] if seed % 2 else COLOR_STEPS, nw, what)
    _check_sqdiff(p, Qs[0], 0.013 if seed % 2 else COLOR_STEPS[0], C, nw, what)
    per_ch = [0.01 * (1 + (c % 7)) for c in range(D)]
    _check_sqdiff(p, p.forward_quant_mixed(C, per_ch, nw), per_ch, C, nw, what + ("per-channel",))


@pytest.mark.parametrize("case", ["level_engine", "narrow_rows", "wide_rows"])
def test_fallback_shapes(rt, case):
    """Shapes the mixed tile kernels do not take: the single calls inside, with their results."""
    nw = 3
    keys, C = _scene(77, 30000, 36, {"level_engine": 59, "narrow_rows": nw + 3, "wide_rows": 80}[case])
    D = C.shape[1]
    p = rt.RahtPlan.from_keys(keys, 36)
    if case == "level_engine":
        p.set_engine("level")
    assert p.mixed_stats(D, nw)["tile_rows"] == 0
    Qs = _check_multi(p, C, COLOR_STEPS[:4], nw, case)
    _check_sqdiff(p, Qs[1], COLOR_STEPS[1], C, nw, case)


def test_truncated_plan_with_root_buffers(rt):
    import torch
    from raht_3dgs_codec_amd import synth
    J, D, nw = 9, 59, 3
    V, keys, C = synth.scene(90000, J, D, seed=53)
    pl = rt.RahtPlan.from_keys(_dev(keys.view(np.int64)), 3 * J, top_level=3 * J - 9)
    Cd = _dev(C)
    nr = pl.n_roots
    bufs = [(torch.full((nr, D), 7.5, dtype=torch.float32, device="cuda"), torch.full((nr, nw), 7.5, dtype=torch.float64, device="cuda"))
            for _ in range(2)]
    steps = COLOR_STEPS[:3]
    # (the roots' Q rows are left to the caller's top stage: compared are the other rows, and the root buffers)
    nonroot = torch.ones(Cd.shape[0], dtype=torch.bool, device="cuda")
    nonroot[pl.inv_order[pl.root_rows]] = False
    Qs = pl.forward_quant_mixed_multi(Cd, steps, nw, roots=bufs[0][0], roots_wide=bufs[0][1])
    for s, Q in zip(steps, Qs):
        Q1 = pl.forward_quant_mixed(Cd, s, nw, roots=bufs[1][0], roots_wide=bufs[1][1])
        assert torch.equal(Q[nonroot], Q1[nonroot]), s
        assert torch.equal(bufs[0][0][:, nw:], bufs[1][0][:, nw:]) and torch.equal(bufs[0][1], bufs[1][1]), s
    rb, rw = bufs[0]
    Cr, sq = _check_sqdiff(pl, Qs[0], steps[0], Cd, nw, "truncated", roots=rb, roots_wide=rw)
    # a row-mapped plan is refused
    tk = np.unique(np.random.default_rng(2).integers(0, 512, size=300)).astype(np.int64)
    top = rt.RahtPlan.from_keys(_dev(tk), 9)
    top.set_row_map(_dev(np.arange(tk.shape[0], dtype=np.int64) * 2), 2 * tk.shape[0])
    X = torch.zeros((2 * tk.shape[0], D), dtype=torch.float32, device="cuda")
    with pytest.raises(rt.RahtError):
        top.forward_quant_mixed_multi(X, steps, nw)
    with pytest.raises(rt.RahtError):
        top.dequant_inverse_mixed_sqdiff(torch.zeros((2 * tk.shape[0], D), dtype=torch.int32, device="cuda"), 0.01, X, nw)


def test_strided_reference_and_unaligned_input(rt):
    import torch
    g = load_golden("mx_n2000_j10_d59")
    p = _plan(rt, g)
    N, D = g["C"].shape
    C = _dev(g["C"])
    Q0 = p.forward_quant_mixed_multi(C, COLOR_STEPS, 3)
    flat = torch.zeros(N * D + 1, dtype=torch.float32, device="cuda")
    flat[1:] = C.reshape(-1)
    for a, b in zip(p.forward_quant_mixed_multi(flat[1:].view(N, D), COLOR_STEPS, 3), Q0):
        assert torch.equal(a, b)
    Cr0, sq0 = p.dequant_inverse_mixed_sqdiff(Q0[0], COLOR_STEPS[0], C, 3)
    big = torch.zeros((N, 64), dtype=torch.float32, device="cuda")
    big[:, :D] = C
    Cr1, sq1 = p.dequant_inverse_mixed_sqdiff(Q0[0], COLOR_STEPS[0], big[:, :D], 3)
    assert torch.equal(Cr1, Cr0) and torch.equal(sq1, sq0)
    _, sq2 = p.dequant_inverse_mixed_sqdiff(Q0[0], COLOR_STEPS[0], flat[1:].view(N, D), 3, want_rec=False)
    assert torch.equal(sq2, sq0)


def test_parseval_at_size(rt):
    """300 000 x 59 at step 0.02: the per-column distortion of the attribute columns is that of uniform quantization noise."""
    import torch
    D, nw, step = 59, 3, 0.02
    keys, C = _scene(11, 300000, 36, D)
    N = C.shape[0]
    p = rt.RahtPlan.from_keys(keys, 36)
    assert p.mixed_stats(D, nw)["tile_rows"] >= 64
    (Q,) = p.forward_quant_mixed_multi(C, [step], nw)
    _, sq = p.dequant_inverse_mixed_sqdiff(Q, step, C, nw, want_rec=False)
    ratio = (sq[nw:] / (N * step * step / 12.0)).mean().item()
    assert 0.5 <= ratio <= 1.5, ratio
    assert bool((sq >= 0).all())


def test_two_streams_from_the_first_call(rt):
    """A fresh plan with concurrent directions: multi for step s+1 on one stream and sqdiff for step s on another, from the very
    first call (the schedule and tile programs are built by whichever comes first); equal to a serial run."""
    import torch
    D, nw = 59, 3
    steps = COLOR_STEPS[:4]
    keys, C = _scene(33, 300000, 36, D)
    ref = rt.RahtPlan.from_keys(keys, 36)
    Qref = [ref.forward_quant_mixed(C, s, nw) for s in steps]
    SQref = [ref.dequant_inverse_mixed_sqdiff(Q, s, C, nw) for Q, s in zip(Qref, steps)]
    torch.cuda.synchronize()
    p = rt.RahtPlan.from_keys(keys, 36)
    p.set_concurrent_directions(True)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got_q, got_sq = [], []
    for i in range(len(steps) - 1):
        got_q.append(p.forward_quant_mixed_multi(C, [steps[i + 1]], nw)[0])
        with torch.cuda.stream(side):
            got_sq.append(p.dequant_inverse_mixed_sqdiff(Qref[i], steps[i], C, nw))
    torch.cuda.synchronize()
    for i in range(len(steps) - 1):
        assert torch.equal(got_q[i], Qref[i + 1]), i
        assert torch.equal(got_sq[i][0], SQref[i][0]) and torch.equal(got_sq[i][1], SQref[i][1]), i
