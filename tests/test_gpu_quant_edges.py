"""The quantizer's out-of-range rule (include/raht.h) on every device path that turns a coefficient into an integer,
bit for bit against tests/numpy_ops.quantize_model on the case matrix of tests/quant_edge_cases.py: quotients at, beside and far
beyond +-2^31, quotients that overflow the type, NaN, +-inf, signed zeros and the float32 round-to-even zone, at steps inside and
outside the fast divider's range.

r = floor(x / step + 0.5) in the matrix's own type is the result within [-2^31, 2^31 - 1]; above it (+inf included) the result is
INT32_MAX, below it (-inf included) INT32_MIN, and 0 when r is NaN.

The fused kernels are reached through the identity plan: keys 2 * arange(N) at 24 bits with top_level = 1 leave no butterfly, so
T == C and the kernels quantize exactly the values placed. The mixed entries send the roots of a truncated plan to root buffers
instead of quantizing them, so they run on a real tree (quant_edge_cases.mixed_frame) against the float64 transform."""
import numpy as np
import pytest

from . import numpy_rate
from . import quant_edge_cases as qe
from .numpy_ops import INT32_MAX, INT32_MIN, quantize_model

pytestmark = pytest.mark.gpu

ENGINES = [("tile", 0, 0, 0, 0), ("tile", 64, 64, 0, 64), ("tile", 128, 64, 8, 64), ("level", 0, 0, 0, 0)]
MIXED_GEOMS = [(0, 0, 0, 0), (64, 64, 0, 64)]                      # (tile rows, tail rows, tail channels, final rows)


@pytest.fixture(scope="module")
def rt():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    _lib.lib()                      # must load: no fallback
    return R


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(Q, want, M, what):
    """Q (device or numpy) == want, element for element; a failure names the first coefficients, what came and what was due"""
    got = Q.cpu().numpy() if hasattr(Q, "cpu") else np.asarray(Q)
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.dtype, got.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, f"{bad.size} of {want.size} differ", "x", np.asarray(M).ravel()[bad[:6]], "got", got.ravel()[bad[:6]],
                           "want", want.ravel()[bad[:6]])


def _identity_plan(rt, engine=ENGINES[0], n=qe.N):
    p = rt.RahtPlan.from_keys(_dev(qe.identity_keys(n)), 24, top_level=1)
    assert p.n_roots == n
    p.set_engine(*engine)
    return p


def _step_sets(dt, D):
    """(name, steps as the numpy array the model takes): per-channel inside the fast divider's range, per-channel with a step
    outside it, and two scalars (an ordinary one and an end of the range)"""
    t = qe.DTYPES[dt]
    return [("table", qe.step_vector(dt, D)), ("table_outside", qe.step_vector(dt, D, outside=True)),
            ("scalar", np.asarray([0.01], dtype=t)), ("scalar_end", np.asarray([2.0 ** -100], dtype=t))]


def _arg(st):
    """steps as the wrappers take them: a Python float for a scalar, a list for a table"""
    return float(st[0]) if st.shape[0] == 1 else [float(x) for x in st]


@pytest.mark.parametrize("D", qe.DS)
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_row_kernels(rt, dt, D):
    """quant_rows / quant_rows_f64 at identity and at permuted positions, quant_reorder and its float64 form through the order of
    a whole tree: the scalar row kernel (float64, float32 below one chunk) and the chunked kernel (float32, D >= 4)"""
    import torch
    from raht_3dgs_codec_amd import ops
    t = qe.DTYPES[dt]
    p = rt.RahtPlan.from_keys(_dev(qe.identity_keys()), 24)
    order = p.order_RAGFT.cpu().numpy()
    assert not np.array_equal(order, np.arange(qe.N))
    perm = np.random.default_rng(D).permutation(qe.N)
    rows = ops.quant_rows if dt == "f32" else ops.quant_rows_f64
    for name, st in _step_sets(dt, D):
        M = qe.case_matrix(dt, st, D)
        want = quantize_model(M, st, t)
        Md = _dev(M)
        Q = torch.full((qe.N, D), 12345, dtype=torch.int32, device="cuda")
        _same(rows(Md, _arg(st), torch.arange(qe.N, device="cuda"), Q), want, M, (name, "rows"))
        Q = torch.full((qe.N, D + 3), 12345, dtype=torch.int32, device="cuda")
        rows(Md, _arg(st), _dev(perm), Q[:, :D])
        got = Q.cpu().numpy()
        _same(got[perm, :D].copy(), want, M, (name, "rows at positions"))
        assert np.all(got[:, D:] == 12345)
        _same(p.quant_reorder(Md, _arg(st)), want[order], M[order], (name, "reorder"))


@pytest.mark.parametrize("engine", ENGINES, ids=lambda e: "-".join(str(x) for x in e))
@pytest.mark.parametrize("D", [3, 59])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_fused_forward(rt, dt, D, engine):
    """forward_quant in float32 and float64 on the identity plan: every engine geometry, scalar and per-channel steps, a
    contiguous and a strided input; and the fused call against the unfused one, inside and outside the fast divider's range"""
    import torch
    t = qe.DTYPES[dt]
    p = _identity_plan(rt, engine)
    order = p.order_RAGFT.cpu().numpy()
    for name, st in _step_sets(dt, D):
        M = qe.case_matrix(dt, st, D)
        want = quantize_model(M, st, t)[order]
        Md = _dev(M)
        Q = p.forward_quant(Md, _arg(st))
        _same(Q, want, M[order], (name, "fused"))
        assert torch.equal(Q, p.quant_reorder(Md, _arg(st))), (name, "fused against unfused")
        wide = torch.full((qe.N, D + 5), 1e30, dtype=Md.dtype, device="cuda")
        wide[:, :D] = Md
        view = wide[:, :D]
        assert view.stride(0) == D + 5
        _same(p.forward_quant(view, _arg(st)), want, M[order], (name, "fused, row stride D + 5"))


def test_multi_step_and_batch(rt):
    """forward_quant_multi at k = 3 scalar steps (the matrix is built for the first; the others scale every quotient by about 1e4
    and by 1 / 300) and forward_quant_batch over two identity plans of different sizes with a per-channel table"""
    from raht_3dgs_codec_amd import ops
    D = 59
    p = _identity_plan(rt)
    order = p.order_RAGFT.cpu().numpy()
    steps = [np.float32(0.01), np.float32(2.0 ** -20), np.float32(3.0)]
    M = qe.case_matrix("f32", np.asarray([steps[0]]), D)
    Qs = p.forward_quant_multi(_dev(M), [float(s) for s in steps])
    assert len(Qs) == 3
    for s, Q in zip(steps, Qs):
        _same(Q, quantize_model(M, s, np.float32)[order], M[order], ("multi", float(s)))
    n2 = 1500
    p2 = _identity_plan(rt, ENGINES[1], n2)
    for outside in (False, True):
        st = qe.step_vector("f32", D, outside)
        M1, M2 = qe.case_matrix("f32", st, D), qe.case_matrix("f32", st, D, n=n2)
        Q1, Q2 = ops.forward_quant_batch([p, p2], [_dev(M1), _dev(M2)], _arg(st))
        _same(Q1, quantize_model(M1, st, np.float32)[order], M1[order], ("batch", 0, outside))
        o2 = p2.order_RAGFT.cpu().numpy()
        _same(Q2, quantize_model(M2, st, np.float32)[o2], M2[o2], ("batch", 1, outside))


# ---- the mixed paths ---------------------------------------------------------------------------------------------------------
def _check_mixed(Q, T64, steps, what):
    """Q: one result of a mixed entry, rows in coded order; T64: the float64 transform, same rows. Saturated elements exactly;
    the band 2^30 <= |q| < 2^32 of the hot columns left out; everything else by the rule of tests/test_gpu_mixed.py: off by one at
    most, and only beside a tie of the model's quotient (wide columns: within 1e-9 relative, the float64 kernels' bar; the others:
    within 4e-6 of the column's largest quotient, the float32 bar). -> counts of saturated elements checked"""
    Q = Q.cpu().numpy()
    q = T64 / steps
    want = quantize_model(T64, steps, np.float64)
    sat, skip = qe.mixed_classes(q)
    assert skip.sum() <= 0.01 * qe.N * len(qe.MIXED_HOT), (what, int(skip.sum()))
    bad = np.flatnonzero(Q[sat] != np.where(q[sat] > 0, INT32_MAX, INT32_MIN))
    assert bad.size == 0, (what, "saturated", bad.size, q[sat][bad[:6]], Q[sat][bad[:6]])
    pre = q + 0.5
    scale = np.abs(T64).max(axis=0) / steps
    rest = ~(sat | skip)
    n_off = 0
    for r, c in np.argwhere(rest & (Q != want)):
        assert abs(int(Q[r, c]) - int(want[r, c])) == 1, (what, r, c, int(Q[r, c]), int(want[r, c]), q[r, c])
        tol = 1e-9 * max(1.0, abs(pre[r, c])) if c < qe.MIXED_WIDE else 4e-6 * max(scale[c], 1.0)
        assert abs(pre[r, c] - np.round(pre[r, c])) <= tol, (what, r, c, pre[r, c])
        n_off += 1
    w = slice(0, qe.MIXED_WIDE)
    n = slice(qe.MIXED_WIDE, None)
    counts = [int((sat[:, cols] & sgn(q[:, cols])).sum()) for cols in (w, n) for sgn in (lambda x: x > 0, lambda x: x < 0)]
    print(f"{what}: saturated checked (wide +, wide -, narrow +, narrow -) {counts}, left out {int(skip.sum())}, off by one beside a tie {n_off}")
    assert min(counts) >= 1000, (what, counts)


@pytest.fixture(scope="module")
def mixed_case(rt):
    """the frame, its plan's order and the float64 transform in coded order: computed once, left unchanged"""
    import torch
    keys, Cm, steps = qe.mixed_frame()
    p = rt.RahtPlan.from_keys(_dev(keys), 3 * qe.MIXED_J)
    order = p.order_RAGFT
    T64 = p.forward(_dev(Cm.astype(np.float64)), want_w=False)[order].cpu().numpy()
    assert torch.is_tensor(order)
    return keys, Cm, steps, T64


@pytest.mark.parametrize("geom", MIXED_GEOMS, ids=lambda g: "-".join(str(x) for x in g))
def test_mixed_paths(rt, mixed_case, geom):
    """forward_quant_mixed, forward_quant_mixed_multi and forward_quant_mixed_batch at D = 59, n_wide = 3 on a real tree of 4097
    keys at J = 10, so that tile stages, tail stages and the top stage all write quantized rows. (This frame's one hot element
    below 2^30 lies in a wide column; in a narrow hot column float32 could not meet the off-by-one rule, its transform being
    exact to about 1e-7 of 1e6 = 1e6 steps.)"""
    from raht_3dgs_codec_amd import ops
    keys, Cm, steps, T64 = mixed_case
    nw = qe.MIXED_WIDE
    p = rt.RahtPlan.from_keys(_dev(keys), 3 * qe.MIXED_J)
    p.set_engine("tile", *geom)
    Cd = _dev(Cm)
    st = [float(x) for x in steps]
    _check_mixed(p.forward_quant_mixed(Cd, st, nw), T64, steps, ("mixed", geom))
    # multi: k = 3 scalar steps, from the hot step down (quant_edge_cases.mixed_frame says why)
    Qs = p.forward_quant_mixed_multi(Cd, [f * qe.MIXED_HOT_STEP for f in qe.MIXED_SCALARS], nw)
    assert len(Qs) == 3
    for f, Q in zip(qe.MIXED_SCALARS, Qs):
        _check_mixed(Q, T64, np.full(qe.MIXED_D, f * qe.MIXED_HOT_STEP), ("mixed multi", geom, f))
    # batch: the frame twice, through two plans of different geometry
    p2 = rt.RahtPlan.from_keys(_dev(keys), 3 * qe.MIXED_J)
    p2.set_engine("tile", *MIXED_GEOMS[1 - MIXED_GEOMS.index(geom)])
    for i, Q in enumerate(ops.forward_quant_mixed_batch([p, p2], [Cd, Cd.clone()], st, nw)):
        _check_mixed(Q, T64, steps, ("mixed batch", geom, i))


# ---- the rate kernel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_rate_kernel(rt, dt):
    """raht_rlgr_seg_rate at seg_len = 64, k = 2 (the table the matrix is built for, and the same turned by one column): the sizes
    are the real encoder's on the model's integers, with every special value in; the squared errors, on the matrix with its
    non-finite coefficients (and, in float64, those whose square is no float64) set to zero, equal the float64 model
    sum((x - q * s)^2) with the saturated q, under the bound of tests/test_gpu_rate.py (the same rounded double operations on both
    sides, sums that differ by the order of at most N additions: rtol = 1e-10)."""
    import torch
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    t, D, S = qe.DTYPES[dt], 7, 64
    st0 = qe.step_vector(dt, D)
    tables = [st0, np.roll(st0, 1)]
    M = qe.case_matrix(dt, st0, D)
    F = np.where(np.isfinite(M) & (np.abs(M.astype(np.float64)) < 1e150), M, t(0))
    for X, want_sse in ((M, False), (F, True)):
        cb, sb, sse = SegmentedCoder.rate(_dev(X), [_arg(s) for s in tables], S, 1, want_sse=want_sse)
        for j, st in enumerate(tables):
            q = quantize_model(X, st, t)
            sc = SegmentedCoder(qe.N, D, S, 1, "cuda")
            sc.encode(_dev(q))
            assert torch.equal(sb[j], sc.seg_bytes.to(sb.dtype)), (dt, j, want_sse)
            assert int(cb[j]) == sc.size_bytes
            if want_sse:
                want = numpy_rate.sse(X, q, st)
                assert np.all(np.isfinite(want)) and (q == INT32_MAX).any() and (q == INT32_MIN).any()
                got = sse[j].cpu().numpy()
                print(f"{dt} table {j}: max relative difference {(np.abs(got - want) / np.maximum(want, 1e-300)).max():.3e}")
                np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)


# ---- the decode side -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", [ENGINES[0], ENGINES[1]], ids=lambda e: "-".join(str(x) for x in e))
def test_dequant_inverse_sqdiff_of_the_models_integers(rt, engine):
    """dequant_inverse_sqdiff on the identity plan with the model's integers, both limits among them: the reconstruction is
    q * s in float32 bit for bit, and the sums of squares agree with the float64 model of the float32 differences under the
    bound of test_dequant_inverse_sqdiff_equals_the_two_passes (rtol 1e-9). The reference matrix is the case matrix with its
    non-finite coefficients set to zero, so that every difference is a number."""
    import torch
    D = 59
    p = _identity_plan(rt, engine)
    order = p.order_RAGFT.cpu().numpy()
    for name, st in _step_sets("f32", D)[:3:2]:                     # the table inside the range, the scalar 0.01
        M = qe.case_matrix("f32", st, D)
        q = quantize_model(M, st, np.float32)
        assert (q == INT32_MAX).any() and (q == INT32_MIN).any()
        F = np.where(np.isfinite(M), M, np.float32(0))
        with np.errstate(over="ignore"):
            want = q.astype(np.float32) * np.broadcast_to(st, (D,)).astype(np.float32)
            dif = (want - F).astype(np.float64)                     # (differences in float32 first, as the kernel forms them)
            ssd_want = (dif * dif).sum(axis=0)
        rec, ssd = p.dequant_inverse_sqdiff(_dev(q[order]), _arg(st), _dev(F))
        assert np.array_equal(rec.cpu().numpy().view(np.int32), want.view(np.int32)), name
        assert torch.equal(rec, p.dequant_inverse(_dev(q[order]), _arg(st)))
        got = ssd.cpu().numpy()
        fin = np.isfinite(ssd_want)
        assert fin.sum() >= D // 2 or st.shape[0] == 1, (name, int(fin.sum()))
        assert np.array_equal(np.isfinite(got), fin), name           # (q * 2^100 overflows float32: an infinite sum on both sides)
        np.testing.assert_allclose(got[fin], ssd_want[fin], rtol=1e-9, atol=1e-300)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
E2E_J, E2E_D, E2E_STEP = 10, 6, 0.01


def _e2e_frames():
    """two frames of 4097 voxels, D = 6, whose column 0 has the mean 1e6: its DC coefficient is 1e6 * sqrt(4097) = 6.4e7, 6.4e9
    steps of 0.01 -- three times 2^31. The second frame is the first with seeded noise."""
    from raht_3dgs_codec_amd import synth
    rng = np.random.default_rng(4097)
    V = np.unique(rng.integers(0, 1 << E2E_J, size=(2 * qe.N, 3), dtype=np.int64), axis=0)
    V = V[rng.permutation(V.shape[0])[:qe.N]]
    V = V[np.argsort(synth.morton_keys(V, E2E_J), kind="stable")]
    A = rng.normal(size=(qe.N, E2E_D)).astype(np.float32)
    A[:, 0] += np.float32(1e6)
    B = (A + 0.05 * rng.normal(size=A.shape)).astype(np.float32)
    return [(V, A), (V, B)]


def test_a_frame_with_a_saturated_dc_term_decodes_to_the_models_integers(rt):
    import torch
    from raht_3dgs_codec_amd import bitstream, ops
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    V, A = _e2e_frames()[0]
    blob = bitstream.encode_frame_bytes(V, A, E2E_J, E2E_STEP, "cuda", seg_len=256)
    keys = ops.get_morton_code(_dev(V), E2E_J)
    p = ops.RahtPlan.from_keys(keys, 3 * E2E_J)
    T = p.forward(_dev(A), want_w=False)[p.order_RAGFT].cpu().numpy()
    q = quantize_model(T, np.float32(E2E_STEP), np.float32)
    assert q[0, 0] == INT32_MAX and float(T[0, 0]) / E2E_STEP > 2.0 ** 32          # the DC term, first in coded order
    assert np.abs(q[1:].astype(np.int64)).max() < 2 ** 30
    h = bitstream.parse_frame(blob)
    ao, al = h["attributes"]
    coded = SegmentedCoder.from_container(blob[ao: ao + al], "cuda").decode(row_major=True)
    _same(coded, q, T, "the integers in the frame's bytes")
    Vd, C = bitstream.decode_frame_bytes(blob, "cuda")
    assert np.array_equal(Vd.cpu().numpy(), V)
    assert torch.equal(C.view(torch.int32), p.dequant_inverse(_dev(q), E2E_STEP).view(torch.int32))
    # what the saturation costs: column 0 comes back with the mean INT32_MAX * step / sqrt(N) instead of 1e6 -- silently
    assert abs(float(C[:, 0].double().mean()) - INT32_MAX * E2E_STEP / qe.N ** 0.5) < 1.0


def test_a_p_frame_with_a_saturated_dc_term_keeps_the_loop_closed(rt):
    """the frame as the P frame of a two-frame sequence: its residual against the (saturated) reconstruction of frame 0 has a DC
    term beyond 2^31 steps again; the encoder's recurrence with public calls (tests/test_gpu_sequence_inter.py) ends on the
    decoder's bits"""
    import torch
    from raht_3dgs_codec_amd import bitstream, ops
    frames = _e2e_frames()
    blob = bitstream.encode_sequence_bytes(frames, E2E_J, E2E_STEP, "cuda", seg_len=256, gop=2, up=0, inter="always")
    assert bitstream.sequence_kinds(blob) == ["I", "P"]
    dec = bitstream.decode_sequence_bytes(blob, device="cuda")
    ref, n_sat = None, []
    for V, A in frames:
        keys = ops.get_morton_code(_dev(V), E2E_J)
        plan = ops.RahtPlan.from_keys(keys, 3 * E2E_J)
        X = _dev(A)
        if ref is not None:
            X = ops.predict(keys, ref[0], ref[1], X=X, up=0)
        Q = plan.forward_quant(X, [E2E_STEP])
        n_sat.append(int((Q == INT32_MAX).sum()))
        C = plan.dequant_inverse(Q, [E2E_STEP])
        if ref is not None:
            C = ops.predict(keys, ref[0], ref[1], X=C, up=0, add=True)
        ref = (keys, C)
    assert n_sat == [1, 1], n_sat
    assert torch.equal(ref[1].view(torch.int32), dec[-1][1].view(torch.int32))
