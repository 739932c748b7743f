"""The quantizer's out-of-range rule (include/raht.h) on the host: the model every test compares against
(tests/numpy_ops.quantize_model) against hand-derived expectations, then the host twins, the oracle's quantizer and the package's
torch conversion helper against the model, bit for bit, on the case matrix of tests/quant_edge_cases.py.

r = floor(x / step + 0.5) in the matrix's own type is the result within [-2^31, 2^31 - 1]; above it (+inf included) the result is
INT32_MAX, below it (-inf included) INT32_MIN, and 0 when r is NaN."""
import ctypes as C

import numpy as np
import pytest

from . import quant_edge_cases as qe
from .numpy_ops import INT32_MAX, INT32_MIN, quantize_model

NAN, INF = float("nan"), float("inf")
# (dtype, x / s, expected), each derived by hand:
TABLE = [
    ("f32", 2147483520.0, 2147483520),          # 2^31 - 128, the largest float32 below 2^31: + 0.5f rounds back to itself
    ("f32", 2147483648.0, INT32_MAX),           # 2^31 > INT32_MAX
    ("f32", -2147483648.0, INT32_MIN),          # -2^31 is in range: itself
    ("f32", -2147483904.0, INT32_MIN),          # -2^31 - 256, the next float32 below: saturated
    ("f32", 8388609.0, 8388610),                # 2^23 + 1: + 0.5f is a tie between 2^23 + 1 and 2^23 + 2, to even
    ("f32", 8388610.0, 8388610),                # ... and its even neighbour stays
    ("f32", 4194305.0, 4194305),                # 2^22 + 1: 2^22 + 1.5 is representable, floor takes it back
    ("f64", 2147483647.4, 2147483647),          # floor(2147483647.9) = INT32_MAX, in range
    ("f64", 2147483647.5, INT32_MAX),           # floor(2147483648.0) = 2^31: saturated (same integer, by the other arm)
    ("f64", -2147483648.5, INT32_MIN),          # floor(-2147483648.0) = -2^31: in range, not saturated
    ("f64", -2147483649.5, INT32_MIN),          # floor(-2147483649.0): saturated
    ("f64", 8388609.0, 8388609),                # float64 has no round-to-even zone here
    ("f64", 4294967296.0, INT32_MAX), ("f64", -4294967296.0, INT32_MIN),
    ("f32", 4294967296.0, INT32_MAX), ("f32", -4294967296.0, INT32_MIN),
    ("f32", 1e30, INT32_MAX), ("f64", -1e300, INT32_MIN),
]
TABLE += [(dt, v, e) for dt in ("f32", "f64") for v, e in ((NAN, 0), (INF, INT32_MAX), (-INF, INT32_MIN), (0.0, 0), (-0.0, 0), (0.49, 0),
                                                           (0.5, 1), (-0.5, 0), (-0.51, -1))]


@pytest.mark.parametrize("dt,q,want", TABLE)
def test_model_table(dt, q, want):
    t = qe.DTYPES[dt]
    got = quantize_model(np.asarray([q], dtype=t), t(1.0), t)
    assert got.dtype == np.int32 and int(got[0]) == want
    # the same quotient through a step that is a power of two (exact in both directions)
    got = quantize_model(np.asarray([q], dtype=t) * t(2.0 ** -20), t(2.0 ** -20), t)
    assert int(got[0]) == want


def test_model_overflowing_quotient_and_in_range_identity():
    for t in (np.float32, np.float64):
        big = np.asarray([np.finfo(t).max, -np.finfo(t).max], dtype=t)
        assert quantize_model(big, t(0.01), t).tolist() == [INT32_MAX, INT32_MIN]          # x / s = +-inf in t
        rng = np.random.default_rng(5)
        x = (rng.normal(size=20000) * 1e4).astype(t)
        s = t(0.01)
        assert np.array_equal(quantize_model(x, s, t), np.floor(x / s + t(0.5)).astype(np.int32))   # in range: today's arithmetic
    # float32 arithmetic is float32 arithmetic: 2^24 + 1 is not a float32, the model refuses to round the coefficients silently
    with pytest.raises(AssertionError):
        quantize_model(np.asarray([1.0], dtype=np.float64), 1.0, np.float32)


def test_case_matrix_covers_every_target_in_every_column():
    tg = qe.targets()
    assert np.gcd(len(tg), 7) == 1 and len(tg) <= qe.N
    for dt in ("f32", "f64"):
        st = qe.step_vector(dt, 59)
        X, M = qe.coefficients(dt, st), qe.case_matrix(dt, st, 59)
        assert M.shape == (qe.N, 59) and M.dtype == qe.DTYPES[dt]
        for c in (0, 1, 2, 3, 56, 57, 58):                        # every lane of a chunk, the ragged last chunk
            col = M[:len(tg), c]
            assert np.array_equal(np.sort(col.view(np.uint64 if dt == "f64" else np.uint32)),
                                  np.sort(X[:, c].view(np.uint64 if dt == "f64" else np.uint32)))
        q = quantize_model(M, st, qe.DTYPES[dt]).astype(np.int64)
        assert (q == INT32_MAX).sum() > 1000 and (q == INT32_MIN).sum() > 1000 and np.isnan(M).sum() > 1000
        assert ((q > 2 ** 22) & (q < 2 ** 26)).sum() > 1000


def test_mixed_frame_saturates_in_both_signs_and_leaves_little_out():
    """what tests/test_gpu_quant_edges.py relies on for the mixed paths, from the float64 model alone: at most 1 % of the hot
    columns' elements fall into the band that is left out (a two-sided normal gives about 3e-4), and at least 1000 elements
    saturate in each sign, in the wide and in the narrow hot columns"""
    import torch
    from .numpy_ops import NumpyPlan
    keys, Cm, steps = qe.mixed_frame()
    p = NumpyPlan(torch.from_numpy(keys), 3 * qe.MIXED_J)
    T = p.forward(torch.from_numpy(Cm.astype(np.float64))).numpy()
    n_hot = qe.N * len(qe.MIXED_HOT)
    narrow_hot = [c for c in qe.MIXED_HOT if c >= qe.MIXED_WIDE]
    for st in [steps] + [np.full(qe.MIXED_D, f * qe.MIXED_HOT_STEP) for f in qe.MIXED_SCALARS]:
        q = T / st
        sat, skip = qe.mixed_classes(q)
        below = np.abs(q[:, list(qe.MIXED_HOT)]) < 2.0 ** 30
        print(f"left out: {int(skip.sum())} of {n_hot} hot elements; in range below 2^30: {int(below.sum())}")
        assert skip.sum() <= 0.01 * n_hot
        for cols in (slice(0, qe.MIXED_WIDE), slice(qe.MIXED_WIDE, None)):
            assert (sat[:, cols] & (q[:, cols] > 0)).sum() >= 1000 and (sat[:, cols] & (q[:, cols] < 0)).sum() >= 1000
        want = quantize_model(T, st, np.float64)
        assert np.array_equal(want[sat], np.where(q[sat] > 0, INT32_MAX, INT32_MIN))
        # a hot element below 2^30 is held to the off-by-one rule on the GPU, which float32 cannot meet at 1e13 steps per unit:
        # this frame has one such element, in a wide column (a frame from another seed may need the rule stated for them)
        assert not (np.abs(q[:, narrow_hot]) < 2.0 ** 30).any()


# ---- host twins ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twins(oracle):
    L = C.CDLL(oracle.CPU_TWINS_SO)
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    L.raht_cpu_last_error.restype = C.c_char_p
    L.raht_cpu_plan_create_from_keys.argtypes = [vp, i64, i32, vp, vp, C.POINTER(vp)]
    L.raht_cpu_plan_destroy.argtypes = [vp]
    L.raht_cpu_plan_order.argtypes = [vp, vp, vp]
    for n in ("quant_reorder", "quant_reorder_f64", "fwd_quant", "fwd_quant_f64"):
        getattr(L, "raht_cpu_" + n).argtypes = [vp, vp, i64, i32, vp, i32, vp, i64, vp]
    return L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _twin_plan(L, keys):
    h = C.c_void_p()
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    assert L.raht_cpu_plan_create_from_keys(_ptr(k), k.shape[0], 24, None, None, C.byref(h)) == 0, L.raht_cpu_last_error()
    order = np.empty(k.shape[0], dtype=np.int64)
    assert L.raht_cpu_plan_order(h, _ptr(order), None) == 0
    return h, order


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("outside", [False, True])
def test_twin_quant_reorder_follows_the_rule(twins, dt, outside):
    """raht_cpu_quant_reorder / _f64 quantize the matrix they are given: every row of the case matrix, through the order of a
    whole tree, with per-channel and scalar steps"""
    t, D = qe.DTYPES[dt], 59
    h, order = _twin_plan(twins, qe.identity_keys())
    fn = twins.raht_cpu_quant_reorder if dt == "f32" else twins.raht_cpu_quant_reorder_f64
    for st in (qe.step_vector(dt, D, outside), np.asarray([0.01], dtype=t), np.asarray([2.0 ** -100], dtype=t)):
        M = qe.case_matrix(dt, st, D)
        Q = np.full((qe.N, D), 12345, dtype=np.int32)
        assert fn(h, _ptr(M), D, D, _ptr(st), st.shape[0], _ptr(Q), D, None) == 0, twins.raht_cpu_last_error()
        want = quantize_model(M, st, t)[order]
        bad = np.flatnonzero(Q != want)
        assert bad.size == 0, (bad.size, M[order].ravel()[bad[:5]], Q.ravel()[bad[:5]], want.ravel()[bad[:5]])
    twins.raht_cpu_plan_destroy(h)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_twin_fwd_quant_follows_the_rule(twins, dt):
    """raht_cpu_fwd_quant / _f64 transform first, and the twins have no truncated plans: their identity plan is the plan of ONE
    point, whose transform is the identity. The case matrix goes through it as one row of N * D channels with per-channel steps."""
    t, D = qe.DTYPES[dt], 59
    h, order = _twin_plan(twins, np.zeros(1))
    assert order.tolist() == [0]
    fn = twins.raht_cpu_fwd_quant if dt == "f32" else twins.raht_cpu_fwd_quant_f64
    st = qe.step_vector(dt, D, outside=True)
    M = qe.case_matrix(dt, st, D)
    wide, steps = np.ascontiguousarray(M.reshape(1, -1)), np.ascontiguousarray(np.tile(st, qe.N))
    Q = np.full(wide.shape, 12345, dtype=np.int32)
    assert fn(h, _ptr(wide), wide.shape[1], wide.shape[1], _ptr(steps), steps.shape[0], _ptr(Q), wide.shape[1], None) == 0, twins.raht_cpu_last_error()
    want = quantize_model(M, st, t)
    bad = np.flatnonzero(Q.reshape(M.shape) != want)
    assert bad.size == 0, (bad.size, M.ravel()[bad[:5]], Q.ravel()[bad[:5]], want.ravel()[bad[:5]])
    twins.raht_cpu_plan_destroy(h)


def test_oracle_quantizer_follows_the_rule(oracle):
    """orc_quant_reorder: float64, one step per call"""
    rng = np.random.default_rng(9)
    order = rng.permutation(qe.N)
    for s in qe.STEPS_INSIDE + (qe.STEP_OUTSIDE,):
        M = qe.case_matrix("f64", np.float64(s), 7)
        Q = oracle.quant_reorder(M, s, order)
        want = quantize_model(M, np.float64(s), np.float64)[order]
        bad = np.flatnonzero(Q != want)
        assert bad.size == 0, (s, bad.size, M[order].ravel()[bad[:5]], Q.ravel()[bad[:5]], want.ravel()[bad[:5]])


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_torch_conversion_helper_follows_the_rule(dt):
    """ops.to_int32, which the unfused drivers convert with (pipeline.py), on CPU tensors: floor(x / s + 0.5) as torch forms
    it, then the helper"""
    import torch
    from raht_3dgs_codec_amd.ops import to_int32
    t = qe.DTYPES[dt]
    st = qe.step_vector(dt, 59, outside=True)
    M = qe.case_matrix(dt, st, 59)
    R = torch.floor(torch.from_numpy(M) / torch.from_numpy(st) + 0.5)
    assert R.dtype == torch.from_numpy(M).dtype
    keep = R.clone()
    Q = to_int32(R)
    assert Q.dtype == torch.int32 and torch.equal(R.nan_to_num(7.0), keep.nan_to_num(7.0))          # (the argument is left alone)
    want = quantize_model(M, st, t)
    bad = np.flatnonzero(Q.numpy() != want)
    assert bad.size == 0, (bad.size, M.ravel()[bad[:5]], Q.numpy().ravel()[bad[:5]], want.ravel()[bad[:5]])
