"""raht_plan_create (csrc/plan.hip, keys_from_coords_kernel<VT>) through RahtPlan.from_coords / RAHT_param_reorder_fast on the
MI355X, over the case table of tests/plan_coord_cases.py: all four element types, origins that are not zero, widths that are no
power of two, points on and next to voxel faces, 256-thread block edges, depth 21 (63-bit keys) built and transformed, every
refused row with its code and row, and the wrapper's argument handling. tests/test_plan_coords_model.py holds the CPU twin and
the oracle to the same table and to the fixtures from the reference (tests/golden/coords/).

Bars, copied from tests/test_gpu_parity.py and not loosened: integers bit for bit; float64 rtol = atol = 1e-12, the absolute
part scaled by the column's magnitude; float32 ``_check_f32`` (2e-6 of the column max, 1e-6 of its rms) and a 1e-5 round trip;
quantized integers differ from the reference's by +-1 only, and only next to a rounding tie."""
import re

import numpy as np
import pytest

from . import plan_coord_cases as pc
from .test_gpu_parity import _check_f32, _dev, rt  # noqa: F401  (rt: the fixture that loads the package and its library)
from .test_plan_coords_model import check_lists, f64_bar, load_coords

pytestmark = pytest.mark.gpu

ENGINES = [("tile", 0, 0, 0, 0), ("tile", 64, 64, 0, 64), ("level", 0, 0, 0, 0)]     # default tiles, one small-tile geometry of test_gpu_parity.ENGINES, levels
_REF = {}


def _reference(oracle, case):
    """(C, T, w, the oracle's lists, the fixture or None) of a case, computed once and shared: T and w are the reference's own where
    there is a fixture, the oracle's otherwise"""
    if case.name not in _REF:
        po = oracle.raht_param(case.V.astype(np.float64), case.minV, case.width, case.J, ref_quirks=False)
        if case.fixture:
            g = load_coords(case)
            C, T, w = g["C"], g["T"], g["w"]
        else:
            g = None
            # (float64 columns holding float32 values, as in the fixtures: the float32 kernels then see the same input)
            C = np.random.default_rng(case.V.shape[0] * 1000 + case.J).standard_normal((case.V.shape[0], 3)).astype(np.float32).astype(np.float64)
            T, w = oracle.raht_fwd(C, po)
            w = w.reshape(-1)
        _REF[case.name] = (C, T, w, po, g)
    return _REF[case.name]


def _plan(R, V, minV, width, J):
    return R.RahtPlan.from_coords(_dev(V), list(minV), width, J)


def _same_plan(p, q):
    assert p.N == q.N and p.nbits == q.nbits and p.levels == q.levels
    for a, b, what in zip(p.arrays(), q.arrays(), ("keys", "lvl", "wl", "wr")):
        assert a.dtype == b.dtype and np.array_equal(a, b), what
    assert np.array_equal(p.order_RAGFT.cpu().numpy(), q.order_RAGFT.cpu().numpy())


def _check_lists_against(p, po, g):
    List, Flags, weights = (([t.numpy() for t in x]) for x in p.export_lists())
    order = p.order_RAGFT.cpu().numpy()
    assert len(List) == po.nlevels
    for l in range(po.nlevels):
        assert np.array_equal(List[l], po.List[l]) and np.array_equal(Flags[l], po.Flags[l]) and np.array_equal(weights[l], po.weights[l]), l
    assert np.array_equal(order, po.order)
    if g is not None:
        assert check_lists(List, Flags, weights, order, g)


def _check_transforms(p, C, T, w):
    """forward and inverse in float64 at the 1e-12 bar, in float32 at _check_f32's bars and the 1e-5 round trip"""
    Td, wd = p.forward(_dev(C))
    assert f64_bar(Td.cpu().numpy(), T)
    assert np.array_equal(wd.cpu().numpy().reshape(-1), w)
    np.testing.assert_allclose(p.inverse(Td).cpu().numpy(), C, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(C).max())))
    C32 = C.astype(np.float32)
    assert np.array_equal(C32.astype(np.float64), C)
    T32, w32 = p.forward(_dev(C32))
    _check_f32(T32.cpu().numpy(), T, "forward f32")
    assert np.array_equal(w32.cpu().numpy().reshape(-1).astype(np.float64), w)
    cmax = max(float(np.abs(C).max()), 1e-30)
    assert np.abs(p.inverse(T32).cpu().numpy() - C32).max() <= 1e-5 * cmax
    assert np.abs(p.inverse(_dev(T.astype(np.float32))).cpu().numpy() - C).max() <= 1e-5 * cmax      # the decoder side on its own


# --------------------------------------------------------------------------------------------------- accepted clouds
@pytest.mark.parametrize("name,dt", [(c.name, dt) for c in pc.ACCEPTED for dt in c.dtypes])
def test_accepted_cloud_builds_the_model_plan(rt, oracle, name, dt):
    case = pc.BY_NAME[name]
    C, T, w, po, g = _reference(oracle, case)
    p = _plan(rt, case.cast(dt), case.minV, case.width, case.J)
    keys = p.arrays()[0]
    assert keys.dtype == np.uint64 and np.array_equal(keys, case.model()[2])
    _check_lists_against(p, po, g)
    _check_transforms(p, C, T, w)


def test_element_types_build_identical_plans(rt):
    """an integer-valued cloud as float32, float64, int32 and int64: identical keys, lvl, wl, wr and order, identical to the plan
    from its Morton keys; the same under the shifted origin"""
    J = 10
    V = pc.integer_cloud(J)
    key = pc.model_keys(V, (0, 0, 0), 2.0 ** J, J)[2]
    ref = rt.RahtPlan.from_keys(_dev(key.view(np.int64)), 3 * J)
    assert np.array_equal(ref.arrays()[0], key)
    for dt in pc.ALL:
        _same_plan(_plan(rt, V.astype(pc.DTYPES[dt]), (0.0, 0.0, 0.0), 2.0 ** J, J), ref)
    case = pc.BY_NAME["shift_int_n1025"]
    ref = rt.RahtPlan.from_keys(_dev(case.model()[2].view(np.int64)), 3 * case.J)
    for dt in pc.ALL:
        _same_plan(_plan(rt, case.cast(dt), case.minV, case.width, case.J), ref)


# --------------------------------------------------------------------------------------------------- refused rows
def _refusal(R, V, minV, width, J):
    with pytest.raises(R.RahtError) as e:
        _plan(R, V, minV, width, J)
    m = re.search(r"row (\d+)", str(e.value))
    return e.value.code, (int(m.group(1)) if m else None), str(e.value)


@pytest.mark.parametrize("name,dt", pc.REFUSED)
def test_refused_row_is_reported_with_the_bounds_code(rt, name, dt):
    """one bad row on every axis in turn, as row 0, as the last row and alone: RAHT_ERR_BOUNDS, and the row named is the one
    that is out of bounds in the model. Non-finite coordinates are refused like any other (a NaN converted to voxel 0 before the
    real value was tested)."""
    for label, V, minV, width, J, row in pc.refused_clouds(name, dt):
        code, named, text = _refusal(rt, V, minV, width, J)
        assert code == pc.RAHT_ERR_BOUNDS, (label, text)
        assert named == row, (label, text)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_two_bad_rows_one_of_them_is_named(rt, dt):
    cfg = pc.CONFIGS["shift"]
    V = cfg.V.astype(pc.DTYPES[dt])
    V[0, 2] = np.nan
    V[170, 0] = np.inf
    V[299, 1] = cfg.minV[1] - 0.5
    bad = np.flatnonzero(pc.model_keys(V, cfg.minV, cfg.width, cfg.J)[1])
    assert bad.tolist() == [0, 170, 299]
    code, named, text = _refusal(rt, V, cfg.minV, cfg.width, cfg.J)
    assert code == pc.RAHT_ERR_BOUNDS and named in bad, text
    code, named, text = _refusal(rt, V[100:], cfg.minV, cfg.width, cfg.J)
    assert code == pc.RAHT_ERR_BOUNDS and named in (70, 199), text


def test_rows_at_the_edge_are_accepted(rt):
    clouds = pc.must_accept_clouds()
    assert len(clouds) >= 24
    for label, dt, V, minV, width, J in clouds:
        p = _plan(rt, V, minV, width, J)
        assert np.array_equal(p.arrays()[0], pc.model_keys(V, minV, width, J)[2]), label


# --------------------------------------------------------------------------------------------------- depth 21
def test_depth_21_from_coords_equals_from_keys(rt, oracle):
    case = pc.DEEP
    C, T, w, po, g = _reference(oracle, case)
    key = case.model()[2]
    assert int(key[-1]) == 2 ** 63 - 1
    ref = rt.RahtPlan.from_keys(_dev(key.view(np.int64)), 63)
    assert np.array_equal(ref.arrays()[0], key) and ref.levels == 63
    _check_lists_against(ref, po, g)
    for dt in case.dtypes:
        p = _plan(rt, case.cast(dt), case.minV, case.width, case.J)
        _same_plan(p, ref)
        _check_lists_against(p, po, g)


def _quant_check(Q, T, order, step, tie):
    """the integers are floor(T / step + 0.5) of the reference coefficients in coded order; a mismatch is +-1 and sits within
    ``tie`` of a rounding tie of the reference value"""
    pre = T[order] / step + 0.5
    ref = np.floor(pre).astype(np.int64)
    bad = np.argwhere(Q != ref)
    for r, c in bad:
        assert abs(int(Q[r, c]) - int(ref[r, c])) == 1
        assert abs(pre[r, c] - np.round(pre[r, c])) <= tie(pre[r, c], c), (r, c)
    return ref


@pytest.mark.parametrize("eng", ENGINES)
def test_depth_21_transforms(rt, oracle, eng):
    """63-bit keys, binary levels up to 62 and the top order bucket through the tile engine (default and small tiles) and the level
    engine: forward / inverse in float64 and float32 against the oracle (and the reference's own coefficients), one fused
    quantize / dequantize pair in each precision"""
    import torch
    case = pc.DEEP
    C, T, w, po, g = _reference(oracle, case)
    To, wo = oracle.raht_fwd(C, po)
    assert f64_bar(To, T)                                            # (T is the reference's, To the oracle's)
    order = po.order
    for dt in ("i64", "f64"):
        p = _plan(rt, case.cast(dt), case.minV, case.width, case.J)
        p.set_engine(*eng)
        _check_transforms(p, C, To, wo.reshape(-1))
        _check_transforms(p, C, T, w)
    step = 0.37
    scale = np.abs(To).max(axis=0) / step
    # float64: equal except on (near-)exact ties (tests/test_cpu_twins.py: 1e-9 of the quotient)
    Q64 = p.forward_quant(_dev(C), step).cpu().numpy()
    ref = _quant_check(Q64, To, order, step, lambda q, c: 1e-9 * max(1.0, abs(q)))
    # float32: the coefficient error (<= 2e-6 of the column max) can only flip values that close to a tie (test_quantize_reorder_and_back)
    Q32 = p.forward_quant(_dev(C.astype(np.float32)), step).cpu().numpy()
    _quant_check(Q32, To, order, step, lambda q, c: 4e-6 * max(scale[c], 1.0))
    # the decoder side from the reference integers
    Td = np.empty_like(To)
    Td[order] = ref.astype(np.float64) * step
    rec = oracle.raht_inv(Td, po)
    R64 = p.dequant_inverse(_dev(ref.astype(np.int32)), step, dtype=torch.float64).cpu().numpy()
    np.testing.assert_allclose(R64, rec, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(rec).max())))
    R32 = p.dequant_inverse(_dev(ref.astype(np.int32)), step).cpu().numpy()
    assert np.abs(R32 - rec).max() <= 1e-5 * max(float(np.abs(rec).max()), 1.0)


# --------------------------------------------------------------------------------------------------- the wrapper
def test_noncontiguous_coordinates_give_the_plan_of_the_copy(rt):
    import torch
    case = pc.BY_NAME["w3_j10_border_f64"]
    N = case.V.shape[0]
    ref = _plan(rt, case.V, case.minV, case.width, case.J)
    wide = torch.full((N, 7), float("nan"), dtype=torch.float64, device="cuda")
    wide[:, 2:5] = _dev(case.V)
    view = wide[:, 2:5]
    assert not view.is_contiguous()
    _same_plan(rt.RahtPlan.from_coords(view, case.minV, case.width, case.J), ref)
    tr = _dev(np.ascontiguousarray(case.V.T)).t()                    # (3, N) storage seen as (N, 3)
    assert tuple(tr.shape) == (N, 3) and not tr.is_contiguous()
    _same_plan(rt.RahtPlan.from_coords(tr, case.minV, case.width, case.J), ref)
    for V in (view, tr):
        ListC, FlagsC, weightsC, order = rt.RAHT_param_reorder_fast(V, torch.tensor(case.minV, dtype=torch.float64), case.width, case.J)
        _same_plan(rt.plan_of(ListC), ref)
        assert torch.equal(order, ref.order_RAGFT)


def test_other_element_types_take_the_float64_path(rt):
    import torch
    J, minV = 8, (0.0, -0.5, -0.25)
    rng = np.random.default_rng(8)
    V = pc.sort_unique(rng.integers(0, 256, size=(900, 3)).astype(np.int64), minV, 256.0, J)
    assert V.shape[0] > 800
    ref = _plan(rt, V.astype(np.float64), minV, 256.0, J)
    assert np.array_equal(ref.arrays()[0], pc.model_keys(V, minV, 256.0, J)[2])
    for tdt in (torch.float16, torch.int16, torch.uint8, torch.bfloat16):
        t = _dev(V).to(tdt)
        assert torch.equal(t.to(torch.int64), _dev(V))              # the type holds every value
        _same_plan(rt.RahtPlan.from_coords(t, minV, 256.0, J), ref)


def test_origin_in_every_form_gives_the_same_plan(rt):
    import torch
    case = pc.BY_NAME["shift_int_n257"]
    V = _dev(case.cast("f32"))
    ref = rt.RahtPlan.from_coords(V, list(case.minV), case.width, case.J)
    assert np.array_equal(ref.arrays()[0], case.model()[2])
    for minV in (tuple(case.minV), torch.tensor(case.minV, dtype=torch.float32), torch.tensor(case.minV, dtype=torch.float64, device="cuda"),
                 np.asarray(case.minV)):
        _same_plan(rt.RahtPlan.from_coords(V, minV, case.width, case.J), ref)
        _same_plan(rt.plan_of(rt.RAHT_param_reorder_fast(V, minV, case.width, case.J)[0]), ref)


def test_wrong_shapes_and_cpu_coordinates_raise(rt):
    import torch
    case = pc.BY_NAME["shift_int_n257"]
    V = _dev(case.cast("f64"))
    for fn in (rt.RahtPlan.from_coords, rt.RAHT_param_reorder_fast):
        with pytest.raises(ValueError):
            fn(V[:, :2], list(case.minV), case.width, case.J)
        with pytest.raises(ValueError):
            fn(V[:, 0], list(case.minV), case.width, case.J)
        with pytest.raises(ValueError):
            fn(V.t(), list(case.minV), case.width, case.J)
        with pytest.raises(ValueError):
            fn(V, list(case.minV)[:2], case.width, case.J)
        with pytest.raises(ValueError):
            fn(V, torch.zeros(4), case.width, case.J)
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(V.cpu(), list(case.minV), case.width, case.J)
        with pytest.raises(RuntimeError, match="CUDA"):
            fn(case.cast("f64"), list(case.minV), case.width, case.J)    # a numpy array is no device tensor either
