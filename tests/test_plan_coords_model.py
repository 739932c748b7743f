"""Plan construction from coordinates, on the CPU: the numpy model of tests/plan_coord_cases.py, the oracle and the host twin
raht_cpu_plan_create against the fixtures recorded from the reference (tests/golden/coords/, written by gen_golden.py's
coord_cases) and against each other, over the whole case table -- every element type, shifted origins, widths that are no power
of two, points on and next to voxel faces, depth 21, and every refused row. The GPU is held to the same table by
tests/test_gpu_plan_coords.py.

Bars: integers bit for bit; float64 coefficients rtol = atol = 1e-12 with the absolute part scaled by the column's magnitude
(tests/test_gpu_parity.py::test_forward_inverse_f64)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from . import plan_coord_cases as pc
from .conftest import load_golden
from .test_cpu_twins import _host_api, _vp, twins  # noqa: F401  (twins: the fixture that loads libraht_cpu.so)

FIXTURES = [c.name for c in pc.FIXTURES]


def load_coords(case):
    """the fixture of a case (tests/golden/coords/<name>.npz), lists unpacked by conftest.load_golden"""
    g = load_golden(os.path.join("coords", case.fixture[0]))
    assert str(g["case"]) == case.name and str(g["lists_from"]) == "RAHT_param_reorder_fast"
    return g


def check_lists(List, Flags, weights, order, g):
    """List / Flags / weights equal the reference's; order_RAGFT equals it where the reference's is a permutation (the rule of
    tests/test_gpu_parity.py::test_plan_lists_and_order_match_reference)"""
    N = g["V"].shape[0]
    assert len(List) == len(g["List"])
    for l in range(len(List)):
        assert np.array_equal(List[l], g["List"][l]), f"List[{l}]"
        assert np.array_equal(Flags[l], g["Flags"][l]), f"Flags[{l}]"
        assert np.array_equal(weights[l], g["weights"][l]), f"weights[{l}]"
    assert np.array_equal(np.sort(order), np.arange(N))
    ref_sane = (not bool(g["order_is_none"])) and np.array_equal(np.sort(g["order"]), np.arange(N))
    if ref_sane:
        assert np.array_equal(order, g["order"])
    return ref_sane


def f64_bar(T, ref):
    """|T - ref| <= 1e-12 * max(1, column max) + 1e-12 * |ref|"""
    atol = 1e-12 * np.maximum(1.0, np.abs(ref).max(axis=0))
    return np.all(np.abs(T - ref) <= atol + 1e-12 * np.abs(ref))


# ------------------------------------------------------------------------------------------ the case table itself
def test_case_table_covers_what_it_promises():
    names = {c.name for c in pc.ACCEPTED}
    assert {f"shift_int_n{n}" for n in (1, 255, 256, 257, 1025)} <= names and "j1_all8" in names
    assert [pc.BY_NAME[f"shift_int_n{n}"].V.shape[0] for n in (1, 255, 256, 257, 1025)] == [1, 255, 256, 257, 1025]
    assert all(pc.BY_NAME[f"shift_int_n{n}"].dtypes == pc.ALL for n in (1, 255, 256, 257, 1025))
    q, _, _ = pc.BY_NAME["j1_all8"].model()
    assert sorted(map(tuple, q)) == [(x, y, z) for x in (0, 1) for y in (0, 1) for z in (0, 1)]
    # border cases hold points ON a face, one step below and one step above it, and the first, second and last voxel of every axis
    # (the float32 twins are these points rounded to float32 and stepped once more in float32: where they fall is the model's say)
    for name in ("w3_j10_border_f64", "w1e-3_j12_border_f64", "shift_border_f64"):
        c = pc.BY_NAME[name]
        q, _, _ = c.model()
        Q = c.width / 2 ** c.J
        frac = (c.V.astype(np.float64) - np.asarray(c.minV)) / Q - q
        assert (frac == 0).any() and (frac > 1 - 1e-6).any() and ((frac > 0) & (frac < 1e-6)).any(), name
        for a in range(3):
            assert {0, 1, 2 ** c.J - 1} <= set(q[:, a].tolist()), (name, a)
    d = pc.DEEP
    q, _, key = d.model()
    assert d.J == 21 and 2900 <= d.V.shape[0] <= 3100 and (q[0] == 0).all() and (q[-1] == 2 ** 21 - 1).all()
    lv = np.array([int(a ^ b).bit_length() - 1 for a, b in zip(key[1:].tolist(), key[:-1].tolist())])
    assert lv.max() == 62 and len(set((lv // 3).tolist())) == 21          # a pair at the top binary level and in every octree level
    assert {n for n, _ in pc.REFUSED} == set(pc.REFUSED_VALUES)
    for n in ("nan", "plus_inf", "minus_inf", "f32_max"):
        assert (n, "f32") in pc.REFUSED and (n, "f64") in pc.REFUSED


def test_model_is_float64_arithmetic_for_every_dtype():
    """the float32 border twins are float32 inputs (the float32 value is the input), and float32 ARITHMETIC on them
    would give other voxels than the model: the cases can tell the two apart"""
    for name in ("w3_j10_border_f32", "w1e-3_j12_border_f32", "shift_border_f32"):
        c = pc.BY_NAME[name]
        assert c.V.dtype == np.float32
        q, _, _ = c.model()
        q32 = np.floor((c.V - np.asarray(c.minV, np.float32)) / np.float32(c.width / 2 ** c.J)).astype(np.int64)
        assert (q32 != q).any(), name


# ------------------------------------------------------------------------------------------ fixtures from the reference
@pytest.mark.parametrize("name", FIXTURES)
def test_model_keys_equal_the_reference_codes(name):
    case = pc.BY_NAME[name]
    g = load_coords(case)
    assert g["V"].dtype == pc.DTYPES[case.fixture[1]] and np.array_equal(g["V"], case.cast(case.fixture[1]))
    assert tuple(g["minV"]) == case.minV and float(g["width"]) == case.width and int(g["J"]) == case.J
    q, bad, key = pc.model_keys(g["V"], g["minV"], float(g["width"]), int(g["J"]))
    assert not bad.any() and key.dtype == np.uint64 and np.array_equal(key, g["morton"])


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_equals_the_reference(oracle, name):
    case = pc.BY_NAME[name]
    g = load_coords(case)
    po = oracle.raht_param(g["V"].astype(np.float64), g["minV"], float(g["width"]), int(g["J"]))
    assert np.array_equal(po.morton, g["morton"])
    assert check_lists(po.List, po.Flags, po.weights, po.order, g)
    T, w = oracle.raht_fwd(g["C"], po)
    assert f64_bar(T, g["T"])
    assert np.array_equal(w.reshape(-1), g["w"])
    np.testing.assert_allclose(oracle.raht_inv(T, po), g["C"], rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(g["C"]).max())))


# ------------------------------------------------------------------------------------------ the host twin
def _twin_create(twins, V, dt, minV, width, J):
    api = _host_api(twins)[0]
    h = C.c_void_p()
    assert V.dtype == pc.DTYPES[dt] and V.flags.c_contiguous
    rc = api.fn("plan_create")(_vp(V), pc.RAHT_DTYPE[dt], C.c_int64(V.shape[0]), (C.c_double * 3)(*minV), C.c_double(width), J, None, C.byref(h))
    return rc, h, api


def _twin_lists(api, h, N):
    List, Flags, weights = [], [], []
    for l in range(api.fn("plan_levels")(h)):
        n = C.c_int64()
        assert api.fn("plan_export_level")(h, l, None, None, None, C.byref(n)) == 0
        a, f, w = np.empty(n.value, np.int64), np.empty(n.value, np.uint8), np.empty(n.value, np.int64)
        assert api.fn("plan_export_level")(h, l, _vp(a), _vp(f), _vp(w), C.byref(n)) == 0
        List.append(a); Flags.append(f.astype(bool)); weights.append(w)
    order = np.empty(N, np.int64)
    assert api.fn("plan_order")(h, _vp(order), None) == 0
    return List, Flags, weights, order


@pytest.mark.parametrize("name", [c.name for c in pc.ACCEPTED + [pc.DEEP]])
def test_twin_builds_every_accepted_case_in_every_dtype(twins, oracle, name):
    case = pc.BY_NAME[name]
    po = oracle.raht_param(case.V.astype(np.float64), case.minV, case.width, case.J, ref_quirks=False)
    assert np.array_equal(po.morton, case.model()[2])
    for dt in case.dtypes:
        rc, h, api = _twin_create(twins, case.cast(dt), dt, case.minV, case.width, case.J)
        assert rc == 0, (dt, api.err())
        List, Flags, weights, order = _twin_lists(api, h, case.V.shape[0])
        assert api.fn("plan_destroy")(h) == 0
        assert len(List) == po.nlevels, dt
        for l in range(po.nlevels):
            assert np.array_equal(List[l], po.List[l]) and np.array_equal(Flags[l], po.Flags[l]) and np.array_equal(weights[l], po.weights[l]), (dt, l)
        assert np.array_equal(order, po.order), dt
        if case.fixture:
            check_lists(List, Flags, weights, order, load_coords(case))


@pytest.mark.parametrize("name,dt", pc.REFUSED)
def test_twin_refuses_with_the_bounds_code_and_the_row(twins, oracle, name, dt):
    for label, V, minV, width, J, row in pc.refused_clouds(name, dt):
        rc, h, api = _twin_create(twins, V, dt, minV, width, J)
        assert rc == pc.RAHT_ERR_BOUNDS, (label, rc, api.err())
        m = re.search(r"row (\d+)", api.err())
        assert m and int(m.group(1)) == row, (label, api.err())
        with pytest.raises(ValueError):                              # the oracle's own builder agrees
            oracle.raht_param(V.astype(np.float64), minV, width, J)


def test_twin_accepts_the_rows_at_the_edge(twins):
    clouds = pc.must_accept_clouds()
    assert len(clouds) >= 24
    for label, dt, V, minV, width, J in clouds:
        rc, h, api = _twin_create(twins, V, dt, minV, width, J)
        assert rc == 0, (label, api.err())
        assert twins.raht_cpu_plan_size(h) == V.shape[0]
        assert api.fn("plan_destroy")(h) == 0
