"""The scalar row kernel of csrc/quant.hip behind its eight entry points, bit for bit against numpy in the same dtype, and the one
step parser everything marshals through (ops.step_list).

Permutation path (raht_quant_reorder / raht_dequant_unreorder and their _f64 twins): float32 rows narrower than one 16-byte chunk
(D < 4) and every float64 width, D = 70 taking the lane loop round twice; both directions gather through the plan's permutation.
Rows path (raht_quant_rows / raht_dequant_rows and their _f64 twins): explicit rows of a taller integer matrix, both sides column
slices of wider matrices; what ``pos`` does not name stays as it was."""
import ctypes

import numpy as np
import pytest

N_PLAN = 300
SENTINEL = -777
NPDT = {"float32": np.float32, "float64": np.float64}


@pytest.fixture(scope="module")
def rt():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    _lib.lib()
    return R


@pytest.fixture(scope="module")
def plan(rt):
    """a plan of 300 random voxels and its order_RAGFT on the host"""
    rng = np.random.default_rng(7)
    keys = np.sort(rng.choice(1 << 21, size=N_PLAN, replace=False)).astype(np.int64)
    p = rt.RahtPlan.from_keys(_dev(keys), 21)
    order = p.order_RAGFT.cpu().numpy()
    assert sorted(order.tolist()) == list(range(N_PLAN))
    return p, order


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _step(kind, D, dt):
    """-> (the step argument, the same as an array of the matrices' dtype, as the kernels see it)"""
    if kind == "scalar":
        return 0.37, np.asarray([0.37], dt)
    steps = [1.0 + 0.5 * c for c in range(D)]
    return steps, np.asarray(steps, dt)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["scalar", "per_channel"])
@pytest.mark.parametrize("dtype,D", [("float32", 1), ("float32", 2), ("float32", 3), ("float64", 1), ("float64", 3), ("float64", 70)])
def test_permutation_path_is_numpy_bit_for_bit(rt, plan, dtype, D, kind):
    import torch
    p, order = plan
    dt = NPDT[dtype]
    tdt = getattr(torch, dtype)
    rng = np.random.default_rng(100 + D)
    wide = (rng.standard_normal((N_PLAN, D + 3)) * 100).astype(dt)
    T = _dev(wide)[:, :D]                                        # row stride D + 3
    assert T.stride(0) == D + 3
    arg, s = _step(kind, D, dt)
    Q = p.quant_reorder(T, arg)
    exp = np.floor(wide[:, :D][order] / s + dt(0.5)).astype(np.int32)
    assert exp.dtype == np.int32 and (wide[:, :D][order] / s).dtype == dt
    assert Q.dtype == torch.int32 and np.array_equal(Q.cpu().numpy(), exp)
    Td = p.dequant_unreorder(Q, arg, dtype=tdt)
    assert Td.dtype == tdt
    back = exp.astype(dt) * s
    assert back.dtype == dt
    assert np.array_equal(Td.cpu().numpy()[order], back)           # T[order[k]] = Q[k] * step


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["scalar", "per_channel"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("D", [1, 59, 130])
@pytest.mark.parametrize("n", [0, 1, 5, 600])
def test_rows_path_is_numpy_bit_for_bit(rt, n, D, dtype, kind):
    import torch
    from raht_3dgs_codec_amd import ops
    dt = NPDT[dtype]
    tdt = getattr(torch, dtype)
    quant, dequant = (ops.quant_rows, ops.dequant_rows) if dtype == "float32" else (ops.quant_rows_f64, ops.dequant_rows_f64)
    rng = np.random.default_rng(1000 * n + D)
    rows = 2 * n + 7                                               # a taller Q: pos picks n distinct rows of it
    pos = rng.permutation(rows)[:n].astype(np.int64)
    Xw = (rng.standard_normal((n, D + 4)) * 50).astype(dt)
    Qw = np.full((rows, D + 5), SENTINEL, np.int32)
    arg, s = _step(kind, D, dt)
    Xd, Qd = _dev(Xw), _dev(Qw)
    X, Q = Xd[:, 1:1 + D], Qd[:, 2:2 + D]                          # column slices of wider matrices
    ret = quant(X, arg, _dev(pos), Q)
    assert ret is Q
    exp = Qw.copy()
    exp[pos, 2:2 + D] = np.floor(Xw[:, 1:1 + D] / s + dt(0.5)).astype(np.int32)
    assert np.array_equal(Qd.cpu().numpy(), exp)                   # n = 0: untouched; unnamed rows and the other columns too
    back = exp[pos, 2:2 + D].astype(dt) * s
    assert back.dtype == dt
    out = dequant(Q, arg, _dev(pos))
    assert out.dtype == tdt and tuple(out.shape) == (n, D)
    assert np.array_equal(out.cpu().numpy(), back)
    Ow = _dev(np.full((n, D + 2), float(SENTINEL), dt))            # into a column slice of a wider matrix
    view = Ow[:, 1:1 + D]
    assert dequant(Q, arg, _dev(pos), view) is view
    Oexp = np.full((n, D + 2), float(SENTINEL), dt)
    Oexp[:, 1:1 + D] = back
    assert np.array_equal(Ow.cpu().numpy(), Oexp)
    assert np.array_equal(Qd.cpu().numpy(), exp)                   # reading Q changed nothing


# ---- the step parser: no GPU ---------------------------------------------------------------------------------------------
def test_step_list_takes_scalars_and_sequences():
    import torch
    from raht_3dgs_codec_amd.ops import step_list
    for st, exp in ((3, [3.0]), (0.5, [0.5]), (np.float32(0.5), [0.5]), (np.float64(0.25), [0.25]), (np.array(0.5), [0.5]),
                    (torch.tensor(0.5), [0.5]), (np.int64(2), [2.0])):
        for D in (None, 1, 4):
            got = step_list(st, D)
            assert got == exp and all(type(x) is float for x in got), (st, D)
    row = [0.5, 2.0, 3.0, 0.125]
    for st in (row, tuple(row), np.asarray(row), np.asarray(row, np.float32), torch.tensor(row), torch.tensor(row, dtype=torch.float64)):
        for D in (None, 4):
            got = step_list(st, D)
            assert got == row and all(type(x) is float for x in got)
    assert step_list([0.5], 4) == [0.5]                            # one entry: a scalar step


@pytest.mark.parametrize("st", [[1.0, 2.0], (1.0, 2.0, 3.0), np.ones(5), []])
def test_step_list_refuses_a_wrong_length(st):
    from raht_3dgs_codec_amd.ops import step_list
    with pytest.raises(ValueError, match="steps must be a scalar or have D entries"):
        step_list(st, 4)


def test_step_array_yields_ctypes_arrays():
    from raht_3dgs_codec_amd.ops import _step_array
    for ctype in (ctypes.c_float, ctypes.c_double):
        a = _step_array(np.float32(0.5), 7, ctype)
        assert isinstance(a, ctypes.Array) and a._type_ is ctype and len(a) == 1 and a[0] == 0.5
        b = _step_array([1.0 + 0.5 * c for c in range(7)], 7, ctype)
        assert isinstance(b, ctypes.Array) and b._type_ is ctype and len(b) == 7 and list(b) == [1.0 + 0.5 * c for c in range(7)]
        with pytest.raises(ValueError, match="steps must be a scalar or have D entries"):
            _step_array([1.0, 2.0], 7, ctype)
    assert _step_array(0.37, 3, ctypes.c_float)[0] == float(np.float32(0.37))      # rounded to float32 once, here


@pytest.mark.parametrize("bad", [0, -1, float("inf"), float("nan")])
def test_bitstream_steps_stay_finite_and_positive(bad):
    from raht_3dgs_codec_amd.bitstream import _step_list
    with pytest.raises(ValueError, match="steps must be finite and positive"):
        _step_list(bad, 3)
    with pytest.raises(ValueError, match="steps must be finite and positive"):
        _step_list([1.0, bad, 2.0], 3)
    with pytest.raises(ValueError, match="steps must be finite and positive"):
        _step_list(np.float64(bad), 3)
    with pytest.raises(ValueError, match="step must be a scalar or have one entry per attribute column"):
        _step_list([1.0, 2.0], 3)
    assert _step_list(0.5, 3) == [0.5] and _step_list(np.asarray([1.0, 2.0, 4.0]), 3) == [1.0, 2.0, 4.0]


def test_step_row_returns_what_it_returned():
    import torch
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    for st in (0.5, 2, np.float32(0.5), np.float64(0.5), np.array(0.5), torch.tensor(0.5)):
        assert SegmentedCoder.step_row(st) == [float(st)]
    for st in ([0.5, 2.0], (0.5, 2.0), np.asarray([0.5, 2.0]), torch.tensor([0.5, 2.0])):
        assert SegmentedCoder.step_row(st) == [0.5, 2.0]
