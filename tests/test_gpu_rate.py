"""raht_rlgr_seg_rate / SegmentedCoder.rate / RahtPlan.rate_curve / bitstream.encode_frame_bytes_target on the GPU.

The oracle of the sizes is the real encoder: quantize with ops.quant_rows / quant_rows_f64, encode with SegmentedCoder, compare
its length table entry for entry and its container size. Three segments of every case are also held against the numpy model of
tests/numpy_rate.py and the host coder (rlgr.membuf). Everything about sizes is exact; the squared errors are compared with a
float64 numpy evaluation of the same formula: every term is non-negative and formed by the same rounded double operations on
both sides, so the sums differ only by the order of at most N = 5000 additions: N * 2^-53 = 6e-13 relative; rtol = 1e-10."""
import ctypes

import numpy as np
import pytest

from . import numpy_rate as model

pytestmark = pytest.mark.gpu

N0, D0 = 5000, 7
# eleven steps: k = 1, 3, 8, 11 take the first k. The escape column is scaled so that |T / step| stays below 2^30 at the finest.
SCALARS = [0.02 * 1.6 ** i for i in range(11)]
TABLE = [1.0, 0.5, 2.0, 1.0, 1.0, 0.25, 3.0]                    # per-column factors of the D-table steps
SEG_LENS = (64, 1000, 4096, 100000)
KS = (1, 3, 8, 11)


def _matrix(dtype):
    """N0 x 7: Laplace coefficients at scales 0.3, 3, 200; zeros; escapes; 0.1 % non-zeros; half zeros then dense"""
    rng = np.random.default_rng(20261017)
    T = np.zeros((N0, D0), np.float64)
    for c, sc in enumerate((0.3, 3.0, 200.0)):
        T[:, c] = rng.laplace(0, sc, N0)
    T[:, 4] = rng.laplace(0, 0.05, N0)
    big = rng.random(N0) < 0.02
    T[big, 4] = rng.uniform(-1, 1, int(big.sum())) * (2.0 ** 30) * min(SCALARS) * 0.99
    T[0, 4] = (2.0 ** 30) * min(SCALARS) * 0.99
    nzi = rng.choice(N0, N0 // 1000, replace=False)
    T[nzi, 5] = rng.laplace(0, 20, nzi.size)
    T[N0 // 2:, 6] = rng.laplace(0, 5, N0 - N0 // 2)
    return T.astype(dtype)


@pytest.fixture(scope="module")
def mats():
    import torch
    out = {}
    for name, dt in (("f32", np.float32), ("f64", np.float64)):
        T = _matrix(dt)
        out[name] = {1: T, 0: np.abs(T)}
    dev = {}
    for name in out:
        for flag in (0, 1):
            T = out[name][flag]
            wide = torch.full((N0, D0 + 5), float("nan"), dtype=torch.from_numpy(T).dtype, device="cuda")
            wide[:, :D0] = torch.from_numpy(T).cuda()
            dev[name, flag, D0] = torch.from_numpy(T).cuda()
            dev[name, flag, D0 + 5] = wide[:, :D0]
    return out, dev


def _step_rows(kind, k):
    if kind == "scalar":
        return [SCALARS[j] for j in range(k)]
    return [[SCALARS[j] * f for f in TABLE] for j in range(k)]


_expected = {}


def _encoder_tables(Td, name, flag, S, step):
    """(seg_bytes, size_bytes, Q) of the real encoder for one step (a scalar or a D-table); computed once per input"""
    import torch
    from raht_3dgs_codec_amd import ops
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    key = (name, flag, S, tuple(step) if isinstance(step, list) else step)
    if key not in _expected:
        N, D = Td.shape
        Q = torch.empty((N, D), dtype=torch.int32, device="cuda")
        pos = torch.arange(N, dtype=torch.int64, device="cuda")
        (ops.quant_rows_f64 if name == "f64" else ops.quant_rows)(Td, step, pos, Q)
        sc = SegmentedCoder(N, D, S, flag, "cuda")
        sc.encode(Q)
        _expected[key] = (sc.seg_bytes.cpu().numpy().astype(np.int64), sc.size_bytes, Q.cpu().numpy())
    return _expected[key]


@pytest.mark.parametrize("name", ["f32", "f64"])
@pytest.mark.parametrize("S", SEG_LENS)
@pytest.mark.parametrize("k", KS)
def test_sizes_equal_the_real_encoder(mats, name, S, k):
    from raht_3dgs_codec_amd import rlgr
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    host, dev = mats
    nseg = -(-N0 // S)
    pick = 0
    for ld in (D0, D0 + 5):
        for kind in ("scalar", "table"):
            for flag in (1, 0):
                Td = dev[name, flag, ld]
                steps = _step_rows(kind, k)
                cb, sb, _ = SegmentedCoder.rate(Td, steps, S, flag, want_sse=False)
                sb = sb.cpu().numpy().astype(np.int64)
                assert sb.shape == (k, D0 * nseg)
                for j in range(k):
                    want_sb, want_size, Q = _encoder_tables(dev[name, flag, D0], name, flag, S, steps[j])
                    print(f"{name} S={S} k={k} ld={ld} {kind} flag={flag} step {j}: {int((sb[j] != want_sb).sum())} of {want_sb.size} lengths differ, "
                          f"container {int(cb[j])} / {want_size}")
                    assert np.array_equal(sb[j], want_sb)
                    assert int(cb[j]) == want_size == model.container_bytes(want_sb)
                # independently: first, last and a middle segment of some (channel, step) against the model and the host coder
                for s in sorted({0, nseg // 2, nseg - 1}):
                    c, j = pick % D0, pick % k
                    pick += 1
                    st = steps[j][c] if kind == "table" else steps[j]
                    q = model.quantize(host[name][flag][s * S: (s + 1) * S, c], st)
                    assert np.array_equal(q, _encoder_tables(dev[name, flag, D0], name, flag, S, steps[j])[2][s * S: (s + 1) * S, c])
                    m = rlgr.membuf()
                    m.rlgrWrite(q.astype(np.int32), flag)
                    assert sb[j, c * nseg + s] == model.rlgr_len(q, flag) == len(m.get_array()), (c, s, j)


@pytest.mark.parametrize("N, D", [(1, 1), (1, 7), (64, 1), (65, 3), (64, 7), (129, 2)])
def test_smallest_shapes(N, D):
    """N = 1, D = 1, N = seg_len, N = seg_len + 1 at seg_len = 64"""
    import torch
    from raht_3dgs_codec_amd import ops
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    rng = np.random.default_rng(N * 100 + D)
    for dt, quant in ((np.float32, ops.quant_rows), (np.float64, ops.quant_rows_f64)):
        T = rng.laplace(0, 2, (N, D)).astype(dt)
        T[rng.random((N, D)) < 0.5] = 0
        Td = torch.from_numpy(T).cuda()
        steps = [0.1, 0.7, 5.0]
        cb, sb, sse = SegmentedCoder.rate(Td, steps, 64)
        for j, st in enumerate(steps):
            Q = torch.empty((N, D), dtype=torch.int32, device="cuda")
            quant(Td, st, torch.arange(N, device="cuda"), Q)
            sc = SegmentedCoder(N, D, 64, 1, "cuda")
            sc.encode(Q)
            assert np.array_equal(sb[j].cpu().numpy(), sc.seg_bytes.cpu().numpy())
            assert int(cb[j]) == sc.size_bytes == len(sc.container())
            q = model.quantize(T, st)
            assert np.array_equal(q, Q.cpu().numpy())
            assert np.array_equal(sb[j].cpu().numpy(), model.segment_table(q, 64))
            np.testing.assert_allclose(sse[j].cpu().numpy(), model.sse(T, q, st), rtol=1e-10, atol=0)


@pytest.mark.parametrize("name", ["f32", "f64"])
@pytest.mark.parametrize("kind", ["scalar", "table"])
def test_sse_equals_the_float64_model_and_is_deterministic(mats, name, kind):
    import torch
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    host, dev = mats
    steps = _step_rows(kind, 11)
    for S, ld in ((1000, D0), (4096, D0 + 5)):
        _, sb1, sse1 = SegmentedCoder.rate(dev[name, 1, ld], steps, S)
        _, sb2, sse2 = SegmentedCoder.rate(dev[name, 1, ld], steps, S)
        assert torch.equal(sse1, sse2) and torch.equal(sb1, sb2)                    # bit-identical
        got = sse1.cpu().numpy()
        assert got.shape == (11, D0) and got.dtype == np.float64
        T = host[name][1]
        for j in range(11):
            st = np.array(steps[j] if kind == "table" else [steps[j]] * D0)
            want = model.sse(T, model.quantize(T, st.astype(T.dtype)), st.astype(T.dtype))
            rel = np.abs(got[j] - want) / np.maximum(want, 1e-300)
            print(f"{name} {kind} S={S} step {j}: max relative difference {rel.max():.3e}")
            np.testing.assert_allclose(got[j], want, rtol=1e-10, atol=0)
            assert got[j, 3] == 0.0                                                 # the all-zero column


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_guard_elements_and_null_sse(mats, name):
    """the C entry point on buffers with 64 guard elements either side; seg_sse = NULL computes the same lengths and writes no sums"""
    import torch
    from raht_3dgs_codec_amd import _lib
    L = _lib.lib()
    host, dev = mats
    S, k, GUARD = 1000, 11, 64
    G = D0 * -(-N0 // S)
    Td = dev[name, 1, D0 + 5]
    ct = ctypes.c_double if name == "f64" else ctypes.c_float
    st = (ct * k)(*SCALARS[:k])
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(with_sse):
        sb = torch.full((k * G + 2 * GUARD,), -1515870811, dtype=torch.int32, device="cuda")          # 0xA5A5A5A5
        se = torch.full((k * G + 2 * GUARD,), -7.25, dtype=torch.float64, device="cuda")
        _lib.check(L.raht_rlgr_seg_rate(ctypes.c_void_p(Td.data_ptr()), 1 if name == "f64" else 0, Td.stride(0), N0, D0, st, k, 1, S, 1,
                                        ctypes.c_void_p(sb.data_ptr() + 4 * GUARD), ctypes.c_void_p(se.data_ptr() + 8 * GUARD) if with_sse else None,
                                        stream))
        torch.cuda.synchronize()
        return sb.cpu().numpy(), se.cpu().numpy()

    sb1, se1 = run(True)
    sb0, se0 = run(False)
    for sb in (sb1, sb0):
        assert np.all(sb[:GUARD] == -1515870811) and np.all(sb[-GUARD:] == -1515870811)
        assert np.all(sb[GUARD:-GUARD] >= 0)
    assert np.array_equal(sb0, sb1)
    assert np.all(se1[:GUARD] == -7.25) and np.all(se1[-GUARD:] == -7.25) and np.all(se1[GUARD:-GUARD] >= 0)
    assert np.all(se0 == -7.25)                                                     # NULL: nothing written


# ---- rate_curve against the codec -----------------------------------------------------------------------------------
CURVE_STEPS = [0.01, 0.05, 0.2, 1.0, 4.0]
FRAMES = {14: (5000, 8, 14, 0), 59: (5000, 8, 59, 0), "59w": (5000, 8, 59, 3)}


@pytest.fixture(scope="module")
def frames():
    import torch
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import synth
    out = {}
    for key, (draws, J, D, n_wide) in FRAMES.items():
        V, keys, C = synth.scene(draws, J, D, seed=31 + D)
        plan = R.RahtPlan.from_keys(torch.from_numpy(keys.view(np.int64)).cuda(), 3 * J)
        out[key] = dict(V=V, keys=keys, C=C, Cd=torch.from_numpy(C).cuda(), plan=plan, J=J, D=D, n_wide=n_wide)
    return out


def _container_len(f, step):
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    plan, Cd = f["plan"], f["Cd"]
    Q = plan.forward_quant_mixed(Cd, step, f["n_wide"]) if f["n_wide"] else plan.forward_quant(Cd, step)
    sc = SegmentedCoder(Cd.shape[0], f["D"], 2048, 1, "cuda")
    sc.encode(Q)
    return len(sc.container()), Q


@pytest.mark.parametrize("key", [14, 59, "59w"])
def test_rate_curve_equals_the_codec(frames, key):
    f = frames[key]
    rc = f["plan"].rate_curve(f["Cd"], CURVE_STEPS, n_wide=f["n_wide"])
    assert rc["bytes"].shape == (5,) and rc["bytes"].dtype == np.int64 and rc["sse"].shape == (5, f["D"]) and rc["sse"].dtype == np.float64
    for j, st in enumerate(CURVE_STEPS):
        want, _ = _container_len(f, st)
        print(f"frame {key} step {st}: rate_curve {int(rc['bytes'][j])}, codec {want}")
        assert int(rc["bytes"][j]) == want
    # a per-column table is a curve point like any other
    table = [0.004 * (1 + (c % 7)) for c in range(f["D"])]
    rt = f["plan"].rate_curve(f["Cd"], [table, [2 * s for s in table]], n_wide=f["n_wide"])
    assert int(rt["bytes"][0]) == _container_len(f, table)[0]
    assert int(rt["bytes"][1]) == _container_len(f, [2 * s for s in table])[0]
    assert np.all(rc["sse"] >= 0) and np.all(np.diff(rc["sse"].sum(axis=1)) > 0)      # coarser steps: more error


def test_rate_curve_refuses_row_mapped_and_truncated_plans(frames):
    import torch
    import raht_3dgs_codec_amd as R
    f = frames[14]
    N = f["Cd"].shape[0]
    kd = torch.from_numpy(f["keys"].view(np.int64)).cuda()
    trunc = R.RahtPlan.from_keys(kd, 3 * f["J"], top_level=3 * f["J"] - 6)
    assert trunc.n_roots > 1
    with pytest.raises(ValueError):
        trunc.rate_curve(f["Cd"], [0.1])
    mapped = R.RahtPlan.from_keys(kd, 3 * f["J"])
    mapped.set_row_map(torch.arange(N, dtype=torch.int64, device="cuda") * 2, 2 * N)
    with pytest.raises(ValueError):
        mapped.rate_curve(torch.zeros((2 * N, 14), device="cuda"), [0.1])


# ---- encode_frame_bytes_target --------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", [14, "59w"])
def test_encode_to_a_byte_budget(frames, key):
    import torch
    from raht_3dgs_codec_amd import bitstream
    f = frames[key]
    V, C, J, n_wide, plan, Cd = f["V"], f["C"], f["J"], f["n_wide"], f["plan"], f["Cd"]
    full = len(bitstream.encode_frame_bytes(V, C, J, 0.01, "cuda", n_wide=n_wide))
    for frac in (0.9, 0.5, 0.2):
        target = int(frac * full)
        blob, info = bitstream.encode_frame_bytes_target(V, C, J, target, step=0.01, n_wide=n_wide)
        print(f"frame {key} target {target}: {len(blob)} bytes at multiplier {info['multiplier']:.5g}, {len(info['tried'])} sizes evaluated")
        assert len(blob) <= target
        assert info["attribute_bytes"] == info["predicted_attribute_bytes"]
        assert info["steps"] == [0.01 * info["multiplier"]]
        h = bitstream.parse_frame(blob)
        assert h["attributes"][1] == info["attribute_bytes"] and h["steps"] == info["steps"] and h["n_wide"] == n_wide
        Vd, Crec = bitstream.decode_frame_bytes(blob, "cuda")
        assert np.array_equal(Vd.cpu().numpy(), V)
        if n_wide:
            want = plan.dequant_inverse_mixed(plan.forward_quant_mixed(Cd, info["steps"], n_wide), info["steps"], n_wide)
        else:
            want = plan.dequant_inverse(plan.forward_quant(Cd, info["steps"]), info["steps"])
        assert torch.equal(Crec.view(torch.int32), want.view(torch.int32))          # bit-identical
        # tight: the next finer multiplier that was evaluated did not fit (or there is none: the range's finest was taken)
        budget = info["attribute_bytes"] + (target - len(blob))
        finer = [(m, b) for m, b in info["tried"] if m < info["multiplier"]]
        if finer:
            m, b = max(finer)
            assert b > budget, (m, b, budget)
        else:
            assert info["multiplier"] == 2 ** -10
        assert dict(info["tried"])[info["multiplier"]] == info["attribute_bytes"]
        assert info["sse"].shape == (f["D"],) and len(info["tried"]) <= 3 * 8


def test_budgets_that_cannot_be_met_and_step_tables(frames):
    from raht_3dgs_codec_amd import bitstream
    f = frames[14]
    V, C, J = f["V"], f["C"], f["J"]
    geo = bitstream.parse_frame(bitstream.encode_frame_bytes(V, C, J, 1.0, "cuda"))["geometry"][1]
    with pytest.raises(ValueError):
        bitstream.encode_frame_bytes_target(V, C, J, geo - 1)                       # smaller than the geometry section
    coarse = len(bitstream.encode_frame_bytes(V, C, J, 0.02, "cuda"))
    with pytest.raises(ValueError):                                                 # no multiplier of the range reaches it
        bitstream.encode_frame_bytes_target(V, C, J, coarse // 2, step=0.01, scale_range=(0.5, 2.0))
    table = [0.004 * (1 + (c % 7)) for c in range(14)]
    full = len(bitstream.encode_frame_bytes(V, C, J, table, "cuda"))
    blob, info = bitstream.encode_frame_bytes_target(V, C, J, int(0.6 * full), step=table)
    assert len(blob) <= int(0.6 * full) and info["multiplier"] > 1
    assert info["steps"] == [s * info["multiplier"] for s in table]
    assert bitstream.parse_frame(blob)["steps"] == info["steps"]
    assert info["attribute_bytes"] == info["predicted_attribute_bytes"]
