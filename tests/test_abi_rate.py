"""CPU-only checks of raht_rlgr_seg_rate at the C-ABI boundary and of the numpy model the GPU tests hold it against: the symbol is
declared, exported and bound; every argument rule is refused with RAHT_ERR_INVALID and the function's name before any HIP call
(the "device pointers" are addresses that must never be read); the model's stream lengths equal those of the host coder, which
tests/test_rlgr.py pins byte for byte to the reference's streams; and the frame container is parsed as before."""
import ctypes
import os

import numpy as np
import pytest

from . import numpy_rate as model
from .conftest import ROOT
from .rlgr_inputs import laplace_stream, random_sequences

INVALID = -1
NAME = "raht_rlgr_seg_rate"
F32, F64 = 0, 1


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def test_the_symbol_is_declared_exported_and_bound(L):
    from raht_3dgs_codec_amd import _lib
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    header = open(os.path.join(ROOT, "include", "raht.h")).read()
    assert "int raht_rlgr_seg_rate(" in header
    assert "#define RAHT_RLGR_RATE_MAX 8" in header
    assert NAME in _lib.EXPORTS
    assert hasattr(L, NAME)
    assert len(getattr(L, NAME).argtypes) == 13
    assert SegmentedCoder.RATE_MAX == 8
    assert callable(SegmentedCoder.rate)


# never dereferenced: every call below is refused before its first HIP call
A, B, Cc = 0x10000, 0x20000, 0x30000


def _f32(*v):
    return (ctypes.c_float * len(v))(*v)


def _f64(*v):
    return (ctypes.c_double * len(v))(*v)


def test_argument_validation(L):
    def call(T=A, dtype=F32, ldt=7, N=5000, D=7, steps=_f32(0.5, 1.0), k=2, n_steps=1, S=1000, flag=1, sb=B, sse=Cc):
        return L.raht_rlgr_seg_rate(T, dtype, ldt, N, D, steps, k, n_steps, S, flag, sb, sse, None)

    inf, nan = float("inf"), float("nan")
    cases = {
        "NULL T": dict(T=None), "NULL steps": dict(steps=None), "NULL seg_bytes": dict(sb=None),
        "N = 0": dict(N=0), "N < 0": dict(N=-3), "D = 0": dict(D=0, ldt=0), "ldt < D": dict(ldt=6), "k = 0": dict(k=0), "k < 0": dict(k=-1),
        "n_steps = 2": dict(n_steps=2), "n_steps = 0": dict(n_steps=0), "n_steps = D + 1": dict(n_steps=8, steps=_f32(*[1.0] * 16)),
        "seg_len = 63": dict(S=63), "seg_len = 0": dict(S=0), "seg_len < 0": dict(S=-64),
        "too many segments": dict(N=2 ** 31, D=64, ldt=64, S=64),
        "a shape the 32-bit tables refuse": dict(N=6_000_000, D=56, ldt=56, S=2048),
        "a segment longer than uint32": dict(N=10 ** 9, D=1, ldt=1, S=400_000_000),
        "flag_signed = 2": dict(flag=2), "flag_signed = -1": dict(flag=-1),
        "dtype int32": dict(dtype=2), "dtype 7": dict(dtype=7), "dtype -1": dict(dtype=-1),
        "float32 step 0": dict(steps=_f32(0.5, 0.0)), "float32 step < 0": dict(steps=_f32(-1.0, 1.0)), "float32 step inf": dict(steps=_f32(1.0, inf)),
        "float32 step nan": dict(steps=_f32(nan, 1.0)), "float32 step below 2^-100": dict(steps=_f32(1.0, 2.0 ** -101)),
        "float32 step above 2^100": dict(steps=_f32(2.0 ** 101, 1.0)),
        "float32 step in a table": dict(n_steps=7, steps=_f32(*([1.0] * 13 + [0.0]))),
        "float64 step 0": dict(dtype=F64, steps=_f64(0.5, 0.0)), "float64 step < 0": dict(dtype=F64, steps=_f64(0.5, -2.0)),
        "float64 step inf": dict(dtype=F64, steps=_f64(inf, 1.0)), "float64 step nan": dict(dtype=F64, steps=_f64(1.0, nan)),
    }
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == INVALID, (what, rc)
        assert NAME.encode() in L.raht_last_error(), (what, L.raht_last_error())
    # the same with seg_sse = NULL (a valid argument): still refused for the other reason
    assert call(sse=None, N=0) == INVALID
    assert call(steps=_f32(0.5, 0.0)) == INVALID and b"step" in L.raht_last_error()


def _host_len(x, flag=1):
    from raht_3dgs_codec_amd import rlgr
    m = rlgr.membuf()
    m.rlgrWrite(np.asarray(x), flag)
    return len(m.get_array())


def test_length_model_equals_the_host_coder_on_the_random_sequences(L):
    for t, x in enumerate(random_sequences()):
        assert model.rlgr_len(x) == _host_len(x), (t, len(x))


def test_length_model_equals_the_host_coder_on_the_laplace_stream_in_segments(L):
    x = laplace_stream().astype(np.int32)
    for S in (64, 1000, 4096):
        for s in range(0, len(x), S):
            assert model.rlgr_len(x[s: s + S]) == _host_len(x[s: s + S]), (S, s)
    assert model.rlgr_len(np.abs(x[:3000]), 0) == _host_len(np.abs(x[:3000]), 0)


def test_quantizer_and_container_formula_of_the_model():
    x = np.array([-1.5, -0.5, -0.49, 0.0, 0.49, 0.5, 1.5, 2.5e6], np.float32)
    assert model.quantize(x, 1.0).tolist() == [-1, 0, 0, 0, 0, 1, 2, 2500000]
    assert model.quantize(x.astype(np.float64), 0.5).tolist() == [-3, -1, -1, 0, 1, 1, 3, 5000000]
    # float32 quotients round in float32: 0.3f / 0.1f is 3.0000002f, 0.3 / 0.1 is 2.9999999999999996
    assert model.quantize(np.array([0.25], np.float32), np.float32(0.1)).tolist() == [3]
    assert model.container_bytes([0, 1, 4, 5]) == 8 + 40 + 16 + 0 + 4 + 4 + 8


def test_parse_frame_accepts_the_layout_as_before():
    """no format change: a hand-laid RAHTF001 frame around a raw geometry section parses to the same fields"""
    from raht_3dgs_codec_amd import bitstream
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    J, N, D = 2, 1, 3
    geo = b"OCTG0001" + np.array([J, N, 0, 2, 2048], np.int64).tobytes() + np.array([1, 1, 1], np.int64).tobytes() + bytes([1, 1])
    att = SegmentedCoder.MAGIC + np.array([N, D, 2048, 1, 12], np.int64).tobytes() + np.array([1, 1, 1], np.uint32).tobytes() + bytes(12)
    blob = (bitstream.MAGIC + np.array([J, N, D, 0, 1], np.int64).tobytes() + np.array([0.25, 1.0, 2.0, 3.0, 8.0], np.float64).tobytes()
            + np.array([len(geo)], np.int64).tobytes() + geo + np.array([len(att)], np.int64).tobytes() + att)
    h = bitstream.parse_frame(blob)
    assert (h["J"], h["N"], h["D"], h["n_wide"], h["steps"], h["vmin"], h["width"]) == (J, N, D, 0, [0.25], [1.0, 2.0, 3.0], 8.0)
    assert h["geometry"][1] == len(geo) and h["attributes"][1] == len(att)
    assert callable(bitstream.encode_frame_bytes_target)


def test_a_step_may_be_any_scalar_or_any_sequence():
    """numpy scalars, 0-d arrays and tensors are scalars to rate / rate_curve, as Python numbers are; containers part again"""
    import torch
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    for st in (0.5, 1, np.float32(0.5), np.float64(0.5), np.array(0.5, np.float32), torch.tensor(0.5)):
        assert SegmentedCoder.step_row(st) == [float(st)]
    for row in np.linspace(0.1, 1.0, 4).astype(np.float32):
        assert SegmentedCoder.step_row(row) == [float(row)]
    for st in ([0.5, 2.0], (0.5, 2.0), np.array([0.5, 2.0], np.float32), torch.tensor([0.5, 2.0])):
        assert SegmentedCoder.step_row(st) == [0.5, 2.0]
    G, cb = 12, np.array([480, 96], np.int64)
    assert (cb - SegmentedCoder.container_size(G, 0)).tolist() == [480 - 96, 0]
