"""CPU-only checks of the predicted octree geometry: its three entry points at the C-ABI boundary (exported, bound as the header
declares them, every argument rule refused with RAHT_ERR_INVALID and the function's name before any HIP call -- the "device
pointers" below are addresses that must never be read), the header parser of the predicted section, and the decoders' refusals
that come before any device work."""
import ctypes
import os

import numpy as np
import pytest

from . import numpy_octree as M
from . import numpy_octree_inter as MI

INVALID = -1
NAMES = {"raht_octree_encode_inter": 8, "raht_octree_decode_inter": 8, "raht_octree_bytes_used": 7}
A, B, Cc, Dd = 0x10000, 0x20000, 0x30000, 0x40000           # never dereferenced
GOOD = (1, 8, 20, 100)                                       # J = 3, N = 100
BAD_COUNTS = {"n_0 = 2": (2, 8, 20, 100), "n_0 = 0": (0, 0, 0, 0), "a level shrinks": (1, 8, 7, 56), "more than 8 children per node": (1, 9, 20, 100),
              "a level of 2^31": (1, 8, 64, 512, 4096, 32768, 262144, 2097152, 16777216, 134217728, 1073741824, 2 ** 31)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def _i64(*vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def _refused(L, name, rc, what):
    assert rc == INVALID, (name, what, rc)
    assert name.encode() + b":" in L.raht_last_error(), (name, what, L.raht_last_error())


def _host_rlgr(sym):
    from raht_3dgs_codec_amd import rlgr
    m = rlgr.membuf()
    m.rlgrWrite(np.ascontiguousarray(sym, np.int32), 0)
    return m.get_array()


def test_the_three_symbols_are_declared_exported_and_bound(L):
    from raht_3dgs_codec_amd import _lib
    header = open(os.path.join(ROOT, "include", "raht.h")).read()
    for name, arity in NAMES.items():
        assert f"int {name}(" in header, name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == arity, name
    assert L.raht_version() == 300                                           # new entry points, no new ABI version


def test_encode_inter_argument_validation(L):
    def call(keys=A, N=100, J=3, counts=GOOD, ref=B, N_ref=50, res=Cc):
        return L.raht_octree_encode_inter(keys, N, J, None if counts is None else _i64(*counts), ref, N_ref, res, None)

    cases = {"NULL keys": dict(keys=None), "NULL res": dict(res=None), "NULL ref_keys": dict(ref=None), "NULL counts": dict(counts=None),
             "N = 0": dict(N=0), "N = 2^31": dict(N=2 ** 31), "J = 0": dict(J=0), "J = 22": dict(J=22), "counts[J] != N": dict(N=99),
             "N_ref = 0": dict(N_ref=0), "N_ref < 0": dict(N_ref=-4), "N_ref = 2^31": dict(N_ref=2 ** 31)}
    for what, cl in BAD_COUNTS.items():
        cases[what] = dict(counts=cl, J=len(cl) - 1, N=cl[-1] if 0 < cl[-1] < 2 ** 31 else 100)
    for what, kw in cases.items():
        _refused(L, "raht_octree_encode_inter", call(**kw), what)


def test_decode_inter_argument_validation(L):
    def call(res=A, counts=GOOD, J=3, ref=B, N_ref=50, keys=Cc, bad=Dd):
        return L.raht_octree_decode_inter(res, None if counts is None else _i64(*counts), J, ref, N_ref, keys, bad, None)

    cases = {"NULL res": dict(res=None), "NULL keys": dict(keys=None), "NULL bad": dict(bad=None), "NULL counts": dict(counts=None),
             "NULL ref_keys": dict(ref=None), "J = 0": dict(J=0), "J = 22": dict(J=22), "N_ref = 0": dict(N_ref=0),
             "N_ref < 0": dict(N_ref=-1), "N_ref = 2^31": dict(N_ref=2 ** 31)}
    for what, cl in BAD_COUNTS.items():
        cases[what] = dict(counts=cl, J=len(cl) - 1)
    for what, kw in cases.items():
        _refused(L, "raht_octree_decode_inter", call(**kw), what)


def test_bytes_used_argument_validation(L):
    table = (ctypes.c_uint8 * 256)(*range(256))
    twice = (ctypes.c_uint8 * 256)(*([1, 1] + list(range(2, 256))))

    def call(s=A, n=1000, tab=table, used=7, res=B, bad=Cc):
        return L.raht_octree_bytes_used(s, n, tab, used, res, bad, None)

    for what, kw in {"NULL sym": dict(s=None), "NULL table": dict(tab=None), "NULL res": dict(res=None), "NULL bad": dict(bad=None),
                     "n_nodes = 0": dict(n=0), "n_nodes < 0": dict(n=-1), "n_nodes = 2^31": dict(n=2 ** 31),
                     "sym not 4-byte aligned": dict(s=A + 1), "a table that is no permutation": dict(tab=twice), "n_used = 0": dict(used=0),
                     "n_used < 0": dict(used=-1), "n_used = 257": dict(used=257)}.items():
        _refused(L, "raht_octree_bytes_used", call(**kw), what)


# ---- the parser ------------------------------------------------------------------------------------------------------------------
J = 6


def _sections():
    from raht_3dgs_codec_amd import synth
    keys, ref = synth.sorted_unique_keys(3000, J, 11), synth.sorted_unique_keys(2500, J, 12)
    return keys, ref, MI.section(keys, ref, J, 0), MI.section(keys, ref, J, 1, 256, _host_rlgr)


def _patched(blob, word, value, base=8):
    b = bytearray(blob)
    b[base + 8 * word: base + 8 * word + 8] = np.array([value], np.int64).tobytes()
    return bytes(b)


def test_parse_accepts_the_models_sections_and_refuses_malformed_headers(L):
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    keys, ref, raw, coded = _sections()
    counts, res = MI.res_stream(keys, ref, J)
    body = MI.header_bytes(J)
    for blob, mode in ((raw, 0), (coded, 1)):
        h = OctreeCoder.parse(blob)
        assert (h["J"], h["N"], h["mode"], h["n_nodes"], h["counts"], h["length"], h["body"]) == (J, len(keys), mode, len(res), counts, len(blob), body)
        assert h["predicted"] is True and h["N_ref"] == len(ref) and h["n_used"] == (len(np.unique(res)) if mode else 0)
        assert OctreeCoder.parse(blob + b"trailing")["length"] == len(blob)
        bad = {
            "magic": b"OCTP0002" + blob[8:], "J = 0": _patched(blob, 0, 0), "J = 22": _patched(blob, 0, 22), "N = 0": _patched(blob, 1, 0),
            "N != n_J": _patched(blob, 1, len(keys) + 1), "mode 2": _patched(blob, 2, 2), "n_nodes off by one": _patched(blob, 3, len(res) + 1),
            "N_ref = 0": _patched(blob, 5, 0), "N_ref < 0": _patched(blob, 5, -1), "N_ref = 2^31": _patched(blob, 5, 2 ** 31),
            "n_used < 0": _patched(blob, 6, -1), "n_used = 257": _patched(blob, 6, 257), "n_used of the other mode": _patched(blob, 6, 0 if mode else 5),
            "n_0 = 2": _patched(blob, 7, 2), "a level shrinks": _patched(blob, 7 + 3, counts[2] - 1),
            "more than 8 children per node": _patched(blob, 7 + 2, 8 * counts[1] + 1), "truncated header": blob[:56],
            "truncated counts": blob[:8 + 56 + 8 * 3], "shorter than its header says": blob[:-1], "body missing": blob[:body],
            "the intra magic on a predicted header": M.GEOMETRY_MAGIC + blob[8:],
        }
        for what, b in bad.items():
            with pytest.raises(ValueError):
                OctreeCoder.parse(b)
                pytest.fail(what)
        with pytest.raises(ValueError, match="more than the caller allows"):
            OctreeCoder.parse(blob, max_voxels=len(keys) - 1)
    for what, b in {"seg_len = 63": _patched(coded, 4, 63), "seg_len = 2^31": _patched(coded, 4, 2 ** 31),
                    "a table that is no permutation": coded[:body] + coded[body + 1: body + 2] + coded[body + 1:],
                    "a segment longer than the blob": coded[:body + 256] + np.array([2 ** 31], np.uint32).tobytes() + coded[body + 260:]}.items():
        with pytest.raises(ValueError):
            OctreeCoder.parse(b)
            pytest.fail(what)
    intra = OctreeCoder.parse(M.geometry_section(keys, J, 0))
    assert intra["predicted"] is False and "N_ref" not in intra


def _frame(geo, N, D=5):
    att = b"RLGS0001" + np.array([N, D, 2048, 1, 0], np.int64).tobytes() + bytes(4 * D * ((N + 2047) // 2048))   # every segment empty
    return M.frame_container(J, N, D, 0, [0.02], geo, att)


def test_decoders_refuse_before_touching_a_device(L):
    """no reference keys, or not N_ref of them: refused from the headers -- these run without a GPU"""
    import torch
    from raht_3dgs_codec_amd import bitstream
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    keys, ref, raw, coded = _sections()
    short = torch.zeros(len(ref) - 1, dtype=torch.int64)
    for blob in (raw, coded):
        with pytest.raises(ValueError, match="predicted from another frame"):
            OctreeCoder.decode(blob, "cuda")
        with pytest.raises(ValueError, match=f"{len(ref)} voxels"):
            OctreeCoder.decode(blob, "cuda", ref_keys=short)
        with pytest.raises(ValueError):
            OctreeCoder.decode(blob[:-1], "cuda", ref_keys=short)
        frame = _frame(blob, len(keys))
        h = bitstream.parse_frame(frame)
        assert h["geometry_ref"] == len(ref) and bitstream.parse_frame(_frame(M.geometry_section(keys, J, 0), len(keys)))["geometry_ref"] is None
        for call in (lambda **kw: bitstream.decode_frame_bytes(frame, "cuda", **kw),
                     lambda **kw: bitstream.decode_region_bytes(frame, 2, (0, 8), "cuda", **kw),
                     lambda **kw: bitstream.decode_cells_bytes(frame, 2, [(0, 8), (9, 20)], "cuda", **kw)):
            with pytest.raises(ValueError, match="predicted from another frame"):
                call()
            with pytest.raises(ValueError, match=f"{len(ref)} voxels"):
                call(ref_keys=short)


def test_a_sequence_refuses_predicted_geometry_without_a_wrapper_and_a_reference_of_another_size(L):
    from raht_3dgs_codec_amd import bitstream
    keys, ref, raw, coded = _sections()
    intra_ref = _frame(M.geometry_section(ref, J, 0), len(ref))
    pframe = bitstream.P_MAGIC + np.array([1, 0], np.int64).tobytes() + _frame(coded, len(keys))
    good = bitstream.pack_sequence([intra_ref, pframe])
    assert bitstream.sequence_geometry(good) == ["intra", "predicted"] and bitstream.sequence_kinds(good) == ["I", "P"]
    with pytest.raises(ValueError, match="frame 1: .*without a wrapper"):
        bitstream.sequence_geometry(bitstream.pack_sequence([intra_ref, _frame(coded, len(keys))]))
    with pytest.raises(ValueError, match="frame 0: .*without a wrapper"):
        bitstream.sequence_kinds(bitstream.pack_sequence([_frame(raw, len(keys)), intra_ref]))
    other = _frame(M.geometry_section(ref[:-1], J, 0), len(ref) - 1)
    with pytest.raises(ValueError, match=f"frame 1: .*{len(ref)} voxels"):
        bitstream.sequence_geometry(bitstream.pack_sequence([other, pframe]))
    with pytest.raises(ValueError, match="frame 1"):                         # before any device work
        bitstream.decode_sequence_bytes(bitstream.pack_sequence([other, pframe]), device="cuda")


def test_the_sequence_encoder_refuses_an_unknown_geometry_inter(L):
    from raht_3dgs_codec_amd import bitstream
    V = np.zeros((1, 3), np.int64)
    with pytest.raises(ValueError, match="geometry_inter"):
        bitstream.encode_sequence_bytes([(V, np.zeros((1, 5), np.float32))], 3, 0.1, "cpu", geometry_inter="sometimes")
