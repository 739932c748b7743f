"""The predictor's definition (tests/numpy_predict.py) on cases whose answer is known without it, and the predicted-frame wrapper
at the host boundary: ``sequence_kinds`` / ``parse_pframe`` / ``parse_sequence`` on hand-built containers, every refusal included.
No GPU."""
import numpy as np
import pytest

from . import numpy_predict as M


def _keys_and_rows(n=500, J=5, D=7, seed=3):
    from raht_3dgs_codec_amd import synth
    keys = synth.sorted_unique_keys(n, J, seed)
    rng = np.random.default_rng(seed)
    return keys, rng.normal(size=(len(keys), D)).astype(np.float32)


def test_up0_of_a_frame_against_itself_is_the_reference():
    keys, C = _keys_and_rows()
    P, n = M.predict(keys, keys, C, 0)
    assert n == len(keys) and np.array_equal(P.view(np.int32), C.view(np.int32))
    assert not M.apply(C, P).any()                                       # the residual is 0 ...
    assert np.array_equal(M.apply(M.apply(C, P), P, add=True), C)        # ... and 0 + P is P


def test_disjoint_key_sets_predict_zero():
    keys, C = _keys_and_rows()
    for up in range(4):
        sh = np.uint64(3 * up)
        cells = np.unique(keys >> sh)
        cur = keys[np.isin(keys >> sh, cells[::2])]
        ref = np.isin(keys >> sh, cells[1::2])
        P, n = M.predict(cur, keys[ref], C[ref], up)
        assert n == 0 and P.shape == (len(cur), C.shape[1]) and not P.any(), up


def test_a_run_of_one_row_returns_that_row_bit_for_bit():
    keys, C = _keys_and_rows()
    C[0, 0], C[1, 1], C[2, 2] = np.float32(1e-42), np.float32(-0.0), np.float32(3.0000002)       # a denormal, -0, an odd mantissa
    for up in (1, 2, 3):
        sh = np.uint64(3 * up)
        first = np.concatenate([[True], (keys[1:] >> sh) != (keys[:-1] >> sh)])                   # the reference keeps one row per cell
        P, n = M.predict(keys, keys[first], C[first], up)
        lo, hi = M.runs(keys, keys[first], up)
        assert n == len(keys) and np.all(hi - lo == 1)
        assert np.array_equal(P.view(np.int32), C[first][lo].view(np.int32)), up


def test_a_run_is_summed_in_row_order_and_divided_once():
    """three rows whose float32 sum depends on the order: (1e8 + 1) - 1e8 = 0 in float32 in this order, 1 in another"""
    keys = np.array([8, 9, 10, 17], np.uint64)
    C = np.array([[1e8], [1.0], [-1e8], [5.0]], np.float32)
    P, n = M.predict(np.array([15, 16, 31], np.uint64), keys, C, 1)
    assert n == 2
    assert P[:, 0].tolist() == [0.0, 5.0, 0.0]                           # cell 1: ((1e8 + 1) - 1e8) / 3 = 0; cell 2: 5 / 1; cell 3: empty


def _seq(frames):
    from raht_3dgs_codec_amd import bitstream
    seq = M.sequence(frames)
    assert seq == bitstream.pack_sequence(frames)                        # the model's container is the product's
    return seq


def test_kinds_and_wrapper_of_hand_built_containers():
    from raht_3dgs_codec_amd import bitstream
    f = M.tiny_frame()
    bitstream.parse_frame(f)
    seq = _seq([f, f, f])                                                # what gop = 1 writes: RAHTF001 frames only
    assert bitstream.sequence_kinds(seq) == ["I", "I", "I"] == M.kinds(seq)
    seq = _seq([f, M.pframe(f, 1, 0), M.pframe(f, 2, 3), f, M.pframe(f, 1, 2)])
    assert bitstream.sequence_kinds(seq) == ["I", "P", "P", "I", "P"] == M.kinds(seq)
    off = bitstream.parse_sequence(seq)
    assert len(off) == 6 and off[2] - off[1] == len(f) + 24
    for i, want in ((1, (1, 0)), (2, (2, 3)), (4, (1, 2))):
        fb = bitstream.sequence_frame(seq, i)
        ref_back, up, inner = bitstream.parse_pframe(fb)
        assert (ref_back, up) == want == M.parse_pframe(fb)[:2]
        assert isinstance(inner, memoryview) and bytes(inner) == f == M.parse_pframe(fb)[2]
    with pytest.raises(ValueError, match="not a RAHT predicted-frame wrapper"):
        bitstream.parse_pframe(f)
    # the one-frame decoders do not know the wrapper (header checks only: no device is touched)
    with pytest.raises(ValueError, match="not a RAHT frame container"):
        bitstream.decode_frame_bytes(bitstream.sequence_frame(seq, 1), "cuda")
    with pytest.raises(ValueError, match="not a RAHT frame container"):
        bitstream.decode_region_bytes(bitstream.sequence_frame(seq, 1), 1, (0, 1), "cuda")


def test_every_refusal_names_the_frame():
    from raht_3dgs_codec_amd import bitstream
    f = M.tiny_frame()
    cut = M.pframe(f)[:24 + bitstream.MIN_FRAME_BYTES - 1]               # a wrapper too short to hold a frame ...
    assert len(cut) >= bitstream.MIN_FRAME_BYTES                         # ... that the sequence container still takes
    broken = bytearray(f)
    broken[8 + 8] = 2                                                    # the frame header's N: no longer the geometry's
    bad = {
        "a predicted frame at index 0": ([M.pframe(f), f], 0),
        "ref_back = 0": ([f, M.pframe(f, 0, 0)], 1),
        "ref_back < 0": ([f, M.pframe(f, -1, 0)], 1),
        "ref_back reaches before frame 0": ([f, f, M.pframe(f, 3, 0)], 2),
        "up = 4": ([f, M.pframe(f, 1, 4)], 1),
        "up = -1": ([f, f, M.pframe(f, 1, -1)], 2),
        "a truncated wrapper": ([f, cut], 1),
        "an inner frame that parse_frame refuses": ([f, M.pframe(bytes(broken))], 1),
        "an inner frame of another magic": ([f, M.pframe(M.pframe(f))], 1),
        "inner D differs from the reference's": ([f, M.pframe(M.tiny_frame(D=4))], 1),
        "inner J differs from the reference's": ([f, f, M.pframe(M.tiny_frame(J=3))], 2),
        "J differs from a reference that is itself predicted": ([f, M.pframe(f), M.pframe(M.tiny_frame(J=3))], 2),
    }
    for what, (frames, i) in bad.items():
        seq = _seq(frames)
        assert bitstream.parse_sequence(seq)                             # the container itself is in order
        for call in (bitstream.sequence_kinds, bitstream.decode_sequence_bytes):       # both refuse from the headers: no device work
            with pytest.raises(ValueError, match=f"frame {i}:"):
                call(seq)
                pytest.fail(what)
    for blob in (cut, M.pframe(f, 0, 0), M.pframe(f, 1, 4), M.pframe(f)[:20]):
        with pytest.raises(ValueError):
            bitstream.parse_pframe(blob)
    # an intra frame's own corruption is still named, and asking for frames that do not depend on a bad one passes the headers
    with pytest.raises(ValueError, match="frame 0:"):
        bitstream.sequence_kinds(_seq([bytes(broken), f]))
    with pytest.raises(ValueError):
        bitstream.encode_sequence_bytes([], 6, 0.01, gop=5)
    for kw in (dict(gop=0), dict(up=4), dict(up=-1), dict(inter="never")):
        with pytest.raises(ValueError, match="gop"):
            bitstream.encode_sequence_bytes([(np.zeros((1, 3), np.int64), np.zeros((1, 2), np.float32))], 6, 0.01, device="cpu", **kw)
