"""The motion model (tests/numpy_motion.py) on cases whose answer is known without it, the candidate order, and the
compensated-frame wrapper at the host boundary: ``parse_mframe`` / ``sequence_kinds`` / ``sequence_motion`` on hand-built containers,
every refusal included. No GPU."""
import numpy as np
import pytest

from . import numpy_motion as MM
from . import numpy_predict as M


def _keys_and_rows(n=500, J=5, D=7, seed=3):
    from raht_3dgs_codec_amd import synth
    keys = synth.sorted_unique_keys(n, J, seed)
    rng = np.random.default_rng(seed)
    return keys, rng.normal(size=(len(keys), D)).astype(np.float32)


def test_morton_and_demorton_are_the_products():
    from raht_3dgs_codec_amd import synth
    rng = np.random.default_rng(1)
    V = rng.integers(0, 1 << 6, size=(200, 3))
    assert np.array_equal(MM.morton(V, 6), synth.morton_keys(V, 6).astype(np.uint64))
    assert np.array_equal(MM.demorton(MM.morton(V, 6), 6), V)


@pytest.mark.parametrize("up", [0, 1, 2, 3])
def test_a_zero_field_is_the_predictor_bit_for_bit(up):
    keys, C = _keys_and_rows()
    ref, Cr = _keys_and_rows(seed=4)
    for m in (1, 3, 5):
        _, first = MM.blocks(keys, m)
        P, n = MM.predict_mc(keys, ref, Cr, 5, m, np.zeros((len(first) - 1, 3), np.int8), up)
        P0, n0 = M.predict(keys, ref, Cr, up)
        assert n == n0 and np.array_equal(P.view(np.int32), P0.view(np.int32)), (up, m)


def test_a_translated_cloud_is_found_with_cost_zero():
    rng = np.random.default_rng(5)
    V = np.unique(rng.integers(4, 28, size=(300, 3)), axis=0)
    A = rng.normal(size=(len(V), 4)).astype(np.float32)
    k0 = MM.morton(V, 5)
    o0 = np.argsort(k0)
    k1 = MM.morton(V + (1, -2, 1), 5)
    o1 = np.argsort(k1)
    table, best_k, best_cost = MM.search(k1[o1], k0[o0], A[o0], A[o1], 5, 2, MM.candidates(2), np.ones(4, np.float32))
    assert not best_cost.any()
    assert np.all(MM.candidates(2)[best_k] == (-1, 2, -1))               # from the current voxel to the reference voxel: -t
    ok, _ = MM.shifted(k1[o1], 5, (0, 0, 40))
    assert not ok.any()                                                  # every row leaves the cube: no match, P = 0
    assert not MM.predict_v(k1[o1], k0[o0], A[o0], 5, (0, 0, 40))[0].any()


def test_the_cap_takes_inf_and_nan_and_zero_weights_leave_columns_out():
    X = np.array([[1.0, np.inf], [np.nan, 2.0], [3.0, 1e30], [0.5, 0.25]], np.float32)
    P = np.zeros_like(X)
    assert MM.row_cost(X, P, [1, 1]).tolist() == [2 ** 30, 2 ** 30, 2 ** 30, 768]
    assert MM.row_cost(X, P, [1, 0]).tolist() == [1024, 2 ** 30, 3072, 512]
    assert MM.row_cost(X, P, [0, 0]).tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("radius,K", [(1, 27), (2, 125), (3, 343)])
def test_candidate_order(radius, K):
    from raht_3dgs_codec_amd import ops
    c = ops.motion_candidates(radius)
    assert c.dtype == np.int32 and c.shape == (K, 3) and np.array_equal(c, MM.candidates(radius))
    assert not c[0].any()
    n2 = (c.astype(np.int64) ** 2).sum(axis=1)
    assert np.all(n2[1:] >= n2[:-1])                                     # norm-sorted
    rows = [tuple(int(x) for x in v) for v in c]
    assert len(set(rows)) == K and int(np.abs(c).max()) == radius        # the whole cube, every vector once
    assert rows == sorted(rows, key=lambda v: (v[0] ** 2 + v[1] ** 2 + v[2] ** 2,) + v)
    for bad in (0, 4, -1):
        with pytest.raises(ValueError, match="radius"):
            ops.motion_candidates(bad)


def _seq(frames):
    from raht_3dgs_codec_amd import bitstream
    return bitstream.pack_sequence(frames)


def test_kinds_motion_and_wrapper_of_hand_built_containers():
    from raht_3dgs_codec_amd import bitstream
    f = M.tiny_frame()                                                   # J = 2, one voxel: one block at every level
    seq = _seq([f, MM.mframe(f, 1, 0, 1, [(1, -2, 3)]), M.pframe(f, 1, 2), MM.mframe(f, 3, 3, 2, [(-128, 127, 0)]), f])
    assert bitstream.sequence_kinds(seq) == ["I", "P", "P", "P", "I"]
    mo = bitstream.sequence_motion(seq)
    assert mo[0] is None and mo[2] is None and mo[4] is None
    assert mo[1][0] == 1 and mo[1][1].dtype == np.int8 and mo[1][1].tolist() == [[1, -2, 3]]
    assert mo[3][0] == 2 and mo[3][1].tolist() == [[-128, 127, 0]]       # every int8 value is legal
    off = bitstream.parse_sequence(seq)
    assert off[2] - off[1] == len(f) + 40 + 8                            # the wrapper, three bytes of field, five of padding
    for i, want in ((1, (1, 0, 1)), (3, (3, 3, 2))):
        fb = bitstream.sequence_frame(seq, i)
        ref_back, up, m, mv, inner = bitstream.parse_mframe(fb)
        assert (ref_back, up, m) == want == MM.parse_mframe(fb)[:3]
        assert np.array_equal(mv, MM.parse_mframe(fb)[3]) and isinstance(inner, memoryview) and bytes(inner) == f == MM.parse_mframe(fb)[4]
    # the two public parsers and the sequence's own heads read one wrapper parser: the same ref_back and up, frame by frame
    for i, hd in enumerate(bitstream._sequence_heads(seq, None, None)):
        if hd["kind"] == "P":
            parse = bitstream.parse_pframe if hd["motion"] is None else bitstream.parse_mframe
            ref_back, up = parse(bitstream.sequence_frame(seq, i))[:2]
            assert (hd["ref"], hd["up"]) == (i - ref_back, up), i
        else:
            assert (hd["ref"], hd["up"], hd["motion"]) == (None, 0, None), i
    with pytest.raises(ValueError, match="not a RAHT motion-compensated frame wrapper"):
        bitstream.parse_mframe(M.pframe(f))
    with pytest.raises(ValueError, match="not a RAHT predicted-frame wrapper"):
        bitstream.parse_pframe(MM.mframe(f))
    # the one-frame decoders do not know the wrapper (header checks only: no device is touched): what they raise for a P frame
    with pytest.raises(ValueError, match="not a RAHT frame container"):
        bitstream.decode_frame_bytes(bitstream.sequence_frame(seq, 1), "cuda")
    with pytest.raises(ValueError, match="not a RAHT frame container"):
        bitstream.decode_region_bytes(bitstream.sequence_frame(seq, 1), 1, (0, 1), "cuda")


def test_every_refusal_names_the_frame():
    from raht_3dgs_codec_amd import bitstream
    f = M.tiny_frame()
    cut = MM.mframe(f)[:40 + 8 + bitstream.MIN_FRAME_BYTES - 1]          # a field, but no room for a frame behind it ...
    assert len(cut) >= bitstream.MIN_FRAME_BYTES                         # ... in a frame that the sequence container still takes
    long_field = MM.mframe(f, n_blocks=30)                               # announces 90 bytes of field: the frame behind is too short
    assert len(long_field) >= 40 + bitstream.MIN_FRAME_BYTES
    broken = bytearray(f)
    broken[8 + 8] = 2                                                    # the frame header's N: no longer the geometry's
    bad = {
        "block_log2 = 0": ([f, MM.mframe(f, block_log2=0)], 1),
        "block_log2 = -1": ([f, MM.mframe(f, block_log2=-1)], 1),
        "block_log2 = J + 1": ([f, MM.mframe(f, block_log2=3)], 1),
        "block_log2 = 22": ([f, MM.mframe(f, block_log2=22)], 1),
        "two vectors, one block in the geometry": ([f, MM.mframe(f, mv=[(0, 0, 1), (0, 0, 0)])], 1),
        "n_blocks = 0": ([f, MM.mframe(f, mv=np.zeros((0, 3)), pad=8)], 1),
        "n_blocks < 0": ([f, MM.mframe(f, n_blocks=-1)], 1),
        "too short for its field plus a frame": ([f, cut], 1),
        "a field longer than the wrapper": ([f, long_field], 1),
        "padding that is not zero": ([f, MM.mframe(f, pad=b"\0\0\0\0\1")], 1),
        "a compensated frame at index 0": ([MM.mframe(f), f], 0),
        "ref_back = 0": ([f, MM.mframe(f, 0)], 1),
        "ref_back < 0": ([f, MM.mframe(f, -1)], 1),
        "ref_back reaches before frame 0": ([f, f, MM.mframe(f, 3)], 2),
        "up = 4": ([f, MM.mframe(f, 1, 4)], 1),
        "up = -1": ([f, f, MM.mframe(f, 1, -1)], 2),
        "an inner frame that parse_frame refuses": ([f, MM.mframe(bytes(broken))], 1),
        "an inner frame of another magic": ([f, MM.mframe(M.pframe(f))], 1),
        "inner D differs from the reference's": ([f, MM.mframe(M.tiny_frame(D=4))], 1),
        "inner J differs from the reference's": ([f, f, MM.mframe(M.tiny_frame(J=3))], 2),
        "J differs from a reference that is itself compensated": ([f, MM.mframe(f), M.pframe(M.tiny_frame(J=3))], 2),
    }
    for what, (frames, i) in bad.items():
        seq = _seq(frames)
        assert bitstream.parse_sequence(seq)                             # the container itself is in order
        for call in (bitstream.sequence_kinds, bitstream.sequence_motion, bitstream.decode_sequence_bytes):   # from the headers: no device work
            with pytest.raises(ValueError, match=f"frame {i}:"):
                call(seq)
                pytest.fail(what)
    for blob in (cut, long_field, MM.mframe(f, 0), MM.mframe(f, 1, 4), MM.mframe(f, block_log2=0), MM.mframe(f, pad=b"\1\0\0\0\0"),
                 MM.mframe(f)[:30]):
        with pytest.raises(ValueError):
            bitstream.parse_mframe(blob)
    enc = [(np.zeros((1, 3), np.int64), np.zeros((1, 2), np.float32))]
    for kw in (dict(motion=-1), dict(motion=4), dict(motion=1, block_log2=0), dict(motion=1, block_log2=7)):
        with pytest.raises(ValueError, match="motion"):
            bitstream.encode_sequence_bytes(enc, 6, 0.01, device="cpu", gop=2, **kw)
