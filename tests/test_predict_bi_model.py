"""The two-reference predictor's definition (tests/numpy_predict_bi.py) on cases whose answer is known without it, the structure
``sequence_plan`` gives a sequence, and the B-frame wrapper at the host boundary: ``parse_bframe`` / ``sequence_kinds`` /
``sequence_refs`` / ``sequence_motion`` on hand-built containers, every refusal included. No GPU."""
import numpy as np
import pytest

from . import numpy_motion as MM
from . import numpy_octree as MO
from . import numpy_octree_inter as MI
from . import numpy_predict as M1
from . import numpy_predict_bi as M


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _scene(n=600, J=5, D=7, seed=5):
    from raht_3dgs_codec_amd import synth
    keys = synth.sorted_unique_keys(n, J, seed)
    other = synth.sorted_unique_keys(n, J, seed + 1)
    rng = np.random.default_rng(seed)
    return keys, other, rng.normal(size=(len(keys), D)).astype(np.float32), rng.normal(size=(len(other), D)).astype(np.float32)


def test_a_row_with_a_run_in_one_reference_only_is_the_one_reference_model():
    keys, other, C, Co = _scene()
    J = 5
    thin = (keys[::3], C[::3])
    for up in range(4):
        P, (n0, n1, nb), h0, h1 = M.predict(keys, thin, (other, Co), up)
        assert (h0 & ~h1).any() and (h1 & ~h0).any() and (h0 & h1).any(), up
        assert (~h0 & ~h1).any() or up > 1, up                           # (64 cells at up = 3: none is empty in both)
        assert (n0, n1, nb) == (h0.sum(), h1.sum(), (h0 & h1).sum())
        P0 = M1.predict(keys, *thin, up)[0]
        P1 = M1.predict(keys, other, Co, up)[0]
        assert np.array_equal(_bits(P[h0 & ~h1]), _bits(P0[h0 & ~h1])), up
        assert np.array_equal(_bits(P[h1 & ~h0]), _bits(P1[h1 & ~h0])), up
        assert not _bits(P[~h0 & ~h1]).any(), up                         # +0, not -0
    # under fields: against the compensated one-reference model
    _, first = MM.blocks(keys, 2)
    rng = np.random.default_rng(1)
    mv0, mv1 = (rng.integers(-3, 4, (len(first) - 1, 3)).astype(np.int8) for _ in range(2))
    P, _, h0, h1 = M.predict(keys, thin, (other, Co), 1, J, 2, mv0, mv1)
    assert (h0 & ~h1).any() and (h1 & ~h0).any()
    assert np.array_equal(_bits(P[h0 & ~h1]), _bits(MM.predict_mc(keys, *thin, J, 2, mv0, 1)[0][h0 & ~h1]))
    assert np.array_equal(_bits(P[h1 & ~h0]), _bits(MM.predict_mc(keys, other, Co, J, 2, mv1, 1)[0][h1 & ~h0]))
    Pz = M.predict(keys, thin, (other, Co), 1, J, 2, np.zeros_like(mv0), np.zeros_like(mv1))[0]
    assert np.array_equal(_bits(Pz), _bits(M.predict(keys, thin, (other, Co), 1)[0]))      # all-zero fields: no fields


def test_identical_references_are_the_one_reference_model():
    keys, other, C, Co = _scene()
    Co[0, 0], Co[1, 1], Co[2, 2] = np.float32(-0.0), np.float32(3.0000002), np.float32(1e30)
    for up in range(4):
        P, (n0, n1, nb), _, _ = M.predict(keys, (other, Co), (other, Co), up)
        want, n = M1.predict(keys, other, Co, up)
        assert n0 == n1 == nb == n
        assert np.array_equal(_bits(P), _bits(want)), up


def test_a_ramp_of_small_integers_has_no_residual():
    keys, _, _, _ = _scene()
    rng = np.random.default_rng(9)
    C0 = rng.integers(-50, 50, (len(keys), 4)).astype(np.float32)
    X = rng.integers(-50, 50, (len(keys), 4)).astype(np.float32)
    C1 = np.float32(2) * X - C0
    P = M.predict(keys, (keys, C0), (keys, C1))[0]
    R = M.apply(X, P)
    assert not R.any()
    assert np.array_equal(_bits(M.apply(R, P, add=True)), _bits(X))


def test_the_sum_is_rounded_before_the_product_and_may_overflow():
    k = np.array([3], np.uint64)
    big = np.array([[3e38]], np.float32)
    P = M.predict(k, (k, big), (k, big))[0]
    assert np.isinf(P[0, 0])                                             # fl(3e38 + 3e38) = inf, and 0.5 inf = inf
    a, b = np.array([[1.0]], np.float32), np.array([[np.float32(2.0 ** -24)]], np.float32)
    assert M.predict(k, (k, a), (k, b))[0][0, 0] == np.float32(0.5)      # 1 + 2^-24 rounds to 1 (ties to even) before the product


def test_sequence_plan():
    from raht_3dgs_codec_amd.bitstream import sequence_plan
    p = sequence_plan(5, 5, 1)
    assert [k for k, _ in p] == list("IBPBP") and [r for _, r in p] == [(), (0, 2), (0,), (2, 4), (2,)]
    p = sequence_plan(7, 7, 2)
    assert [k for k, _ in p] == list("IBBPBBP") and [r for _, r in p] == [(), (0, 3), (0, 3), (0,), (3, 6), (3, 6), (3,)]
    p = sequence_plan(6, 4, 1)                                           # GOP 0: anchors {0, 2, 3}, B {1}; GOP 1: anchors {4, 5}
    assert [k for k, _ in p] == list("IBPPIP") and [r for _, r in p] == [(), (0, 2), (0,), (2,), (), (4,)]
    for n in (1, 2, 5):
        for b in (1, 2, 7):
            assert "B" not in [k for k, _ in sequence_plan(n, 2, b)]     # a GOP of two frames has nothing between its anchors
            assert [k for k, _ in sequence_plan(n, 1, b)] == ["I"] * n
    for n, gop in ((1, 3), (7, 3), (8, 4), (5, 8)):
        p = sequence_plan(n, gop, 0)                                     # bframes = 0: chains with ref_back 1
        assert p == sequence_plan(n, gop) == [("I", ()) if i % gop == 0 else ("P", (i - 1,)) for i in range(n)]
    for n in range(1, 20):                                               # every B frame lies strictly between two anchors of its GOP
        for gop in range(1, 9):
            for b in range(4):
                p = sequence_plan(n, gop, b)
                assert len(p) == n
                for i, (kind, refs) in enumerate(p):
                    assert kind == ("I" if i % gop == 0 else kind)
                    assert all(p[r][0] != "B" and r // gop == i // gop for r in refs)
                    if kind == "B":
                        a, c = refs
                        assert a < i < c and c - a <= b + 1 and all(p[j][0] == "B" for j in range(a + 1, c))
                    elif kind == "P":
                        assert refs[0] < i and all(p[j][0] == "B" for j in range(refs[0] + 1, i))
                    else:
                        assert refs == ()
    for bad in ((0, 1, 0), (3, 0, 0), (3, 2, -1)):
        with pytest.raises(ValueError):
            sequence_plan(*bad)


def _seq(frames):
    from raht_3dgs_codec_amd import bitstream
    return bitstream.pack_sequence(frames)


def test_kinds_refs_motion_and_wrapper_of_hand_built_containers():
    from raht_3dgs_codec_amd import bitstream
    f = M1.tiny_frame()
    mv0, mv1 = [[1, -2, 3]], [[-128, 127, 0]]                             # every int8 vector is legal
    seq = _seq([f, M.bframe(f), M1.pframe(f, 2, 1), M.bframe(f, 1, 1, 2, 1, mv0, mv1), MM.mframe(f, 2, 0, 2, [(0, 1, 0)])])
    assert bitstream.sequence_kinds(seq) == ["I", "B", "P", "B", "P"] == M.kinds(seq)
    assert bitstream.sequence_refs(seq) == [(), (0, 2), (0,), (2, 4), (2,)]
    mo = bitstream.sequence_motion(seq)
    assert mo[0] is None and mo[1] is None and mo[2] is None and len(mo[3]) == 3 and len(mo[4]) == 2
    assert mo[3][0] == 1 and mo[3][1].tolist() == mv0 and mo[3][2].tolist() == mv1 and mo[3][1].dtype == np.int8
    fb = bitstream.sequence_frame(seq, 1)
    assert len(fb) == len(f) + 48 == len(f) + bitstream.B_HEAD
    rb, rf, up, m, a, b, inner = bitstream.parse_bframe(fb)
    assert (rb, rf, up, m, a, b) == (1, 1, 0, 0, None, None) == M.parse_bframe(fb)[:6] and bytes(inner) == f
    fb = bitstream.sequence_frame(seq, 3)
    assert len(fb) == len(f) + 48 + 16
    rb, rf, up, m, a, b, inner = bitstream.parse_bframe(fb)
    assert (rb, rf, up, m) == (1, 1, 2, 1) == M.parse_bframe(fb)[:4] and a.tolist() == mv0 and b.tolist() == mv1
    assert isinstance(inner, memoryview) and bytes(inner) == f == M.parse_bframe(fb)[6]
    with pytest.raises(ValueError, match="not a RAHT B-frame wrapper"):
        bitstream.parse_bframe(f)
    with pytest.raises(ValueError, match="not a RAHT B-frame wrapper"):
        bitstream.parse_bframe(M1.pframe(f))
    with pytest.raises(ValueError, match="not a RAHT predicted-frame wrapper"):
        bitstream.parse_pframe(fb)
    # the one-frame decoders do not know the wrapper (header checks only: no device is touched)
    with pytest.raises(ValueError, match="not a RAHT frame container"):
        bitstream.decode_frame_bytes(fb, "cuda")
    with pytest.raises(ValueError, match="not a RAHT frame container"):
        bitstream.decode_region_bytes(fb, 1, (0, 1), "cuda")
    # a region of a B frame is refused from the headers, by name
    with pytest.raises(ValueError, match="frame 3 is a B frame"):
        bitstream.decode_sequence_region(seq, 3, 1, (0, 1), "cuda")


def _geo_frames():
    """(an intra frame, an intra frame of one voxel fewer, a frame of other voxels whose geometry section is predicted from the
    first's keys), J = 3, D = 5"""
    from raht_3dgs_codec_amd import synth
    J, D = 3, 5
    keys, ref = synth.sorted_unique_keys(40, J, 11), synth.sorted_unique_keys(30, J, 12)

    def frame(geo, N):
        att = b"RLGS0001" + np.array([N, D, 2048, 1, 0], np.int64).tobytes() + bytes(4 * D)       # every segment empty
        return MO.frame_container(J, N, D, 0, [0.02], geo, att)
    return (frame(MO.geometry_section(ref, J, 0), len(ref)), frame(MO.geometry_section(ref[:-1], J, 0), len(ref) - 1),
            frame(MI.section(keys, ref, J, 0), len(keys)), len(ref))


def test_every_refusal_names_the_frame(monkeypatch):
    import torch
    from raht_3dgs_codec_amd import bitstream

    def touched(*a, **k):
        raise AssertionError("device work before the headers were judged")
    for name in ("init", "_lazy_init", "synchronize"):
        monkeypatch.setattr(torch.cuda, name, touched)
    f = M1.tiny_frame()                                                  # J = 2, one voxel: every level has one cell
    z = [(0, 0, 0)]
    cut = M.bframe(f)[:48 + bitstream.MIN_FRAME_BYTES - 1]               # a wrapper too short to hold a frame ...
    assert len(cut) >= bitstream.MIN_FRAME_BYTES                         # ... that the sequence container still takes
    wz = M.bframe(f, 1, 1, 0, 1, z, z)                                   # 48 bytes, then per field 3 bytes and 5 of padding
    cut_fields = wz[:48 + 16 + bitstream.MIN_FRAME_BYTES - 1]
    intra, shorter, predicted, n_ref = _geo_frames()
    bad = {
        "a B frame at index 0": ([M.bframe(f), f, f], 0),
        "ref_back = 0": ([f, M.bframe(f, 0, 1), f], 1),
        "ref_back < 0": ([f, M.bframe(f, -1, 1), f], 1),
        "ref_back reaches before frame 0": ([f, M.bframe(f, 2, 1), f], 1),
        "ref_fwd = 0": ([f, M.bframe(f, 1, 0), f], 1),
        "ref_fwd < 0": ([f, M.bframe(f, 1, -2), f], 1),
        "ref_fwd reaches past the last frame": ([f, f, M.bframe(f, 1, 1)], 2),
        "ref_fwd reaches far past the last frame": ([f, M.bframe(f, 1, 2), f], 1),
        "up = 4": ([f, M.bframe(f, 1, 1, 4), f], 1),
        "up = -1": ([f, M.bframe(f, 1, 1, -1), f], 1),
        "block_log2 without blocks": ([f, M.bframe(f, 1, 1, 0, 1), f], 1),
        "blocks without block_log2": ([f, M.bframe(f, 1, 1, 0, 0, z, z), f], 1),
        "block_log2 < 0": ([f, M.bframe(f, 1, 1, 0, -1, z, z), f], 1),
        "block_log2 = 22": ([f, M.bframe(f, 1, 1, 0, 22, z, z), f], 1),
        "block_log2 > J": ([f, M.bframe(f, 1, 1, 0, 3, z, z), f], 1),
        "n_blocks is not the geometry's level count": ([f, M.bframe(f, 1, 1, 0, 1, z + z, z + z), f], 1),
        "n_blocks announced one too many": ([f, M.bframe(f, 1, 1, 0, 1, z, z, n_blocks=2), f], 1),
        "n_blocks < 0": ([f, M.bframe(f, 1, 1, 0, 1, z, z, n_blocks=-1), f], 1),
        "non-zero padding behind field 0": ([f, wz[:48 + 7] + b"\x01" + wz[48 + 8:], f], 1),
        "non-zero padding behind field 1": ([f, wz[:48 + 8 + 5] + b"\x07" + wz[48 + 8 + 6:], f], 1),
        "a truncated wrapper": ([f, cut, f], 1),
        "a wrapper truncated behind its fields": ([f, cut_fields, f], 1),
        "reference 1 is a B frame": ([f, M.bframe(f, 1, 1), M.bframe(f, 2, 1), f], 1),
        "reference 0 is a B frame": ([f, M.bframe(f, 1, 2), M.bframe(f, 1, 1), f], 2),
        "a P frame whose reference is a B frame": ([f, M.bframe(f, 1, 2), M1.pframe(f), f], 2),
        "reference 0's D differs": ([M1.tiny_frame(D=4), M.bframe(f), f], 1),
        "reference 1's D differs": ([f, M.bframe(f), M1.tiny_frame(D=4)], 1),
        "reference 0's J differs": ([M1.tiny_frame(J=3), M.bframe(f), f], 1),
        "reference 1's J differs": ([f, M.bframe(f), M1.tiny_frame(J=3)], 1),
        "an inner frame of another magic": ([f, M.bframe(M.bframe(f)), f], 1),
        "predicted geometry from another voxel count than reference 0's": ([shorter, M.bframe(predicted), intra], 1),
    }
    for what, (frames, i) in bad.items():
        seq = _seq(frames)
        assert bitstream.parse_sequence(seq)                             # the container itself is in order
        for call in (bitstream.sequence_kinds, bitstream.sequence_refs, bitstream.sequence_motion, bitstream.decode_sequence_bytes):
            with pytest.raises(ValueError, match=f"frame {i}:"):
                call(seq)
                pytest.fail(what)
    # the same predicted section against reference 0 of the right size passes the headers, whatever reference 1 holds
    good = _seq([intra, M.bframe(predicted), shorter])
    assert bitstream.sequence_kinds(good) == ["I", "B", "I"] and bitstream.sequence_geometry(good) == ["intra", "predicted", "intra"]
    assert bitstream.parse_frame(predicted)["geometry_ref"] == n_ref
    # what parse_bframe judges by itself
    for blob in (cut, cut_fields, M.bframe(f, 0, 1), M.bframe(f, 1, 0), M.bframe(f, 1, 1, 4), M.bframe(f, 1, 1, 0, 1),
                 M.bframe(f, 1, 1, 0, 0, z, z), M.bframe(f, 1, 1, 0, 22, z, z), M.bframe(f, 1, 1, 0, 1, z, z, n_blocks=2 ** 31),
                 M.bframe(f, 1, 1, 0, 1, z, z, pad=b"\0\0\0\0\x07"), M.bframe(f)[:40]):
        with pytest.raises(ValueError):
            bitstream.parse_bframe(blob)
    # asking for frames that do not depend on a bad B frame passes the headers: its bytes are not parsed
    seq = _seq([f, M.bframe(f, 1, 1, 4), M1.pframe(f, 2, 0)])
    with pytest.raises(ValueError, match="frame 1:"):
        bitstream.sequence_kinds(seq)
    assert sorted(bitstream._frame_heads(memoryview(seq), bitstream.parse_sequence(seq), [0, 2], None)) == [0, 2]
    for kw in (dict(bframes=-1),):
        with pytest.raises(ValueError, match="bframes"):
            bitstream.encode_sequence_bytes([(np.zeros((1, 3), np.int64), np.zeros((1, 2), np.float32))], 6, 0.01, device="cpu", gop=4, **kw)
