"""The block-mode model on the host (tests/numpy_block_modes.py): what the definition promises before any kernel is
asked -- identical references choose mode 0, a wipe chooses its side in every block and by a wide margin, the RAHTB002 builder and
parser round-trip, and the sequence's header checks refuse every malformed wrapper on hand-laid bytes, the frame named."""
import numpy as np

from . import numpy_block_modes as M
from . import numpy_motion as MM

J, D, STEP, M_LOG2 = 6, 5, 0.01, 2


def _scene():
    from raht_3dgs_codec_amd import synth
    V, keys, A = synth.scene(3000, J, D, seed=21)
    assert len(V) == 2779
    return V, np.asarray(keys, np.uint64), A.astype(np.float32)


def _wipe():
    V, keys, A = _scene()
    A0, A1, X, left = M.wipe(V, A, step=STEP)
    w = np.full(D, 1.0 / STEP, np.float32)
    return keys, (keys, A0), (keys, A1), X, left, w


def test_identical_references_choose_mode_0_everywhere():
    V, keys, A = _scene()
    X = (A + 1e-3 * np.random.default_rng(1).standard_normal(A.shape)).astype(np.float32)
    T, mode, best = M.search(keys, (keys, A), (keys, A), X, J, M_LOG2, np.full(D, 1.0 / STEP, np.float32))
    assert T.shape == (748, 4) and T.dtype == np.int64
    assert np.array_equal(T[:, 0], T[:, 1]) and np.array_equal(T[:, 0], T[:, 2])
    assert not mode.any() and mode.dtype == np.uint8 and np.array_equal(best, T[:, 0])


def test_a_wipe_chooses_its_side_in_every_block():
    keys, ref0, ref1, X, left, w = _wipe()
    T, mode, best = M.search(keys, ref0, ref1, X, J, M_LOG2, w)
    want = M.wipe_modes(keys, left, M_LOG2)
    assert (int((want == 1).sum()), int((want == 2).sum())) == (318, 430)
    assert np.array_equal(mode, want)
    rows = np.diff(MM.blocks(keys, M_LOG2)[1])
    assert rows.min() == 1 and rows.max() == 21


def test_the_second_best_cost_of_a_wipe_is_at_least_twice_the_best():
    keys, ref0, ref1, X, left, w = _wipe()
    T, mode, best = M.search(keys, ref0, ref1, X, J, M_LOG2, w)
    second = np.sort(T, axis=1)[:, 1]
    ratio = second / np.maximum(best, 1)
    print("second-best / best cost over the blocks: min %.2f median %.2f" % (ratio.min(), np.median(ratio)))
    assert np.all(second >= 2 * best) and best.min() > 0
    # the residual the frame is left with: the frame-wide mean against the per-block choice, in steps
    P0 = M.predictions(keys, ref0, ref1)[0]
    Pm = M.predict(keys, ref0, ref1, mode, J, M_LOG2)
    print("mean |residual| in steps: frame-wide mean %.2f, per-block modes %.2f" % (np.abs(X - P0).mean() / STEP, np.abs(X - Pm).mean() / STEP))
    assert np.abs(X - Pm).mean() < 0.1 * np.abs(X - P0).mean()


def test_the_predictor_under_uniform_modes_is_the_plain_predictors():
    keys, ref0, ref1, X, left, w = _wipe()
    Ps = M.predictions(keys, ref0, ref1)
    n_blocks = len(MM.blocks(keys, M_LOG2)[1]) - 1
    for k in range(4):
        P = M.predict(keys, ref0, ref1, np.full(n_blocks, k, np.uint8), J, M_LOG2)
        assert np.array_equal(P.view(np.int32), Ps[k].view(np.int32)), k
    assert np.array_equal(Ps[1], ref0[1]) and np.array_equal(Ps[2], ref1[1]) and not Ps[3].any()


def test_the_wrapper_builder_and_parser_round_trip():
    rng = np.random.default_rng(3)
    inner = bytes(rng.integers(0, 256, 300, dtype=np.uint8))
    for n in (1, 7, 8, 13):
        modes = rng.integers(0, 4, n).astype(np.uint8)
        mv0, mv1 = rng.integers(-128, 128, (2, n, 3)).astype(np.int8)
        for fields in (False, True):
            fb = M.bframe2(inner, modes, 2, 3, 1, 4, *((mv0, mv1) if fields else ()))
            assert fb[:8] == b"RAHTB002" and len(fb) == 56 + (2 * ((3 * n + 7) // 8 * 8) if fields else 0) + (n + 7) // 8 * 8 + len(inner)
            rb, rf, up, m, p0, p1, pm, pin = M.parse_bframe2(fb)
            assert (rb, rf, up, m) == (2, 3, 1, 4) and pin == inner and np.array_equal(pm, modes)
            if fields:
                assert np.array_equal(p0, mv0) and np.array_equal(p1, mv1)
            else:
                assert p0 is None and p1 is None
    # the knobs: another count, other padding, another flag word
    fb = M.bframe2(inner, [1, 2, 3], n_blocks=4, flags=2, pad=b"\x01" * 5)
    assert [int(x) for x in np.frombuffer(fb, np.int64, 2, 40)] == [4, 2] and fb[56:64] == b"\x01\x02\x03" + b"\x01" * 5


def test_the_sequence_checks_refuse_hand_laid_wrappers_without_a_device():
    import pytest
    from raht_3dgs_codec_amd import bitstream
    from . import numpy_predict as M1
    inner = M1.tiny_frame(J=2)                                           # one voxel: one block at every level
    good = M.bframe2(inner, [2], block_log2=1)
    seq = M1.sequence([inner, good, inner])
    assert bitstream.sequence_kinds(seq) == ["I", "B", "I"] == M.kinds(seq) and bitstream.sequence_refs(seq)[1] == (0, 2)
    modes = bitstream.sequence_modes(seq)
    assert modes[0] is None and modes[2] is None and modes[1].tolist() == [2] and modes[1].dtype == np.uint8
    assert bitstream.sequence_motion(seq) == [None] * 3
    rb, rf, up, m, mv0, mv1, md, pin = bitstream.parse_bframe2(good)
    assert (rb, rf, up, m, mv0, mv1) == (1, 1, 0, 1, None, None) and md.tolist() == [2] and bytes(pin) == inner
    fields = M.bframe2(inner, [3], 1, 1, 2, 2, mv0=[(1, -2, 3)], mv1=[(-128, 127, 0)])
    rb, rf, up, m, mv0, mv1, md, pin = bitstream.parse_bframe2(fields)
    assert (rb, rf, up, m) == (1, 1, 2, 2) and mv0.tolist() == [[1, -2, 3]] and mv1.tolist() == [[-128, 127, 0]] and md.tolist() == [3]
    assert bitstream.sequence_motion(M1.sequence([inner, fields, inner]))[1][0] == 2
    bad = {"a mode above 3": (1, [inner, M.bframe2(inner, [4], block_log2=1), inner]),
           "an unknown flag bit": (1, [inner, M.bframe2(inner, [1], block_log2=1, flags=2), inner]),
           "an unknown flag bit beside bit 0": (1, [inner, M.bframe2(inner, [1], block_log2=1, mv0=[(0, 0, 0)], mv1=[(0, 0, 0)], flags=5), inner]),
           "padding behind the modes": (1, [inner, M.bframe2(inner, [1], block_log2=1, pad=b"\x00" * 6 + b"\x01"), inner]),
           "padding behind a field": (1, [inner, M.bframe2(inner, [1], block_log2=1, mv0=[(0, 0, 0)], mv1=[(0, 0, 0)], pad=b"\x00" * 4 + b"\x01"), inner]),
           "n_blocks off by one": (1, [inner, M.bframe2(inner, [1, 0], block_log2=1), inner]),
           "n_blocks = 0": (1, [inner, M.bframe2(inner, [1], block_log2=1, n_blocks=0), inner]),
           "block_log2 = 0": (1, [inner, M.bframe2(inner, [1], block_log2=0), inner]),
           "block_log2 = J + 1": (1, [inner, M.bframe2(inner, [1], block_log2=3), inner]),
           "a wrapper cut short": (1, [inner, good[:56 + len(inner) - 1], inner]),
           "the frame at index 0": (0, [good, inner, inner]),
           "ref_fwd past the end": (1, [inner, M.bframe2(inner, [1], 1, 2, block_log2=1), inner]),
           "ref_back before frame 0": (1, [inner, M.bframe2(inner, [1], 2, 1, block_log2=1), inner]),
           "up = 4": (1, [inner, M.bframe2(inner, [1], up=4, block_log2=1), inner]),
           "a reference that is a B frame": (2, [inner, M.bframe2(inner, [1], 1, 2, block_log2=1), good, inner])}
    for what, (i, frames) in bad.items():
        for call in (bitstream.sequence_kinds, bitstream.sequence_modes, bitstream.sequence_refs):
            with pytest.raises(ValueError, match=f"frame {i}:"):
                call(M1.sequence(frames))
                pytest.fail(what)
    with pytest.raises(ValueError, match="not a RAHT B-frame wrapper"):
        bitstream.parse_bframe2(inner)
    with pytest.raises(ValueError, match="not a RAHT frame container"):
        bitstream.parse_frame(good)
