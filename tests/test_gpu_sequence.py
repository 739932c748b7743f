"""A sequence of frames as bytes (bitstream.encode_sequence_bytes / decode_sequence_bytes): a container of ordinary
frame containers whose transform and entropy stages ran in common launches. Frame i of it is ``encode_frame_bytes`` of that frame
byte for byte, what comes out of it is ``decode_frame_bytes`` of its slice bit for bit, and the one-frame tools (the region
decoder) work on the slices."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

J, S = 6, 64


def _hand(n, D, seed):
    """a frame of n <= 8 voxels, in Morton order whichever axis leads: all three coordinates ascend together"""
    rng = np.random.default_rng(seed)
    V = np.array([[2, 3, 1], [5, 5, 5], [9, 8, 8], [17, 16, 18], [33, 32, 32], [34, 34, 34], [40, 41, 40], [60, 60, 61]][:n], np.int64)
    return V, rng.normal(size=(n, D)).astype(np.float32)


def _build(name):
    from raht_3dgs_codec_amd import synth
    if name == "A":                                                     # float32 path, scalar step, frames of one and of two voxels
        D, n_wide, step = 5, 0, 0.02                                    # ... and two of exactly D voxels: the coder reads a square matrix its own way
        frames = [synth.scene(3000, J, D, seed=41)[::2], synth.scene(700, J, D, seed=42)[::2], synth.scene(3000, J, D, seed=43)[::2],
                  _hand(1, D, 1), _hand(2, D, 2), _hand(D, D, 3), _hand(D, D, 4), _hand(D + 1, D, 5)]
    elif name == "B":                                                   # xyz wide, per-channel steps
        D, n_wide = 59, 3
        step = [0.004 * (1 + (c % 7)) for c in range(D)]
        frames = [synth.scene(n, J, D, seed=50 + i)[::2] for i, n in enumerate((3000, 1500, 40))]
    else:                                                               # 13 small frames: two chunks of the 12 a launch takes
        D, n_wide, step = 3, 0, 0.05
        frames = [synth.scene(60 + 37 * i, J, D, seed=60 + i)[::2] for i in range(12)] + [_hand(D, D, 6)]       # (the last: D voxels)
    return frames, D, n_wide, step


_CACHE = {}


def _sequence(name):
    """(frames, n_wide, step, sequence blob, [one-frame blobs], [one-frame decodes]), computed once and left unchanged"""
    from raht_3dgs_codec_amd import bitstream
    if name not in _CACHE:
        frames, D, n_wide, step = _build(name)
        seq = bitstream.encode_sequence_bytes(frames, J, step, "cuda", n_wide=n_wide, seg_len=S, vmin=(0.5, -1.0, 2.0), width=3.0)
        alone = [bitstream.encode_frame_bytes(V, A, J, step, "cuda", n_wide=n_wide, seg_len=S, vmin=(0.5, -1.0, 2.0), width=3.0) for V, A in frames]
        dec = [bitstream.decode_frame_bytes(b, "cuda") for b in alone]
        _CACHE[name] = (frames, n_wide, step, seq, alone, dec)
    return _CACHE[name]


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_a_sequence_is_its_frames(name):
    import torch
    from raht_3dgs_codec_amd import bitstream
    frames, n_wide, step, seq, alone, dec = _sequence(name)
    off = bitstream.parse_sequence(seq)
    assert len(off) == len(frames) + 1
    for i, b in enumerate(alone):
        assert bytes(bitstream.sequence_frame(seq, i)) == b, (name, i)
    out = bitstream.decode_sequence_bytes(seq, device="cuda")
    assert len(out) == len(frames)
    for i, ((V, C), (V1, C1), (V0, _)) in enumerate(zip(out, dec, frames)):
        assert V.dtype == torch.int64 and C.dtype == torch.float32
        assert torch.equal(V, V1) and np.array_equal(V.cpu().numpy(), V0), (name, i)
        assert torch.equal(C.view(torch.int32), C1.view(torch.int32)), (name, i)                       # bit for bit
    # ... and of the slice itself
    V2, C2 = bitstream.decode_frame_bytes(bitstream.sequence_frame(seq, 1), "cuda")
    assert torch.equal(V2, out[1][0]) and torch.equal(C2, out[1][1])
    # chosen frames, in the order they were asked for
    two = bitstream.decode_sequence_bytes(seq, frames=[2, 0])
    assert len(two) == 2
    for (V, C), i in zip(two, (2, 0)):
        assert torch.equal(V, dec[i][0]) and torch.equal(C, dec[i][1]), (name, i)
    for bad in ([len(frames)], [-1], 3):
        with pytest.raises(ValueError):
            bitstream.decode_sequence_bytes(seq, frames=bad)
    with pytest.raises(ValueError):
        bitstream.decode_sequence_bytes(seq, max_frames=len(frames) - 1)
    with pytest.raises(ValueError, match="frame 0"):
        bitstream.decode_sequence_bytes(seq, max_voxels=frames[0][0].shape[0] - 1)
    # the region decoder on a slice
    Vr, Cr, info = bitstream.decode_region_bytes(bitstream.sequence_frame(seq, 0), 1, (0, 4), "cuda")
    a, b = info["rows"]
    assert a == 0 and 0 < b < frames[0][0].shape[0]                     # cells 0 .. 3 of 8 at depth 1: the first half of the Morton order
    assert torch.equal(Vr, dec[0][0][a:b])
    assert torch.equal(Cr, dec[0][1][a:b])                              # (bit-identical to the whole-frame decoder: tests/test_gpu_region.py)


def test_frames_of_different_kinds_are_groups_of_one():
    """pack_sequence of frames that share nothing (D, n_wide, steps): every frame takes the one-frame path"""
    import torch
    from raht_3dgs_codec_amd import bitstream
    a = _sequence("A")
    b = _sequence("B")
    blobs = [a[4][1], b[4][2], a[4][0]]
    seq = bitstream.pack_sequence(blobs)
    out = bitstream.decode_sequence_bytes(seq)
    for (V, C), (V1, C1) in zip(out, (a[5][1], b[5][2], a[5][0])):
        assert torch.equal(V, V1) and torch.equal(C, C1)


def test_a_corrupt_frame_is_named_and_the_others_still_decode():
    import torch
    from raht_3dgs_codec_amd import bitstream
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    frames, n_wide, step, seq, alone, dec = _sequence("A")
    off = bitstream.parse_sequence(seq)
    h = bitstream.parse_frame(bitstream.sequence_frame(seq, 1))
    ao, _ = h["attributes"]
    table = off[1] + ao + len(SegmentedCoder.MAGIC) + 40                # the uint32 length of frame 1's first attribute segment
    bad = bytearray(seq)
    bad[table] ^= 0xFF
    bad = bytes(bad)
    with pytest.raises(ValueError, match="frame 1"):
        bitstream.decode_sequence_bytes(bad)
    with pytest.raises(ValueError):
        bitstream.decode_frame_bytes(bitstream.sequence_frame(bad, 1), "cuda")
    (V, C), = bitstream.decode_sequence_bytes(bad, frames=[0])
    assert torch.equal(V, dec[0][0]) and torch.equal(C, dec[0][1])
    # a table that still adds up but points a segment's bytes elsewhere is caught by the decoder's own bounds, not here; one that no
    # longer adds up never reaches the device
    with pytest.raises(ValueError):
        bitstream.encode_sequence_bytes([], J, 0.01)
    with pytest.raises(ValueError, match="frame 1"):
        bitstream.encode_sequence_bytes([frames[0], (frames[1][0], frames[1][1][:, :3])], J, 0.01)


def test_frames_of_exactly_D_voxels():
    """N == D: the one-frame coder reads the square matrix of such a frame as (D, N). In a sequence the frame gets the same bytes
    and the same voxels back, alone, among others and when blobs of ``encode_frame_bytes`` are packed side by side."""
    import torch
    from raht_3dgs_codec_amd import bitstream
    frames, n_wide, step, seq, alone, dec = _sequence("A")
    D = frames[0][1].shape[1]
    square = [i for i, (V, _) in enumerate(frames) if V.shape[0] == D]
    assert len(square) == 2 and square[1] == square[0] + 1
    for i in square:
        assert bytes(bitstream.sequence_frame(seq, i)) == alone[i]
        # what comes back is the frame, not its transpose (unit normal attributes: a transposed matrix would be off by about 1). The
        # transform keeps norms and every coefficient is off by half a step at most, so a column's error has norm <= step / 2 * sqrt(N),
        # which bounds its largest entry; float32 arithmetic on values of a few units adds far less than the 1e-4 allowed for it
        V, C = dec[i]
        assert torch.equal(V.cpu(), torch.from_numpy(frames[i][0]))
        assert float((C.cpu() - torch.from_numpy(frames[i][1])).abs().max()) <= 0.5 * step * D ** 0.5 + 1e-4
    for pick in (square, [square[1], 0, square[0]], [square[0]]):
        for (V, C), i in zip(bitstream.decode_sequence_bytes(seq, frames=pick), pick):
            assert torch.equal(V, dec[i][0]) and torch.equal(C, dec[i][1]), (pick, i)
    packed = bitstream.pack_sequence([alone[i] for i in square] + [alone[-1]])
    for (V, C), i in zip(bitstream.decode_sequence_bytes(packed), square + [len(frames) - 1]):
        assert torch.equal(V, dec[i][0]) and torch.equal(C, dec[i][1]), i
    only = bitstream.encode_sequence_bytes([frames[i] for i in square], J, step, "cuda", n_wide=n_wide, seg_len=S, vmin=(0.5, -1.0, 2.0), width=3.0)
    assert [bytes(bitstream.sequence_frame(only, k)) for k in range(2)] == [alone[i] for i in square]
