"""The frame-sequence container (bitstream.pack_sequence / parse_sequence / sequence_frame): pure host code.
    RAHTS001 | int64 n_frames | int64 offset[n_frames + 1] (from the start of the blob) | the frames"""
import numpy as np
import pytest


def _blobs(n, seed=0):
    from raht_3dgs_codec_amd import bitstream
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=bitstream.MIN_FRAME_BYTES + int(rng.integers(0, 500)), dtype=np.uint8).tobytes() for _ in range(n)]


@pytest.mark.parametrize("n", [1, 2, 13])
def test_round_trip_on_arbitrary_byte_strings(n):
    from raht_3dgs_codec_amd import bitstream
    blobs = _blobs(n, seed=n)
    seq = bitstream.pack_sequence(blobs)
    assert seq[:8] == b"RAHTS001" and len(seq) == 8 + 8 * (n + 2) + sum(len(b) for b in blobs)
    off = bitstream.parse_sequence(seq)
    assert len(off) == n + 1 and off[0] == 8 + 8 * (n + 2) and off[-1] == len(seq)
    assert bitstream.parse_sequence(seq, max_frames=n) == off
    for i, b in enumerate(blobs):
        v = bitstream.sequence_frame(seq, i)
        assert isinstance(v, memoryview) and bytes(v) == b
        assert bytes(bitstream.sequence_frame(seq, i, off)) == b
    for i in (-1, n):
        with pytest.raises(ValueError):
            bitstream.sequence_frame(seq, i)
    # bytearray and memoryview inputs
    assert bitstream.parse_sequence(bytearray(seq)) == off and bitstream.parse_sequence(memoryview(seq)) == off


def test_pack_refuses_nothing_and_stubs():
    from raht_3dgs_codec_amd import bitstream
    with pytest.raises(ValueError):
        bitstream.pack_sequence([])
    with pytest.raises(ValueError):
        bitstream.pack_sequence(_blobs(1) + [b"short"])


def _with_offsets(seq, off):
    return seq[:16] + np.asarray(off, np.int64).tobytes() + seq[16 + 8 * len(off):]


def test_refusals():
    from raht_3dgs_codec_amd import bitstream
    blobs = _blobs(3, seed=5)
    seq = bitstream.pack_sequence(blobs)
    off = bitstream.parse_sequence(seq)
    i64 = lambda x: np.array([x], np.int64).tobytes()                   # noqa: E731
    bad = {
        "wrong magic": b"RAHTF001" + seq[8:],
        "truncated magic": seq[:5],
        "truncated header (no count)": seq[:12],
        "truncated header (no offsets)": seq[:16],
        "truncated header (half the offsets)": seq[:16 + 8 * 2],
        "n_frames = 0": seq[:8] + i64(0) + seq[16:],
        "n_frames < 0": seq[:8] + i64(-3) + seq[16:],
        "n_frames = 2^40": seq[:8] + i64(2 ** 40) + seq[16:],
        "n_frames = 2^62": seq[:8] + i64(2 ** 62) + seq[16:],
        "n_frames one too many": seq[:8] + i64(4) + seq[16:],
        "offsets not ascending": _with_offsets(seq, [off[0], off[2], off[1], off[3]]),
        "two equal offsets": _with_offsets(seq, [off[0], off[1], off[1], off[3]]),
        "a negative offset": _with_offsets(seq, [off[0], -off[1], off[2], off[3]]),
        "first offset wrong": _with_offsets(seq, [off[0] + 8, off[1], off[2], off[3]]),
        "first offset 0": _with_offsets(seq, [0, off[1], off[2], off[3]]),
        "last offset beyond the blob": _with_offsets(seq, [off[0], off[1], off[2], off[3] + 1]),
        "last offset short of the blob": _with_offsets(seq, [off[0], off[1], off[2], off[3] - 1]),
        "blob cut": seq[:-1],
        "blob extended": seq + b"\0",
    }
    for what, blob in bad.items():
        with pytest.raises(ValueError):
            bitstream.parse_sequence(blob)
            pytest.fail(what)
    with pytest.raises(ValueError, match="more than the caller allows"):
        bitstream.parse_sequence(seq, max_frames=2)
    assert bitstream.parse_sequence(seq, max_frames=3) == off
