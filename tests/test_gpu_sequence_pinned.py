"""Inter-coded sequences against recorded results (tests/golden/sequence_digests.json: SHA-256 of the sequence blob and of every
decoded frame's attribute bytes, per case name; ``digest`` below is what wrote it and what is compared with it): the frame sets of
test_gpu_sequence_inter.py and test_gpu_sequence_motion.py under every mode of the encoder; one sequence in which ``inter="auto"``
takes all three of its outcomes; and a reference carried across a ``SEQ_CHUNK`` boundary."""
import hashlib
import json
import os

import numpy as np
import pytest

from . import test_gpu_sequence_inter as INTER
from . import test_gpu_sequence_motion as MOTION

pytestmark = pytest.mark.gpu

J, STEP, BLOCK, FRAMES = INTER.J, INTER.STEP, MOTION.BLOCK, INTER.FRAMES
SHAPES = INTER.SHAPES
KW = INTER.KW
SETS = [("static", 0), ("drifting", 0), ("drifting", 1), ("independent", 0), ("moving", 0)]     # (frame set, up)
MODES = [(inter, motion) for inter in ("auto", "always") for motion in (0, 1)]
LONG_J, LONG_FRAMES, LONG_BLOCK = 5, 14, 3
DIGESTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sequence_digests.json")
_CACHE = {}


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def digest(blob, dec):
    """what the digest file holds for one case"""
    return dict(blob=_sha(blob), frames=[_sha(np.ascontiguousarray(C.cpu().numpy()).tobytes()) for _, C in dec])


def _recorded(name):
    if "digests" not in _CACHE:
        with open(DIGESTS) as f:
            _CACHE["digests"] = json.load(f)
    return _CACHE["digests"][name]


def _frames(kind, D):
    return MOTION._frames(kind, D) if kind == "moving" else INTER._frames(kind, D)


def _mixed_frames(D):
    """a base frame, the base with other noise, that frame moved by one voxel, an unrelated scene, the base again"""
    still, moving = MOTION._frames("static", D), MOTION._frames("moving", D)
    return [still[0], still[1], moving[1], INTER._frames("independent", D)[0], still[0]]


def _long_frames(D):
    """test_gpu_sequence_motion's moving cloud at J = 5: a few hundred voxels, one voxel a frame for 14 frames"""
    from raht_3dgs_codec_amd import synth
    rng = np.random.default_rng(41)
    V = np.unique(rng.integers((0, 0, 13), (19, 32, 32), size=(400, 3)), axis=0).astype(np.int64)       # 13 steps of (1, 0, -1) stay inside
    A = synth.gaussian_attributes(len(V), D, 42)
    out = []
    for t in range(LONG_FRAMES):
        Vt = V + t * np.array(MOTION.STEP_T, np.int64)
        At = (A + MOTION.SIGMA * rng.standard_normal(A.shape)).astype(np.float32)
        o = np.argsort(synth.morton_keys(Vt, LONG_J), kind="stable")
        out.append((Vt[o], np.ascontiguousarray(At[o])))
    return out


def _coded(name, frames, J, n_wide, **enc):
    """(blob, full decode) of a case, computed once and left unchanged"""
    from raht_3dgs_codec_amd import bitstream
    if name not in _CACHE:
        blob = bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", n_wide=n_wide, **KW, **enc)
        _CACHE[name] = (blob, bitstream.decode_sequence_bytes(blob, device="cuda"))
    return _CACHE[name]


def coded_set(kind, up, D, n_wide):
    """{case name: (blob, full decode)} of one frame set under the four modes"""
    return {f"{kind}-up{up}-D{D}-{inter}-motion{motion}":
            _coded(f"{kind}-up{up}-D{D}-{inter}-motion{motion}", _frames(kind, D), J, n_wide, gop=FRAMES, up=up, inter=inter,
                   motion=motion, block_log2=BLOCK) for inter, motion in MODES}


def coded_mixed(D, n_wide):
    return _coded(f"mixed-D{D}", _mixed_frames(D), J, n_wide, gop=5, inter="auto", motion=1, block_log2=BLOCK)


def coded_long(D, n_wide):
    return _coded(f"long-D{D}", _long_frames(D), LONG_J, n_wide, gop=LONG_FRAMES, inter="always", motion=1, block_log2=LONG_BLOCK)


def _same_bits(a, b):
    import torch
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.mark.parametrize("D,n_wide", SHAPES)
@pytest.mark.parametrize("kind,up", SETS)
def test_blobs_and_decoded_frames_are_the_recorded_ones(kind, up, D, n_wide):
    for name, (blob, dec) in coded_set(kind, up, D, n_wide).items():
        assert len(dec) == FRAMES
        assert digest(blob, dec) == _recorded(name), name


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_auto_takes_each_of_its_three_outcomes_in_one_sequence(D, n_wide):
    from raht_3dgs_codec_amd import bitstream
    blob, dec = coded_mixed(D, n_wide)
    kinds, motion = bitstream.sequence_kinds(blob), bitstream.sequence_motion(blob)
    print("kinds:", kinds, "motion fields:", [None if m is None else m[1].tolist()[:2] for m in motion])
    assert kinds[:4] == ["I", "P", "P", "I"]                             # frame 3: intra at an index that is no multiple of gop
    assert motion[1] is None                                             # a plain P frame: the search found no motion
    assert motion[2] is not None and motion[2][0] == BLOCK and motion[2][1].any()         # a P frame with a motion field
    assert bytes(bitstream.sequence_frame(blob, 1)[:8]) == b"RAHTP001" and bytes(bitstream.sequence_frame(blob, 2)[:8]) == b"RAHTM001"
    assert bytes(bitstream.sequence_frame(blob, 3)[:8]) == b"RAHTF001"
    assert digest(blob, dec) == _recorded(f"mixed-D{D}")
    for i in range(len(dec)):
        one, = bitstream.decode_sequence_bytes(blob, frames=[i])
        assert _same_bits(one, dec[i]), i


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_the_reference_is_carried_across_a_chunk_boundary(D, n_wide):
    import torch
    from raht_3dgs_codec_amd import bitstream
    assert LONG_FRAMES > bitstream.SEQ_CHUNK + 1                         # the second chunk holds a frame predicted from a frame of its own
    frames = _long_frames(D)
    blob, dec = coded_long(D, n_wide)
    assert len(dec) == LONG_FRAMES and bitstream.sequence_kinds(blob) == ["I"] + ["P"] * (LONG_FRAMES - 1)
    assert all(m is not None for m in bitstream.sequence_motion(blob)[1:])
    assert digest(blob, dec) == _recorded(f"long-D{D}")
    last, = bitstream.decode_sequence_bytes(blob, frames=[LONG_FRAMES - 1])
    assert _same_bits(last, dec[-1])
    # the closed loop's bound (derived in test_gpu_sequence_inter.py): the quantizer of the last frame alone, whatever the length
    N = len(frames[-1][0])
    assert np.array_equal(dec[-1][0].cpu().numpy(), frames[-1][0])
    err = (dec[-1][1].cpu() - torch.from_numpy(frames[-1][1])).norm(dim=0)
    print("closed loop, frame 13: max column error", float(err.max()), "bound", (0.5 * STEP + 1e-4) * N ** 0.5)
    assert float(err.max()) <= (0.5 * STEP + 1e-4) * N ** 0.5
