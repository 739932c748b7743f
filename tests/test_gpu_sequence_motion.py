"""Motion-compensated frames in a sequence (bitstream.encode_sequence_bytes(..., motion, block_log2) / decode_sequence_bytes;
DESIGN.md 19) on a cloud that moves by one voxel a frame: every predicted frame carries a motion field, decodes to its inner frame's
reconstruction plus the model's compensated prediction from the decoded previous frame, bit for bit; the encoder's closed loop lands
on the decoder's bits; subsets close under their dependencies; a sequence without motion, and a call without the new arguments, give
the bytes they gave before; and compensation pays what it must."""
import numpy as np
import pytest

from . import numpy_motion as MM
from . import numpy_predict as M

pytestmark = pytest.mark.gpu

J, S, STEP, DRAWS, FRAMES, BLOCK, SIGMA = 6, 256, 0.01, 3000, 5, 4, 0.002
STEP_T = (1, 0, -1)                                                      # the cloud's translation per frame
SHAPES = [(5, 0), (59, 3)]
KW = dict(seg_len=S, vmin=(0.5, -1.0, 2.0), width=3.0)
_CACHE = {}


def _frames(kind, D):
    from raht_3dgs_codec_amd import synth
    key = ("frames", kind, D)
    if key not in _CACHE:
        rng = np.random.default_rng(31)
        V = np.unique(rng.integers(4, 60, size=(DRAWS, 3)), axis=0).astype(np.int64)
        A = synth.gaussian_attributes(len(V), D, 32)
        out = []
        for t in range(FRAMES):
            Vt = V + (t * np.array(STEP_T, np.int64) if kind == "moving" else 0)
            At = (A + SIGMA * rng.standard_normal(A.shape)).astype(np.float32)
            o = np.argsort(synth.morton_keys(Vt, J), kind="stable")
            out.append((Vt[o], np.ascontiguousarray(At[o])))
        _CACHE[key] = out
    return _CACHE[key]


def _coded(kind, D, n_wide, **enc):
    """(frames, blob, full decode), computed once and left unchanged"""
    from raht_3dgs_codec_amd import bitstream
    key = (kind, D, n_wide, tuple(sorted(enc.items())))
    if key not in _CACHE:
        frames = _frames(kind, D)
        blob = bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", n_wide=n_wide, **KW, **enc)
        _CACHE[key] = (frames, blob, bitstream.decode_sequence_bytes(blob, device="cuda"))
    return _CACHE[key]


MOVING = dict(gop=FRAMES, inter="always", motion=1, block_log2=BLOCK)


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_a_compensated_frame_is_its_inner_frame_plus_the_models_prediction(D, n_wide):
    import torch
    from raht_3dgs_codec_amd import bitstream, synth
    frames, blob, dec = _coded("moving", D, n_wide, **MOVING)
    assert bitstream.sequence_kinds(blob) == ["I"] + ["P"] * (FRAMES - 1)
    motion = bitstream.sequence_motion(blob)
    assert motion[0] is None and len(dec) == FRAMES
    keys = [synth.morton_keys(V, J) for V, _ in frames]
    for i, ((V, C), (V0, _)) in enumerate(zip(dec, frames)):
        assert V.dtype == torch.int64 and C.dtype == torch.float32 and tuple(C.shape) == (len(V0), D)
        assert np.array_equal(V.cpu().numpy(), V0), i
        fb = bitstream.sequence_frame(blob, i)
        if i == 0:
            assert bytes(fb[:8]) == b"RAHTF001"
            continue
        assert bytes(fb[:8]) == b"RAHTM001"                              # every P frame carries a motion field
        ref_back, up, m, mv, inner = bitstream.parse_mframe(fb)
        assert (ref_back, up, m) == (1, 0, BLOCK) == MM.parse_mframe(fb)[:3] and bytes(inner) == MM.parse_mframe(fb)[4]
        assert motion[i][0] == BLOCK and np.array_equal(motion[i][1], mv) and np.array_equal(mv, MM.parse_mframe(fb)[3])
        assert len(mv) == len(MM.blocks(keys[i], BLOCK)[1]) - 1
        assert (mv == -np.array(STEP_T)).all()                           # from the voxel to its reference voxel: -t, for every block
        V1, R_rec = bitstream.decode_frame_bytes(inner, "cuda")
        P, _ = MM.predict_mc(keys[i], keys[i - 1], dec[i - 1][1].cpu().numpy(), J, BLOCK, mv, 0)
        want = M.apply(R_rec.cpu().numpy(), P, add=True)
        assert torch.equal(V, V1)
        assert np.array_equal(C.cpu().numpy().view(np.int32), want.view(np.int32)), i
        with pytest.raises(ValueError, match="not a RAHT frame container"):
            bitstream.decode_frame_bytes(fb, "cuda")
        with pytest.raises(ValueError, match="not a RAHT frame container"):
            bitstream.decode_region_bytes(fb, 1, (0, 4), "cuda")


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_the_encoders_closed_loop_ends_on_the_decoders_bits(D, n_wide):
    """the encoder's recurrence with public calls: search, compensated residual, transform + quantize, dequantize + inverse, add"""
    import torch
    from raht_3dgs_codec_amd import bitstream, ops
    frames, blob, dec = _coded("moving", D, n_wide, **MOVING)
    motion = bitstream.sequence_motion(blob)
    w = np.full(D, 1.0 / STEP).astype(np.float32)
    ref = None
    for i, (V, A) in enumerate(frames):
        keys = ops.get_morton_code(torch.from_numpy(V).cuda(), J)
        plan = ops.RahtPlan.from_keys(keys, 3 * J)
        X = torch.from_numpy(A).cuda()
        if ref is not None:
            bf = ops.motion_blocks(keys, J, BLOCK, len(motion[i][1]))
            mv, _ = ops.motion_search(keys, ref[0], ref[1], X, J, BLOCK, bf, ops.motion_candidates(1), w)
            assert np.array_equal(mv.cpu().numpy(), motion[i][1]), i   # the field in the wrapper is the search's
            X = ops.predict_mc(keys, ref[0], ref[1], mv, bf, J, BLOCK, X=X)
        if n_wide:
            C = plan.dequant_inverse_mixed(plan.forward_quant_mixed(X, [STEP], n_wide), [STEP], n_wide)
        else:
            C = plan.dequant_inverse(plan.forward_quant(X, [STEP]), [STEP])
        if ref is not None:
            C = ops.predict_mc(keys, ref[0], ref[1], mv, bf, J, BLOCK, X=C, add=True)
        ref = (keys, C)
    assert torch.equal(ref[1].view(torch.int32), dec[-1][1].view(torch.int32))
    # the loop is closed: the reconstruction is the input up to the quantizer of the LAST frame alone (test_gpu_sequence_inter.py has
    # the bound's derivation: an orthonormal transform, half a step per coefficient, 1e-4 per element for float32 rounding)
    N = len(frames[-1][0])
    err = (ref[1].cpu() - torch.from_numpy(frames[-1][1])).norm(dim=0)
    assert float(err.max()) <= (0.5 * STEP + 1e-4) * N ** 0.5


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_a_subset_is_closed_under_its_dependencies(D, n_wide):
    import torch
    from raht_3dgs_codec_amd import bitstream
    frames, blob, dec = _coded("moving", D, n_wide, **MOVING)
    (V, C), = bitstream.decode_sequence_bytes(blob, frames=[3])
    assert torch.equal(V, dec[3][0]) and torch.equal(C.view(torch.int32), dec[3][1].view(torch.int32))
    two = bitstream.decode_sequence_bytes(blob, frames=[4, 1])
    assert len(two) == 2
    for (V, C), i in zip(two, (4, 1)):
        assert torch.equal(V, dec[i][0]) and torch.equal(C.view(torch.int32), dec[i][1].view(torch.int32)), i


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_without_motion_the_bytes_are_what_they_were(D, n_wide):
    from raht_3dgs_codec_amd import bitstream
    for inter in ("always", "auto"):
        frames, plain, _ = _coded("static", D, n_wide, gop=FRAMES, inter=inter)              # the new arguments omitted ...
        assert bitstream.sequence_kinds(plain) == ["I"] + ["P"] * (FRAMES - 1)
        assert all(mo is None for mo in bitstream.sequence_motion(plain))
        assert bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", n_wide=n_wide, gop=FRAMES, inter=inter, motion=0, block_log2=2,
                                               **KW) == plain           # ... are motion = 0 ...
        # ... and a search that finds no motion (a static cloud: every vector is 0) falls through to the same frames
        assert bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", n_wide=n_wide, gop=FRAMES, inter=inter, motion=1,
                                               block_log2=BLOCK, **KW) == plain
    frames = _frames("moving", D)
    plain = bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", n_wide=n_wide, **KW)
    assert bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", n_wide=n_wide, motion=2, **KW) == plain       # gop = 1: no candidate


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_compensation_pays_on_a_moving_cloud(D, n_wide):
    """The compensated residual of a translated frame is the reference's quantization error plus noise of a fifth of a step: the
    project's own figures for such residuals are x0.23 of an intra frame and less (profiles/predict.json; test_gpu_sequence_inter's
    static case), while the uncompensated residual has no related co-located voxel and costs an intra frame or more. So: below half."""
    from raht_3dgs_codec_amd import bitstream
    _, blob, _ = _coded("moving", D, n_wide, **MOVING)
    frames, plain, _ = _coded("moving", D, n_wide, gop=FRAMES, inter="always", motion=0)
    assert all(mo is None for mo in bitstream.sequence_motion(plain)) and bitstream.sequence_kinds(plain) == ["I"] + ["P"] * (FRAMES - 1)
    sizes = []
    for i in range(1, FRAMES):
        with_mc = bitstream.parse_frame(bitstream.parse_mframe(bitstream.sequence_frame(blob, i))[4])["attributes"][1]
        without = bitstream.parse_frame(bitstream.parse_pframe(bitstream.sequence_frame(plain, i))[2])["attributes"][1]
        sizes.append((with_mc, without))
    print(f"D = {D}: attribute bytes per predicted frame (compensated, uncompensated):", sizes,
          "ratios:", [round(a / b, 4) for a, b in sizes])
    assert all(2 * a < b for a, b in sizes), sizes
    # inter="auto" takes the smallest of the three exact sizes; frame 1's reference (the intra frame 0) is the same in every
    # encode, so its frame is no longer than any of the three ways to code it
    auto = bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", n_wide=n_wide, gop=FRAMES, inter="auto", motion=1, block_log2=BLOCK, **KW)
    intra = bitstream.encode_frame_bytes(*frames[1], J, STEP, "cuda", n_wide=n_wide, **KW)
    ways = [len(intra), len(bitstream.sequence_frame(plain, 1)), len(bitstream.sequence_frame(blob, 1))]
    assert len(bitstream.sequence_frame(auto, 1)) == min(ways), ways
    dec = bitstream.decode_sequence_bytes(auto)
    assert len(dec) == FRAMES
