"""The hierarchical motion search in a sequence (ops.motion_search_hier, bitstream.encode_sequence_bytes(..., motion_levels);
DESIGN.md 23) on a cloud that moves further per frame than the exhaustive search reaches. t is a motion vector in the codec's
sense -- from a voxel to its reference voxel --, so the reference of a frame holds the frame's voxels at x + t, and frame k of the
sequence holds frame 0's at x - k t.
  (a) a rigid translation by t = (8, -4, 12), a multiple of 2^L: every level's cells keep their members and their row order, the
      cost at t / 2^l is 0 and the zero refinement has index 0 -- every block whose voxels all stay inside gets exactly t.
  (b) four noisy frames: the kinds, the wrappers, the sizes against the exhaustive search, the fields, the decoder against the
      model's closed loop, a region, B frames, the bytes without the argument, the refusals."""
import numpy as np
import pytest

from . import numpy_motion as MM
from . import numpy_motion_hier as MH
from . import numpy_predict as M
from . import numpy_predict_bi as MB

pytestmark = pytest.mark.gpu

J, BLOCK, LEVELS, S, STEP, SIGMA, FRAMES = 7, 3, 2, 256, 0.01, 0.002, 4
T = np.array([8, -4, 12], np.int64)
SHAPES = [(5, 0), (59, 3)]
KW = dict(seg_len=S, vmin=(0.5, -1.0, 2.0), width=3.0)
_CACHE = {}


def _cloud(lo, hi, seed):
    """~3000 voxels in blobs inside the box [lo, hi) per axis"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo), np.asarray(hi)
    centres = rng.uniform(lo + 6, hi - 6, size=(14, 3))
    V = np.rint(centres[rng.integers(0, len(centres), size=3300)] + 3.5 * rng.standard_normal((3300, 3))).astype(np.int64)
    V = np.unique(V[np.all((V >= lo) & (V < hi), axis=1)], axis=0)
    assert 2500 < len(V) < 3600, len(V)
    return V


def _sorted(V, A):
    from raht_3dgs_codec_amd import synth
    o = np.argsort(synth.morton_keys(V, J), kind="stable")
    return V[o], np.ascontiguousarray(A[o])


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


@pytest.mark.parametrize("D", [5, 59])
def test_a_rigid_translation_beyond_the_flat_reach_is_found_exactly(D):
    import torch
    from raht_3dgs_codec_amd import ops, synth
    V = _cloud((0, 0, 0), (128, 128, 128), 50)                           # the whole cube: some voxels leave it under t
    V, X = _sorted(V, synth.gaussian_attributes(len(V), D, 51))
    keys = synth.morton_keys(V, J)
    stays = np.all((V + T >= 0) & (V + T < (1 << J)), axis=1)
    Vr, C = _sorted(V[stays] + T, X[stays])
    ref = synth.morton_keys(Vr, J)
    b, first = MM.blocks(keys, BLOCK)
    n_blocks = len(first) - 1
    whole = np.ones(n_blocks, bool)
    np.logical_and.at(whole, b, stays)                                   # the blocks whose voxels all stay inside
    assert 2 * whole.sum() >= n_blocks and not whole.all() and n_blocks > 100
    w = np.ones(D, np.float32)
    if D == 5:                                                           # the model agrees (and was asked when the seed was chosen)
        mv_m, cost_m, _ = MH.search_hier(keys, ref, C, X, J, BLOCK, LEVELS, 3, w)
        assert (mv_m[whole] == T).all() and not cost_m[whole].any()
    k, r, Cd, Xd = _dev(keys), _dev(ref), _dev(C), _dev(X)
    bf = ops.motion_blocks(k, J, BLOCK, n_blocks)
    mv, cost, info = ops.motion_search_hier(k, r, Cd, Xd, J, BLOCK, bf, LEVELS, 3, w)
    mv, cost = mv.cpu().numpy(), cost.cpu().numpy()
    assert (mv[whole] == T).all() and not cost[whole].any()
    for l in range(LEVELS + 1):
        assert (info["mv"][l].cpu().numpy()[whole].astype(np.int64) * 2 ** l == T).all(), l
    flat = ops.motion_search(k, r, Cd, Xd, J, BLOCK, bf, ops.motion_candidates(3), w)[0].cpu().numpy()
    assert np.abs(flat).max() <= 3 and not (flat == T).all(axis=1).any()


def _frames(D):
    """frame k: frame 0's voxels at x - k t (every voxel stays inside in every frame), attributes plus noise of a fifth of a step"""
    from raht_3dgs_codec_amd import synth
    if ("frames", D) not in _CACHE:
        span = (FRAMES - 1) * T
        V0 = _cloud(np.maximum(span, 0), (1 << J) + np.minimum(span, 0), 52)
        A = synth.gaussian_attributes(len(V0), D, 53)
        rng = np.random.default_rng(54)
        _CACHE[("frames", D)] = [_sorted(V0 - k * T, (A + SIGMA * rng.standard_normal(A.shape)).astype(np.float32)) for k in range(FRAMES)]
    return _CACHE[("frames", D)]


def _coded(D, n_wide, **enc):
    """(frames, blob, full decode), computed once and left unchanged"""
    from raht_3dgs_codec_amd import bitstream
    key = (D, n_wide, tuple(sorted(enc.items())))
    if key not in _CACHE:
        frames = _frames(D)
        blob = bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", n_wide=n_wide, gop=FRAMES, motion=3, block_log2=BLOCK, **KW, **enc)
        _CACHE[key] = (frames, blob, bitstream.decode_sequence_bytes(blob, device="cuda"))
    return _CACHE[key]


def _modal(mv):
    vecs, n = np.unique(np.asarray(mv, np.int64), axis=0, return_counts=True)
    return vecs[n.argmax()]


def _matches_the_models_closed_loop(frames, blob, dec):
    """every frame of the whole decode is its inner frame's reconstruction plus the model's prediction from the DECODED references
    under the parsed fields, bit for bit -> the fields per frame"""
    import torch
    from raht_3dgs_codec_amd import bitstream, synth
    keys = [synth.morton_keys(V, J) for V, _ in frames]
    refs, fields = bitstream.sequence_refs(blob), []
    assert len(dec) == len(frames)
    for i, ((V, C), (V0, _)) in enumerate(zip(dec, frames)):
        assert np.array_equal(V.cpu().numpy(), V0) and C.dtype == torch.float32, i
        fb = bitstream.sequence_frame(blob, i)
        ref = [(keys[r], dec[r][1].cpu().numpy()) for r in refs[i]]
        magic = bytes(fb[:8])
        if magic == b"RAHTF001":
            fields.append(None)
            continue
        if magic == b"RAHTB001":
            _, _, up, m, mv0, mv1, inner = bitstream.parse_bframe(fb)
            P = MB.predict(keys[i], ref[0], ref[1], up, J, m, mv0, mv1)[0]
            fields.append((mv0, mv1))
        elif magic == b"RAHTM001":
            _, up, m, mv, inner = bitstream.parse_mframe(fb)
            P = MM.predict_mc(keys[i], *ref[0], J, m, mv, up)[0]
            fields.append((mv,))
        else:
            _, up, inner = bitstream.parse_pframe(fb)
            P = M.predict(keys[i], *ref[0], up)[0]
            fields.append(())
        R_rec = bitstream.decode_frame_bytes(inner, "cuda")[1].cpu().numpy()
        assert np.array_equal(C.cpu().numpy().view(np.int32), M.apply(R_rec, P, add=True).view(np.int32)), i
    return fields


def _a_region_is_the_rows_of_the_whole_decode(frames, blob, dec, i):
    import torch
    from raht_3dgs_codec_amd import bitstream, synth
    keys = synth.morton_keys(frames[i][0], J)
    cell = keys >> np.uint64(3 * (J - 2))
    c = int(cell[len(cell) // 2])                                        # one occupied depth-2 cell
    a, b = int(np.searchsorted(cell, c, "left")), int(np.searchsorted(cell, c, "right"))
    assert 0 < b - a < len(keys)
    V, C, _ = bitstream.decode_sequence_region(blob, i, 2, (c, c + 1), "cuda")
    assert torch.equal(V, dec[i][0][a:b]) and torch.equal(C.view(torch.int32), dec[i][1][a:b].view(torch.int32))


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_a_fast_sequence_is_followed(D, n_wide):
    from raht_3dgs_codec_amd import bitstream
    frames, blob, dec = _coded(D, n_wide, inter="auto", motion_levels=LEVELS)
    _, flat, _ = _coded(D, n_wide, inter="auto", motion_levels=0)
    assert bitstream.sequence_kinds(blob) == ["I", "P", "P", "P"]
    motion = bitstream.sequence_motion(blob)
    sizes = []
    for i in range(1, FRAMES):
        fb = bitstream.sequence_frame(blob, i)
        assert bytes(fb[:8]) == b"RAHTM001", i                          # every predicted frame carries a field
        assert motion[i][0] == BLOCK and (_modal(motion[i][1]) == T).all(), (i, _modal(motion[i][1]))
        sizes.append((len(fb), len(bitstream.sequence_frame(flat, i))))
    print(f"D = {D}: bytes of the predicted frames (motion_levels = {LEVELS}, motion_levels = 0):", sizes, "kinds without:",
          "".join(bitstream.sequence_kinds(flat)), "ratios:", [round(a / b, 4) for a, b in sizes])
    assert all(a < b for a, b in sizes), sizes
    fields = _matches_the_models_closed_loop(frames, blob, dec)
    assert fields[0] is None and all(len(f) == 1 for f in fields[1:])
    _a_region_is_the_rows_of_the_whole_decode(frames, blob, dec, FRAMES - 1)


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_b_frames_carry_two_fields_of_opposite_sign(D, n_wide):
    """bframes = 1 in a GOP of four: the anchors 0, 2, 3 and the B candidate 1, which lies one frame from either anchor (the anchor
    2 lies two frames, 2 t = (16, -8, 24), from its reference: beyond 3 * 4 + 3). Under inter="auto" the coder may take any way
    for a frame, so what the B frame carries is asserted under inter="always" and the decoder is checked under both."""
    from raht_3dgs_codec_amd import bitstream
    for inter in ("auto", "always"):
        frames, blob, dec = _coded(D, n_wide, inter=inter, bframes=1, motion_levels=LEVELS)
        kinds = bitstream.sequence_kinds(blob)
        assert bitstream.sequence_refs(blob)[2:] == [(0,), (2,)] or inter == "auto"
        fields = _matches_the_models_closed_loop(frames, blob, dec)
        for kind, f in zip(kinds, fields):
            if kind == "B" and len(f) == 2 and f[0] is not None:
                assert (_modal(f[0]) == T).all() and (_modal(f[1]) == -T).all(), (inter, _modal(f[0]), _modal(f[1]))
        if inter == "always":
            assert kinds == ["I", "B", "P", "P"] and bytes(bitstream.sequence_frame(blob, 1)[:8]) == b"RAHTB001"
            assert len(fields[1]) == 2 and fields[1][0] is not None and (_modal(fields[3][0]) == T).all()
        _a_region_is_the_rows_of_the_whole_decode(frames, blob, dec, FRAMES - 1)


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_no_levels_are_the_bytes_without_the_argument(D, n_wide):
    from raht_3dgs_codec_amd import bitstream
    frames, flat, _ = _coded(D, n_wide, inter="auto", motion_levels=0)
    assert bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", n_wide=n_wide, gop=FRAMES, motion=3, block_log2=BLOCK, inter="auto",
                                           **KW) == flat


def test_the_refusals():
    from raht_3dgs_codec_amd import bitstream
    frames = _frames(5)
    ok = dict(gop=FRAMES, motion=3, block_log2=BLOCK, motion_levels=LEVELS, **KW)
    for what, kw in {"motion_levels < 0": dict(motion_levels=-1), "motion_levels without motion": dict(motion=0),
                     "motion_levels > 3": dict(motion_levels=4, block_log2=6), "motion_levels > block_log2 - 1": dict(motion_levels=3),
                     "motion_levels = block_log2": dict(motion_levels=1, block_log2=1)}.items():
        with pytest.raises(ValueError, match="motion_levels"):
            bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", **{**ok, **kw})
            pytest.fail(what)
    # J - motion_levels < 1: with block_log2 <= J this is also motion_levels > block_log2 - 1, refused under either name
    with pytest.raises(ValueError, match="motion_levels"):
        bitstream.encode_sequence_bytes(frames, 1, STEP, "cuda", **{**ok, "block_log2": 1, "motion_levels": 1})
