"""B frames in a sequence (bitstream.encode_sequence_bytes(..., bframes) / decode_sequence_bytes): a B frame decodes
to its inner frame's reconstruction plus the two-reference model's prediction from the DECODED anchors, bit for bit; anchors are
predicted from the anchor before them; the encoder's closed loop lands on the decoder's bits; a fade is coded cheaper between its
anchors than from one; the anchors decode without the B frames' bytes; corrupt wrappers are named."""
import numpy as np
import pytest

from . import numpy_motion as MM
from . import numpy_predict as M1
from . import numpy_predict_bi as M
from . import numpy_region as MR

pytestmark = pytest.mark.gpu

J, S, STEP, DRAWS, FRAMES = 6, 256, 0.01, 3000, 5                        # (the constants of tests/test_gpu_sequence_inter.py)
SHAPES = [(5, 0), (59, 3)]
KW = dict(seg_len=S, vmin=(0.5, -1.0, 2.0), width=3.0)
_CACHE = {}


def _frames(kind, D, n=FRAMES):
    from raht_3dgs_codec_amd import synth
    V, _, A = synth.scene(DRAWS, J, D, seed=21)
    if kind == "fade":                                                   # static voxels, A_t = A_0 + t delta
        delta = (0.05 * np.random.default_rng(23).standard_normal(A.shape)).astype(np.float32)
        out = []
        for t in range(n):
            At = (A + np.float32(t) * delta).astype(np.float32)
            if D == 59:
                At[:, :3] = V
            out.append((V, At))
        return out
    # drifting: one voxel in x per frame, re-sorted, attributes plus 1e-3 seeded noise (xyz columns, where there are any, follow)
    keep = V[:, 0] < (1 << J) - (n - 1)
    V, A = V[keep], A[keep]
    rng = np.random.default_rng(22)
    out = []
    for t in range(n):
        Vt = V + np.array([t, 0, 0], np.int64)
        At = A + (1e-3 * rng.standard_normal(A.shape)).astype(np.float32)
        if D == 59:
            At[:, :3] = Vt
        o = np.argsort(synth.morton_keys(Vt, J), kind="stable")
        out.append((Vt[o], At[o].astype(np.float32)))
    return out


def _coded(kind, D, n_wide, n=FRAMES, **enc):
    """(frames, blob, full decode), computed once and left unchanged"""
    from raht_3dgs_codec_amd import bitstream
    key = (kind, D, n_wide, n, tuple(sorted(enc.items())))
    if key not in _CACHE:
        frames = _frames(kind, D, n)
        blob = bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", n_wide=n_wide, **KW, **enc)
        _CACHE[key] = (frames, blob, bitstream.decode_sequence_bytes(blob, device="cuda"))
    return _CACHE[key]


def _same(a, b):
    import torch
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def _matches_the_model(frames, blob, dec, up):
    """every frame of the full decode is its inner frame's reconstruction plus the model's prediction from the decoded references,
    under the parsed fields -> the wrappers' (kind, ref_back, ref_fwd, block_log2, mv0, mv1) per frame"""
    import torch
    from raht_3dgs_codec_amd import bitstream, synth
    keys = [synth.morton_keys(V, J) for V, _ in frames]
    kinds, refs = bitstream.sequence_kinds(blob), bitstream.sequence_refs(blob)
    assert kinds == M.kinds(blob) and len(dec) == len(frames)
    seen = []
    for i, ((V, C), (V0, _)) in enumerate(zip(dec, frames)):
        assert V.dtype == torch.int64 and C.dtype == torch.float32 and np.array_equal(V.cpu().numpy(), V0), i
        fb = bitstream.sequence_frame(blob, i)
        ref = [(keys[r], dec[r][1].cpu().numpy()) for r in refs[i]]
        if kinds[i] == "I":
            assert refs[i] == () and _same((V, C), bitstream.decode_frame_bytes(fb, "cuda"))
            seen.append(("I", None, None, 0, None, None))
            continue
        if kinds[i] == "B":
            rb, rf, up_coded, m, mv0, mv1, inner = bitstream.parse_bframe(fb)
            assert refs[i] == (i - rb, i + rf) and bytes(inner) == M.parse_bframe(fb)[6]
            P = M.predict(keys[i], ref[0], ref[1], up, J, m, mv0, mv1)[0]
        elif bytes(fb[:8]) == bitstream.M_MAGIC:
            rb, up_coded, m, mv0, inner = bitstream.parse_mframe(fb)
            rf, mv1 = None, None
            P = MM.predict_mc(keys[i], *ref[0], J, m, mv0, up)[0]
        else:
            rb, up_coded, inner = bitstream.parse_pframe(fb)
            rf, m, mv0, mv1 = None, 0, None, None
            P = M1.predict(keys[i], *ref[0], up)[0]
        assert up_coded == up and refs[i][0] == i - rb
        rk = None                                                        # a predicted geometry section: against reference 0's keys
        if bitstream.parse_frame(inner)["geometry_ref"] is not None:
            rk = torch.from_numpy(keys[refs[i][0]].view(np.int64)).cuda()
        V1, R_rec = bitstream.decode_frame_bytes(inner, "cuda", ref_keys=rk)
        want = M.apply(R_rec.cpu().numpy(), P, add=True)
        assert torch.equal(V, V1)
        assert np.array_equal(C.cpu().numpy().view(np.int32), want.view(np.int32)), (i, kinds[i])
        seen.append((kinds[i], rb, rf, m, mv0, mv1))
    return seen


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_a_fade_between_two_anchors(D, n_wide):
    from raht_3dgs_codec_amd import bitstream
    frames, blob, dec = _coded("fade", D, n_wide, gop=FRAMES, bframes=1, inter="always")
    assert bitstream.sequence_kinds(blob) == ["I", "B", "P", "B", "P"]
    assert bitstream.sequence_refs(blob) == [(), (0, 2), (0,), (2, 4), (2,)] == [r for _, r in bitstream.sequence_plan(FRAMES, FRAMES, 1)]
    assert bitstream.sequence_motion(blob) == [None] * FRAMES
    seen = _matches_the_model(frames, blob, dec, 0)
    assert [s[:4] for s in seen] == [("I", None, None, 0), ("B", 1, 1, 0), ("P", 2, None, 0), ("B", 1, 1, 0), ("P", 2, None, 0)]
    # the default is today's path, byte for byte
    plain = bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", n_wide=n_wide, gop=FRAMES, inter="always", **KW)
    assert plain == bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", n_wide=n_wide, gop=FRAMES, inter="always", bframes=0, **KW)
    assert bitstream.sequence_kinds(plain) == ["I", "P", "P", "P", "P"] and bitstream.sequence_refs(plain) == [(), (0,), (1,), (2,), (3,)]
    assert bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", n_wide=n_wide, bframes=3, **KW) == \
        bitstream.encode_sequence_bytes(frames, J, STEP, "cuda", n_wide=n_wide, **KW)          # gop = 1: no frame is a candidate


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_the_encoders_closed_loop_ends_on_the_decoders_bits(D, n_wide):
    """the encoder's recurrence with public calls: anchors from the anchor before, then the B frames from both"""
    import torch
    from raht_3dgs_codec_amd import bitstream, ops
    frames, blob, dec = _coded("fade", D, n_wide, gop=FRAMES, bframes=1, inter="always")

    def coded(plan, X):
        if n_wide:
            return plan.dequant_inverse_mixed(plan.forward_quant_mixed(X, [STEP], n_wide), [STEP], n_wide)
        return plan.dequant_inverse(plan.forward_quant(X, [STEP]), [STEP])
    order = bitstream.sequence_plan(FRAMES, FRAMES, 1)
    keys = [ops.get_morton_code(torch.from_numpy(V).cuda(), J) for V, _ in frames]
    plans = [ops.RahtPlan.from_keys(k, 3 * J) for k in keys]
    rec = {}
    for i in sorted(range(FRAMES), key=lambda i: (order[i][0] == "B", i)):
        X, refs = torch.from_numpy(frames[i][1]).cuda(), [(keys[r], rec[r]) for r in order[i][1]]
        if len(refs) == 2:
            C = coded(plans[i], ops.predict_bi(keys[i], *refs, X=X))
            rec[i] = ops.predict_bi(keys[i], *refs, X=C, add=True)
        elif refs:
            C = coded(plans[i], ops.predict(keys[i], *refs[0], X=X))
            rec[i] = ops.predict(keys[i], *refs[0], X=C, add=True)
        else:
            rec[i] = coded(plans[i], X)
    for i in range(FRAMES):
        assert torch.equal(rec[i].view(torch.int32), dec[i][1].view(torch.int32)), i


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_a_fade_is_cheaper_between_its_anchors_than_from_one(D, n_wide):
    """The B residual of a fade's middle frame is the anchors' quantization error; the P residual of the same frame is delta, about
    five steps a voxel. Measured on an MI355X: see the printed sizes."""
    from raht_3dgs_codec_amd import bitstream
    frames, blob, _ = _coded("fade", D, n_wide, gop=FRAMES, bframes=1, inter="auto")
    kinds = bitstream.sequence_kinds(blob)
    _, chain, _ = _coded("fade", D, n_wide, gop=FRAMES, bframes=0, inter="always")
    off_b, off_p = bitstream.parse_sequence(blob), bitstream.parse_sequence(chain)
    sizes = [(off_b[i + 1] - off_b[i], off_p[i + 1] - off_p[i]) for i in range(FRAMES)]
    print("kinds", kinds, "frame bytes (bframes=1 auto, bframes=0 always):", sizes)
    assert kinds[1] == "B" and kinds[3] == "B", kinds
    assert sizes[1][0] < sizes[1][1] and sizes[3][0] < sizes[3][1], sizes


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_a_drifting_scene_under_two_motion_fields(D, n_wide):
    from raht_3dgs_codec_amd import bitstream
    frames, blob, dec = _coded("drifting", D, n_wide, gop=FRAMES, bframes=1, inter="always", motion=2, block_log2=2)
    assert bitstream.sequence_kinds(blob) == ["I", "B", "P", "B", "P"]
    seen = _matches_the_model(frames, blob, dec, 0)
    motion = bitstream.sequence_motion(blob)
    for i in (1, 3):
        kind, rb, rf, m, mv0, mv1 = seen[i]
        assert (kind, rb, rf, m) == ("B", 1, 1, 2) and mv0.shape == mv1.shape and mv0.dtype == np.int8
        assert motion[i][0] == 2 and np.array_equal(motion[i][1], mv0) and np.array_equal(motion[i][2], mv1)
        modal = [tuple(int(x) for x in max(set(map(tuple, mv.tolist())), key=list(map(tuple, mv.tolist())).count)) for mv in (mv0, mv1)]
        print("frame", i, "modal vectors", modal)
        assert modal == [(-1, 0, 0), (1, 0, 0)], (i, modal)              # the cloud moves +1 in x a frame: back to frame i - 1, on to i + 1


@pytest.mark.parametrize("n,gop,b", [(7, 7, 2), (6, 4, 1)])
def test_kinds_and_refs_are_the_plan_and_a_full_decode_matches_the_model(n, gop, b):
    from raht_3dgs_codec_amd import bitstream
    frames, blob, dec = _coded("fade", 5, 0, n=n, gop=gop, bframes=b, inter="always", up=1)
    plan = bitstream.sequence_plan(n, gop, b)
    assert bitstream.sequence_kinds(blob) == [k for k, _ in plan] and bitstream.sequence_refs(blob) == [r for _, r in plan]
    assert "B" in bitstream.sequence_kinds(blob)
    _matches_the_model(frames, blob, dec, 1)


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_subsets_and_temporal_scalability(D, n_wide):
    from raht_3dgs_codec_amd import bitstream
    frames, blob, dec = _coded("fade", D, n_wide, gop=FRAMES, bframes=1, inter="always")
    (one,) = bitstream.decode_sequence_bytes(blob, frames=[3])
    assert _same(one, dec[3])
    two = bitstream.decode_sequence_bytes(blob, frames=[3, 1])
    assert _same(two[0], dec[3]) and _same(two[1], dec[1])
    # the anchors alone: every byte of the B frames' inner containers may be gone
    off = bitstream.parse_sequence(blob)
    bad = bytearray(blob)
    for i in (1, 3):
        bad[off[i] + bitstream.B_HEAD: off[i + 1]] = b"\xff" * (off[i + 1] - off[i] - bitstream.B_HEAD)
    anchors = bitstream.decode_sequence_bytes(bytes(bad), frames=[0, 2, 4])
    assert all(_same(a, dec[i]) for a, i in zip(anchors, (0, 2, 4)))
    with pytest.raises(ValueError, match="frame 1:"):
        bitstream.decode_sequence_bytes(bytes(bad))


def test_predicted_geometry_with_b_frames_round_trips_the_voxels():
    from raht_3dgs_codec_amd import bitstream
    frames, blob, dec = _coded("drifting", 5, 0, gop=FRAMES, bframes=1, inter="always", geometry_inter="always")
    assert bitstream.sequence_kinds(blob) == ["I", "B", "P", "B", "P"]
    assert bitstream.sequence_geometry(blob) == ["intra"] + ["predicted"] * 4
    for (V, _), (V0, _) in zip(dec, frames):
        assert np.array_equal(V.cpu().numpy(), V0)
    _matches_the_model(frames, blob, dec, 0)
    _, plain, dec_plain = _coded("drifting", 5, 0, gop=FRAMES, bframes=1, inter="always")
    assert all(_same(a, b) for a, b in zip(dec, dec_plain)) and len(blob) != len(plain)


def test_a_region_of_an_anchor_and_the_refusal_of_a_b_frame():
    import torch
    from raht_3dgs_codec_amd import bitstream, synth
    frames, blob, dec = _coded("drifting", 5, 0, gop=FRAMES, bframes=1, inter="always", up=1)
    with pytest.raises(ValueError, match="frame 1 is a B frame"):
        bitstream.decode_sequence_region(blob, 1, 2, (3, 9), "cuda")
    keys = synth.morton_keys(frames[4][0], J)
    for depth, cells in ((2, (3, 40)), (J - 1, (1000, 9000))):
        a, b = MR.region_rows(keys, J, depth, *cells)
        assert b > a
        V, C, info = bitstream.decode_sequence_region(blob, 4, depth, cells, "cuda")
        assert info["chain"] == [0, 2, 4]                                # the B frames are on nobody's chain
        assert torch.equal(V, dec[4][0][a:b]) and torch.equal(C.view(torch.int32), dec[4][1][a:b].view(torch.int32))


def test_corrupt_b_wrappers_are_named():
    from raht_3dgs_codec_amd import bitstream
    frames, blob, dec = _coded("drifting", 5, 0, gop=FRAMES, bframes=1, inter="always", motion=2, block_log2=2)
    off = bitstream.parse_sequence(blob)
    n_blocks = len(bitstream.sequence_motion(blob)[3][1])
    assert (3 * n_blocks) % 8                                            # (there is padding to corrupt)

    def patched(at, value):
        bad = bytearray(blob)
        bad[at: at + len(value)] = value
        return bytes(bad)
    cases = {"n_blocks off by one": patched(off[3] + 8 + 32, np.array([n_blocks + 1], np.int64).tobytes()),
             "n_blocks one short": patched(off[3] + 8 + 32, np.array([n_blocks - 1], np.int64).tobytes()),
             "non-zero padding": patched(off[3] + bitstream.B_HEAD + 3 * n_blocks, b"\x01"),
             "ref_fwd past the end": patched(off[3] + 8 + 8, np.array([2], np.int64).tobytes())}
    for what, bad in cases.items():
        for call in (bitstream.decode_sequence_bytes, bitstream.sequence_kinds):
            with pytest.raises(ValueError, match="frame 3:"):
                call(bad)
                pytest.fail(what)
        assert len(bitstream.decode_sequence_bytes(bad, frames=[0, 1, 2, 4])) == 4, what       # nobody depends on frame 3
    with pytest.raises(ValueError, match="not a RAHT frame container"):
        bitstream.decode_frame_bytes(bitstream.sequence_frame(blob, 1), "cuda")
    with pytest.raises(ValueError, match="not a RAHT frame container"):
        bitstream.decode_region_bytes(bitstream.sequence_frame(blob, 1), 1, (0, 4), "cuda")
