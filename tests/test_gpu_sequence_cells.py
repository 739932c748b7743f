"""bitstream.decode_sequence_cells on the frame sets of tests/test_gpu_sequence_bidir.py and
tests/test_gpu_sequence_block_modes.py: the voxels of a SET of cell ranges of a B frame are the rows of the ranges of what
decode_sequence_bytes returns for that frame, bit for bit; the chain is the closure under both references; the keys of one call
spare the next one every geometry decode; every byte outside the ranges the call names may be missing; on a wipe a region on one
side of the cut needs no attribute byte of the other anchor; and for P and motion-compensated frames the one-range call is
decode_sequence_region."""
import numpy as np
import pytest

from . import numpy_motion as MM
from . import numpy_region_set as N
from . import test_gpu_sequence_bidir as BIDIR
from . import test_gpu_sequence_block_modes as MODES
from . import test_gpu_sequence_motion as MOTION
from .test_gpu_sequence_region import _scrambled

pytestmark = pytest.mark.gpu

J, FRAMES, SHAPES = BIDIR.J, BIDIR.FRAMES, BIDIR.SHAPES
RANGE_SETS = [(2, [(3, 9)]), (2, [(0, 2), (5, 6), (40, 64)]), (5, [(1000, 9000)])]
WIPE = dict(gop=3, bframes=1, inter="always", block_log2=MODES.M_LOG2, block_modes=True)
# name -> (frames, blob, full decode)
SCENES = {
    "drifting, up 1": lambda D, w: BIDIR._coded("drifting", D, w, gop=FRAMES, bframes=1, inter="always", up=1),
    "drifting under two fields": lambda D, w: BIDIR._coded("drifting", D, w, gop=FRAMES, bframes=1, inter="always", motion=2, block_log2=2),
    "drifting, references 4 apart": lambda D, w: BIDIR._coded("drifting", D, w, gop=FRAMES, bframes=3, inter="always"),
    "drifting, predicted geometry": lambda D, w: BIDIR._coded("drifting", D, w, gop=FRAMES, bframes=1, inter="always", geometry_inter="always"),
    "wipe under block modes": lambda D, w: _wipe("wipe", D, w, **WIPE),
    "drifting wipe: fields and modes": lambda D, w: _wipe("drifting wipe", D, w, motion=1, **WIPE),
}


def _wipe(kind, D, n_wide, **enc):
    frames, _, blob, dec = MODES._coded(kind, D, n_wide, **enc)
    return frames, blob, dec


def _keys(frames):
    from raht_3dgs_codec_amd import synth
    return [synth.morton_keys(V, J) for V, _ in frames]


def _closure(refs, i):
    out, todo = set(), [i]
    while todo:
        f = todo.pop()
        if f not in out:
            out.add(f)
            todo += list(refs[f])
    return sorted(out)


def _rows_of(dec, keys, i, depth, ranges):
    import torch
    rows = N.set_rows(keys[i], J, depth, ranges)
    return rows, torch.cat([dec[i][0][a:b] for a, b in rows]), torch.cat([dec[i][1][a:b] for a, b in rows])


def _check(blob, dec, keys, refs, i, depth, ranges, name=""):
    """one region of frame i: the rows of the whole decode, the closure, cached keys, missing bytes -> info"""
    import torch
    from raht_3dgs_codec_amd import bitstream
    what = (name, i, depth, ranges)
    rows, Vw, Cw = _rows_of(dec, keys, i, depth, ranges)
    n = sum(b - a for a, b in rows)
    assert n > 0, what
    V, C, info = bitstream.decode_sequence_cells(blob, i, depth, ranges, "cuda")
    assert V.dtype == torch.int64 and C.dtype == torch.float32 and tuple(V.shape) == (n, 3), what
    assert torch.equal(V, Vw) and torch.equal(C.view(torch.int32), Cw.view(torch.int32)), what
    chain = _closure(refs, i)
    fr = info["frames"]
    assert info["chain"] == chain and sorted(fr) == chain, what
    assert fr[i]["ranges"] == ranges and fr[i]["rows"] == n, what
    assert info["bytes_needed"] == sum(fr[f]["bytes_needed"] for f in chain), what
    assert all(fr[f]["bytes_needed"] == sum(ln for _, ln in fr[f]["byte_ranges"]) for f in chain), what
    assert all(len(fr[f]["ranges"]) <= 512 and all(p[1] < q[0] for p, q in zip(fr[f]["ranges"], fr[f]["ranges"][1:])) for f in chain if f != i), what
    assert info["frames"][i]["geometry_decoded"] is True, what
    # the keys of the first call spare the second one every geometry decode
    V2, C2, info2 = bitstream.decode_sequence_cells(blob, i, depth, ranges, "cuda", keys=info["keys"])
    assert torch.equal(V2, V) and torch.equal(C2.view(torch.int32), C.view(torch.int32)), what
    assert not any(info2["frames"][f]["geometry_decoded"] for f in chain) and sorted(info2["keys"]) == sorted(info["keys"]), what
    drop = ("geometry_decoded",)
    assert [{k: v for k, v in info2["frames"][f].items() if k not in drop} for f in chain] == \
           [{k: v for k, v in fr[f].items() if k not in drop} for f in chain], what
    # every byte outside the named ranges may be missing
    spans = info["byte_ranges"]
    assert all(p[0] + p[1] <= q[0] for p, q in zip(spans, spans[1:])), what
    other, kept = _scrambled(blob, spans)
    assert kept == info["bytes_needed"] + spans[0][1] <= len(blob), what
    V3, C3, info3 = bitstream.decode_sequence_cells(other, i, depth, ranges, "cuda")
    assert torch.equal(V3, V) and torch.equal(C3.view(torch.int32), C.view(torch.int32)) and info3["byte_ranges"] == spans, what
    return info


@pytest.mark.parametrize("D,n_wide", SHAPES)
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_a_set_of_ranges_of_every_b_frame_is_rows_of_the_whole_decode(scene, D, n_wide):
    from raht_3dgs_codec_amd import bitstream
    frames, blob, dec = SCENES[scene](D, n_wide)
    keys, kinds, refs = _keys(frames), bitstream.sequence_kinds(blob), bitstream.sequence_refs(blob)
    b_frames = [i for i, k in enumerate(kinds) if k == "B"]
    assert b_frames and all(len(refs[i]) == 2 for i in b_frames), kinds
    if scene == "drifting, references 4 apart":
        assert [refs[i] for i in b_frames] == [(0, 4)] * 3
    if scene == "drifting, predicted geometry":
        assert bitstream.sequence_geometry(blob)[1:] == ["predicted"] * (len(frames) - 1)
    if scene == "drifting wipe: fields and modes":
        assert bitstream.sequence_motion(blob)[1] is not None and bitstream.sequence_modes(blob)[1] is not None
    for i in b_frames:
        for depth, ranges in RANGE_SETS:
            info = _check(blob, dec, keys, refs, i, depth, ranges, scene)
            if ranges == [(3, 9)]:                                            # six cells of 64: not every segment of every frame
                assert info["bytes_needed"] < len(blob), (scene, i, ranges)


@pytest.mark.parametrize("D,n_wide", SHAPES)
def test_on_a_wipe_a_side_of_the_cut_needs_one_anchor(D, n_wide):
    from raht_3dgs_codec_amd import bitstream
    frames, left, blob, dec = MODES._coded("wipe", D, n_wide, **WIPE)
    keys, refs = _keys(frames), bitstream.sequence_refs(blob)
    assert refs == [(), (0, 2), (0,)]
    modes = bitstream.sequence_modes(blob)[1]
    block = MM.blocks(keys[1], MODES.M_LOG2)[0]
    # depth-1 cells (0, 4) are x < 32 -- x is the key's top bit --, and every block there follows anchor 0
    a, b = N.set_rows(keys[1], J, 1, [(0, 4)])[0]
    assert np.array_equal(frames[1][0][a:b, 0] < MODES.CUT, np.ones(b - a, bool)) and a == 0 and np.all(frames[1][0][b:, 0] >= MODES.CUT)
    assert np.all(modes[block[a:b]] == 1) and np.all(modes[block[b:]] == 2)
    info = _check(blob, dec, keys, refs, 1, 1, [(0, 4)], "left of the cut")
    fr = info["frames"]
    occ = np.unique(keys[2] >> np.uint64(3))                                 # an unoccupied depth-5 cell of frame 2: an empty region of it
    gap = int(next(p + 1 for p, q in zip(occ, occ[1:]) if q > p + 1))
    empty = bitstream.decode_sequence_region(blob, 2, 5, (gap, gap + 1), "cuda")[2]["frames"][2]
    assert empty["rows"] == 0 and empty["segments_decoded"] == 0
    assert fr[2]["ranges"] == [] and fr[2]["rows"] == 0 and fr[2]["segments_decoded"] == 0 and fr[2]["bytes_needed"] == empty["bytes_needed"]
    assert fr[2]["byte_ranges"] == empty["byte_ranges"]
    assert fr[0]["ranges"] == [(0, 4)]
    # right of the cut: frame 2, and frame 0 only through frame 2
    fr = _check(blob, dec, keys, refs, 1, 1, [(4, 8)], "right of the cut")["frames"]
    assert fr[2]["ranges"] == [(4, 8)] and fr[2]["segments_decoded"] > 0
    through = bitstream.decode_sequence_cells(blob, 2, 1, fr[2]["ranges"], "cuda")[2]["frames"][0]
    assert fr[0]["ranges"] == through["ranges"] == [(4, 8)] and fr[0]["byte_ranges"] == through["byte_ranges"]
    # across the cut: frame 0 serves frame 1's left half directly and its right half through frame 2 -- a union
    fr = _check(blob, dec, keys, refs, 1, 1, [(2, 6)], "across the cut")["frames"]
    assert fr[2]["ranges"] == [(4, 6)] and fr[0]["ranges"] == [(2, 6)]
    # two ranges that leave a gap in frame 0's union
    fr = _check(blob, dec, keys, refs, 1, 1, [(0, 1), (7, 8)], "both corners")["frames"]
    assert fr[2]["ranges"] == [(7, 8)] and fr[0]["ranges"] == [(0, 1), (7, 8)]


@pytest.mark.parametrize("which", ["static", "moving"])
def test_for_p_and_m_frames_the_one_range_call_is_decode_sequence_region(which):
    import torch
    from raht_3dgs_codec_amd import bitstream
    enc = dict(gop=MOTION.FRAMES, inter="always") if which == "static" else MOTION.MOVING
    frames, blob, dec = MOTION._coded(which, 5, 0, **enc)
    magic = bitstream.M_MAGIC if which == "moving" else bitstream.P_MAGIC
    i = MOTION.FRAMES - 1
    assert bytes(bitstream.sequence_frame(blob, i)[:8]) == magic
    for f, depth, cells in ((i, 2, (3, 40)), (i, 5, (1000, 9000)), (2, 1, (0, 3)), (0, 2, (0, 64))):
        V, C, info = bitstream.decode_sequence_region(blob, f, depth, cells, "cuda")
        V2, C2, info2 = bitstream.decode_sequence_cells(blob, f, depth, [cells], "cuda")
        assert torch.equal(V, V2) and torch.equal(C.view(torch.int32), C2.view(torch.int32))
        k, k2 = info.pop("keys"), info2.pop("keys")
        assert sorted(k) == sorted(k2) and all(torch.equal(k[g], k2[g]) for g in k)
        assert info == info2 and info["chain"] == list(range(f + 1))


def test_refusals_from_the_headers_alone():
    from raht_3dgs_codec_amd import bitstream
    frames, blob, dec = SCENES["drifting under two fields"](5, 0)
    for what, ranges in {"no range": [], "an empty range": [(1, 1)], "ranges that overlap": [(0, 3), (2, 4)], "descending": [(4, 5), (0, 1)],
                         "past the last cell": [(0, 1), (63, 65)], "below 0": [(-1, 1)], "no pairs": [1, 2], "513 ranges": [(0, 1)] * 513}.items():
        with pytest.raises(ValueError, match="decode_sequence_cells"):
            bitstream.decode_sequence_cells(blob, 1, 2, ranges, "cpu")          # a device that would fail: it is never reached
            pytest.fail(what)
    with pytest.raises(ValueError, match="frame index must be in 0 .. 4"):
        bitstream.decode_sequence_cells(blob, 5, 2, [(0, 1)], "cpu")
    with pytest.raises(ValueError, match="depth"):
        bitstream.decode_sequence_cells(blob, 1, J, [(0, 1)], "cpu")
    off = bitstream.parse_sequence(blob)
    bad = bytearray(blob)
    bad[off[3] + 16: off[3] + 24] = np.array([2], np.int64).tobytes()        # ref_fwd past the last frame
    with pytest.raises(ValueError, match="sequence container: frame 3:") as e:
        bitstream.decode_sequence_cells(bytes(bad), 3, 2, [(0, 64)], "cpu")
    with pytest.raises(ValueError) as e2:
        bitstream.decode_sequence_bytes(bytes(bad), [3], "cpu")
    assert str(e.value) == str(e2.value)
    with pytest.raises(ValueError, match="frame 1 is a B frame"):
        bitstream.decode_sequence_region(blob, 1, 2, (3, 9), "cpu")
