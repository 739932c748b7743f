"""CPU-only checks of the model of a region made of several cell ranges (tests/numpy_region_set.py) and of the host
code of bitstream.decode_cells_bytes / decode_sequence_region: the runs of a set of ranges against the oracle's order_RAGFT, the
float64 transform over ONE truncated plan against the whole-frame inverse, the needed set of a predicted frame against the
predictor's model on the whole reference, and the refusals that the headers alone decide."""
import numpy as np
import pytest

from . import numpy_motion as MM
from . import numpy_predict as P0
from . import numpy_region as M
from . import numpy_region_set as N
from .test_region_model import _order

# (draws, J, depths)
SHAPES = [(3000, 6, (1, 2)), (400, 5, (4,))]


def _frames():
    from raht_3dgs_codec_amd import synth
    return [(synth.sorted_unique_keys(n, J, 40 + J), J, depths) for n, J, depths in SHAPES]


def range_sets(keys, J, depth):
    """{name: [(c0, c1)]}: two and three ranges, with the cases a single range cannot show"""
    occ, cnt = np.unique(np.asarray(keys, np.uint64) >> np.uint64(3 * (J - depth)), return_counts=True)
    occ = [int(c) for c in occ]
    one = lambda c: (c, c + 1)
    out = {"first + last": [one(occ[0]), one(occ[-1])], "three": [one(occ[0]), (occ[len(occ) // 3], occ[len(occ) // 2] + 1), one(occ[-1])]}
    touching = [i for i in range(len(occ) - 1) if occ[i + 1] == occ[i] + 1]
    if touching:
        i = touching[len(touching) // 2]
        out["adjacent cells as two ranges"] = [one(occ[i]), one(occ[i + 1])]
    gaps = [(p, q) for p, q in zip(occ, occ[1:]) if q > p + 1]
    if gaps:
        p, q = gaps[len(gaps) // 2]
        out["empty cells between occupied ones"] = [one(p), (p + 1, q), one(q)]
    if np.any(cnt == 1):
        c = occ[int(np.nonzero(cnt == 1)[0][-1])]
        out["a one-voxel cell"] = [one(occ[0]), one(c)] if c != occ[0] else [one(c), one(occ[-1])]
    return out


def test_runs_of_a_set_against_the_oracles_order(oracle):
    from raht_3dgs_codec_amd import bitstream
    seen = set()
    for keys, J, depths in _frames():
        order = _order(oracle, keys, J)
        b = M.buckets(keys)
        for depth in depths:
            tl = 3 * (J - depth)
            for name, ranges in range_sets(keys, J, depth).items():
                seen.add(name)
                rows = N.set_rows(keys, J, depth, ranges)
                reg = np.concatenate([np.arange(a, e) for a, e in rows])             # the frame row of every region row
                kr = keys[reg]
                n_roots = len(np.unique(kr >> np.uint64(tl)))
                table = N.layout_set(keys, [x for r in rows for x in r])
                n_top, runs = bitstream.region_runs_set(table.tolist(), J, depth, n_roots)
                assert (n_top, runs) == N.coded_runs_set(keys, J, depth, rows), (J, depth, name)
                assert n_top == len(M.cells(keys, tl)[0])
                own = np.argsort(-M.buckets(kr), kind="stable")                       # the region plan's own coded order
                assert np.all(M.buckets(kr)[own[:n_roots]] >= J - depth) and np.all(M.buckets(kr)[own[n_roots:]] < J - depth)
                got, end = [], n_roots
                for src, dst, n in runs:
                    fr = order[src: src + n]
                    assert dst == end and np.all(np.diff(fr) > 0) and len(set(b[fr])) == 1 and np.all(np.isin(fr, reg)), (J, depth, name)
                    assert np.array_equal(np.searchsorted(reg, fr), own[dst: dst + n]), (J, depth, name)
                    got.append(fr)
                    end = dst + n
                assert end == len(reg), (J, depth, name)
                fine = reg[b[reg] < J - depth]
                assert np.array_equal(np.sort(np.concatenate(got)) if got else np.zeros(0, np.int64), fine), (J, depth, name)
                if len(ranges) == 1 or name == "first + last":
                    # one range at a time is the one-range rule
                    for (a, e) in rows:
                        nr = len(np.unique(keys[a:e] >> np.uint64(tl)))
                        assert bitstream.region_runs(M.layout(keys, a, e).tolist(), J, depth, nr) == M.coded_runs(keys, J, depth, a, e)
    assert seen == {"first + last", "three", "adjacent cells as two ranges", "empty cells between occupied ones", "a one-voxel cell"}


def test_float64_transform_of_a_set_equals_the_whole_frame_inverse():
    rng = np.random.default_rng(6)
    for keys, J, depths in _frames():
        Nv, D = len(keys), 4
        Q = rng.integers(-40, 41, size=(Nv, D)).astype(np.int32)
        Q[0] += 1000                                                     # a DC row that matters
        steps = np.array([0.01, 0.02, 0.5, 0.004])
        whole = M.decode_frame(keys, J, Q, steps)
        for depth in depths:
            for name, ranges in range_sets(keys, J, depth).items():
                rows, C, read = N.decode_cells(keys, J, Q, steps, depth, ranges)
                want = np.concatenate([whole[a:b] for a, b in rows])
                assert C.shape == want.shape
                assert np.abs(C - want).max(initial=0.0) <= 1e-12 * np.abs(whole).max(), (Nv, J, depth, name)     # (test_region_model's bound)
                assert len(read) == len(set(read)) and len(read) < Nv, (Nv, J, depth, name)
                # and the concatenation of the one-range model, to the same bound
                parts = np.concatenate([M.decode_region(keys, J, Q, steps, depth, c0, c1)[2] for c0, c1 in ranges])
                assert np.abs(C - parts).max(initial=0.0) <= 1e-12 * np.abs(whole).max(), (Nv, J, depth, name)


# ---- the needed set -------------------------------------------------------------------------------------------------------------
J5, BLOCK = 5, 2
# (name, vector of every block or None for no field or "mixed", up, depth)
NEEDS = [("no field, up 0", None, 0, 2), ("no field, up 1", None, 1, 2), ("a zero field", (0, 0, 0), 0, 2),
         ("(1, -2, 1) at the cube's faces", (1, -2, 1), 0, 2), ("(1, -2, 1), up 1", (1, -2, 1), 1, 3), ("a field of many vectors", "mixed", 1, 2),
         ("up above J - depth: groups of 8", (1, -2, 1), 2, 4), ("up above J - depth without a field: groups of 64", None, 3, 4)]


def _two_frames():
    from raht_3dgs_codec_amd import synth
    rng = np.random.default_rng(8)
    cur = synth.sorted_unique_keys(400, J5, 51)
    face = MM.morton(np.array([[31, 3, 7], [30, 1, 0], [5, 0, 31], [0, 1, 2], [31, 31, 31], [0, 0, 0]]), J5)      # voxels on faces and corners
    cur = np.unique(np.concatenate([cur, face]))
    ok, moved = MM.shifted(cur, J5, (1, -2, 1))
    ref = np.unique(np.concatenate([moved[ok][::2], cur[::3], synth.sorted_unique_keys(300, J5, 52)]))
    return cur, ref, rng.standard_normal((len(ref), 2)).astype(np.float32)


@pytest.mark.parametrize("name, vec, up, depth", NEEDS)
def test_needed_set_holds_every_run_the_predictor_resolves(name, vec, up, depth):
    import torch
    from raht_3dgs_codec_amd import bitstream
    cur, ref, C_ref = _two_frames()
    tl, group = 3 * (J5 - depth), 8 ** max(up - (J5 - depth), 0)
    occ = np.unique(cur >> np.uint64(tl)).astype(np.int64)
    S = [(int(occ[1]), int(occ[len(occ) // 3]) + 1), (int(occ[-1]), int(occ[-1]) + 1), ] if depth < 4 else \
        [(int(occ[0]), int(occ[2]) + 1), (int(occ[len(occ) // 2]), int(occ[len(occ) // 2]) + 3), (int(occ[-1]), 8 ** depth)]
    rows = N.set_rows(cur, J5, depth, S)
    reg = np.concatenate([np.arange(a, b) for a, b in rows])
    kr = cur[reg]
    if vec is None:
        bf_r = mv_r = None
        P_whole = P0.predict(cur, ref, C_ref, up)[0][reg]
    else:
        _, bf = MM.blocks(cur, BLOCK)
        mv = np.random.default_rng(9).integers(-2, 3, size=(len(bf) - 1, 3)).astype(np.int8) if vec == "mixed" else \
            np.tile(np.array(vec, np.int8), (len(bf) - 1, 1))
        bf_r, mv_r = N.region_motion(bf, mv, rows)
        assert bf_r[0] == 0 and bf_r[-1] == len(kr) and np.all(np.diff(bf_r) > 0) and len(mv_r) == len(bf_r) - 1
        P_whole = MM.predict_mc(cur, ref, C_ref, J5, BLOCK, mv, up)[0][reg]
        got_bf, got_mv = bitstream._region_motion(torch.from_numpy(bf), torch.from_numpy(mv), rows, "cpu")
        assert np.array_equal(got_bf.numpy(), bf_r) and np.array_equal(got_mv.numpy(), mv_r), name
        if vec == (1, -2, 1):
            assert not MM.shifted(kr, J5, vec)[0].all()                      # rows that leave the cube: they ask for nothing
    need = N.needs(kr, J5, tl, up, bf_r, mv_r)
    assert np.all(need % np.uint64(group) == 0) and np.all(np.diff(need.astype(np.int64)) >= group)
    Sg = N.merge(need, group)
    assert all(p[1] < q[0] for p, q in zip(Sg, Sg[1:])) and sum(c1 - c0 for c0, c1 in Sg) == group * len(need) < 8 ** depth, name
    assert bitstream._merge_cells(torch.from_numpy(need.astype(np.int64)), group) == Sg, name
    few = bitstream._merge_cells(torch.from_numpy(need.astype(np.int64)), group, limit=2)
    assert len(few) <= 2 and all(any(a <= c0 and c1 <= b for a, b in few) for c0, c1 in Sg), name
    # the predictor on the region and on the needed rows of the reference alone gives the bits it gives on the whole frames
    g_rows = N.set_rows(ref, J5, depth, Sg)
    gr = np.concatenate([np.arange(a, b) for a, b in g_rows]).astype(np.int64)
    assert 0 < len(gr) < len(ref), name
    if vec is None:
        P_reg = P0.predict(kr, ref[gr], C_ref[gr], up)[0]
    else:
        blk = np.searchsorted(bf_r, np.arange(len(kr)), "right") - 1
        P_reg = MM.predict_v(kr, ref[gr], C_ref[gr], J5, mv_r[blk].astype(np.int64), up)[0]
    assert np.array_equal(P_reg.view(np.int32), P_whole.view(np.int32)) and np.any(P_whole != 0), name


# ---- what the headers decide ----------------------------------------------------------------------------------------------------
def test_refusals_from_the_headers_alone():
    from raht_3dgs_codec_amd import bitstream
    f = P0.tiny_frame(J=3)
    seq = P0.sequence([f, P0.pframe(f, 1, 0), P0.pframe(f, 2, 1)])
    bad = {"an index past the end": dict(i=3), "a negative index": dict(i=-1), "an index that is no number": dict(i="x"),
           "depth = 0": dict(depth=0), "depth = J": dict(depth=3), "c0 = c1": dict(cells=(2, 2)), "c0 < 0": dict(cells=(-1, 2)),
           "c1 > 8^depth": dict(cells=(0, 65)), "three cells": dict(cells=(0, 1, 2)), "keys that are no dict": dict(keys=[1]),
           "more frames than the caller allows": dict(max_frames=2), "more voxels than the caller allows": dict(max_voxels=0)}
    for what, kw in bad.items():
        args = dict(blob=seq, i=2, depth=2, cells=(0, 64), device="cpu")           # a device that would fail: it is never reached
        args.update(kw)
        with pytest.raises(ValueError):
            bitstream.decode_sequence_region(**args)
            pytest.fail(what)
    with pytest.raises(ValueError, match="frame index must be in 0 .. 2"):
        bitstream.decode_sequence_region(seq, 3, 1, (0, 1), "cpu")
    # a chain that reaches before frame 0, a broken link in the chain, a J that changes along it: named by the frame, as decode_sequence_bytes does
    for frames, i, named in (([f, f, P0.pframe(f, 3, 0)], 2, 2), ([f, P0.pframe(f, 0, 0), P0.pframe(f, 1, 0)], 2, 1),
                             ([f, P0.pframe(P0.tiny_frame(J=2)), P0.pframe(f, 2, 0)], 1, 1), ([P0.pframe(f), P0.pframe(f)], 1, 0)):
        s = P0.sequence(frames)
        with pytest.raises(ValueError, match=f"sequence container: frame {named}:") as e:
            bitstream.decode_sequence_region(s, i, 1, (0, 8), "cpu")
        with pytest.raises(ValueError) as e2:
            bitstream.decode_sequence_bytes(s, [i], "cpu")
        assert str(e.value) == str(e2.value)
    # frames the chain does not pass are not looked at
    s = P0.sequence([f, P0.pframe(f, 1, 0), f, P0.pframe(f, 4, 0)])
    with pytest.raises(ValueError, match="depth"):
        bitstream.decode_sequence_region(s, 1, 3, (0, 8), "cpu")
    # the one-frame decoders keep refusing a wrapped frame, and the set decoder its arguments
    with pytest.raises(ValueError, match="not a RAHT frame container"):
        bitstream.decode_cells_bytes(bitstream.sequence_frame(seq, 1), 1, [(0, 1)], "cpu")
    for what, ranges in {"no range": [], "an empty range": [(1, 1)], "ranges that overlap": [(0, 3), (2, 4)], "descending": [(4, 5), (0, 1)],
                         "past the last cell": [(0, 1), (7, 9)], "below 0": [(-1, 1)], "no pairs": [1, 2], "513 ranges": [(0, 1)] * 513}.items():
        with pytest.raises(ValueError, match="decode_cells_bytes"):
            bitstream.decode_cells_bytes(f, 1, ranges, "cpu")
            pytest.fail(what)
    with pytest.raises(ValueError, match="depth"):
        bitstream.decode_cells_bytes(f, 3, [(0, 1)], "cpu")
