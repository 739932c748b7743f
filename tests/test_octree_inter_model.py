"""The numpy model of the predicted octree geometry (tests/numpy_octree_inter.py) on the CPU: against the definition written
out by brute force, through its own decoder, and the two size claims the sequence coder's choice rests on -- an identical
reference costs 8 bytes per segment, an unrelated one costs more than the intra section."""
import numpy as np
import pytest

from . import numpy_octree as M
from . import numpy_octree_inter as MI


def _host_rlgr(sym):
    from raht_3dgs_codec_amd import rlgr
    m = rlgr.membuf()
    m.rlgrWrite(np.ascontiguousarray(sym, np.int32), 0)
    return m.get_array()


def _pairs():
    rng = np.random.default_rng(20261020)
    out = [("one voxel each", np.array([5], np.uint64), np.array([2], np.uint64), 1),
           ("one voxel, the same", np.array([5], np.uint64), np.array([5], np.uint64), 1),
           ("deep, one voxel each", np.array([8 ** 21 - 1], np.uint64), np.array([8 ** 21 - 1], np.uint64), 21),
           ("deep, first and last", np.array([0, 8 ** 21 - 1], np.uint64), np.array([8 ** 21 - 2], np.uint64), 21),
           ("full cube against one voxel", np.arange(8 ** 3, dtype=np.uint64), np.array([77], np.uint64), 3),
           ("one voxel against the full cube", np.array([77], np.uint64), np.arange(8 ** 3, dtype=np.uint64), 3)]
    for J in (1, 2, 3, 5, 8, 21):
        for n, m in ((1, 7), (7, 1), (60, 60), (200, 90)):
            k = np.unique(rng.integers(0, 8 ** J, size=n, dtype=np.uint64))
            r = np.unique(rng.integers(0, 8 ** J, size=m, dtype=np.uint64))
            out.append((f"random J={J} n={n} m={m}", k, r, J))
            mixed = np.unique(np.concatenate([k[::2], r]))                   # shares voxels with k
            out.append((f"overlapping J={J} n={n} m={m}", k, mixed, J))
    return out


def test_model_equals_the_definition():
    for name, k, r, J in _pairs():
        got, want = MI.pred_levels(k, r, J), MI.pred_brute_force(k, r, J)
        assert len(got) == J and all(np.array_equal(a, b) for a, b in zip(got, want)), name
        counts, res = MI.res_stream(k, r, J)
        assert len(res) == sum(counts[:-1]) and np.array_equal(res, M.occ_stream(k, J)[1] ^ np.concatenate(want)), name


def test_an_identical_reference_predicts_every_byte():
    for name, k, _, J in _pairs():
        assert not MI.res_stream(k, k, J)[1].any(), name
        assert np.array_equal(np.concatenate(MI.pred_levels(k, k, J)), M.occ_stream(k, J)[1]), name


def test_model_round_trip_and_its_refusals():
    for name, k, r, J in _pairs():
        counts, res = MI.res_stream(k, r, J)
        assert np.array_equal(MI.res_decode(res, counts, r, J), k), name
    k, r, J = _pairs()[-1][1:]
    counts, res = MI.res_stream(k, r, J)
    occ = M.occ_stream(k, J)[1]
    zero = res.copy()
    zero[3] ^= occ[3]                                                        # the reconstructed byte becomes 0
    with pytest.raises(ValueError, match="is 0"):
        MI.res_decode(zero, counts, r, J)
    flip = res.copy()
    at = int(np.flatnonzero(occ != 0xff)[-1])
    flip[at] ^= np.uint8(1 << int(np.flatnonzero(np.unpackbits(occ[at: at + 1], bitorder="little") == 0)[0]))   # one child more
    with pytest.raises(ValueError, match="do not add up"):
        MI.res_decode(flip, counts, r, J)


def test_an_identical_reference_costs_eight_bytes_per_segment():
    """all residuals are 0: the table is the identity, n_used is 1, and a segment of up to 256 zeros codes to 3 bytes at most --
    one 4-byte slot and its 4-byte length"""
    from raht_3dgs_codec_amd import synth
    for n, J, seed, S in ((3000, 6, 11, 256), (20000, 10, 5, 256), (3000, 6, 11, 64), (1, 3, 1, 256)):
        k = synth.sorted_unique_keys(n, J, seed)
        blob = MI.section(k, k, J, 1, S, _host_rlgr)
        n_nodes = sum(M.occ_stream(k, J)[0][:-1])
        nseg = (n_nodes + S - 1) // S
        assert len(blob) == MI.header_bytes(J) + 256 + 8 * nseg, (n, J, S)
        body = MI.header_bytes(J)
        assert np.array_equal(np.frombuffer(blob, np.uint8, 256, body), np.arange(256, dtype=np.uint8))
        assert [int(x) for x in np.frombuffer(blob, np.int64, 7, 8)] == [J, len(k), 1, n_nodes, S, len(k), 1]
    for n in (1, 2, 63, 64, 255, 256, 257):                                  # the claim about the coder itself
        assert len(_host_rlgr(np.zeros(n, np.int32))) <= 3, n


def test_an_unrelated_reference_costs_more_than_the_intra_section():
    """independent scenes at J = 10: the reference's occupancy is noise to the frame's, and the residual's 256 values are spread
    more evenly than the occupancy's -- prediction must be a per-frame choice"""
    from raht_3dgs_codec_amd import synth
    keys = [np.unique(synth.scene(20000, 10, 5, seed=s)[1].astype(np.uint64)) for s in range(1, 6)]
    for i in range(1, 5):
        intra = M.geometry_section(keys[i], 10, 1, 256, _host_rlgr)
        pred = MI.section(keys[i], keys[i - 1], 10, 1, 256, _host_rlgr)
        print(f"frame {i}: intra {len(intra)} B, predicted {len(pred)} B")
        assert len(pred) > len(intra), (i, len(pred), len(intra))
