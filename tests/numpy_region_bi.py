"""Test-only model of the needed sets of a B frame (raht_region_needs_bi, bitstream.decode_sequence_cells) in numpy,
on top of tests/numpy_region_set.py: the cells of both references that the two-reference predictor reaches into under two motion
fields and the block modes, the blocks of a region for any number of per-block arrays, and the union of range lists."""
import numpy as np

from . import numpy_region_set as N

USES = ((0, 1), (0, 2))                                                   # the modes that use reference 0, reference 1


def needs_bi(keys, J, top_level, up, block_first=None, mv0=None, mv1=None, mode=None):
    """-> (cells0, cells1), ascending uint64: ``numpy_region_set.needs`` under mv_r over the rows whose block's mode uses reference
    r (0: both, 1: reference 0, 2: reference 1, 3 and above: none); a field that is None is zero, modes that are None all 0"""
    k = np.asarray(keys, np.uint64)
    if block_first is None:
        assert mv0 is None and mv1 is None and mode is None
        both = N.needs(k, J, top_level, up)
        return both, both.copy()
    bf = np.asarray(block_first, np.int64)
    blk = np.searchsorted(bf, np.arange(len(k)), "right") - 1
    md = np.zeros(len(bf) - 1, np.int64) if mode is None else np.minimum(np.asarray(mode, np.int64), 3)
    out = []
    for mv, uses in zip((mv0, mv1), USES):
        rows = np.flatnonzero(np.isin(md[blk], uses))
        field = np.zeros((len(bf) - 1, 3), np.int8) if mv is None else np.asarray(mv, np.int8)
        # the rows that use the reference, each as a block of its own under its block's vector
        out.append(N.needs(k[rows], J, top_level, up, np.arange(len(rows) + 1), field[blk[rows]]) if len(rows) else np.zeros(0, np.uint64))
    return tuple(out)


def region_blocks(block_first, rows, *per_block):
    """``numpy_region_set.region_motion`` for any number of per-block arrays (None stays None): block_first (n_blocks + 1 rows of
    the whole frame), rows [(a, b)] of the region's ranges -> (block_first over the rows of the region matrix, [every array over
    the same blocks]): per range, the blocks with rows in it, each with its first row in the region"""
    bf = np.asarray(block_first, np.int64)
    first, pick, base = [], [], 0
    for a, b in rows:
        for blk in range(len(bf) - 1):
            if b > a and bf[blk] < b and bf[blk + 1] > a:
                first.append(max(int(bf[blk]) - a, 0) + base)
                pick.append(blk)
        base += b - a
    pick = np.array(pick, np.int64)
    return np.array(first + [base], np.int64), [None if t is None else np.asarray(t)[pick] for t in per_block]


def union(range_lists, limit=512):
    """ascending lists of disjoint ranges -> the ascending disjoint ranges that cover them, overlapping and touching ones merged;
    above ``limit`` ranges the narrowest gaps are closed, the first of equally narrow ones first, until ``limit`` are left. A
    single non-empty list is returned as it is."""
    lists = [list(r) for r in range_lists if len(r)]
    if len(lists) <= 1:
        return [tuple(r) for r in lists[0]] if lists else []
    cover = set()
    for rs in lists:
        for c0, c1 in rs:
            cover.update(range(c0, c1))
    out = []
    for c in sorted(cover):
        if out and out[-1][1] == c:
            out[-1][1] = c + 1
        else:
            out.append([c, c + 1])
    while len(out) > limit:
        gaps = [q[0] - p[1] for p, q in zip(out, out[1:])]
        g = gaps.index(min(gaps))
        out[g: g + 2] = [[out[g][0], out[g + 1][1]]]
    return [tuple(r) for r in out]
