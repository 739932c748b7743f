"""Test-only model of the region decoder over a SET of cell ranges and of the needed set of a predicted frame
(bitstream.decode_cells_bytes / decode_sequence_region) in numpy, on top of tests/numpy_region.py: the layout of R row
ranges in a frame's coded order, the float64 transform put together from the tree above the cells and ONE truncated plan over the
concatenated rows, the cells a prediction reaches into, and the motion field of a region. tests/test_region_set_model.py holds the
layout to the oracle's order_RAGFT and the transform to the whole-frame inverse; the GPU tests compare the kernels with this file."""
import numpy as np
import torch

from . import numpy_motion as MM
from . import numpy_region as M
from .numpy_ops import NumpyPlan

BUCKETS = M.BUCKETS


def layout_set(keys, bounds):
    """bounds: lo_0, hi_0, lo_1, ... ascending -> (1 + 2 R, 22): rows per bucket in the whole frame, then per range in [0, lo_r) and
    in [lo_r, hi_r)"""
    b = M.buckets(keys)
    bounds = [int(x) for x in bounds]
    parts = [b] + [x for lo, hi in zip(bounds[0::2], bounds[1::2]) for x in (b[:lo], b[lo:hi])]
    return np.stack([np.bincount(x, minlength=BUCKETS) for x in parts]).astype(np.int64)


def set_rows(keys, J, depth, ranges):
    """[(a, b)] of every range of cells"""
    return [M.region_rows(keys, J, depth, c0, c1) for c0, c1 in ranges]


def coded_runs_set(keys, J, depth, rows):
    """-> (n_top, runs): one (coded row, row of the region's own coded matrix, count) per (bucket finer than the cells, range) with
    rows, buckets coarse to fine and ranges ascending inside a bucket; the region's matrix starts with one root slot per occupied
    cell of the set"""
    table = layout_set(keys, [x for r in rows for x in r])
    whole, cut = table[0], J - depth
    n_top = int(whole[cut:].sum())
    coded, dst, runs = n_top, int(sum(table[2 + 2 * r][cut:].sum() for r in range(len(rows)))), []
    for beta in range(cut - 1, -1, -1):
        for r in range(len(rows)):
            before, inside = int(table[1 + 2 * r][beta]), int(table[2 + 2 * r][beta])
            if inside:
                runs.append((coded + before, dst, inside))
            dst += inside
        coded += int(whole[beta])
    return n_top, runs


def assemble(src, runs, n_dst_rows):
    src = np.asarray(src)
    out = np.zeros((n_dst_rows, src.shape[1]), src.dtype)
    for s, d, n in runs:
        out[d: d + n] = src[s: s + n]
    return out


def decode_cells(keys, J, Q, steps, depth, ranges):
    """float64 decoder of a set of cell ranges from the coded rows it needs only -> (rows [(a, b)], (n, D) float64, coded rows read)"""
    k = np.asarray(keys, np.uint64)
    Q = np.asarray(Q)
    st = torch.as_tensor(np.asarray(steps, np.float64))
    tl = 3 * (J - depth)
    rows = set_rows(k, J, depth, ranges)
    n = sum(b - a for a, b in rows)
    if n == 0:
        return rows, np.zeros((0, Q.shape[1])), np.zeros(0, np.int64)
    ck, cf = M.cells(k, tl)
    pick = np.concatenate([np.arange(np.searchsorted(ck, np.uint64(c0)), np.searchsorted(ck, np.uint64(c1))) for c0, c1 in ranges])
    n_top, runs = coded_runs_set(k, J, depth, rows)
    assert n_top == ck.shape[0]
    top = NumpyPlan(M._t(ck), 3 * depth, leaf_weights=torch.from_numpy(np.diff(cf)))
    roots = top.dequant_inverse(torch.from_numpy(Q[:n_top]), st)[torch.from_numpy(pick)]
    kr = np.concatenate([k[a:b] for a, b in rows])
    plan = NumpyPlan(M._t(kr), 3 * J, top_level=tl)
    assert plan.n_roots == len(pick) == (runs[0][1] if runs else n)
    read = np.concatenate([np.arange(n_top)] + [np.arange(s, s + c) for s, _, c in runs])
    return rows, plan.dequant_inverse(torch.from_numpy(assemble(Q, runs, n)), st, roots=roots).numpy(), read


# ---- the needed set -------------------------------------------------------------------------------------------------------------
def region_motion(block_first, mv, rows):
    """block_first (n_blocks + 1 rows of the whole frame) and mv of a frame, rows [(a, b)] of the region's ranges -> (block_first, mv)
    over the rows of the region matrix: per range, the blocks with rows in it, each with its first row in the region"""
    bf = np.asarray(block_first, np.int64)
    first, field, base = [], [], 0
    for a, b in rows:
        for blk in range(len(bf) - 1):
            if b > a and bf[blk] < b and bf[blk + 1] > a:
                first.append(max(int(bf[blk]) - a, 0) + base)
                field.append(mv[blk])
        base += b - a
    return np.array(first + [base], np.int64), np.array(field, np.int8).reshape(-1, 3)


def needs(keys, J, top_level, up, block_first=None, mv=None):
    """np.unique of the cells of the shifted keys: (k' >> w) << (w - top_level), w = max(top_level, 3 up), over the rows with a match
    (all of them without a field) -> ascending uint64"""
    k = np.asarray(keys, np.uint64)
    if mv is not None:
        blk = np.searchsorted(np.asarray(block_first, np.int64), np.arange(len(k)), "right") - 1
        ok, k = MM.shifted(k, J, np.asarray(mv, np.int64)[blk])
        k = k[ok]
    w = max(int(top_level), 3 * int(up))
    return np.unique((k >> np.uint64(w)) << np.uint64(w - int(top_level)))


def merge(cells, group):
    """ascending first cells of aligned groups of `group` cells -> [(c0, c1)], neighbours merged"""
    out = []
    for c in (int(x) for x in cells):
        if out and out[-1][1] == c:
            out[-1] = (out[-1][0], c + group)
        else:
            out.append((c, c + group))
    return out
