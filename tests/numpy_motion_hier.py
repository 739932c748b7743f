"""The hierarchical motion search (include/raht.h, "Hierarchical search") as a numpy model built on
``numpy_motion``: the pyramid of a frame, the search around a base, and the coarse-to-fine search. Costs are ``numpy_motion``'s,
bit for bit; tables are int64, so the entry 2^64 - 1 of an invalid pair reads -1."""
import numpy as np

from . import numpy_motion as MM
from . import numpy_predict as P0

INVALID = -1                                                             # 2^64 - 1 as int64


def pyramid(keys, C, levels):
    """-> per level l = 1 .. levels (keys_l uint64: the distinct keys >> 3 l, ascending; C_l float32: the run mean of C over every
    cell, ``numpy_predict.predict``'s sequential float32 sum and one division)"""
    keys, out = np.asarray(keys, np.uint64), []
    for l in range(1, levels + 1):
        cells = np.unique(keys >> np.uint64(3 * l))
        out.append((cells, P0.predict(cells << np.uint64(3 * l), keys, C, l)[0]))
    return out


def search_around(keys, ref_keys, C_ref, X, J, block_log2, base, cand, w, up=0):
    """-> (table (n_blocks, K) int64, best_k (n_blocks,) int32, best_cost (n_blocks,) int64, mv (n_blocks, 3) int8)"""
    b, first = MM.blocks(keys, block_log2)
    base, cand = np.asarray(base, np.int64).reshape(len(first) - 1, 3), np.asarray(cand, np.int64)
    table = np.zeros((len(base), len(cand)), np.int64)
    valid = np.zeros(table.shape, bool)
    for k, c in enumerate(cand):
        v = base + c                                                     # per block, in integers
        valid[:, k] = np.all(np.abs(v) <= 127, axis=1)
        q = MM.row_cost(X, MM.predict_v(keys, ref_keys, C_ref, J, v[b], up)[0], w)
        np.add.at(table[:, k], b, q.astype(np.int64))
    table[~valid] = INVALID
    big = np.where(valid, table, np.iinfo(np.int64).max)                 # (a cost is below 2^61)
    best_k = big.argmin(axis=1).astype(np.int32)                         # the first of the smallest valid ones
    none = ~valid.any(axis=1)
    best_cost = table[np.arange(len(table)), best_k]
    mv = (base + cand[best_k]).astype(np.int64)
    best_k[none], best_cost[none], mv[none] = -1, INVALID, 0
    return table, best_k, best_cost, mv.astype(np.int8)


def reach(levels, radius):
    return radius * 2 ** levels + 2 ** levels - 1


def search_hier(keys, ref_keys, C_ref, X, J, block_log2, levels, radius, w, up=0):
    """-> (mv of level 0 (n_blocks, 3) int8, best_cost of level 0, the vectors per level 0 .. levels)"""
    L, m = int(levels), int(block_log2)
    assert 0 <= L <= min(3, m - 1) and J - L >= 1 and 1 <= radius <= 3
    cur = [(np.asarray(keys, np.uint64), np.asarray(X, np.float32))] + pyramid(keys, X, L)
    ref = [(np.asarray(ref_keys, np.uint64), np.asarray(C_ref, np.float32))] + pyramid(ref_keys, C_ref, L)
    cand = MM.candidates(radius)
    _, best_k, cost = MM.search(cur[L][0], ref[L][0], ref[L][1], cur[L][1], J - L, m - L, cand, w, up if L == 0 else 0)
    mv = cand[best_k].astype(np.int8)
    per_level = [mv]
    for l in range(L - 1, -1, -1):
        _, _, cost, mv = search_around(cur[l][0], ref[l][0], ref[l][1], cur[l][1], J - l, m - l, 2 * mv.astype(np.int64), MM.candidates(1), w,
                                       up if l == 0 else 0)
        per_level.insert(0, mv)
    return mv, cost, per_level
