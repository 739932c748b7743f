"""Test-only model of the region decoder (bitstream.decode_region_bytes) in numpy: where the rows of a run of octree
cells lie in a frame's coded order, which segments hold them, and the float64 transform put together from the tree above the cells
and a truncated plan over the region (tests/numpy_ops.NumpyPlan). tests/test_region_model.py holds the layout to the oracle's
order_RAGFT and the transform to the whole-frame inverse; the GPU tests compare the kernels and the decoder with this file."""
import numpy as np
import torch

from .numpy_ops import NumpyPlan, _msb

BUCKETS = 22                                                 # RAHT_REGION_BUCKETS


def buckets(keys):
    """bucket of every row: msb(key[i] ^ key[i-1]) / 3, row 0: 21"""
    k = np.asarray(keys, np.uint64)
    b = np.full(k.shape[0], BUCKETS - 1, np.int64)
    if k.shape[0] > 1:
        b[1:] = _msb(k[1:] ^ k[:-1]) // 3
    return b


def layout(keys, row_lo, row_hi):
    """(3, 22): rows per bucket in the whole frame, in [0, row_lo), in [row_lo, row_hi)"""
    b = buckets(keys)
    return np.stack([np.bincount(x, minlength=BUCKETS) for x in (b, b[:row_lo], b[row_lo:row_hi])]).astype(np.int64)


def cells(keys, top_level):
    """-> (cell_keys uint64 (n,), cell_first int64 (n + 1,)): the rows with i == 0 or lvl >= top_level, and N"""
    k = np.asarray(keys, np.uint64)
    head = np.ones(k.shape[0], bool)
    if k.shape[0] > 1:
        head[1:] = _msb(k[1:] ^ k[:-1]) >= top_level
    first = np.nonzero(head)[0]
    return k[first] >> np.uint64(top_level), np.concatenate([first, [k.shape[0]]]).astype(np.int64)


def region_rows(keys, J, depth, c0, c1):
    """rows [a, b) of the voxels inside the depth-`depth` cells [c0, c1), from the keys themselves"""
    cell = np.asarray(keys, np.uint64) >> np.uint64(3 * (J - depth))
    return int(np.searchsorted(cell, np.uint64(c0), "left")), int(np.searchsorted(cell, np.uint64(c1), "left"))


def coded_runs(keys, J, depth, a, b):
    """-> (n_top, runs): the first n_top coded rows of the frame are the tree above `depth`; runs = [(coded row, row of the
    region's own coded matrix, count)] for every bucket finer than the cells with rows in [a, b), coarse to fine. The region's
    own matrix starts with one root slot per occupied cell."""
    whole, before, inside = layout(keys, a, b)
    cut = J - depth
    n_top = int(whole[cut:].sum())
    coded, dst, runs = n_top, int(inside[cut:].sum()), []
    for beta in range(cut - 1, -1, -1):
        if inside[beta]:
            runs.append((coded + int(before[beta]), dst, int(inside[beta])))
        coded += int(whole[beta])
        dst += int(inside[beta])
    return n_top, runs


def segments(n_top, runs, seg_len):
    """ascending indices of the segments that hold coded rows [0, n_top) and the runs"""
    need = set(range(0, (n_top - 1) // seg_len + 1))
    for r, _, n in runs:
        need |= set(range(r // seg_len, (r + n - 1) // seg_len + 1))
    return sorted(need)


def covered_rows(seg_ids, seg_len, N):
    """the coded rows the selected segments hold, in the order they decode to"""
    return np.concatenate([np.arange(s * seg_len, min((s + 1) * seg_len, N)) for s in seg_ids])


def regions(keys, J, depth):
    """{name: (c0, c1)}: first cells, last cells, a middle range, all cells and, where the scene has them, a range of empty cells
    only and a cell that holds one voxel"""
    occ, cnt = np.unique(np.asarray(keys, np.uint64) >> np.uint64(3 * (J - depth)), return_counts=True)
    occ = [int(c) for c in occ]
    n, full = len(occ), 8 ** depth
    out = {"first": (0, occ[min(1, n - 1)] + 1), "last": (occ[max(n - 2, 0)], full), "middle": (occ[n // 3], occ[(2 * n) // 3] + 1),
           "all": (0, full)}
    gaps = [(p + 1, q) for p, q in zip([-1] + occ, occ + [full]) if q > p + 1]
    if gaps:
        out["empty"] = gaps[len(gaps) // 2]
    if np.any(cnt == 1):
        c = occ[int(np.nonzero(cnt == 1)[0][0])]
        out["one voxel"] = (c, c + 1)
    return out


def _t(keys):
    return torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64).copy())


def decode_frame(keys, J, Q, steps):
    """float64 whole-frame inverse: Q (N, D) integers in coded order, steps scalar or (D,) -> (N, D) float64"""
    st = torch.as_tensor(np.asarray(steps, np.float64))
    return NumpyPlan(_t(keys), 3 * J).dequant_inverse(torch.from_numpy(np.asarray(Q)), st).numpy()


def decode_region(keys, J, Q, steps, depth, c0, c1):
    """float64 region decoder from the coded rows it needs only -> (a, b, (b - a, D) float64, coded rows read)"""
    k = np.asarray(keys, np.uint64)
    Q = np.asarray(Q)
    st = torch.as_tensor(np.asarray(steps, np.float64))
    tl = 3 * (J - depth)
    a, b = region_rows(k, J, depth, c0, c1)
    if a == b:
        return a, b, np.zeros((0, Q.shape[1])), np.zeros(0, np.int64)
    ck, cf = cells(k, tl)
    j0, j1 = int(np.searchsorted(ck, np.uint64(c0))), int(np.searchsorted(ck, np.uint64(c1)))
    n_top, runs = coded_runs(k, J, depth, a, b)
    assert n_top == ck.shape[0] and (int(cf[j0]), int(cf[j1])) == (a, b)
    top = NumpyPlan(_t(ck), 3 * depth, leaf_weights=torch.from_numpy(np.diff(cf)))
    roots = top.dequant_inverse(torch.from_numpy(Q[:n_top]), st)[j0:j1]
    Qr = np.zeros((b - a, Q.shape[1]), Q.dtype)
    read = [np.arange(n_top)]
    for src, dst, n in runs:
        Qr[dst: dst + n] = Q[src: src + n]
        read.append(np.arange(src, src + n))
    plan = NumpyPlan(_t(k[a:b]), 3 * J, top_level=tl)
    assert plan.n_roots == j1 - j0
    return a, b, plan.dequant_inverse(torch.from_numpy(Qr), st, roots=roots).numpy(), np.concatenate(read)


def container(Q, seg_len, encode, flag=1):
    """SegmentedCoder.container() of the (N, D) integers Q with `encode(symbols, flag) -> uint8 stream` as the segment coder:
    magic | int64 N, D, seg_len, flag, payload bytes | uint32 length of every segment, channel-major | the streams in 4-byte slots"""
    Q = np.asarray(Q)
    N, D = Q.shape
    streams = [np.asarray(encode(Q[s: s + seg_len, c], flag), np.uint8) for c in range(D) for s in range(0, N, seg_len)]
    lens = np.array([len(x) for x in streams], np.uint32)
    slots = b"".join(x.tobytes() + b"\0" * (-len(x) % 4) for x in streams)
    return b"RLGS0001" + np.array([N, D, seg_len, flag, len(slots)], np.int64).tobytes() + lens.tobytes() + slots


def attribute_bytes(att, seg_ids):
    """bytes of an attribute container a decoder of the segments `seg_ids` reads: header + table + their slots in every channel"""
    N, D, S, _, _ = [int(x) for x in np.frombuffer(att, np.int64, 5, 8)]
    nseg = (N + S - 1) // S
    lens = np.frombuffer(att, np.uint32, nseg * D, 48).astype(np.int64).reshape(D, nseg)
    return 48 + 4 * nseg * D + int(((lens[:, list(seg_ids)] + 3) // 4 * 4).sum())
