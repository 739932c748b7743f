"""numpy model of the predicted octree geometry (include/raht.h, "Predicted octree geometry"): the reference frame's occupancy of
a frame's cells (``pred``), the residual stream ``occ ^ pred``, the ``OCTP0001`` section byte for byte, and its decoder. The
entropy-coded body takes the host RLGR coder as a function argument, as tests/numpy_octree.py does; ``pred_brute_force`` is the
definition itself."""
import numpy as np

from . import numpy_octree as M

MAGIC = b"OCTP0001"


def level_nodes(keys, J):
    """sorted unique uint64 keys -> the ascending cell keys of every level 0 .. J - 1"""
    keys = keys.astype(np.uint64)
    return [np.unique(keys >> np.uint64(3 * (J - g))) for g in range(J)]


def pred_of_nodes(nodes, g, ref, J):
    """the reference's occupancy byte of the cells ``nodes`` (ascending cell keys of level g)"""
    child = np.unique(ref.astype(np.uint64) >> np.uint64(3 * (J - g) - 3))          # the reference's cells one level deeper
    parent, bit = child >> np.uint64(3), (1 << (child & np.uint64(7)).astype(np.int64)).astype(np.uint8)
    cells, first = np.unique(parent, return_index=True)
    byte = np.bitwise_or.reduceat(bit, first)
    at = np.searchsorted(cells, nodes)
    hit = (at < len(cells)) & (cells[np.minimum(at, len(cells) - 1)] == nodes)
    return np.where(hit, byte[np.minimum(at, len(cells) - 1)], 0).astype(np.uint8)


def pred_levels(keys, ref, J):
    return [pred_of_nodes(n, g, ref, J) for g, n in enumerate(level_nodes(keys, J))]


def pred_brute_force(keys, ref, J):
    """bit d of pred[v] <=> some r has r >> (s - 3) == 8 c + d, s = 3 (J - g), v the node of level g with cell key c"""
    keys, ref = [int(k) for k in keys], [int(r) for r in ref]
    out = []
    for g in range(J):
        s = 3 * (J - g)
        out.append(np.array([sum(1 << d for d in range(8) if any(r >> (s - 3) == 8 * c + d for r in ref))
                             for c in sorted({k >> s for k in keys})], np.uint8))
    return out


def res_stream(keys, ref, J):
    """-> (counts n_0 .. n_J, the residual stream)"""
    counts, occ = M.occ_stream(keys, J)
    return counts, occ ^ np.concatenate(pred_levels(keys, ref, J))


def res_decode(res, counts, ref, J):
    """the decoder: level by level pred of the node keys, occ = res ^ pred, expansion -> keys (ValueError for a stream that does
    not go with the counts)"""
    cur, off = np.zeros(1, np.uint64), 0
    for g in range(J):
        occ = res[off: off + counts[g]] ^ pred_of_nodes(cur, g, ref, J)
        if not occ.all():
            raise ValueError("a reconstructed occupancy byte is 0")
        rows, dig = np.nonzero(np.unpackbits(occ[:, None], axis=1, bitorder="little"))
        cur = (cur[rows] << np.uint64(3)) | dig.astype(np.uint64)
        if len(cur) != counts[g + 1]:
            raise ValueError("the popcounts of a level do not add up to the next count")
        off += counts[g]
    return cur


def section(keys, ref, J, mode, seg_len=0, rlgr_encode=None):
    counts, res = res_stream(keys, ref, J)
    n_nodes = len(res)
    table = M.rank_table(res)
    n_used = len(np.unique(res)) if mode else 0
    hdr = MAGIC + np.array([J, len(keys), mode, n_nodes, seg_len if mode else 0, len(ref), n_used] + counts, np.int64).tobytes()
    if mode == 0:
        return hdr + res.tobytes()
    rank_of = np.zeros(256, np.int32)
    rank_of[table] = np.arange(256, dtype=np.int32)
    sym = rank_of[res]
    segs = [np.asarray(rlgr_encode(sym[a: a + seg_len]), np.uint8) for a in range(0, n_nodes, seg_len)]
    lens = np.array([len(s) for s in segs], np.uint32)
    return hdr + table.tobytes() + lens.tobytes() + b"".join(s.tobytes() + b"\0" * (-len(s) % 4) for s in segs)


def header_bytes(J):
    return len(MAGIC) + 8 * 7 + 8 * (J + 1)
