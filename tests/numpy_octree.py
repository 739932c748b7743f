"""numpy model of the octree geometry coder (include/raht.h, "Octree geometry"): occupancy stream, rank table, geometry section
and frame container, byte for byte what the GPU path must produce. The entropy-coded body takes the host RLGR coder as a
function argument (``rlgr_encode(symbols int32 array) -> uint8 array``, unsigned), so the model itself is plain numpy."""
import numpy as np

GEOMETRY_MAGIC = b"OCTG0001"
FRAME_MAGIC = b"RAHTF001"


def occ_encode(keys, J):
    """sorted unique uint64 keys -> (counts n_0..n_J, occupancy bytes per level, coarse -> fine)"""
    cur, levels, counts = keys.astype(np.uint64), [], [len(keys)]
    for _ in range(J):
        parent, digit = cur >> np.uint64(3), (cur & np.uint64(7)).astype(np.uint8)
        head = np.ones(len(cur), bool)
        head[1:] = parent[1:] != parent[:-1]
        occ = np.zeros(int(head.sum()), np.uint8)
        np.bitwise_or.at(occ, np.cumsum(head) - 1, (1 << digit).astype(np.uint8))
        levels.append(occ)
        cur = parent[head]
        counts.append(len(cur))
    return counts[::-1], levels[::-1]


def occ_decode(levels, J):
    cur = np.zeros(1, np.uint64)
    for g in range(J):
        rows, dig = np.nonzero(np.unpackbits(levels[g][:, None], axis=1, bitorder="little"))
        cur = (cur[rows] << np.uint64(3)) | dig.astype(np.uint64)
    return cur


def occ_brute_force(keys, J):
    """the definition itself: a node of level g is a distinct prefix key >> 3 (J - g); bit d of its byte <=> prefix * 8 + d exists"""
    keys = [int(k) for k in keys]
    nodes = [sorted({k >> (3 * (J - g)) for k in keys}) for g in range(J + 1)]
    levels = []
    for g in range(J):
        below = set(nodes[g + 1])
        levels.append(np.array([sum(1 << d for d in range(8) if p * 8 + d in below) for p in nodes[g]], np.uint8))
    return [len(n) for n in nodes], levels


def occ_stream(keys, J):
    counts, levels = occ_encode(keys, J)
    return counts, np.concatenate(levels)


def rank_table(stream):
    """byte_of_rank (256,) uint8: descending count over the whole stream, ties by ascending byte value"""
    cnt = np.bincount(stream, minlength=256)
    return np.array(sorted(range(256), key=lambda b: (-int(cnt[b]), b)), np.uint8)


def geometry_section(keys, J, mode, seg_len=0, rlgr_encode=None):
    counts, stream = occ_stream(keys, J)
    n_nodes = len(stream)
    hdr = GEOMETRY_MAGIC + np.array([J, len(keys), mode, n_nodes, seg_len if mode else 0] + counts, np.int64).tobytes()
    if mode == 0:
        return hdr + stream.tobytes()
    table = rank_table(stream)
    rank_of = np.zeros(256, np.int32)
    rank_of[table] = np.arange(256, dtype=np.int32)
    sym = rank_of[stream]
    segs = [np.asarray(rlgr_encode(sym[a: a + seg_len]), np.uint8) for a in range(0, n_nodes, seg_len)]
    lens = np.array([len(s) for s in segs], np.uint32)
    slots = b"".join(s.tobytes() + b"\0" * (-len(s) % 4) for s in segs)
    return hdr + table.tobytes() + lens.tobytes() + slots


def frame_container(J, N, D, n_wide, steps, geometry, attributes, vmin=(0.0, 0.0, 0.0), width=0.0):
    return (FRAME_MAGIC + np.array([J, N, D, n_wide, len(steps)], np.int64).tobytes()
            + np.array(list(steps) + list(vmin) + [width], np.float64).tobytes()
            + np.array([len(geometry)], np.int64).tobytes() + geometry + np.array([len(attributes)], np.int64).tobytes() + attributes)
