"""Motion compensation (include/raht.h, "Motion compensation") as a numpy model built on ``numpy_predict.predict``:
shifted keys, the cost table, the selection, the compensated predictor, and pure-host builders and parsers of the compensated-frame
wrapper. The arithmetic of a cost is np.float32 in the order of the definition: per weighted column, ascending, t = X - P, |t|,
w t (rounded), c + t (rounded); then the cap with ``np.fmin`` (a NaN takes the cap) and 2^-10 fixed point."""
import numpy as np

from . import numpy_predict as P0

M_MAGIC = b"RAHTM001"
CAP = np.float32(1048576.0)


def demorton(keys, J):
    """-> (N, 3) int64 (x, y, z): digit = z + 2 y + 4 x, the finest digit in bits 0-2"""
    k = np.asarray(keys, np.uint64)
    V = np.zeros((len(k), 3), np.int64)
    for b in range(J):
        d = (k >> np.uint64(3 * b)) & np.uint64(7)
        V[:, 0] |= (((d >> np.uint64(2)) & np.uint64(1)).astype(np.int64)) << b
        V[:, 1] |= (((d >> np.uint64(1)) & np.uint64(1)).astype(np.int64)) << b
        V[:, 2] |= ((d & np.uint64(1)).astype(np.int64)) << b
    return V


def morton(V, J):
    V = np.asarray(V, np.int64)
    k = np.zeros(len(V), np.uint64)
    for b in range(J):
        for a, s in ((0, 2), (1, 1), (2, 0)):
            k |= (((V[:, a] >> b) & 1).astype(np.uint64)) << np.uint64(3 * b + s)
    return k


def blocks(keys, block_log2):
    """-> (block index of every row, block_first (n_blocks + 1,) int64)"""
    cell = np.asarray(keys, np.uint64) >> np.uint64(3 * block_log2)
    first = np.flatnonzero(np.concatenate([[True], cell[1:] != cell[:-1]]))
    return np.cumsum(np.concatenate([[0], (cell[1:] != cell[:-1]).astype(np.int64)])), np.concatenate([first, [len(cell)]]).astype(np.int64)


def shifted(keys, J, v):
    """v: (3,) or (N, 3) integers -> (ok (N,) bool, shifted keys (N,) uint64: 0 where not ok)"""
    W = demorton(keys, J) + np.asarray(v, np.int64)
    ok = np.all((W >= 0) & (W < (1 << J)), axis=1)
    return ok, morton(np.where(ok[:, None], W, 0), J)


def predict_v(keys, ref_keys, C_ref, J, v, up=0):
    """P_v: ``numpy_predict.predict`` for the shifted keys (they need not be sorted), 0 for a row that leaves the cube
    -> (P, n_matched)"""
    ok, k2 = shifted(keys, J, v)
    P = np.zeros((len(k2), np.asarray(C_ref).shape[1]), np.float32)
    n = 0
    if ok.any():
        lo, hi = P0.runs(k2[ok], ref_keys, up)
        P[ok], _ = P0.predict(k2[ok], ref_keys, C_ref, up)
        n = int((hi > lo).sum())
    return P, n


def predict_mc(keys, ref_keys, C_ref, J, block_log2, mv, up=0):
    """row i under the vector of its block -> (P, n_matched)"""
    b, _ = blocks(keys, block_log2)
    return predict_v(keys, ref_keys, C_ref, J, np.asarray(mv, np.int64)[b], up)


def candidates(radius):
    r = range(-radius, radius + 1)
    return np.array(sorted(((x, y, z) for x in r for y in r for z in r), key=lambda v: (v[0] ** 2 + v[1] ** 2 + v[2] ** 2,) + v), np.int32)


def row_cost(X, P, w):
    """-> q (N,) uint64"""
    X, w = np.asarray(X, np.float32), np.asarray(w, np.float32)
    c = np.zeros(len(X), np.float32)
    with np.errstate(all="ignore"):
        for ch in range(X.shape[1]):
            if w[ch] != 0:
                t = X[:, ch] - P[:, ch]
                t = np.abs(t)
                t = w[ch] * t
                c = c + t
        assert c.dtype == np.float32
        return np.floor(np.fmin(c, CAP) * np.float32(1024.0)).astype(np.uint64)


def search(keys, ref_keys, C_ref, X, J, block_log2, cand, w, up=0):
    """-> (table (n_blocks, K) int64, best_k (n_blocks,) int32, best_cost (n_blocks,) int64)"""
    b, first = blocks(keys, block_log2)
    table = np.zeros((len(first) - 1, len(cand)), np.int64)
    for k, v in enumerate(np.asarray(cand, np.int64)):
        q = row_cost(X, predict_v(keys, ref_keys, C_ref, J, v, up)[0], w)
        np.add.at(table[:, k], b, q.astype(np.int64))
    best_k = table.argmin(axis=1).astype(np.int32)                       # (argmin: the first of the smallest)
    return table, best_k, table[np.arange(len(table)), best_k]


# ---- containers (host bytes only) ----------------------------------------------------------------------------------------------
def mframe(inner, ref_back=1, up=0, block_log2=1, mv=((0, 0, 0),), n_blocks=None, pad=None):
    """the wrapper; n_blocks / pad: to announce another count, to write other padding bytes"""
    field = np.asarray(mv, np.int8).reshape(-1, 3).tobytes()
    n = len(field) // 3 if n_blocks is None else n_blocks
    padding = bytes(-len(field) % 8) if pad is None else bytes(pad)
    return M_MAGIC + np.array([ref_back, up, block_log2, n], np.int64).tobytes() + field + padding + bytes(inner)


def parse_mframe(fb):
    """-> (ref_back, up, block_log2, mv, inner bytes); no checks beyond the magic"""
    fb = bytes(fb)
    assert fb[:8] == M_MAGIC
    ref_back, up, m, n = (int(x) for x in np.frombuffer(fb, np.int64, 4, 8))
    mv = np.frombuffer(fb, np.int8, 3 * n, 40).reshape(n, 3)
    return ref_back, up, m, mv, fb[40 + (3 * n + 7) // 8 * 8:]
