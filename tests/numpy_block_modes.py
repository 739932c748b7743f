"""Block modes of a B frame (include/raht.h, "Block modes") as a numpy model built on ``numpy_predict_bi.one``,
``numpy_motion.row_cost`` and ``numpy_motion.blocks``: the four predictions of a row, the cost table, the selection, the predictor
under a mode array, the "wipe" scene of the tests, and pure-host builders and parsers of the RAHTB002 wrapper."""
import numpy as np

from . import numpy_motion as M0
from . import numpy_predict_bi as B0

B2_MAGIC = b"RAHTB002"
N_MODES = 4


def predictions(keys, ref0, ref1, up=0, J=None, block_log2=0, mv0=None, mv1=None):
    """-> [P under mode 0, 1, 2, 3], each (N, D) float32: the two-reference rule, reference 0 alone (+0 where it has no run),
    reference 1 alone, +0"""
    m0, _ = B0.one(keys, ref0, up, J, block_log2, mv0)
    m1, _ = B0.one(keys, ref1, up, J, block_log2, mv1)
    P = B0.predict(keys, ref0, ref1, up, J, block_log2, mv0, mv1)[0]
    return [P, m0, m1, np.zeros_like(m0)]


def table(keys, ref0, ref1, X, J, block_log2, w, up=0, mv0=None, mv1=None):
    """-> (n_blocks, 4) int64: per block and mode the sum of ``numpy_motion.row_cost`` over the block's rows"""
    b, first = M0.blocks(keys, block_log2)
    T = np.zeros((len(first) - 1, N_MODES), np.int64)
    for k, P in enumerate(predictions(keys, ref0, ref1, up, J, block_log2, mv0, mv1)):
        np.add.at(T[:, k], b, M0.row_cost(X, P, w).astype(np.int64))
    return T


def select(T):
    """-> (mode (n_blocks,) uint8, best_cost (n_blocks,) int64); argmin: the first of the smallest"""
    mode = T.argmin(axis=1)
    return mode.astype(np.uint8), T[np.arange(len(T)), mode]


def search(keys, ref0, ref1, X, J, block_log2, w, up=0, mv0=None, mv1=None):
    """-> (table, mode, best_cost)"""
    T = table(keys, ref0, ref1, X, J, block_log2, w, up, mv0, mv1)
    return (T,) + select(T)


def predict(keys, ref0, ref1, modes, J, block_log2, up=0, mv0=None, mv1=None):
    """the prediction of every row under the mode of its block (a value above 3 predicts as 3) -> P (N, D) float32"""
    b, _ = M0.blocks(keys, block_log2)
    m = np.minimum(np.asarray(modes, np.int64), 3)[b]
    Ps = predictions(keys, ref0, ref1, up, J, block_log2, mv0, mv1)
    P = np.zeros_like(Ps[0])
    for k in range(N_MODES):
        P[m == k] = Ps[k][m == k]
    return P


def used_runs(keys, ref0, ref1, modes, J, block_log2, up=0, mv0=None, mv1=None):
    """-> the rows whose prediction uses a run of reference 0, of reference 1, of both"""
    b, _ = M0.blocks(keys, block_log2)
    m = np.asarray(modes, np.int64)[b]
    h0 = B0.one(keys, ref0, up, J, block_log2, mv0)[1] & ((m == 0) | (m == 1))
    h1 = B0.one(keys, ref1, up, J, block_log2, mv1)[1] & ((m == 0) | (m == 2))
    return int(h0.sum()), int(h1.sum()), int((h0 & h1).sum())


apply = B0.apply


# ---- the wipe: two anchors that disagree, a frame that follows one left of a cut and the other right of it ------------------------
def wipe(V, A, cut=32, seed=5, step=0.01):
    """-> (A0, A1, X, left): anchor 0 carries ``A``, anchor 1 a row permutation of ``A`` on the same voxels (the rows rotated by
    half their number: no row keeps its place, where the two anchors would agree and the choice be open), both perturbed by half
    a step; the frame between them takes ``A`` where x < cut (``left``) and the permutation elsewhere, plus 1e-3 noise"""
    rng = np.random.default_rng(seed)
    A = np.asarray(A, np.float32)
    Ap = np.roll(A, len(A) // 2, axis=0)
    left = np.asarray(V)[:, 0] < cut
    X = (np.where(left[:, None], A, Ap) + 1e-3 * rng.standard_normal(A.shape)).astype(np.float32)
    A0 = (A + 0.5 * step * rng.uniform(-1, 1, A.shape)).astype(np.float32)
    A1 = (Ap + 0.5 * step * rng.uniform(-1, 1, A.shape)).astype(np.float32)
    return A0, A1, X, left


def wipe_modes(keys, left, block_log2):
    """the pattern a wipe must choose: mode 1 in every block whose voxels lie left of the cut, mode 2 elsewhere; a block is on one
    side when the cut is a multiple of the block's width (asserted)"""
    b, first = M0.blocks(keys, block_log2)
    side = left[first[:-1]]
    assert np.array_equal(side[b], left)
    return np.where(side, 1, 2).astype(np.uint8)


# ---- containers (host bytes only) ----------------------------------------------------------------------------------------------
def bframe2(inner, modes, ref_back=1, ref_fwd=1, up=0, block_log2=1, mv0=None, mv1=None, n_blocks=None, pad=None, flags=None):
    """the wrapper; n_blocks / pad / flags: to announce another count, to write other padding bytes behind each field and behind
    the modes, to write another flag word"""
    modes = np.asarray(modes, np.uint8).reshape(-1)
    body = b""
    if mv0 is not None:
        for mv in (mv0, mv1):
            f = np.asarray(mv, np.int8).reshape(-1, 3).tobytes()
            body += f + (bytes(-len(f) % 8) if pad is None else bytes(pad))
    body += modes.tobytes() + (bytes(-len(modes) % 8) if pad is None else bytes(pad))
    n = len(modes) if n_blocks is None else n_blocks
    fl = int(mv0 is not None) if flags is None else flags
    return B2_MAGIC + np.array([ref_back, ref_fwd, up, block_log2, n, fl], np.int64).tobytes() + body + bytes(inner)


def parse_bframe2(fb):
    """-> (ref_back, ref_fwd, up, block_log2, mv0, mv1, modes, inner bytes); no checks beyond the magic"""
    fb = bytes(fb)
    assert fb[:8] == B2_MAGIC
    ref_back, ref_fwd, up, m, n, fl = (int(x) for x in np.frombuffer(fb, np.int64, 6, 8))
    pos, mv0, mv1 = 56, None, None
    if fl & 1:
        w = (3 * n + 7) // 8 * 8
        mv0 = np.frombuffer(fb, np.int8, 3 * n, pos).reshape(n, 3)
        mv1 = np.frombuffer(fb, np.int8, 3 * n, pos + w).reshape(n, 3)
        pos += 2 * w
    modes = np.frombuffer(fb, np.uint8, n, pos)
    return ref_back, ref_fwd, up, m, mv0, mv1, modes, fb[pos + (n + 7) // 8 * 8:]


def kinds(seq):
    n = int(np.frombuffer(seq, np.int64, 1, 8)[0])
    off = np.frombuffer(seq, np.int64, n + 1, 16)
    name = {B0.P0.P_MAGIC: "P", M0.M_MAGIC: "P", B0.B_MAGIC: "B", B2_MAGIC: "B"}
    return [name.get(bytes(seq[int(o): int(o) + 8]), "I") for o in off[:-1]]
