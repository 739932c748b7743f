"""The inter-frame predictor (include/raht.h, "Inter-frame prediction") as a numpy model, and pure-host builders and
parsers of the predicted-frame wrapper. All arithmetic is np.float32, sequential over the position in a run -- at most 8^up <= 512
vectorised steps -- because that order is the definition."""
import numpy as np

P_MAGIC = b"RAHTP001"
SEQ_MAGIC = b"RAHTS001"
FRAME_MAGIC = b"RAHTF001"


def runs(keys, ref_keys, up):
    """-> (lo, hi): row i's run in the reference is [lo[i], hi[i]), every r with ref_keys[r] >> 3 up == keys[i] >> 3 up"""
    sh = np.uint64(3 * int(up))
    c, rc = np.asarray(keys, np.uint64) >> sh, np.asarray(ref_keys, np.uint64) >> sh
    return np.searchsorted(rc, c, "left"), np.searchsorted(rc, c, "right")


def predict(keys, ref_keys, C_ref, up=0):
    """-> (P (N, D) float32, n_matched)"""
    C_ref = np.asarray(C_ref, np.float32)
    lo, hi = runs(keys, ref_keys, up)
    n = hi - lo
    hit = n > 0
    P = np.zeros((len(lo), C_ref.shape[1]), np.float32)
    if hit.any():
        l, m = lo[hit], n[hit]
        s = C_ref[l].copy()                                              # s = C'[lo]
        for t in range(1, int(m.max())):                                 # s = s + C'[lo + t], in this order
            w = m > t
            s[w] = s[w] + C_ref[l[w] + t]
        P[hit] = s / m.astype(np.float32)[:, None]                       # one float32 division (by 1.0: exact)
    assert P.dtype == np.float32
    return P, int(hit.sum())


def apply(X, P, add=False):
    """R = X - P, or C_rec = X + P: one float32 operation per element"""
    X = np.asarray(X, np.float32)
    out = X + P if add else X - P
    assert out.dtype == np.float32
    return out


# ---- containers (host bytes only) ----------------------------------------------------------------------------------------------
def pframe(inner, ref_back=1, up=0):
    return P_MAGIC + np.array([ref_back, up], np.int64).tobytes() + bytes(inner)


def parse_pframe(fb):
    """-> (ref_back, up, inner bytes); no checks beyond the magic"""
    fb = bytes(fb)
    assert fb[:8] == P_MAGIC
    ref_back, up = (int(x) for x in np.frombuffer(fb, np.int64, 2, 8))
    return ref_back, up, fb[24:]


def sequence(frame_blobs):
    blobs = [bytes(b) for b in frame_blobs]
    head = 8 + 8 * (len(blobs) + 2)
    off = head + np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.int64)
    return SEQ_MAGIC + np.array([len(blobs)], np.int64).tobytes() + off.tobytes() + b"".join(blobs)


def kinds(seq):
    n = int(np.frombuffer(seq, np.int64, 1, 8)[0])
    off = np.frombuffer(seq, np.int64, n + 1, 16)
    return ["P" if bytes(seq[int(o): int(o) + 8]) == P_MAGIC else "I" for o in off[:-1]]


def tiny_frame(J=2, D=3, step=0.25):
    """a hand-laid RAHTF001 frame of one voxel that ``bitstream.parse_frame`` accepts (250 bytes; nothing in it is decodable data)"""
    N = 1
    geo = b"OCTG0001" + np.array([J, N, 0, J, 2048], np.int64).tobytes() + np.ones(J + 1, np.int64).tobytes() + bytes([1] * J)
    att = b"RLGS0001" + np.array([N, D, 2048, 1, 4 * D], np.int64).tobytes() + np.ones(D, np.uint32).tobytes() + bytes(4 * D)
    return (FRAME_MAGIC + np.array([J, N, D, 0, 1], np.int64).tobytes() + np.array([step, 0.0, 0.0, 0.0, 0.0], np.float64).tobytes()
            + np.array([len(geo)], np.int64).tobytes() + geo + np.array([len(att)], np.int64).tobytes() + att)
