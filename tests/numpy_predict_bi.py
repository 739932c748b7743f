"""The two-reference predictor of a B frame (include/raht.h, "Two references") as a numpy model built on
``numpy_predict.predict`` / ``runs`` and ``numpy_motion.predict_v``, and pure-host builders and parsers of the B-frame wrapper. The
two means are the one-reference model's; where both references have a run the prediction is 0.5 * (m0 + m1) in np.float32, the
sum rounded before the product."""
import numpy as np

from . import numpy_motion as M0
from . import numpy_predict as P0

B_MAGIC = b"RAHTB001"


def one(keys, ref, up=0, J=None, block_log2=0, mv=None):
    """the one-reference model of a row against ``ref`` = (ref_keys, C_ref), under the field ``mv`` over the frame's blocks when
    given -> (m (N, D) float32, has_run (N,) bool)"""
    ref_keys, C_ref = ref
    if mv is None:
        lo, hi = P0.runs(keys, ref_keys, up)
        return P0.predict(keys, ref_keys, C_ref, up)[0], hi > lo
    b, _ = M0.blocks(keys, block_log2)
    ok, k2 = M0.shifted(keys, J, np.asarray(mv, np.int64)[b])
    lo, hi = P0.runs(k2, ref_keys, up)
    return M0.predict_mc(keys, ref_keys, C_ref, J, block_log2, mv, up)[0], ok & (hi > lo)


def predict(keys, ref0, ref1, up=0, J=None, block_log2=0, mv0=None, mv1=None):
    """-> (P (N, D) float32, n_matched: the rows with a run in reference 0, in reference 1, in both, hit0, hit1)"""
    m0, h0 = one(keys, ref0, up, J, block_log2, mv0)
    m1, h1 = one(keys, ref1, up, J, block_log2, mv1)
    with np.errstate(over="ignore"):
        s = m0 + m1                                                      # rounded ...
        assert s.dtype == np.float32
        avg = np.float32(0.5) * s                                        # ... before the product
    P = np.where((h0 & h1)[:, None], avg, np.where(h0[:, None], m0, m1))     # (m1 is +0 where reference 1 has no run either)
    assert P.dtype == np.float32
    return P, (int(h0.sum()), int(h1.sum()), int((h0 & h1).sum())), h0, h1


apply = P0.apply


# ---- containers (host bytes only) ----------------------------------------------------------------------------------------------
def bframe(inner, ref_back=1, ref_fwd=1, up=0, block_log2=0, mv0=None, mv1=None, n_blocks=None, pad=None):
    """the wrapper; n_blocks / pad: to announce another count, to write other padding bytes behind each field"""
    fields, n = b"", 0
    if mv0 is not None:
        for mv in (mv0, mv1):
            f = np.asarray(mv, np.int8).reshape(-1, 3).tobytes()
            n = len(f) // 3
            fields += f + (bytes(-len(f) % 8) if pad is None else bytes(pad))
    n = n if n_blocks is None else n_blocks
    return B_MAGIC + np.array([ref_back, ref_fwd, up, block_log2, n], np.int64).tobytes() + fields + bytes(inner)


def parse_bframe(fb):
    """-> (ref_back, ref_fwd, up, block_log2, mv0, mv1, inner bytes); no checks beyond the magic"""
    fb = bytes(fb)
    assert fb[:8] == B_MAGIC
    ref_back, ref_fwd, up, m, n = (int(x) for x in np.frombuffer(fb, np.int64, 5, 8))
    if m == 0:
        return ref_back, ref_fwd, up, 0, None, None, fb[48:]
    w = (3 * n + 7) // 8 * 8
    mv0 = np.frombuffer(fb, np.int8, 3 * n, 48).reshape(n, 3)
    mv1 = np.frombuffer(fb, np.int8, 3 * n, 48 + w).reshape(n, 3)
    return ref_back, ref_fwd, up, m, mv0, mv1, fb[48 + 2 * w:]


def kinds(seq):
    n = int(np.frombuffer(seq, np.int64, 1, 8)[0])
    off = np.frombuffer(seq, np.int64, n + 1, 16)
    name = {P0.P_MAGIC: "P", M0.M_MAGIC: "P", B_MAGIC: "B"}
    return [name.get(bytes(seq[int(o): int(o) + 8]), "I") for o in off[:-1]]
