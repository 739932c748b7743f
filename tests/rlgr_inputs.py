"""Seeded inputs of tests/test_rlgr.py's randomised RLGR cross-checks, shared with tests/golden/gen_golden.py, which records
the reference coder's streams for them in tests/golden/rlgr_random.npz as SHA-256 digests (inputs are digested too, so a
change of numpy's generators shows up as such and not as a coder mismatch)."""
import hashlib

import numpy as np


def laplace_stream():
    """30 000 Laplacian symbols, half of them zeroed (int64)."""
    rng = np.random.default_rng(77)
    x = rng.laplace(0, 40, 30000).astype(np.int64)
    x[rng.random(30000) < 0.5] = 0
    return x


def random_sequences():
    """300 int32 sequences of 0-2999 symbols: all-zero, sparse, dense, full int32 range, rare large values, wide normals."""
    rng = np.random.default_rng(7)
    xs = []
    for t in range(300):
        n = int(rng.integers(0, 3000))
        kind = t % 6
        if kind == 0:
            x = np.zeros(n, dtype=np.int32)
        elif kind == 1:
            x = np.round(rng.laplace(0, 0.05, n)).astype(np.int32)
        elif kind == 2:
            x = np.round(rng.laplace(0, 30, n)).astype(np.int32)
        elif kind == 3:
            x = rng.integers(-2 ** 31 + 1, 2 ** 31 - 1, n).astype(np.int32)
        elif kind == 4:
            x = np.zeros(n, dtype=np.int32)
            if n:
                x[rng.integers(0, n, max(1, n // 500))] = rng.integers(-2 ** 30, 2 ** 30, max(1, n // 500))
        else:
            x = np.round(rng.normal(0, 10 ** rng.uniform(-1, 6), n)).astype(np.int32)
        xs.append(x)
    return xs


INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def extreme_sequences():
    """The two limits of int32, which a saturated quantizer writes (include/raht.h) and the seeded draws above never hold:
    -> [(name, int32 array)], every sequence 200 symbols long (more than three segments of 64, ending inside one): runs of
    each limit of 1, 2, 63, 64 and 65 symbols starting at symbol 0 (so that they end before, on and behind a segment border of
    64), followed by small symbols; the two alternating; each isolated inside a long zero run; each as the first and as the
    last symbol."""
    n = 200
    small = (np.arange(n) % 7 - 3).astype(np.int32)
    out = []
    for tag, v in (("min", INT32_MIN), ("max", INT32_MAX)):
        for run in (1, 2, 63, 64, 65):
            x = small.copy()
            x[:run] = v
            out.append((f"run{run}_{tag}", x))
        x = np.zeros(n, dtype=np.int32)
        x[131] = v
        out.append((f"isolated_{tag}", x))
        x = np.zeros(n, dtype=np.int32)                          # (run1_*: first before small symbols; here: before a zero run)
        x[0] = v
        out.append((f"first_{tag}", x))
        x = small.copy()
        x[-1] = v
        out.append((f"last_{tag}", x))
    x = np.where(np.arange(n) % 2 == 0, INT32_MIN, INT32_MAX).astype(np.int32)
    out.append(("alternating", x))
    return out


def digest(a):
    """SHA-256 of an array's little-endian bytes, as 32 uint8."""
    a = np.ascontiguousarray(a)
    return np.frombuffer(hashlib.sha256(a.astype(a.dtype.newbyteorder("<")).tobytes()).digest(), dtype=np.uint8)
