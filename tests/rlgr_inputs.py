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


def digest(a):
    """SHA-256 of an array's little-endian bytes, as 32 uint8."""
    a = np.ascontiguousarray(a)
    return np.frombuffer(hashlib.sha256(a.astype(a.dtype.newbyteorder("<")).tobytes()).digest(), dtype=np.uint8)
