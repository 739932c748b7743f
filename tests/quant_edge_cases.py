"""Shared case builder for the quantizer's out-of-range rule (include/raht.h; the model is tests/numpy_ops.quantize_model): plain
numpy, imported by the CPU tests (tests/test_quant_edges_model.py) and the GPU tests (tests/test_gpu_quant_edges.py), so that the
device, the host twins, the oracle and the torch helper are held to one list.

A case is a quotient target k and a step s: the coefficient is x = k * s, formed in the element type T, with its two neighbours
(``nextafter`` up and down), so that the quotient x / s lands on, just below and just above k. The targets sit where the
conversion to int32 changes its answer (+-(2^31 - 1), +-2^31, +-(2^31 + 1), the halves beside them), far beyond it (2^32, 2^40,
1e30, a quotient that overflows T), and in the zone [2^22, 2^25] where ``q + 0.5f`` rounds to even in float32. +-0, NaN, +-inf and
+-max(T) (whose quotient overflows for every step below 1) come as they are.

``case_matrix`` lays them into N x D by rotation, ``(7 * row + col) mod len``: every target then meets every column, i.e. every
lane of a 16-byte chunk, the ragged last chunk of a row and every step of a per-channel step vector. N = 4097 is the smallest size
with more than one stage-0 tile at the default tile height plus a ragged last tile."""
import math

import numpy as np

N = 4097
DS = (1, 3, 59, 70)                                                # below a chunk, the mixed split, the frame's rows, > one wave of chunks
DTYPES = {"f32": np.float32, "f64": np.float64}
# the steps of the issue: ordinary ones, the ends of the fast-divide range [2^-100, 2^100] (raht_device.h: fill_step_table) ...
STEPS_INSIDE = (1.0, 0.01, 3.0, 2.0 ** -20, 1e-6, 2.0 ** -100, 2.0 ** 100)
STEP_OUTSIDE = 1e-38                                               # ... and one outside it (float32: the plain-division branch runs)

_ZONE = (2 ** 22, 2 ** 22 + 1, 2 ** 23 - 1, 2 ** 23, 2 ** 23 + 1, 2 ** 23 + 2, 2 ** 23 + 3, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1,
         2 ** 24 + 2, 2 ** 24 + 6, 2 ** 25 - 2, 2 ** 25)
_EDGE = (2.0 ** 31 - 1, 2.0 ** 31, 2.0 ** 31 + 1, 2.0 ** 31 - 0.5, 2.0 ** 31 + 0.5, 2.0 ** 32, 2.0 ** 40, 1e30)
_FILL = (0.25, 7.5, -7.5, 1000.0)                                  # ordinary quotients, only to make the list's length coprime to 7


def step_vector(dt, D, outside=False):
    """(D,) steps of dtype ``dt``: the listed steps in turn over the columns (D = 1: the step 1 alone); ``outside``: with the
    step outside the fast-divide range among them, which sends every column of a float32 call to the plain division"""
    lst = STEPS_INSIDE + ((STEP_OUTSIDE,) if outside else ())
    if outside and D < len(lst):                                   # (narrow rows: the outside step first)
        lst = (STEP_OUTSIDE,) + STEPS_INSIDE
    return np.asarray([lst[c % len(lst)] for c in range(D)], dtype=DTYPES[dt] if isinstance(dt, str) else dt)


def targets():
    """the list of cases: (k, nudge) with nudge in (-1, 0, +1) ulps of the coefficient, or (special value, None)"""
    out = []
    for k in _EDGE + tuple(float(z) for z in _ZONE):
        for sgn in (1.0, -1.0):
            out += [(sgn * k, 0), (sgn * k, 1), (sgn * k, -1)]
    out += [(0.0, None), (-0.0, None), (float("nan"), None), (float("inf"), None), (float("-inf"), None), ("max", None), ("-max", None)]
    i = 0
    while math.gcd(len(out), 7) != 1:
        out.append((_FILL[i], 0))
        i += 1
    return out


def coefficients(dt, steps):
    """(len(targets()), len(steps)) coefficients of dtype ``dt``: row v holds target v for every step, x = k * s in ``dt``"""
    dt = np.dtype(DTYPES[dt] if isinstance(dt, str) else dt)
    s = np.atleast_1d(np.asarray(steps, dtype=dt))
    tg = targets()
    X = np.empty((len(tg), s.shape[0]), dtype=dt)
    up, dn = dt.type(np.inf), dt.type(-np.inf)
    with np.errstate(all="ignore"):
        for v, (k, nudge) in enumerate(tg):
            if nudge is None:
                X[v] = {"max": np.finfo(dt).max, "-max": -np.finfo(dt).max}.get(k, k)
                continue
            x = dt.type(k) * s
            X[v] = x if nudge == 0 else np.nextafter(x, up if nudge > 0 else dn)
    return X


def case_matrix(dt, steps, D, n=N):
    """(n, D) matrix of dtype ``dt`` for ``steps`` (a scalar or (D,)): element [r, c] is target (7 r + c) mod len at step[c]"""
    s = np.broadcast_to(np.atleast_1d(np.asarray(steps)), (D,))
    X = coefficients(dt, s)
    v = (7 * np.arange(n)[:, None] + np.arange(D)[None, :]) % X.shape[0]
    return np.ascontiguousarray(X[v, np.arange(D)[None, :]])


# ---- the mixed paths: a real tree, because a truncated plan sends its roots to root buffers instead of quantizing them ------------
MIXED_J, MIXED_D, MIXED_WIDE = 10, 59, 3
MIXED_HOT = (0, 1, 2, 3, 30, 58)                                   # the wide columns and three narrow ones (first, middle, last)
MIXED_HOT_STEP = 1e-7
MIXED_SCALARS = (1.0, 0.5, 0.25)                                   # the scalar steps of the multi-step entry, in units of the hot step


def mixed_frame():
    """-> (keys (N,) int64 sorted, C (N, 59) float32, steps (59,) float64). The hot columns hold normal * 1e6 at step 1e-7: an
    orthonormal transform of independent normals is independent normals, so nearly every quotient there is about +-1e13, beyond
    2^32 in both signs; |q| < 2^32 needs |T| < 430, which a normal of scale 1e6 meets with probability 3.4e-4. The other columns
    hold ordinary data for steps of that size, normal * 1e-5 at steps of 1e-7, 2e-7 and 3e-7 in turn (quotients of some hundreds),
    so that the multi-step entry, whose steps are scalars, has ordinary columns too. Its steps only go down from 1e-7: a hot
    element that is in range at a step is in range at every larger one, so no step adds such elements to those of 1e-7."""
    rng = np.random.default_rng(20261020)
    keys = np.unique(rng.integers(0, 2 ** (3 * MIXED_J), size=2 * N, dtype=np.int64))
    keys = np.sort(rng.permutation(keys)[:N])
    assert keys.shape[0] == N
    C = rng.normal(size=(N, MIXED_D))
    hot = np.isin(np.arange(MIXED_D), MIXED_HOT)
    C *= np.where(hot, 1e6, 1e-5)
    steps = np.where(hot, MIXED_HOT_STEP, (1 + np.arange(MIXED_D) % 3) * MIXED_HOT_STEP)
    return keys, C.astype(np.float32), steps


def mixed_classes(q):
    """the float64 model quotients of ``mixed_frame`` (any row order) -> (sat, skip): boolean (N, 59) masks of the elements that
    must be saturated (hot columns, |q| >= 2^32) and of those left out (hot columns, 2^30 <= |q| < 2^32, where the float32 and the
    float64 transform may fall on different sides of the range's end)"""
    hot = np.zeros(q.shape, dtype=bool)
    hot[:, list(MIXED_HOT)] = True
    a = np.abs(q)
    return hot & (a >= 2.0 ** 32), hot & (a >= 2.0 ** 30) & (a < 2.0 ** 32)


def identity_keys(n=N):
    """keys of the identity plan, for 24 bits and top_level = 1: all even, so no two rows share a parent below the truncation
    level, no butterfly runs (T == C) and the fused kernels quantize exactly the values placed"""
    return 2 * np.arange(n, dtype=np.int64)
