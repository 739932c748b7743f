"""Shared case table for plan construction from coordinates (raht_plan_create, its CPU twin raht_cpu_plan_create and
RahtPlan.from_coords): plain numpy, imported by the CPU tests, the GPU tests and tests/golden/gen_golden.py, so that the
device, the twin and the fixtures from the reference are held to one list.

The model is the arithmetic of the reference's RAHT_param (python/RAHT_param.py:21-24): ``minV`` is promoted to float64
there, so float32 and integer ``V`` are promoted too, and ``Vint = floor((V - minV) / (width / 2^depth))`` is float64
arithmetic whatever the element type of ``V``. A row is out of bounds when an axis is not in [0, 2^depth) -- NaN included
(RAHT_param.py:26-27: a NaN converts to INT64_MIN on the CPU and fails the check).

Every cloud is built from seeded candidates: rows the model refuses are dropped, the first point of every voxel is kept,
the rest is sorted by Morton key. What ``floor`` makes of a border point is whatever the model says; the point of the
border cases is that the device's subtract, divide and floor agree with IEEE double at the voxel faces."""
import numpy as np

RAHT_ERR_BOUNDS = -3
DTYPES = {"f32": np.float32, "f64": np.float64, "i32": np.int32, "i64": np.int64}
RAHT_DTYPE = {"f32": 0, "f64": 1, "i32": 2, "i64": 3}              # enum raht_dtype (include/raht.h)
ALL = ("f32", "f64", "i32", "i64")
_I64_LO, _I64_HI = -2.0 ** 63, 2.0 ** 63 - 1024.0                  # the float64 values every int64 can hold


def morton(q, J):
    """(N, 3) int64 voxel indices in [0, 2^J) -> uint64 keys: digit_k = z_k + 2 y_k + 4 x_k at bits [3k, 3k + 2] (x highest)"""
    q = np.asarray(q, dtype=np.int64).astype(np.uint64)
    k = np.zeros(q.shape[0], dtype=np.uint64)
    one = np.uint64(1)
    for i in range(J):
        s = np.uint64(i)
        k |= (((q[:, 2] >> s) & one) | (((q[:, 1] >> s) & one) << one) | (((q[:, 0] >> s) & one) << np.uint64(2))) << np.uint64(3 * i)
    return k


def model_keys(V, minV, width, J):
    """-> (q, bad, key). q: (N, 3) int64, floor((V.astype(float64) - minV) / (width / 2^J)) per axis; bad: (N,) bool, the row has
    an axis with ``not (0 <= q < 2^J)`` (NaN counts as out); key: (N,) uint64 Morton keys of the rows that are in bounds (0 for
    the others). float64 arithmetic for every element type of V: RAHT_param.py:21-24 promotes minV, and with it V, to float64.
    (q of a value no int64 holds is clipped to the int64 range, NaN to INT64_MIN: only ``bad`` speaks for such rows.)"""
    Vd = np.asarray(V).astype(np.float64).reshape(-1, 3)
    m = np.asarray(minV, dtype=np.float64).reshape(1, 3)
    Q = np.float64(width) / np.float64(2 ** J)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((Vd - m) / Q)
        ok = (f >= 0) & (f < np.float64(2 ** J))                   # False for NaN
        q = np.where(np.isnan(f), _I64_LO, np.clip(f, _I64_LO, _I64_HI)).astype(np.int64)
    bad = ~ok.all(axis=1)
    key = np.where(bad, np.uint64(0), morton(np.where(ok, q, 0), J))
    return q, bad, key


def sort_unique(cand, minV, width, J, n=None, rng=None, keep=()):
    """candidates (already of the dtype they are fed in) -> the rows the model accepts, first point per voxel, Morton-sorted;
    with ``n``: a seeded choice of exactly n of them (the candidate rows ``keep`` always among them)"""
    _, bad, key = model_keys(cand, minV, width, J)
    idx = np.flatnonzero(~bad)
    _, first = np.unique(key[idx], return_index=True)              # np.unique: sorted keys, index of each one's first row
    idx = idx[first]
    if n is not None:
        assert idx.size >= n, (idx.size, n)
        must = np.flatnonzero(np.isin(idx, np.asarray(keep, dtype=np.int64)))
        rest = np.setdiff1d(np.arange(idx.size), must)
        pick = np.concatenate([must, rng.permutation(rest)[: n - must.size]])
        idx = idx[np.sort(pick)]
    return np.ascontiguousarray(cand[idx])


class Case:
    """One cloud: ``V`` in the dtype it was built in (``cast(dt)`` gives it as another listed dtype: the values are exact there),
    origin, width, depth and the element types it runs in. ``fixture``: (name of the reference fixture under tests/golden/coords/,
    the dtype V was fed to the reference in), if there is one."""

    def __init__(self, name, V, minV, width, J, dtypes, fixture=None):
        self.name, self.V, self.minV, self.width, self.J, self.dtypes, self.fixture = name, V, tuple(float(x) for x in minV), float(width), int(J), tuple(dtypes), fixture
        for dt in self.dtypes:                                     # a listed dtype holds every value exactly
            assert np.array_equal(self.cast(dt).astype(np.float64), self.V.astype(np.float64)), (name, dt)
        _, bad, key = self.model()
        assert not bad.any() and (key.size == 1 or np.all(key[1:] > key[:-1])), name

    def cast(self, dt):
        return np.ascontiguousarray(self.V.astype(DTYPES[dt]))

    def model(self):
        return model_keys(self.V, self.minV, self.width, self.J)

    def __repr__(self):
        return self.name


# ---- accepted clouds ------------------------------------------------------------------------------------------------------
SHIFT_MINV = (-37.0, 1000.5, 0.25)            # an origin with a negative and two fractional entries; Q = 1 at width = 2^J


def _shifted_ints(rng, n_cand, J, minV=SHIFT_MINV):
    """integer coordinates whose voxel index under ``minV`` (Q = 1) is uniform in [0, 2^J): ceil(minV) + index"""
    return (np.ceil(np.asarray(minV)).astype(np.int64)[None, :] + rng.integers(0, 2 ** J, size=(n_cand, 3))).astype(np.int64)


def _border_candidates(rng, minV, width, J, n_rand):
    """minV + k Q computed in float64, and one float64 step below and above it, for k in {0, 1, 2^J - 1} on every axis in turn
    (the other axes strictly inside a voxel) and for random k on all three axes at once"""
    m = np.asarray(minV, dtype=np.float64)
    Q = np.float64(width) / np.float64(2 ** J)
    rows = []
    for a in range(3):
        for k in (0, 1, 2 ** J - 1):
            for step in (0, -1, 1):
                r = m + (rng.integers(0, 2 ** J, size=3) + rng.uniform(0.2, 0.8, size=3)) * Q
                b = m[a] + k * Q
                r[a] = b if step == 0 else np.nextafter(b, -np.inf if step < 0 else np.inf)
                rows.append(r)
    k = rng.integers(0, 2 ** J, size=(n_rand, 3))
    b = m[None, :] + k * Q
    step = rng.integers(-1, 2, size=(n_rand, 3))
    b = np.where(step == 0, b, np.nextafter(b, np.where(step < 0, -np.inf, np.inf)))
    return np.concatenate([np.array(rows), b], axis=0)


def _f32_twin(cand):
    """the candidates rounded to float32, and one FLOAT32 step below and above that"""
    c = cand.astype(np.float32)
    return np.concatenate([c, np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))])


def _accepted():
    rng = np.random.default_rng(20261020)
    out = []
    # integer coordinates under a shifted origin, every size around the kernel's 256 threads per block, in all four dtypes
    for n in (1, 255, 256, 257, 1025):
        V = sort_unique(_shifted_ints(rng, 3 * n + 8, 10), SHIFT_MINV, 1024.0, 10, n=n, rng=rng)
        out.append(Case(f"shift_int_n{n}", V, SHIFT_MINV, 1024.0, 10, ALL, fixture={1025: ("shift_int_n1025", "f64"), 257: ("shift_int_n257_f32", "f32")}.get(n)))
    # every voxel of depth 1
    V = sort_unique(_shifted_ints(rng, 200, 1), SHIFT_MINV, 2.0, 1)
    assert V.shape[0] == 8
    out.append(Case("j1_all8", V, SHIFT_MINV, 2.0, 1, ALL))
    # real-valued points, widths that are no power of two; the float32 twin rounds the CANDIDATES to float32 first: the float32
    # value is the input, and what the model makes of it in float64 is the answer
    for name, minV, width, J, n_cand in (("w3_j10", (-1.5, 0.1, 7.0), 3.0, 10, 1500), ("w1e-3_j12", (1000.0, 999.5, 1000.25), 1e-3, 12, 1500)):
        cand = np.asarray(minV)[None, :] + rng.uniform(0.0, 1.0, size=(n_cand, 3)) * width
        out.append(Case(name + "_f64", sort_unique(cand, minV, width, J), minV, width, J, ("f64",), fixture=(name + "_f64", "f64")))
        out.append(Case(name + "_f32", sort_unique(cand.astype(np.float32), minV, width, J), minV, width, J, ("f32", "f64")))
        bc = _border_candidates(rng, minV, width, J, 600)
        out.append(Case(name + "_border_f64", sort_unique(bc, minV, width, J), minV, width, J, ("f64",), fixture=(name + "_border_f64", "f64")))
        out.append(Case(name + "_border_f32", sort_unique(_f32_twin(bc), minV, width, J), minV, width, J, ("f32", "f64")))
    # border points at Q = 1 under the shifted origin: exact in float32 as well (halves and quarters of small numbers), so the
    # float32 twin is the same cloud
    bc = _border_candidates(rng, SHIFT_MINV, 1024.0, 10, 600)
    out.append(Case("shift_border_f64", sort_unique(bc, SHIFT_MINV, 1024.0, 10), SHIFT_MINV, 1024.0, 10, ("f64",)))
    out.append(Case("shift_border_f32", sort_unique(_f32_twin(bc), SHIFT_MINV, 1024.0, 10), SHIFT_MINV, 1024.0, 10, ("f32", "f64")))
    return out


def _deep():
    """depth 21, 63-bit keys: ~3000 voxels with both corners of the cube, spread so that pairs meet at every octree level (two fifths
    of the points uniform, the rest in clusters of shrinking size around the corners and random centres)"""
    rng = np.random.default_rng(21212121)
    J, top = 21, 2 ** 21 - 1
    minV = (-5.0, 3.0, 100.0)
    idx = [rng.integers(0, 2 ** J, size=(1200, 3)), np.array([[0, 0, 0], [top, top, top]])]
    for bits in range(1, 21):
        c = np.concatenate([rng.integers(0, 2 ** J, size=(2, 3)), [[0, 0, 0]], [[top, top, top]]])
        idx.append(np.clip(c[rng.integers(0, 4, size=100)] + rng.integers(-(2 ** bits), 2 ** bits, size=(100, 3)), 0, top))
    cand = (np.concatenate(idx) + np.asarray(minV, dtype=np.int64)[None, :]).astype(np.int64)
    V = sort_unique(cand, minV, float(2 ** J), J)
    q, _, key = model_keys(V, minV, float(2 ** J), J)
    assert key[0] == 0 and int(key[-1]) == 2 ** 63 - 1 and 2900 <= V.shape[0] <= 3100
    return Case("deep_j21", V, minV, float(2 ** J), J, ALL, fixture=("deep_j21", "f64"))


ACCEPTED = _accepted()
DEEP = _deep()
BY_NAME = {c.name: c for c in ACCEPTED + [DEEP]}
FIXTURES = [c for c in ACCEPTED + [DEEP] if c.fixture]


# ---- refused rows ---------------------------------------------------------------------------------------------------------
class Config:
    """a valid 300-row cloud of integer coordinates (exact in all four dtypes) that one bad row is put into"""

    def __init__(self, name, minV, J, seed):
        rng = np.random.default_rng(seed)
        self.name, self.minV, self.width, self.J = name, tuple(float(x) for x in minV), float(2 ** J), J
        self.V = sort_unique(_shifted_ints(rng, 1000, J, minV), minV, self.width, J, n=300, rng=rng)


CONFIGS = {c.name: c for c in (Config("shift", SHIFT_MINV, 10, 1), Config("zero", (0.0, 0.0, 0.0), 10, 2),
                               Config("intorg", (-37.0, 1000.0, 5.0), 10, 3), Config("deep", (0.0, 0.0, 0.0), 21, 4))}
PLACES = ("row0", "last", "alone")
_F32_BIG = float(np.finfo(np.float32).max)


def _rel(off):
    return lambda cfg, a: cfg.minV[a] + off(cfg)


# name -> (configuration, dtypes, value(cfg, axis)); every value is exact in every dtype listed with it
REFUSED_VALUES = {
    "minus_half_Q": ("shift", ("f32", "f64"), _rel(lambda c: -0.5)),                     # minV - Q / 2 (Q = 1): floors to -1
    "minus_1e-300": ("zero", ("f64",), lambda c, a: -1e-300),                           # floors to -1
    "minus_f32_denormal": ("zero", ("f32", "f64"), lambda c, a: -float(np.float32(1e-45))),   # the same for float32 inputs
    "minV_plus_width": ("shift", ("f32", "f64"), _rel(lambda c: c.width)),              # index 2^J exactly
    "minV_plus_width_int": ("intorg", ALL, _rel(lambda c: c.width)),
    "minus_one_int": ("intorg", ALL, _rel(lambda c: -1.0)),
    "plus_inf": ("shift", ("f32", "f64"), lambda c, a: np.inf),
    "minus_inf": ("shift", ("f32", "f64"), lambda c, a: -np.inf),
    "nan": ("shift", ("f32", "f64"), lambda c, a: np.nan),
    "nan_zero_origin": ("zero", ("f32", "f64"), lambda c, a: np.nan),
    "1e300": ("shift", ("f64",), lambda c, a: 1e300),
    "minus_1e300": ("shift", ("f64",), lambda c, a: -1e300),
    "f32_max": ("shift", ("f32", "f64"), lambda c, a: _F32_BIG),
    "minus_f32_max": ("shift", ("f32", "f64"), lambda c, a: -_F32_BIG),
    "int32_min": ("intorg", ("i32", "i64"), lambda c, a: -2 ** 31),
    "int32_max": ("intorg", ("i32", "i64"), lambda c, a: 2 ** 31 - 1),
    "int64_min": ("intorg", ("i64",), lambda c, a: -2 ** 63),
    "int64_max": ("intorg", ("i64",), lambda c, a: 2 ** 63 - 1),
    "two_pow_21_at_depth_21": ("deep", ALL, lambda c, a: 2 ** 21),
}
REFUSED = [(name, dt) for name, (_, dts, _) in REFUSED_VALUES.items() for dt in dts]


def refused_clouds(name, dt):
    """-> [(label, V of dtype dt, minV, width, J, bad row)]: the value on every axis in turn, as row 0 of the 300-row cloud, as
    its last row, and alone (N = 1). Every cloud has exactly that one row out of bounds in the model."""
    cfg_name, _, value = REFUSED_VALUES[name]
    cfg = CONFIGS[cfg_name]
    out = []
    for a in range(3):
        for place in PLACES:
            V = cfg.V.astype(DTYPES[dt]) if place != "alone" else cfg.V[:1].astype(DTYPES[dt])
            row = {"row0": 0, "last": V.shape[0] - 1, "alone": 0}[place]
            V[row, a] = value(cfg, a)
            _, bad, _ = model_keys(V, cfg.minV, cfg.width, cfg.J)
            assert np.array_equal(np.flatnonzero(bad), [row]), (name, dt, a, place)
            out.append((f"{name}-{dt}-axis{a}-{place}", np.ascontiguousarray(V), cfg.minV, cfg.width, cfg.J, row))
    return out


# ---- rows at the edge that must be ACCEPTED ---------------------------------------------------------------------------------
def must_accept_clouds():
    """-> [(label, dtype name, V, minV, width, J)]: -0.0 on every axis (index 0), and the last value below minV + width where the
    model puts it into the last voxel -- alone and as a row of a sorted 300-row cloud"""
    out = []
    for dt in ("f32", "f64"):
        T = DTYPES[dt]
        for cfg_name in ("zero", "shift"):
            cfg = CONFIGS[cfg_name]
            specials = {}
            if cfg_name == "zero":
                specials["neg_zero"] = np.full(3, -0.0, dtype=T)
            hi = np.nextafter((np.asarray(cfg.minV) + cfg.width).astype(T), T(-np.inf))
            q, bad, _ = model_keys(hi[None, :], cfg.minV, cfg.width, cfg.J)
            if not bad[0] and np.all(q[0] == 2 ** cfg.J - 1):
                specials["below_top"] = hi
            for label, row in specials.items():
                for a in range(3):
                    one = cfg.V[:1].astype(T)
                    one[0, a] = row[a]
                    assert np.signbit(one[0, a]) == np.signbit(row[a])
                    out.append((f"{label}-{cfg_name}-{dt}-axis{a}-alone", dt, one, cfg.minV, cfg.width, cfg.J))
                    cand = np.concatenate([one, cfg.V.astype(T)])
                    V = sort_unique(cand, cfg.minV, cfg.width, cfg.J, n=300, rng=np.random.default_rng(a), keep=(0,))
                    assert (V == one[0]).all(axis=1).any()
                    out.append((f"{label}-{cfg_name}-{dt}-axis{a}-cloud", dt, V, cfg.minV, cfg.width, cfg.J))
    assert any(l.startswith("below_top") and "f64" in l for l, *_ in out) and any(l.startswith("neg_zero") for l, *_ in out)
    return out


def integer_cloud(J=10, n=700, seed=5):
    """an integer-valued cloud with origin 0 and Q = 1 (every dtype holds it, and its Morton keys can be fed to from_keys)"""
    rng = np.random.default_rng(seed)
    return sort_unique(rng.integers(0, 2 ** J, size=(2 * n, 3)).astype(np.int64), (0.0, 0.0, 0.0), float(2 ** J), J, n=n, rng=rng)
