"""Test-only float64 model of the reference's Gaussian merge (cuda/merge_cluster.cu, merge_weighted_mean_kernel), with an
error bar for every output. Written from the kernel's semantics, vectorised over clusters with ``np.add.reduceat`` over the
member rows; it does not follow the operation order of any float32 implementation, and it is independent of the C
restatement in oracle/raht_oracle.c.

Semantics (per cluster k with members i in cluster_indices[offsets[k]:offsets[k+1]], weight w_i = opacity_i or 1):
  * empty cluster: every output 0;
  * W = sum w_i; means, scales: sum x_i w_i / W, with W replaced by 1 when W == 0;
  * quaternion: S = sum q_i w_i, S / |S|, or the identity (0, 0, 0, 1) when the norm is 0 (exactly, or in float32);
  * opacity: min(sum o_i, 1) (the plain sum, not weighted);
  * colours: sum c_i w_i / W if W > 0, else 0.
Weights are taken to be >= 0 (opacities are sigmoid outputs), so the float32 tests W == 0 and W > 0 decide exactly as the
exact sums do. The bars assume IEEE float32 with subnormals kept, as the HIP kernels are built (-fno-fast-math). A
flush-to-zero build (the reference's setup.py passes --use_fast_math to nvcc, which implies -ftz=true) would send clusters of
subnormal weights down the zero-weight branch, which the model does not.

Error bars. The float32 kernel accumulates a cluster of n members with one rounding per member (fma, or an add for the
opacity), then divides. Standard model of float32 arithmetic, u = 2^-24 (unit roundoff) and eta = 2^-150 (the absolute
error of a result that rounds into the subnormal range; sums and differences of floats are exact there):
    fl(a op b) = (a op b)(1 + d) + e,   |d| <= u,  |e| <= eta.
  * Weighted sum A = sum x_i w_i: |A32 - A| <= n u sum|x_i w_i| + n eta (each member's term passes through at most n
    roundings).  W32 = sum w_i: |W32 - W| <= (n - 1) u W (w >= 0; no eta, the sum of floats is exact when subnormal).
    R = A / W:  |R32 - R| <= |A32 - A| / W + |R| |W32 - W| / W + u |R| + eta
              <= (n + 1) u (sum|x w| / W + |R|) + u |R| + n eta / W + eta.
  * Opacity: a sum of n non-negative terms, n - 1 roundings: (n - 1) u sum o + eta; min(., 1) does not enlarge it.
  * Quaternion: component errors |e_k| <= n u sum|q_ik| w_i + n eta; |e| <= n u sum w_i |q_i| + 2 n eta = E.  The norm is
    |S32| (1 + 2u) after four roundings of the squares (x u, plus 4 eta absolute in the squared norm), a correctly rounded
    sqrt (+u) and the division (+u).  Linearising S/|S|:
        |q32_k - s_k| <= (|e_k| + |s_k| E) / |S| + 4 u |s_k| + (2 eta / |S|^2) |s_k| + u,   s = S / |S|.
    The float32 squared norm is exactly 0 -- identity branch -- when (|S| + E)^2 < eta (every square and every partial sum
    rounds to 0), which is what subnormal or tiny weights give.  Where the two branches cannot be told apart from the bound,
    (|S| - E)^2 < 2^-126, the bar is 2, the distance between any two unit quaternions' components (unpinned).
The bound is first order in n u; the tests multiply it by SAFETY = 2 to absorb the second-order terms (at n = 100 000,
(n u)^2 / (n u) = n u = 0.006) and the linearisation.  Nothing in it is fitted to observed errors.
"""
import os

import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -150
SAFETY = 2.0
OUTPUTS = ("means", "quats", "scales", "opacities", "colors")


def merge_f64(cluster_indices, cluster_offsets, means, quats, scales, opacities, colors, weight_by_opacity=True):
    """-> (values, bars): two dicts keyed by OUTPUTS, float64 arrays of the output shapes. ``cluster_offsets`` may be any
    monotone slice of an offsets array (it need not start at 0): the clusters are cluster_offsets[k]..[k+1]."""
    co = np.asarray(cluster_offsets, np.int64)
    K = co.size - 1
    n = np.diff(co)
    full = n > 0
    starts = co[:-1][full] - co[0]
    idx = np.asarray(cluster_indices, np.int64)[co[0]:co[-1]]
    nf = n[full].astype(np.float64)

    def seg(a):                                   # per non-empty cluster sums of member rows
        return np.add.reduceat(a, starts, axis=0) if starts.size else np.zeros((0,) + a.shape[1:])

    o = np.asarray(opacities, np.float32)[idx].astype(np.float64)
    w = o if weight_by_opacity else np.ones_like(o)
    W = seg(w)
    Wd = np.where(W == 0, 1.0, W)
    vals, bars = {}, {}

    def put(name, v, b, cols):
        shape = (K,) if cols is None else (K, cols)
        vals[name], bars[name] = np.zeros(shape), np.zeros(shape)
        vals[name][full], bars[name][full] = v, b

    def weighted_mean(x, zero_if_no_weight):
        xw = x * w[:, None]
        R = seg(xw) / Wd[:, None]
        bar = ((nf + 1) * U)[:, None] * (seg(np.abs(xw)) / Wd[:, None] + np.abs(R)) + U * np.abs(R) \
            + (nf * ETA / Wd)[:, None] + ETA
        if zero_if_no_weight:
            R = np.where((W > 0)[:, None], R, 0.0)
            bar = np.where((W > 0)[:, None], bar, 0.0)
        return R, bar

    for name, a, cols, zero in (("means", means, 3, False), ("scales", scales, 3, False), ("colors", colors, None, True)):
        a = np.asarray(a, np.float32)
        cols = a.shape[1] if cols is None else cols
        x = a.reshape(a.shape[0], cols)[idx].astype(np.float64)
        put(name, *weighted_mean(x, zero), cols)

    osum = seg(o)
    put("opacities", np.minimum(osum, 1.0), (nf - 1) * U * osum + ETA, None)

    q = np.asarray(quats, np.float32)[idx].astype(np.float64)
    qw = q * w[:, None]
    S = seg(qw)
    nrm = np.sqrt(np.sum(S * S, axis=1))
    E = nf * U * seg(np.linalg.norm(q, axis=1) * w) + 2 * nf * ETA
    ek = (nf * U)[:, None] * seg(np.abs(qw)) + (nf * ETA)[:, None]
    zero = (nrm + E) ** 2 < ETA
    unsure = ~zero & ((np.maximum(nrm - E, 0.0)) ** 2 < 2.0 ** -126)
    safe = np.where(nrm > 0, nrm, 1.0)
    s = S / safe[:, None]
    qbar = (ek + np.abs(s) * E[:, None]) / safe[:, None] + 4 * U * np.abs(s) + (2 * ETA / safe ** 2)[:, None] * np.abs(s) + U
    ident = np.array([0.0, 0.0, 0.0, 1.0])
    s = np.where((zero | (nrm == 0))[:, None], ident, s)
    qbar = np.where(zero[:, None], 0.0, np.where(unsure[:, None], 2.0, qbar))
    put("quats", s, qbar, 4)
    return vals, bars


def worst_ratio(got, vals, bars):
    """max |got - model| / (SAFETY * bar) over one output (0 where both are exact); inf for a mismatch on an exact output
    and for any non-finite output (the model's values are finite for finite inputs: a NaN or inf is always an error)."""
    got = np.asarray(got, np.float64)
    d = np.abs(got - vals)
    b = SAFETY * bars
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / b)
    r = np.where(np.isfinite(got) & np.isfinite(d), r, np.inf)
    return float(r.max()) if r.size else 0.0


def compare(got, cluster_indices, cluster_offsets, means, quats, scales, opacities, colors, weight_by_opacity=True,
            block_rows=1 << 18):
    """Worst error / bar per output of ``got`` (5 arrays in OUTPUTS order, [K, ...]) against the model, computed over blocks
    of clusters holding about ``block_rows`` members each (host memory stays bounded at millions of rows)."""
    co = np.asarray(cluster_offsets, np.int64)
    K = co.size - 1
    worst = dict.fromkeys(OUTPUTS, 0.0)
    k0 = 0
    while k0 < K:
        k1 = int(np.searchsorted(co, co[k0] + block_rows, side="right")) - 1
        k1 = min(max(k1, k0 + 1), K)
        vals, bars = merge_f64(cluster_indices, co[k0:k1 + 1], means, quats, scales, opacities, colors, weight_by_opacity)
        for name, g in zip(OUTPUTS, got):
            g = np.asarray(g)[k0:k1]
            if name == "colors":
                g = g.reshape(k1 - k0, -1)
            worst[name] = float(np.maximum(worst[name], worst_ratio(g, vals[name], bars[name])))   # (NaN would propagate)
        k0 = k1
    return worst


# ---------------------------------------------------------------- test inputs

def clusters_of(rng, sizes, shuffle=True):
    """Cluster sizes (zeros allowed: empty clusters) -> (cluster_indices int32, cluster_offsets int32, N). With ``shuffle``
    the members are a random permutation of the rows, so member order differs from row order."""
    sizes = np.asarray(sizes, np.int64)
    co = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    N = int(co[-1])
    ci = (rng.permutation(N) if shuffle else np.arange(N)).astype(np.int32)
    return ci, co, N


def gaussians(rng, N, color_dim, opacity="sigmoid"):
    """(means, quats, scales, opacities, colors) float32. opacity: 'sigmoid' (with a few exact zeros), 'big' (sums above 1),
    'zero', 'subnormal' (~1e-40), 'tiny' (~1e-38, normal)."""
    means = rng.normal(0, 2, size=(N, 3)).astype(np.float32)
    q = rng.normal(size=(N, 4))
    quats = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    scales = np.exp(rng.normal(-3, 1, size=(N, 3))).astype(np.float32)
    colors = rng.normal(0, 0.5, size=(N, color_dim)).astype(np.float32)
    if opacity == "sigmoid":
        op = 1 / (1 + np.exp(-rng.normal(0, 2, size=N)))
        op[rng.random(N) < 0.02] = 0.0
    elif opacity == "big":
        op = rng.uniform(0.4, 1.0, size=N)
    elif opacity == "zero":
        op = np.zeros(N)
    elif opacity == "subnormal":
        op = rng.uniform(1.0, 2.0, size=N) * 1e-40
    elif opacity == "tiny":
        op = rng.uniform(1.0, 2.0, size=N) * 1e-38
    else:
        raise ValueError(opacity)
    return means, quats, scales, op.astype(np.float32), colors


def size_mix(rng, kind, K):
    """K cluster sizes of one family: 'single', 'small' (1-9), 'around16' (15/16/17), 'around64' (63/64/65), 'empties'
    (1-9 with every fourth cluster empty)."""
    if kind == "single":
        return np.ones(K, np.int64)
    if kind == "small":
        return rng.integers(1, 10, size=K)
    if kind == "around16":
        return rng.choice([15, 16, 17], size=K)
    if kind == "around64":
        return rng.choice([63, 64, 65], size=K)
    if kind == "empties":
        s = rng.integers(1, 10, size=K)
        s[rng.random(K) < 0.25] = 0
        return s
    raise ValueError(kind)


# ---------------------------------------------------------------- the shape matrix and the prepare_cluster_data fixture

# the shape matrix of tests/test_merge_model.py (CPU sizes); tests/test_gpu_merge_reference.py adds 3000 clusters per case
CDS = [0, 1, 2, 3, 4, 5, 48, 52, 53, 54, 55, 117, 118, 245]
SIZES = ["single", "small", "around16", "around64", "empties"]
OPACITY = ["sigmoid", "big", "zero", "subnormal", "tiny"]


def matrix_case(k):
    """Case k of the matrix: every colour width, every size family, every opacity mode, both weightings, and every
    residue of the cluster count mod 16."""
    cd, sizes, opacity, wbo = CDS[k % len(CDS)], SIZES[k % len(SIZES)], OPACITY[(k // 2) % len(OPACITY)], k % 3 != 0
    K = 160 + k % 16 + 16 * (k % 5)
    return cd, sizes, opacity, wbo, K


MERGE_PREPARE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge", "merge_prepare.npz")


def merge_prepare_sets():
    z = np.load(MERGE_PREPARE)
    lo, oo = z["lab_off"], z["off_off"]
    return [(str(z["names"][k]), z["labels"][lo[k]:lo[k + 1]], z["indices"][lo[k]:lo[k + 1]], z["offsets"][oo[k]:oo[k + 1]])
            for k in range(len(z["names"]))]


def check_prepare(ci, co, ref_ci, ref_co):
    """Offsets exact; per cluster the same members as the reference, in strictly increasing row order."""
    ci, co = np.asarray(ci, np.int64), np.asarray(co, np.int64)
    assert np.array_equal(co, ref_co)
    assert ci.shape == ref_ci.shape
    cid = np.repeat(np.arange(co.size - 1), np.diff(co))
    assert np.array_equal(np.sort(ci + cid * (1 << 40)), np.sort(ref_ci.astype(np.int64) + cid * (1 << 40)))
    same = cid[1:] == cid[:-1]
    assert np.all(ci[1:][same] > ci[:-1][same])
