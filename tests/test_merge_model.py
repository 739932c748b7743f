"""The Gaussian merge stage pinned where it can be pinned without a GPU.

* ``merge.prepare_cluster_data`` against the reference's own ``prepare_cluster_data`` (cuda/merge_cluster_cuda/__init__.py:30-75),
  through the fixture tests/golden/merge/merge_prepare.npz: offsets exactly, indices as a set per cluster (the reference's argsort
  is unstable), and the members of every cluster in increasing row order (the stable sort this project adds).
* The float64 model of cuda/merge_cluster.cu (tests/numpy_merge.py) against the C restatement ``oracle.merge_clusters``,
  within the model's error bars: the bars are tested here, on the same shape matrix the GPU tests use (smaller N), before
  they judge the HIP kernels (tests/test_gpu_merge_reference.py).
"""
import numpy as np
import pytest
import torch

from tests import numpy_merge as nm


def test_merge_prepare_fixture_is_the_docstring_example():
    name, labels, ci, co = nm.merge_prepare_sets()[0]
    assert name == "docstring" and labels.tolist() == [2, 0, 2, 1, 0, 2]
    assert ci.tolist() == [1, 4, 3, 0, 2, 5] and co.tolist() == [0, 2, 3, 6]


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_prepare_cluster_data_matches_reference_cpu(dtype):
    from raht_3dgs_codec_amd import merge
    for name, labels, ref_ci, ref_co in nm.merge_prepare_sets():
        if dtype == torch.int32 and np.abs(labels).max() >= 2 ** 31:
            continue                                              # (the 1e12 ids exist as int64 only)
        ci, co = merge.prepare_cluster_data(torch.from_numpy(labels).to(dtype))
        assert ci.dtype == torch.int32 and co.dtype == torch.int32, name
        nm.check_prepare(ci.numpy(), co.numpy(), ref_ci, ref_co)


def test_model_known_answers():
    """Hand-computed clusters: a weighted pair, an empty cluster, an all-zero-weight pair, opposite quaternions."""
    ci = np.array([0, 1, 2, 3, 4, 5], np.int32)
    co = np.array([0, 2, 2, 4, 6], np.int32)
    means = np.array([[1, 2, 3], [4, 5, 6], [1, 1, 1], [3, 3, 3], [0, 0, 0], [0, 0, 0]], np.float32)
    quats = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, -1, 0, 0]], np.float32)
    scales = means + 1
    op = np.array([0.25, 0.75, 0, 0, 0.75, 0.75], np.float32)
    colors = np.arange(12, dtype=np.float32).reshape(6, 2)
    v, b = nm.merge_f64(ci, co, means, quats, scales, op, colors, True)
    assert np.allclose(v["means"], [[3.25, 4.25, 5.25], [0, 0, 0], [0, 0, 0], [0, 0, 0]])
    assert np.allclose(v["quats"], [[0.25 / np.sqrt(0.625), 0.75 / np.sqrt(0.625), 0, 0], [0] * 4, [0, 0, 0, 1], [0, 0, 0, 1]])
    assert np.allclose(v["opacities"], [1.0, 0, 0, 1.0])
    assert np.allclose(v["colors"], [[0.25 * 0 + 0.75 * 2, 0.25 * 1 + 0.75 * 3], [0, 0], [0, 0], [9, 10]])
    assert np.all(b["means"][0] > 0) and np.all(b["means"][0] < 1e-5)
    v, _ = nm.merge_f64(ci, co, means, quats, scales, op, colors, False)
    assert np.allclose(v["means"][2], [2, 2, 2]) and np.allclose(v["quats"][2], [np.sqrt(0.5), 0, np.sqrt(0.5), 0])
    assert np.allclose(v["colors"][2], [5, 6])


def test_compare_fails_on_non_finite_output(oracle):
    """A NaN or inf anywhere in an output -- what 0/0 gives when a zero-weight or zero-norm guard is missing -- is an
    error of ratio inf, even beside other errors in the same block, and a plain out-of-bar error still reads above 1."""
    rng = np.random.default_rng(3)
    ci, co, N = nm.clusters_of(rng, nm.size_mix(rng, "empties", 400))
    g = nm.gaussians(rng, N, 4, "sigmoid")
    good = oracle.merge_clusters(ci, co, *g, True)
    assert max(nm.compare(good, ci, co, *g, True).values()) <= 1.0
    full = np.flatnonzero(np.diff(co) > 0)
    for name, j in (("means", 0), ("quats", 1), ("opacities", 3), ("colors", 4)):
        for bad in (np.nan, np.inf):
            out = [a.copy() for a in good]
            out[j] = out[j] * np.float32(1.01)                   # 1 % off everywhere ...
            out[j][full[7]] = bad                                 # ... and one non-finite cluster
            worst = nm.compare(out, ci, co, *g, True)
            assert worst[name] == np.inf, (name, bad, worst)
            out[j][full[7]] = good[j][full[7]]
            assert 1.0 < nm.compare(out, ci, co, *g, True)[name] < np.inf, name
    out = [a.copy() for a in good]
    out[0][np.flatnonzero(np.diff(co) == 0)[0]] = np.nan      # an empty cluster must read 0, not NaN
    assert nm.compare(out, ci, co, *g, True)["means"] == np.inf


@pytest.mark.parametrize("k", range(32))
def test_model_bars_hold_for_restatement(oracle, k):
    cd, sizes, opacity, wbo, K = nm.matrix_case(k)
    rng = np.random.default_rng(1000 + k)
    ci, co, N = nm.clusters_of(rng, nm.size_mix(rng, sizes, K))
    g = nm.gaussians(rng, N, cd, opacity)
    got = oracle.merge_clusters(ci, co, *g, wbo)
    worst = nm.compare(got, ci, co, *g, wbo)
    print(f"k={k} cd={cd} sizes={sizes} opacity={opacity} wbo={wbo} K={K}: worst err/bar", worst)
    assert max(worst.values()) <= 1.0, worst


def test_model_bars_hold_for_restatement_large_cluster(oracle):
    """One cluster of 100 000 members beside small ones: the bar grows with n."""
    rng = np.random.default_rng(77)
    ci, co, N = nm.clusters_of(rng, np.concatenate([[100_000], rng.integers(1, 10, size=100)]))
    g = nm.gaussians(rng, N, 5, "sigmoid")
    got = oracle.merge_clusters(ci, co, *g, True)
    worst = nm.compare(got, ci, co, *g, True)
    print("one 100k cluster: worst err/bar", worst)
    assert max(worst.values()) <= 1.0, worst
