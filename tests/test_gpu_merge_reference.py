"""The Gaussian merge kernels against what cuda/merge_cluster.cu computes, not against their own restatement.

tests/test_gpu_merge.py pins both kernels (``merge_kernel``, csrc/merge.hip; ``raht::voxel_merge_chunk_kernel``, csrc/voxelize.hip;
both finish a column with ``merge_finish``, csrc/raht_device.h) bit for bit to the C restatement ``oracle.merge_clusters``, which
shares their float32 operation order: that proves determinism.
Here they are compared with the independent float64 model of the reference kernel (tests/numpy_merge.py) within its error
bars, at the shapes where the kernels' geometry changes (column chunks of 64 lanes in merge_kernel, 4-column chunks and 17 /
33 / 65-column steps in the voxel kernel, 16 clusters per wave, the grid-stride loops past 524 288 clusters or voxels), and
``merge.prepare_cluster_data`` on the device against the reference's fixture. Bit parity with a CUDA build of the reference
stays unpinned. Every test prints its worst error as a fraction of its bar (``pytest -rP`` or ``-s`` shows it).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import numpy_merge as nm

pytestmark = pytest.mark.gpu


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _merge_on_gpu(ci, co, g, wbo):
    from raht_3dgs_codec_amd import merge
    out = merge.merge_gaussian_clusters_with_indices(*[_t(a) for a in g], _t(ci), _t(co), wbo)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def _report(tag, worst):
    print(f"{tag}: worst err/bar " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, (tag, worst)


@pytest.mark.parametrize("k", range(32))
def test_merge_kernel_against_model(k):
    """The CPU test's matrix (tests/test_merge_model.py) at GPU sizes: every colour width of CDS (chunk edges 53/54 and
    117/118 of the 64-lane column map), every size family, every opacity mode (sums above 1, all zero, subnormal, tiny
    normal), both weightings, every residue of the cluster count mod 16, members a random permutation of the rows."""
    cd, sizes, opacity, wbo, K = nm.matrix_case(k)
    K += 3000
    rng = np.random.default_rng(5000 + k)
    ci, co, N = nm.clusters_of(rng, nm.size_mix(rng, sizes, K))
    g = nm.gaussians(rng, N, cd, opacity)
    got = _merge_on_gpu(ci, co, g, wbo)
    _report(f"merge k={k} cd={cd} sizes={sizes} opacity={opacity} wbo={wbo} K={K}", nm.compare(got, ci, co, *g, wbo))


@pytest.mark.parametrize("cd", nm.CDS)
def test_merge_kernel_every_color_width(cd):
    """Every colour width once more, with mixed cluster sizes 1-9 / 15-17 / 63-65, empty clusters between full ones and
    opacity sums above 1."""
    rng = np.random.default_rng(cd)
    sizes = np.concatenate([nm.size_mix(rng, kind, 400) for kind in ("empties", "around16", "around64", "single")])
    ci, co, N = nm.clusters_of(rng, rng.permutation(sizes))
    g = nm.gaussians(rng, N, cd, "big" if cd % 2 else "sigmoid")
    got = _merge_on_gpu(ci, co, g, True)
    _report(f"merge cd={cd} K={co.size - 1}", nm.compare(got, ci, co, *g, True))


@pytest.mark.parametrize("wbo", [True, False])
def test_merge_kernel_one_huge_cluster(wbo):
    rng = np.random.default_rng(11)
    sizes = np.concatenate([rng.integers(0, 10, size=500), [100_000], rng.integers(0, 10, size=500)])
    ci, co, N = nm.clusters_of(rng, sizes)
    g = nm.gaussians(rng, N, 48, "sigmoid")
    got = _merge_on_gpu(ci, co, g, wbo)
    _report(f"merge one 100k cluster wbo={wbo}", nm.compare(got, ci, co, *g, wbo))


def test_merge_kernel_past_the_grid():
    """1.2 M clusters: the kernel's grid holds 8192 blocks x 4 waves x 16 clusters = 524 288, so its loop runs three times."""
    rng = np.random.default_rng(12)
    K = 1_200_003
    sizes = rng.integers(1, 4, size=K)
    sizes[rng.random(K) < 0.1] = 0
    ci, co, N = nm.clusters_of(rng, sizes)
    g = nm.gaussians(rng, N, 3, "sigmoid")
    got = _merge_on_gpu(ci, co, g, True)
    _report(f"merge K={K} N={N}", nm.compare(got, ci, co, *g, True))


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
def test_prepare_cluster_data_matches_reference_gpu(dtype):
    from raht_3dgs_codec_amd import merge
    for name, labels, ref_ci, ref_co in nm.merge_prepare_sets():
        if dtype == torch.int32 and np.abs(labels).max() >= 2 ** 31:
            continue
        ci, co = merge.prepare_cluster_data(torch.from_numpy(labels).to(dtype).cuda())
        assert ci.is_cuda and ci.dtype == torch.int32 and co.dtype == torch.int32, name
        nm.check_prepare(ci.cpu().numpy(), co.cpu().numpy(), ref_ci, ref_co)


def _rows(rng, N, cd, spread=1.0):
    means, quats, scales, op, colors = nm.gaussians(rng, N, cd, "sigmoid")
    means = rng.uniform(0, spread, size=(N, 3)).astype(np.float32)
    return np.concatenate([means, quats, scales, op[:, None], colors], axis=1).astype(np.float32)


def _voxel_check(G, J, Gvox, info, wbo, tag):
    """Columns 0-2: the voxelizer's integer coordinates, exactly, and every member inside its voxel; columns 3.. and
    merged_means: the model on the returned sort permutation / voxel starts, within the bars."""
    from raht_3dgs_codec_amd import ops
    N = G.shape[0]
    Gd = _t(G)
    PCvox, _, vidx, _, vinfo = ops.voxelize_pc_batched(Gd[:, :3].contiguous(), J=J, residuals=False, sorted_points=False)
    gv = Gvox.cpu().numpy()
    assert np.array_equal(gv[:, :3], PCvox[:, :3].cpu().numpy()), tag
    ci = info["sort_idx"].cpu().numpy().astype(np.int64)
    co = np.concatenate([info["voxel_indices"].cpu().numpy(), [N]]).astype(np.int64)
    assert np.all(np.diff(co) > 0) and np.array_equal(np.sort(ci), np.arange(N))
    cell = (G[ci, :3].astype(np.float64) - info["vmin"].cpu().numpy().astype(np.float64)) / info["voxel_size"]
    own = np.repeat(gv[:, :3].astype(np.float64), np.diff(co), axis=0)
    assert np.all(cell >= own - 1e-4) and np.all(cell <= own + 1 + 1e-4), tag
    got = [info["merged_means"].cpu().numpy(), gv[:, 3:7], gv[:, 7:10], gv[:, 10], gv[:, 11:]]
    _report(tag, nm.compare(got, ci, co, G[:, :3], G[:, 3:7], G[:, 7:10], G[:, 10], G[:, 11:], wbo))


@pytest.mark.parametrize("width", [11, 12, 13, 16, 17, 33, 64, 65, 68, 69, 128, 129])
def test_voxelize_merge_against_model(width):
    """Row widths across the voxel kernel's steps: 4-column chunks with an overlapping last one, 4 / 8 / 16 lanes per row
    (17 and 33 columns), several blocks of chunks past 64 columns; J = 4 puts about five Gaussians in every voxel."""
    from raht_3dgs_codec_amd import ops
    rng = np.random.default_rng(width)
    G = _rows(rng, 20000, width - 11)
    for wbo in (True, False):
        Gvox, info = ops.voxelize_merge(_t(G), J=4, weight_by_opacity=wbo)
        assert info["Nvox"] < G.shape[0] // 3
        _voxel_check(G, 4, Gvox, info, wbo, f"voxelize_merge width={width} wbo={wbo} Nvox={info['Nvox']}")


def _voxelize_merge_raw(buf, ld, N, cd, J, wbo):
    """raht_voxelize_merge on a [N, ld] row view of ``buf`` (a CUDA float32 tensor whose rows are ld >= 11 + cd apart)."""
    from raht_3dgs_codec_amd import _lib
    from raht_3dgs_codec_amd._lib import check
    dev = buf.device
    keys, idx, vidx = (torch.empty(N, dtype=torch.int64, device=dev) for _ in range(3))
    gv = torch.empty((N, 11 + cd), dtype=torch.float32, device=dev)
    mm = torch.empty((N, 3), dtype=torch.float32, device=dev)
    nvox, vmin_out, w_out, vs_out = C.c_int64(), (C.c_float * 3)(), C.c_double(), C.c_double()
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    check(_lib.lib().raht_voxelize_merge(p(buf), ld, N, cd, 1 if wbo else 0, None, -1.0, J, p(keys), p(idx), p(vidx), p(gv), p(mm),
                                         C.byref(nvox), vmin_out, C.byref(w_out), C.byref(vs_out),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    nv = nvox.value
    return gv[:nv].clone(), mm[:nv].clone(), idx.clone(), vidx[:nv].clone()


@pytest.mark.parametrize("cd,pad", [(0, 1), (2, 3), (6, 5), (22, 1), (54, 7), (118, 4)])
def test_voxelize_merge_row_stride(cd, pad):
    """ldg = 11 + cd + pad: the rows of a wider buffer, padding columns NaN. Bit-identical to the contiguous call."""
    rng = np.random.default_rng(100 + cd)
    N, ld = 9000, 11 + cd
    G = _rows(rng, N, cd)
    wide = np.full((N, ld + pad), np.nan, np.float32)
    wide[:, :ld] = G
    for wbo in (True, False):
        a = _voxelize_merge_raw(_t(G), ld, N, cd, 4, wbo)
        b = _voxelize_merge_raw(_t(wide), ld + pad, N, cd, 4, wbo)
        for x, y in zip(a, b):
            assert torch.equal(x, y), (cd, pad, wbo)
        assert not torch.isnan(b[0]).any()
    print(f"voxelize_merge ldg={ld + pad} (11 + {cd} + {pad}): bit-identical to ldg={ld}, Nvox={a[0].shape[0]}")


def test_checkpoint_sized_merge():
    """A whole-checkpoint frame, as the reference merges one (python/test_voxelize_3dgs.py:160-257): 3 M Gaussians with
    48 colour columns, J = 7, about 1.6 M voxels -- both kernels' grid-stride loops run. Both kernels against the model,
    and against each other bit for bit."""
    from raht_3dgs_codec_amd import merge, ops
    rng = np.random.default_rng(3)
    N, cd, J = 3_000_000, 48, 7
    G = _rows(rng, N, cd)
    Gd = _t(G)
    Gvox, info = ops.voxelize_merge(Gd, J=J, weight_by_opacity=True)
    assert info["Nvox"] > 1_048_576
    _voxel_check(G, J, Gvox, info, True, f"voxelize_merge N={N} cd={cd} Nvox={info['Nvox']}")
    ci = info["sort_idx"].int()
    co = torch.cat([info["voxel_indices"], torch.tensor([N], dtype=torch.int64, device="cuda")]).int()
    cols = [Gd[:, 0:3], Gd[:, 3:7], Gd[:, 7:10], Gd[:, 10], Gd[:, 11:]]
    out = merge.merge_gaussian_clusters_with_indices(*[c.contiguous() for c in cols], ci, co, True)
    got = [o.cpu().numpy() for o in out]
    _report(f"merge_kernel N={N} cd={cd} K={info['Nvox']}",
            nm.compare(got, ci.cpu().numpy(), co.cpu().numpy(), G[:, :3], G[:, 3:7], G[:, 7:10], G[:, 10], G[:, 11:], True))
    assert torch.equal(out[0], info["merged_means"]) and torch.equal(out[1], Gvox[:, 3:7]) and torch.equal(out[4], Gvox[:, 11:])
