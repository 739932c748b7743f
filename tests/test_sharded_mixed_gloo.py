"""Mixed-precision Morton-prefix sharded RAHT (ShardedRaht(n_wide=3)) on CPU over gloo, world 2, 3 and 8.

The shard-local arithmetic is injected (tests/numpy_mixed_ops.py: float64 numpy on tests/numpy_ops.NumpyPlan); under test
is the host-side plumbing of the mixed step -- the wide roots' own buffer set and gather, the second (float64) top tree, the
top rows quantized column-split -- checked against the C oracle run on the WHOLE scene: the xyz integers must be the
reference's float64 integers (python/encode_3dgs.py:82-83,204)."""
import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests.rank_procs import run_ranks

NW = 3


def near_ties(To, step, rel=1e-9):
    """entries whose quotient T / step lies within `rel` (relative) of k + 0.5: float64 transforms that differ in the last
    bits may round those either way"""
    x = To / step
    return np.abs(x - np.floor(x) - 0.5) <= rel * np.maximum(np.abs(x), 1.0)


def _worker(rank, world, J, n, D, steps, prefix_range=None):
    from raht_3dgs_codec_amd import sharded, synth
    from tests.numpy_mixed_ops import NumpyMixedLocalOps
    from oracle import oracle as orc

    V, keys, C = synth.scene(n, J, D, seed=41, prefix_range=prefix_range)
    nbits, pb = 3 * J, 9
    cuts = sharded.balanced_prefix_cuts(torch.from_numpy(keys.view(np.int64).copy()), nbits, world, pb)
    mine = np.arange(cuts[rank], cuts[rank + 1])
    k_loc = torch.from_numpy(keys[mine].view(np.int64).copy())
    C_loc = torch.from_numpy(C[mine].astype(np.float64))
    sh = sharded.ShardedRaht(k_loc, nbits, prefix_bits=pb, local_ops=NumpyMixedLocalOps, n_wide=NW)
    assert sh.n_wide == NW and sh.total_rows == keys.shape[0]
    po = orc.raht_param(V.astype(np.float64), np.zeros(3), 2 ** J, J)
    To, _ = orc.raht_fwd(C.astype(np.float64), po)
    ties = 0
    for step in steps:
        st = np.asarray(step, dtype=np.float64).reshape(-1)
        Q = sh.forward_quant(C_loc, step)
        assert Q.dtype == torch.int32 and tuple(Q.shape) == (mine.size, D)
        if mine.size:
            Qr = Q[sh.plan.inv_order].numpy().astype(np.int64)          # row order
            ref = np.floor(To[mine] / st + 0.5).astype(np.int64)
            tie = near_ties(To[mine], st)
            bad = (Qr != ref) & ~tie
            assert not bad[:, :NW].any(), (step, np.argwhere(bad[:, :NW])[:5])
            assert not bad.any(), (step, np.argwhere(bad)[:5])
            ties += int(((Qr != ref) & tie)[:, :NW].sum())
            # dequantized coefficients within half a step of the whole scene's; the round trip inverts them exactly
            Tq = Qr * st
            assert np.all(np.abs(Tq - To[mine]) <= 0.5 * st * (1 + 1e-9) + 1e-9 * np.abs(To[mine]))
        R = sh.dequant_inverse(Q, step)
        assert R.dtype == torch.float64 and tuple(R.shape) == (mine.size, D)
        e = torch.tensor([float(((R - C_loc) ** 2).sum()),
                          float(((Qr * st - To[mine]) ** 2).sum()) if mine.size else 0.0], dtype=torch.float64)
        dist.all_reduce(e)                       # orthonormal transform: reconstruction error energy == quantization error energy
        assert abs(e[0].item() - e[1].item()) <= 1e-6 * max(e[1].item(), 1e-30), e
        chk = sh.check_mixed_against_unsharded(C_loc, step, keys_sorted=k_loc)
        assert chk["ok"], chk
        # the unquantized entries and the float32 path are untouched by n_wide
        plain = sharded.ShardedRaht(k_loc, nbits, prefix_bits=pb, local_ops=NumpyMixedLocalOps)
        Qp = plain.forward_quant(C_loc, torch.as_tensor(step, dtype=torch.float64))
        if mine.size:
            assert torch.equal(Qp[:, NW:], Q[:, NW:])
    dist.all_reduce(torch.zeros(1))
    return ties


def _run(world, args):
    print("near-ties on the wide columns per rank:", run_ranks(_worker, world, *args))


PER_CHANNEL = [0.01, 0.02, 0.5] + [0.05 + 0.01 * i for i in range(56)]


@pytest.mark.parametrize("world,J,n", [(2, 8, 6000), (3, 10, 5000), (8, 7, 8000)])
def test_sharded_mixed_matches_the_oracle_integers(world, J, n):
    _run(world, (J, n, 59, [0.01, 1.0, PER_CHANNEL]))


@pytest.mark.parametrize("world,J,n,prefix_range", [(3, 6, 3000, (0, 300, 9)), (8, 6, 2500, (70, 330, 9))])
def test_sharded_mixed_rank_without_rows(world, J, n, prefix_range):
    _run(world, (J, n, 59, [0.01], prefix_range))


def test_mixed_needs_mixed_local_ops():
    from raht_3dgs_codec_amd import sharded, synth
    from tests.numpy_ops import NumpyLocalOps
    from tests.numpy_mixed_ops import NumpyMixedLocalOps
    _, keys, C = synth.scene(2000, 7, 8, seed=5)
    k = torch.from_numpy(keys.view(np.int64).copy())
    with pytest.raises(ValueError, match="lacks"):
        sharded.ShardedRaht(k, 21, prefix_bits=9, local_ops=NumpyLocalOps, n_wide=3)
    with pytest.raises(ValueError):
        sharded.ShardedRaht(k, 21, prefix_bits=9, local_ops=NumpyMixedLocalOps, n_wide=5)
    for f in sharded.MIXED_OPS:
        assert callable(getattr(sharded.HipLocalOps, f))
    # world = 1: bytes of the gathers stay 0; the mixed step of a single process is the plain mixed transform
    sh = sharded.ShardedRaht(k, 21, prefix_bits=9, local_ops=NumpyMixedLocalOps, n_wide=3)
    assert sh.gathered_bytes_per_step(8) == 0
    Cd = torch.from_numpy(C.astype(np.float64))
    Q = sh.forward_quant(Cd, 0.01)
    assert sh.check_mixed_against_unsharded(Cd, 0.01)["ok"]
    assert float((sh.step(Cd, 0.01) - Cd).abs().max()) < 0.01 * np.sqrt(Cd.shape[0])
    assert tuple(Q.shape) == tuple(Cd.shape)
