"""ShardedRaht(n_wide=3) on the MI355X: the mixed-precision sharded step (float64 xyz columns, float32 attributes) over
a one-rank RCCL group with forced collectives, 4 and 5 gloo ranks sharing the GPU, and the direct exchange.

Bars, at steps 0.01, 1.0 and per-channel steps: check_mixed_against_unsharded (whole scene gathered, the UNSHARDED mixed
kernels run on it) returns exact equality on all 59 columns; the xyz integers are the float64 oracle's on the whole scene
except at near-ties (the oracle's T / step within 1e-9 relative of k + 0.5); columns [3, 59) are bit-identical to the same
ShardedRaht built without n_wide."""
import numpy as np
import pytest

from tests.rank_procs import run_ranks

pytestmark = pytest.mark.gpu
NW, D = 3, 59
PER_CHANNEL = [0.01, 0.02, 0.05] + [0.002 * (1 + c % 9) for c in range(D - 3)]


@pytest.fixture(scope="module")
def rt():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    _lib.lib()
    return R


def _check_rank(rank, world, J, n, seed, force, direct):
    """one rank's checks; returns the number of near-tie differences on the wide columns"""
    import torch
    from raht_3dgs_codec_amd import sharded, synth
    from oracle import oracle as orc
    V, keys, C = synth.scene(n, J, D, seed=seed)
    nbits = 3 * J
    cuts = sharded.balanced_prefix_cuts(torch.from_numpy(keys.view(np.int64).copy()), nbits, world, 9)
    a, b = cuts[rank], cuts[rank + 1]
    kd = torch.from_numpy(keys[a:b].view(np.int64).copy()).cuda()
    Cd = torch.from_numpy(C[a:b]).cuda()
    sh = sharded.ShardedRaht(kd, nbits, prefix_bits=9, force_collectives=force, direct=direct, n_wide=NW)
    plain = sharded.ShardedRaht(kd, nbits, prefix_bits=9, force_collectives=force, direct=direct)
    if world > 1:
        assert sh.gathered_bytes_per_step(D) == plain.gathered_bytes_per_step(D) + 2 * sh.gather_rows * NW * 8
    po = orc.raht_param(V.astype(np.float64), np.zeros(3), 2 ** J, J)
    To, _ = orc.raht_fwd(C[:, :NW].astype(np.float64), po)            # the xyz columns of the whole scene, float64
    To = To[a:b]
    ties = 0
    for step in (0.01, 1.0, PER_CHANNEL):
        chk = sh.check_mixed_against_unsharded(Cd, step, keys_sorted=kd)
        assert chk["ok"], (step, chk)
        Q = sh.forward_quant(Cd, step)
        Qp = plain.forward_quant(Cd, step)
        if b > a:
            assert torch.equal(Q[:, NW:], Qp[:, NW:]), step
            Qr = Q[sh.plan.inv_order].cpu().numpy().astype(np.int64)[:, :NW]
            sw = np.asarray(step[:NW] if isinstance(step, list) else [step] * NW, dtype=np.float64)
            ref = np.floor(To / sw + 0.5).astype(np.int64)
            x = To / sw
            tie = np.abs(x - np.floor(x) - 0.5) <= 1e-9 * np.maximum(np.abs(x), 1.0)
            diff = Qr != ref
            assert not (diff & ~tie).any(), (step, np.argwhere(diff & ~tie)[:5])
            ties += int(diff.sum())
        R = sh.dequant_inverse(Q, step)
        Rp = plain.dequant_inverse(Q, step)
        assert R.dtype == torch.float32 and tuple(R.shape) == tuple(Cd.shape)
        if b > a:
            assert torch.equal(R[:, NW:], Rp[:, NW:]), step                # the attribute columns: the float32 step's
            smax = max(step) if isinstance(step, list) else step
            assert float((R - Cd).abs().max()) <= smax * np.sqrt(sh.total_rows)
    for _ in range(3):
        sh.step(Cd, 0.01)
        sh.local_step(Cd, 0.01)
    if direct:
        assert sh.exchange_status() == 0
        sh.close()
        plain.close()
    return ties


def _gloo_main(rank, world, direct):
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    ties = _check_rank(rank, world, 10, 240000, 61, direct, direct)
    dist.barrier()
    return ties


def _spawn(target, world, *args, backend="gloo"):
    ties = run_ranks(target, world, *args, backend=backend, report_timeout=600, join_timeout=120)
    print("near-tie differences on the xyz columns per rank:", ties)


@pytest.mark.parametrize("world", [4, 5])
def test_mixed_sharded_gloo_ranks_share_the_gpu(rt, world):
    _spawn(_gloo_main, world, False)


def test_mixed_sharded_direct_exchange(rt):
    _spawn(_gloo_main, 3, True)


def _rccl_main(rank, world):
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    from raht_3dgs_codec_amd import sharded
    ties = _check_rank(0, 1, 11, 300000, 67, True, False)
    # the mixed step's collective time covers both gathers of a direction
    from raht_3dgs_codec_amd import synth
    _, keys, C = synth.scene(100000, 11, D, seed=5)
    kd = torch.from_numpy(keys.view(np.int64).copy()).cuda()
    sh = sharded.ShardedRaht(kd, 33, prefix_bits=9, force_collectives=True, n_wide=NW)
    Cd = torch.from_numpy(C).cuda()
    sh.step(Cd, 0.01)
    sh.time_collectives(True)
    for _ in range(3):
        sh.step(Cd, 0.01)
    assert len(sh._ev["fwd"]) == 3 and len(sh._ev["inv"]) == 3
    f, i = sh.collective_ms()
    assert f > 0 and i > 0
    t = torch.ones(4, device="cuda")
    dist.all_reduce(t); dist.barrier()
    torch.cuda.synchronize()
    return ties


def test_mixed_sharded_one_rank_rccl_group(rt):
    _spawn(_rccl_main, 1, backend="nccl")
