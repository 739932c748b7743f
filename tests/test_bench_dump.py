"""bench.py --dump-outputs DIR: what the timed path computed in its last step, as DIR/<name>.npy, so that two builds can be
compared output for output on identical inputs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_is_a_fixed_sample_under_the_size_cap(tmp_path):
    import torch
    b = _bench_module()
    g = torch.Generator().manual_seed(1)
    big = {"Q": torch.randint(-1000, 1000, (3_000_000, 59), dtype=torch.int32, generator=g),
           "C_rec": torch.randn((3_000_000, 59), generator=g)}
    small = torch.arange(12, dtype=torch.float64).reshape(4, 3)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), dict(big, T=small))
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["C_rec.npy", "Q.npy", "T.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and x.dtype == y.dtype and np.array_equal(x, y)
    assert np.load(tmp_path / "a" / "C_rec.npy").dtype == np.float32
    assert np.load(tmp_path / "a" / "Q.npy").dtype == np.float64
    assert np.array_equal(np.load(tmp_path / "a" / "T.npy"), small.numpy())          # small outputs whole
    q = np.load(tmp_path / "a" / "Q.npy")
    assert 0 < q.shape[0] < 3_000_000 and q.shape[1] == 59
    assert np.all(q == np.round(q)) and np.abs(q).max() <= 1000                         # integers carried exactly


def test_steps_below_one_are_refused():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120, cwd=ROOT)
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    """Two runs with the same arguments write the same arrays, and they are what the step's own kernels give on the scene:
    the quantized integers of the fused forward and the reconstruction decoded from them."""
    import torch
    assert torch.cuda.is_available(), "this test needs the MI355X"
    args = ["--gpus", "1", "--workload", "cfg2", "--rows", "200000", "--steps", "3", "--warmup", "1", "--settle-steps", "0",
            "--skip-legs", "--skip-prelude", "--skip-cpu-baseline"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    outs = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-4000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        outs.append(json.loads(lines[0]))
    assert outs[0]["steps"] == 3 and outs[0]["ms_per_step"] > 0
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["C_rec.npy", "Q.npy"] and sorted(os.listdir(tmp_path / "b")) == files
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for f in files:
        assert np.array_equal(got[f[:-4]], np.load(tmp_path / "b" / f))

    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import synth
    _, J, D, seed = synth.CONFIGS["cfg2"]
    V, keys, C = synth.scene(200000, J, D, seed)
    assert got["Q"].shape == C.shape and got["C_rec"].shape == C.shape             # under the cap: whole arrays
    plan = R.RahtPlan.from_keys(torch.from_numpy(keys.view(np.int64)).cuda(), 3 * J)
    plan.set_engine("tile", 0, 0, 0, 0)
    Cd = torch.from_numpy(C).cuda()
    mixed = outs[0]["dtype"].startswith("f32 (xyz")
    Q = plan.forward_quant_mixed(Cd, 0.01, 3) if mixed else plan.forward_quant(Cd, 0.01)
    Crec = plan.dequant_inverse_mixed(Q, 0.01, 3) if mixed else plan.dequant_inverse(Q, 0.01)
    torch.cuda.synchronize()
    assert np.array_equal(got["Q"], Q.cpu().numpy().astype(np.float64))
    assert np.array_equal(got["C_rec"], Crec.cpu().numpy())
