"""Whole frames through bitstream.encode_frame_bytes / decode_frame_bytes: the blob is written to a file and decoded by a FRESH
child process that is given nothing but that file, so nothing can leak through Python state. What comes back must be the
coordinates that went in and, bit for bit, what dequant_inverse*(forward_quant*(C, step), step) gives on a plan made from the
coordinates the usual way; the attribute part of the blob must be SegmentedCoder.container() of the same integers."""
import os
import subprocess
import sys

import numpy as np
import pytest

from .conftest import ROOT

pytestmark = pytest.mark.gpu

CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import torch
from raht_3dgs_codec_amd import bitstream
blob = open(sys.argv[2], "rb").read()
V, C = bitstream.decode_frame_bytes(blob, "cuda", max_voxels=int(sys.argv[4]))
torch.cuda.synchronize()
np.savez(sys.argv[3], V=V.cpu().numpy(), C=C.cpu().numpy())
"""

# (draws, J, D, n_wide, per-channel steps)
CASES = [(300, 6, 56, 0, False), (300, 6, 59, 3, True), (20_000, 10, 56, 0, False), (20_000, 10, 56, 0, True), (20_000, 10, 59, 3, False),
         (20_000, 10, 59, 3, True), (1_000_000, 10, 56, 0, True), (1_000_000, 10, 59, 3, False)]


def _steps(D, per_channel):
    return [0.004 * (1 + (c % 7)) for c in range(D)] if per_channel else 0.01


def _decode_in_child(tmp_path, blob, max_voxels):
    src, out = str(tmp_path / "frame.bin"), str(tmp_path / "decoded.npz")
    with open(src, "wb") as f:
        f.write(blob)
    r = subprocess.run([sys.executable, "-c", CHILD, ROOT, src, out, str(max_voxels)], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    os.remove(src)
    return z["V"], z["C"]


@pytest.mark.parametrize("draws, J, D, n_wide, per_channel", CASES)
def test_frame_round_trip_through_a_file_and_a_fresh_process(tmp_path, draws, J, D, n_wide, per_channel):
    import torch
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import bitstream, synth
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    V, keys, C = synth.scene(draws, J, D, seed=31 + D)
    N = V.shape[0]
    steps = _steps(D, per_channel)
    blob = bitstream.encode_frame_bytes(V, C, J, steps, "cuda", n_wide=n_wide, vmin=(-1.5, 0.25, 3.0), width=12.5)
    h = bitstream.parse_frame(blob)
    assert (h["J"], h["N"], h["D"], h["n_wide"], h["vmin"], h["width"]) == (J, N, D, n_wide, [-1.5, 0.25, 3.0], 12.5)
    assert h["steps"] == ([float(s) for s in steps] if per_channel else [0.01])
    # the reference computation, on a plan made from the coordinates
    plan = R.RahtPlan.from_coords(torch.from_numpy(V.astype(np.float64)).cuda(), [0.0, 0.0, 0.0], 2 ** J, J)
    Cd = torch.from_numpy(C).cuda()
    if n_wide:
        Q = plan.forward_quant_mixed(Cd, steps, n_wide)
        want = plan.dequant_inverse_mixed(Q, steps, n_wide)
    else:
        Q = plan.forward_quant(Cd, steps)
        want = plan.dequant_inverse(Q, steps)
    sc = SegmentedCoder(N, D, 2048, 1, "cuda")
    sc.encode(Q)
    ao, al = h["attributes"]
    assert blob[ao: ao + al] == sc.container()
    Vout, Cout = _decode_in_child(tmp_path, blob, N)
    assert Vout.dtype == np.int64 and np.array_equal(Vout, V)
    assert Cout.dtype == np.float32 and Cout.shape == (N, D)
    assert np.array_equal(Cout.view(np.int32), want.cpu().numpy().view(np.int32))          # bit-identical
    # and in this process, raw geometry: the same frame
    blob0 = bitstream.encode_frame_bytes(V, C, J, steps, "cuda", n_wide=n_wide, geometry="raw")
    V0, C0 = bitstream.decode_frame_bytes(blob0, "cuda")
    assert np.array_equal(V0.cpu().numpy(), V) and torch.equal(C0, want)
    assert len(blob) <= len(blob0) or N < 5000


def test_frames_the_decoder_refuses(tmp_path):
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import bitstream, synth
    V, keys, C = synth.scene(5000, 8, 56, seed=2)
    blob = bitstream.encode_frame_bytes(V, C, 8, 0.02, "cuda", geometry="raw")
    h = bitstream.parse_frame(blob)
    go, gl = h["geometry"]
    with pytest.raises(ValueError):
        bitstream.decode_frame_bytes(blob, "cuda", max_voxels=V.shape[0] - 1)
    with pytest.raises(ValueError):
        bitstream.decode_frame_bytes(blob[:-5], "cuda")
    zeroed = bytearray(blob)
    zeroed[go + gl - 7] = 0                                           # an occupancy byte of the finest internal level
    with pytest.raises(ValueError):
        bitstream.decode_frame_bytes(bytes(zeroed), "cuda")
    with pytest.raises(R.RahtError):                                  # rows that are not in Morton order are refused by the encoder
        bitstream.encode_frame_bytes(V[::-1].copy(), C, 8, 0.02, "cuda")
    Vd, Cd = bitstream.decode_frame_bytes(blob, "cuda")
    assert np.array_equal(Vd.cpu().numpy(), V)
