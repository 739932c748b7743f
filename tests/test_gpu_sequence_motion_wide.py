"""One motion-compensated sequence at D = 80, where raht_motion_search takes its 128-row tile (raht_debug_motion_tile), with blocks
of 4 voxels a side: the five-frame moving cloud of tests/test_gpu_sequence_motion.py, by the recipe of its closed-loop test -- the
encoder's recurrence with public calls ends on the decoder's bits."""
import numpy as np
import pytest

from .test_gpu_sequence_motion import FRAMES, J, STEP, _coded

pytestmark = pytest.mark.gpu

D, N_WIDE, BLOCK = 80, 3, 2                                              # n_wide: what the suite's 59-column shape uses
MOVING = dict(gop=FRAMES, inter="always", motion=1, block_log2=BLOCK)


def test_the_closed_loop_ends_on_the_decoders_bits_at_128_rows_per_tile():
    import torch
    from raht_3dgs_codec_amd import _lib, bitstream, ops
    assert _lib.lib().raht_debug_motion_tile(D) == 128 and (J, FRAMES) == (6, 5)
    frames, blob, dec = _coded("moving", D, N_WIDE, **MOVING)
    assert bitstream.sequence_kinds(blob) == ["I"] + ["P"] * (FRAMES - 1) and len(dec) == FRAMES
    motion = bitstream.sequence_motion(blob)
    assert motion[0] is None
    fields = [mo[1] for mo in motion[1:] if mo is not None]
    assert fields and any(np.asarray(mv).any() for mv in fields)         # a non-zero field: the search's choice is in the loop
    assert all(mo[0] == BLOCK for mo in motion[1:] if mo is not None)
    w = np.full(D, 1.0 / STEP).astype(np.float32)
    ref = None
    for i, (V, A) in enumerate(frames):
        keys = ops.get_morton_code(torch.from_numpy(V).cuda(), J)
        plan = ops.RahtPlan.from_keys(keys, 3 * J)
        X = torch.from_numpy(A).cuda()
        field = ref is not None and motion[i] is not None
        if ref is not None:
            bf = ops.motion_blocks(keys, J, BLOCK, len(motion[i][1]) if field else len(np.unique(keys.cpu().numpy() >> (3 * BLOCK))))
            mv, _ = ops.motion_search(keys, ref[0], ref[1], X, J, BLOCK, bf, ops.motion_candidates(1), w)
            if field:
                assert np.array_equal(mv.cpu().numpy(), motion[i][1]), i   # the field in the wrapper is the search's
            else:
                assert not bool(mv.any()), i                             # no field in the wrapper: the search found no motion
            X = ops.predict_mc(keys, ref[0], ref[1], mv, bf, J, BLOCK, X=X)
        C = plan.dequant_inverse_mixed(plan.forward_quant_mixed(X, [STEP], N_WIDE), [STEP], N_WIDE)
        if ref is not None:
            C = ops.predict_mc(keys, ref[0], ref[1], mv, bf, J, BLOCK, X=C, add=True)
        assert torch.equal(C.view(torch.int32), dec[i][1].view(torch.int32)), i
        ref = (keys, C)
    assert torch.equal(ref[1].view(torch.int32), dec[-1][1].view(torch.int32))
    # the loop is closed: the reconstruction is the input up to the quantizer of the LAST frame alone (tests/test_gpu_sequence_inter.py
    # has the bound's derivation: an orthonormal transform, half a step per coefficient, 1e-4 per element for float32 rounding)
    N = len(frames[-1][0])
    err = (ref[1].cpu() - torch.from_numpy(frames[-1][1])).norm(dim=0)
    assert float(err.max()) <= (0.5 * STEP + 1e-4) * N ** 0.5
