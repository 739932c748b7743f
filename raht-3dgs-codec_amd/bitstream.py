"""A frame as self-contained bytes: geometry (geometry.OctreeCoder) + quantized RAHT coefficients (rlgr.SegmentedCoder) + the few
numbers a decoder needs. ``decode_frame_bytes`` is handed nothing but the blob: it rebuilds the voxel keys, builds its own plan
from them and runs the inverse kernels that match the encoder's.

    RAHTF001 | int64 J, N, D, n_wide, n_steps | float64 steps[n_steps] | float64 vmin[3], width |
    int64 length + geometry section | int64 length + attribute container (SegmentedCoder.container())

``n_wide = 0``: ``forward_quant`` / ``dequant_inverse`` (float32; the float64 steps of the header are cast to float32 on both
sides, as ``ops._steps`` does). ``n_wide = 3``: ``forward_quant_mixed`` / ``dequant_inverse_mixed`` (float64 steps), for 59-column
frames whose first three columns are xyz. ``vmin`` / ``width`` are metadata (the voxel grid's box; 0 when not given).
"""
import math

import numpy as np

from .geometry import MAX_J, OctreeCoder
from .rlgr import SegmentedCoder

MAGIC = b"RAHTF001"


def _step_list(step, D):
    if isinstance(step, (int, float)):
        step = [step]
    steps = [float(s) for s in step]
    if len(steps) not in (1, D):
        raise ValueError("step must be a scalar or have one entry per attribute column")
    if any(not (math.isfinite(s) and s > 0) for s in steps):
        raise ValueError("steps must be finite and positive")
    return steps


def encode_frame_bytes(V_int, attributes, J, step, device="cuda", n_wide=0, seg_len=2048, geometry="rlgr", vmin=None, width=None):
    """V_int: (N, 3) integer voxel coordinates in Morton order, no voxel twice (what the voxelizer yields); attributes: (N, D)
    float32; numpy arrays or tensors. -> bytes. Raises RahtError when the rows are not in strictly ascending Morton order."""
    import torch
    from . import ops
    dev = torch.device(device)
    J = int(J)
    V = torch.as_tensor(V_int).to(dev, torch.int64)
    A = torch.as_tensor(attributes).to(dev, torch.float32)
    if V.dim() != 2 or V.shape[1] != 3 or A.dim() != 2 or A.shape[0] != V.shape[0] or V.shape[0] < 1:
        raise ValueError("encode_frame_bytes: expected (N, 3) coordinates and (N, D) attributes, N >= 1")
    if not 1 <= J <= MAX_J:
        raise ValueError("encode_frame_bytes: J outside 1 .. 21")
    N, D = A.shape
    n_wide = int(n_wide)
    if not 0 <= n_wide <= D:
        raise ValueError("encode_frame_bytes: n_wide outside 0 .. D")
    steps = _step_list(step, D)
    with torch.cuda.device(dev):
        keys = ops.get_morton_code(V, J)
        geo = OctreeCoder.encode(keys, J, entropy=geometry)               # (also refuses rows that are not sorted and unique)
        plan = ops.RahtPlan.from_keys(keys, 3 * J)
        Q = plan.forward_quant_mixed(A, steps, n_wide) if n_wide else plan.forward_quant(A, steps)
        sc = SegmentedCoder(N, D, seg_len, 1, dev)
        sc.encode(Q)
        att = sc.container()
    box = [0.0, 0.0, 0.0] if vmin is None else [float(x) for x in vmin]
    if len(box) != 3:
        raise ValueError("encode_frame_bytes: vmin must have 3 entries")
    box.append(0.0 if width is None else float(width))
    return (MAGIC + np.array([J, N, D, n_wide, len(steps)], np.int64).tobytes() + np.array(steps + box, np.float64).tobytes()
            + np.array([len(geo)], np.int64).tobytes() + geo + np.array([len(att)], np.int64).tobytes() + att)


def parse_frame(blob, max_voxels=None):
    """The header of a frame container, checked against the blob (pure Python, nothing allocated on a device) -> dict: J, N, D,
    n_wide, steps, vmin, width, geometry (offset, length), attributes (offset, length). ``ValueError`` when it does not add up."""
    m = len(MAGIC)
    if bytes(blob[:m]) != MAGIC:
        raise ValueError("not a RAHT frame container")
    if len(blob) < m + 40:
        raise ValueError("frame container: truncated header")
    J, N, D, n_wide, n_steps = [int(x) for x in np.frombuffer(blob, np.int64, 5, m)]
    if not (1 <= J <= MAX_J and 1 <= N < 2 ** 31 and 1 <= D <= 65536 and 0 <= n_wide <= D and n_steps in (1, D)):
        raise ValueError("frame container: implausible header")
    if max_voxels is not None and N > int(max_voxels):
        raise ValueError(f"frame container: {N} voxels, more than the caller allows ({max_voxels})")
    pos = m + 40
    if len(blob) < pos + 8 * (n_steps + 4) + 8:
        raise ValueError("frame container: shorter than its header says")
    nums = [float(x) for x in np.frombuffer(blob, np.float64, n_steps + 4, pos)]
    steps = nums[:n_steps]
    if any(not (math.isfinite(s) and s > 0) for s in steps):
        raise ValueError("frame container: a quantization step is not a positive number")
    pos += 8 * (n_steps + 4)
    parts = []
    for what in ("geometry section", "attribute container"):
        if len(blob) < pos + 8:
            raise ValueError(f"frame container: the {what} is missing")
        ln = int(np.frombuffer(blob, np.int64, 1, pos)[0])
        if ln < 48 or ln > len(blob) - pos - 8:
            raise ValueError(f"frame container: the {what} is shorter than its length says")
        parts.append((pos + 8, ln))
        pos += 8 + ln
    (go, gl), (ao, al) = parts
    g = OctreeCoder.parse(blob[go: go + gl], max_voxels)
    if (g["J"], g["N"]) != (J, N) or g["length"] != gl:
        raise ValueError("frame container: the geometry section is not the one the header announces")
    am = len(SegmentedCoder.MAGIC)
    if bytes(blob[ao: ao + am]) != SegmentedCoder.MAGIC or [int(x) for x in np.frombuffer(blob, np.int64, 2, ao + am)] != [N, D]:
        raise ValueError("frame container: the attribute container is not the one the header announces")
    return dict(J=J, N=N, D=D, n_wide=n_wide, steps=steps, vmin=nums[n_steps: n_steps + 3], width=nums[n_steps + 3],
                geometry=(go, gl), attributes=(ao, al))


def decode_frame_bytes(blob, device="cuda", max_voxels=None):
    """-> (V_int (N, 3) int64, C_rec (N, D) float32), CUDA tensors on ``device``, from the bytes alone. ``max_voxels``: refuse
    frames that announce more voxels than this before anything is allocated for them. ``ValueError`` for a corrupt frame."""
    import torch
    from . import ops
    h = parse_frame(blob, max_voxels)
    dev = torch.device(device)
    (go, gl), (ao, al) = h["geometry"], h["attributes"]
    with torch.cuda.device(dev):
        keys = OctreeCoder.decode(blob[go: go + gl], dev, max_voxels)
        V = ops.demorton(keys, h["J"])
        plan = ops.RahtPlan.from_keys(keys, 3 * h["J"])
        sc = SegmentedCoder.from_container(blob[ao: ao + al], dev, max_symbols=h["N"] * h["D"])
        Q = sc.decode(row_major=True)
        steps = h["steps"]
        C_rec = plan.dequant_inverse_mixed(Q, steps, h["n_wide"]) if h["n_wide"] else plan.dequant_inverse(Q, steps)
        if int(sc.bad.item()) != 0:
            raise ValueError("frame container: an attribute segment reaches outside its payload")
    return V, C_rec
