"""A frame as self-contained bytes: geometry (geometry.OctreeCoder) + quantized RAHT coefficients (rlgr.SegmentedCoder) + the few
numbers a decoder needs. ``decode_frame_bytes`` is handed nothing but the blob: it rebuilds the voxel keys, builds its own plan
from them and runs the inverse kernels that match the encoder's. ``decode_region_bytes`` rebuilds the voxels of a run of octree
cells from the geometry and the attribute segments those voxels depend on.

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
    return _frame_blob(J, N, D, n_wide, steps, vmin, width, geo, att)


def _frame_blob(J, N, D, n_wide, steps, vmin, width, geo, att):
    box = [0.0, 0.0, 0.0] if vmin is None else [float(x) for x in vmin]
    if len(box) != 3:
        raise ValueError("encode_frame_bytes: vmin must have 3 entries")
    box.append(0.0 if width is None else float(width))
    return (MAGIC + np.array([J, N, D, n_wide, len(steps)], np.int64).tobytes() + np.array(steps + box, np.float64).tobytes()
            + np.array([len(geo)], np.int64).tobytes() + geo + np.array([len(att)], np.int64).tobytes() + att)


def encode_frame_bytes_target(V_int, attributes, J, target_bytes, step=1.0, scale_range=(2 ** -10, 2 ** 10), rounds=3, n_wide=0,
                              seg_len=2048, geometry="rlgr", vmin=None, width=None, device="cuda"):
    """A frame in at most ``target_bytes`` bytes: the quantization table is ``step * m`` (``step``: a scalar or one entry per column)
    and the multiplier m is the smallest the search finds inside ``scale_range`` whose frame fits. The geometry is coded once; every
    round asks ``RahtPlan.rate_curve`` for the exact attribute bytes at ``SegmentedCoder.RATE_MAX`` geometrically spaced multipliers
    (one transform, one read of the coefficients, nothing coded), takes the smallest that fits and narrows the bracket to
    (the next finer grid point, that one]. RLGR sizes need not be monotone in the step: taking a grid point that was SEEN to fit
    keeps the result valid whatever the curve looks like. The frame is then coded by the ordinary path at the chosen table and its
    length checked; should it not fit (it cannot while the sizes are exact), the next coarser multiplier that was tried is taken.
    -> (blob, info): an ordinary RAHTF001 frame for ``decode_frame_bytes``; info: multiplier, steps, predicted_attribute_bytes,
    attribute_bytes, tried (every (multiplier, bytes) in evaluation order), sse (float64 [D] at the chosen point).
    ``ValueError`` when the geometry alone exceeds the target or not even the coarsest multiplier fits."""
    import torch
    from . import ops
    dev = torch.device(device)
    J = int(J)
    target = int(target_bytes)
    V = torch.as_tensor(V_int).to(dev, torch.int64)
    A = torch.as_tensor(attributes).to(dev, torch.float32)
    if V.dim() != 2 or V.shape[1] != 3 or A.dim() != 2 or A.shape[0] != V.shape[0] or V.shape[0] < 1:
        raise ValueError("encode_frame_bytes_target: expected (N, 3) coordinates and (N, D) attributes, N >= 1")
    if not 1 <= J <= MAX_J:
        raise ValueError("encode_frame_bytes_target: J outside 1 .. 21")
    N, D = A.shape
    n_wide = int(n_wide)
    if not 0 <= n_wide <= D:
        raise ValueError("encode_frame_bytes_target: n_wide outside 0 .. D")
    base = _step_list(SegmentedCoder.step_row(step), D)                  # (any scalar or sequence, as rate and rate_curve take them)
    lo, hi = float(scale_range[0]), float(scale_range[1])
    if not (math.isfinite(lo) and math.isfinite(hi) and 0 < lo <= hi) or int(rounds) < 1:
        raise ValueError("encode_frame_bytes_target: scale_range must be 0 < lo <= hi, rounds >= 1")
    K = SegmentedCoder.RATE_MAX
    with torch.cuda.device(dev):
        keys = ops.get_morton_code(V, J)
        geo = OctreeCoder.encode(keys, J, entropy=geometry)               # (also refuses rows that are not sorted and unique)
        # the frame around the attribute container: header, steps + box, the geometry section and the two length words
        budget = target - (len(MAGIC) + 40 + 8 * (len(base) + 4)) - (8 + len(geo)) - 8
        if budget < 0:
            raise ValueError(f"encode_frame_bytes_target: the geometry section and the header alone take {target - budget} bytes, target {target}")
        plan = ops.RahtPlan.from_keys(keys, 3 * J)
        tried, sse_of, fits = [], {}, {}
        chosen = None
        for rnd in range(int(rounds)):
            if rnd == 0:                                                 # the whole range, both ends included
                grid = [lo] if hi == lo else [lo * (hi / lo) ** (i / (K - 1)) for i in range(K - 1)] + [hi]
            else:                                                        # strictly inside (lo, hi): lo did not fit, hi = chosen did
                grid = [lo * (hi / lo) ** ((i + 1) / (K + 1)) for i in range(K)]
            rc = plan.rate_curve(A, [[s * m for s in base] for m in grid], n_wide, seg_len)
            for m, nb, e in zip(grid, rc["bytes"], rc["sse"]):
                tried.append((m, int(nb)))
                sse_of[m] = e
                fits[m] = int(nb) <= budget
            ok = [i for i, m in enumerate(grid) if fits[m]]
            if not ok:
                break                                                    # round 0: nothing fits at all; later: hi stays the answer
            i = ok[0]
            chosen = grid[i]
            if i == 0 and rnd == 0:
                break                                                    # the finest multiplier of the range fits
            lo, hi = (grid[i - 1] if i else lo), chosen
            if not lo < hi:
                break
        if chosen is None:
            raise ValueError(f"encode_frame_bytes_target: no multiplier in [{scale_range[0]}, {scale_range[1]}] brings the attributes "
                             f"below {budget} bytes (smallest seen: {min(b for _, b in tried)})")
        predicted = dict(tried)
        # the candidates that were seen to fit, from the chosen one towards coarser steps
        for m in sorted(x for x in fits if fits[x] and x >= chosen):
            steps = [s * m for s in base]
            Q = plan.forward_quant_mixed(A, steps, n_wide) if n_wide else plan.forward_quant(A, steps)
            sc = SegmentedCoder(N, D, seg_len, 1, dev)
            sc.encode(Q)
            att = sc.container()
            blob = _frame_blob(J, N, D, n_wide, steps, vmin, width, geo, att)
            if len(blob) <= target:
                info = dict(multiplier=m, steps=steps, predicted_attribute_bytes=predicted[m], attribute_bytes=len(att), tried=tried,
                            sse=sse_of[m])
                return blob, info
    raise ValueError("encode_frame_bytes_target: no candidate that was predicted to fit did fit")


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


def region_runs(table, J, depth, n_roots):
    """Where a region lies in the coded order of its frame, from the three bucket histograms of ``ops.region_layout`` (host
    integers, (3, 22): whole frame, rows before the region, rows inside it) -> (n_top, runs). The first ``n_top`` coded rows are the
    tree above ``depth`` (row 0 and every row of a bucket >= J - depth); ``runs`` holds one (coded row, row of the region's own coded
    matrix, count) per finer bucket that has rows in the region, coarse to fine. The region's matrix starts with its ``n_roots``
    root slots (one per occupied cell)."""
    whole, before, inside = table
    cut = int(J) - int(depth)
    n_top = int(sum(whole[cut:]))
    coded, dst, runs = n_top, int(n_roots), []
    for beta in range(cut - 1, -1, -1):
        if inside[beta]:
            runs.append((coded + int(before[beta]), dst, int(inside[beta])))
        coded += int(whole[beta])
        dst += int(inside[beta])
    return n_top, runs


def region_segments(n_top, runs, seg_len):
    """-> (seg_ids, compact): the ascending segment indices that hold the coded rows [0, n_top) and the runs, and the map from a
    coded row inside them to its row of the matrix those segments decode to"""
    S = int(seg_len)
    spans = [(0, n_top)] + [(r, r + n) for r, _, n in runs]
    ids = np.unique(np.concatenate([np.arange(lo // S, (hi - 1) // S + 1) for lo, hi in spans]))

    def compact(row):
        return int(np.searchsorted(ids, row // S)) * S + row % S
    return ids, compact


def decode_region_bytes(blob, depth, cells, device="cuda", max_voxels=None, keys=None):
    """The voxels of the octree cells ``cells = (c0, c1)`` (Morton indices at ``depth``, 1 <= depth <= J - 1, 0 <= c0 < c1 <=
    8^depth) of a frame, from the geometry and the attribute segments they depend on -> (V_int (n, 3) int64, C_rec (n, D) float32,
    info): rows [a, b) of what ``decode_frame_bytes`` returns, up to the rounding of the tree above ``depth``, which the two
    decoders compute in different launches. ``keys``: ``info["keys"]`` of an earlier call on the same frame; the geometry is then
    not decoded again. info: rows (a, b), n_cells (occupied cells in the range), segments_decoded / segments_total (per channel),
    byte_ranges ((offset, length) within ``blob``: everything outside them may be missing) and bytes_needed, geometry_decoded,
    keys. No N x D matrix is allocated: the only full-length arrays are the keys and the cell search's flags.
    ``ValueError`` for a corrupt frame or arguments outside the ranges above."""
    import torch
    from . import ops
    h = parse_frame(blob, max_voxels)
    J, N, D, n_wide, steps = h["J"], h["N"], h["D"], h["n_wide"], h["steps"]
    try:
        depth, (c0, c1) = int(depth), (int(c) for c in cells)
    except (TypeError, ValueError):
        raise ValueError("decode_region_bytes: depth is an integer, cells a pair of integers") from None
    if not 1 <= depth <= J - 1:
        raise ValueError(f"decode_region_bytes: depth must be 1 .. J - 1 = {J - 1}")
    if not 0 <= c0 < c1 <= 8 ** depth:
        raise ValueError(f"decode_region_bytes: cells must satisfy 0 <= c0 < c1 <= 8^depth = {8 ** depth}")
    dev = torch.device(device)
    (go, gl), (ao, al) = h["geometry"], h["attributes"]
    view = memoryview(blob)
    n_d = OctreeCoder.parse(view[go: go + gl], max_voxels)["counts"][depth]
    att = view[ao: ao + al]
    _, _, S, _, _, _, pay = SegmentedCoder._parse(att, N * D)
    nseg = (N + S - 1) // S
    ranges = [(0, ao + pay)]                                              # frame header, geometry section, attribute header + table
    if keys is not None:
        if not isinstance(keys, torch.Tensor) or not keys.is_cuda or keys.dtype != torch.int64 or tuple(keys.shape) != (N,):
            raise ValueError(f"decode_region_bytes: keys must be the ({N},) int64 CUDA tensor an earlier call returned")
        keys = keys.contiguous()
    tl = 3 * (J - depth)
    with torch.cuda.device(dev):
        decoded = keys is None
        if decoded:
            keys = OctreeCoder.decode(view[go: go + gl], dev, max_voxels)
        try:
            cell_keys, cell_first = ops.region_cells(keys, 3 * J, tl, n_d)
        except ops.RahtError as e:
            raise ValueError(f"decode_region_bytes: the keys are not this frame's ({e})") from None
        j = torch.searchsorted(cell_keys, torch.tensor([c0, c1], dtype=torch.int64, device=dev))
        j0, j1, a, b = torch.cat([j, cell_first[j]]).tolist()
        info = dict(rows=(a, b), n_cells=j1 - j0, segments_decoded=0, segments_total=nseg, byte_ranges=ranges,
                    bytes_needed=ranges[0][1], geometry_decoded=decoded, keys=keys)
        if j0 == j1:
            return (torch.empty((0, 3), dtype=torch.int64, device=dev), torch.empty((0, D), dtype=torch.float32, device=dev), info)
        n_top, runs = region_runs(ops.region_layout(keys, 3 * J, a, b).tolist(), J, depth, j1 - j0)
        if n_top != n_d:
            raise ValueError("decode_region_bytes: the keys are not this frame's")
        seg_ids, compact = region_segments(n_top, runs, S)
        sc, att_ranges = SegmentedCoder.from_container_segments(att, seg_ids, dev, max_symbols=N * D)
        Qc = sc.decode(row_major=True)
        # the tree above `depth`: a weighted plan over the occupied cells; its inverse gives every cell's low-pass row
        top = ops.RahtPlan.from_keys(cell_keys, 3 * depth, leaf_weights=cell_first[1:] - cell_first[:-1])
        roots = top.dequant_inverse(Qc[:n_top], steps)[j0:j1]
        # the region: a plan truncated at the cells over its own rows, its coded matrix put together from the decoded runs
        plan = ops.RahtPlan.from_keys(keys[a:b], 3 * J, top_level=tl)
        Qr = ops.region_assemble(Qc, [(compact(r), d, n) for r, d, n in runs], b - a)
        if n_wide:
            wide = top.dequant_inverse(Qc[:n_top, :n_wide], steps[:n_wide], dtype=torch.float64)[j0:j1]
            C_rec = plan.dequant_inverse_mixed(Qr, steps, n_wide, roots=roots.contiguous(), roots_wide=wide.contiguous())
        else:
            C_rec = plan.dequant_inverse(Qr, steps, roots=roots.contiguous())
        V = ops.demorton(keys[a:b], J)
        if int(sc.bad.item()) != 0:
            raise ValueError("frame container: an attribute segment reaches outside its payload")
    ranges = [(0, ao)]                                                    # frame header, geometry section, the attributes' length word
    for off, ln in att_ranges:                                            # the first: header + table (+ the slots that follow them)
        if ranges[-1][0] + ranges[-1][1] == ao + off:
            ranges[-1] = (ranges[-1][0], ranges[-1][1] + ln)
        else:
            ranges.append((ao + off, ln))
    info.update(segments_decoded=len(seg_ids), byte_ranges=ranges, bytes_needed=sum(ln for _, ln in ranges))
    return V, C_rec, info
