"""A frame as self-contained bytes: geometry (geometry.OctreeCoder) + quantized RAHT coefficients (rlgr.SegmentedCoder) + the few
numbers a decoder needs. ``decode_frame_bytes`` is handed nothing but the blob: it rebuilds the voxel keys, builds its own plan
from them and runs the inverse kernels that match the encoder's. ``decode_region_bytes`` rebuilds the voxels of a run of octree
cells from the geometry and the attribute segments those voxels depend on.

    RAHTF001 | int64 J, N, D, n_wide, n_steps | float64 steps[n_steps] | float64 vmin[3], width |
    int64 length + geometry section | int64 length + attribute container (SegmentedCoder.container())

A SEQUENCE of frames (a different voxel count in every frame) is a container OF such frames: every frame is an ordinary RAHTF001
blob -- ``sequence_frame`` hands out its slice, and ``decode_frame_bytes`` / ``decode_region_bytes`` work on it -- coded and decoded
with the transform and entropy stages of all frames in common launches:

    RAHTS001 | int64 n_frames | int64 offset[n_frames + 1] (from the start of the blob) | the frames

Inside a sequence a frame may be PREDICTED from the reconstruction of an earlier one (``encode_sequence_bytes(..., gop, up,
inter)``): a wrapper around an ordinary frame whose attributes are the residual ``A - P``, P being ``ops.predict`` of
the reference's reconstruction (the mean of the reference voxels in the same cell ``up`` octree levels above the voxels; ``up = 0``:
the co-located voxel). ``decode_frame_bytes`` / ``decode_region_bytes`` refuse the wrapper; ``decode_sequence_bytes`` resolves it,
and ``decode_sequence_region`` resolves it for a range of cells of the frame, from the cells of the chain's frames that the
prediction reaches into (``decode_cells_bytes``: a frame's region made of several cell ranges).

    RAHTP001 | int64 ref_back (>= 1: the reference is ref_back frames earlier; this version writes 1) | int64 up (0 .. 3) |
    a whole RAHTF001 frame

With ``motion`` > 0 the prediction may follow a MOTION FIELD: one integer vector per occupied block of
``2^block_log2`` voxels a side, found by ``ops.motion_search`` against the reference's reconstruction; P is then
``ops.predict_mc``. Such a frame is still a predicted frame (kind "P"); ``sequence_motion`` hands out its field.

    RAHTM001 | int64 ref_back | int64 up | int64 block_log2 | int64 n_blocks | int8 mv[n_blocks][3] | zero bytes up to a
    multiple of 8 | a whole RAHTF001 frame

With ``motion_levels`` > 0 the field is found coarse to fine (``ops.motion_search_hier``) and may hold vectors of up
to 31 voxels a component; the container and the decoders are the same.

With ``geometry_inter`` the GEOMETRY of such a frame may be predicted as well: its geometry section is then an
``OCTP0001`` one, coded against the keys of the frame its wrapper names; ``sequence_geometry`` tells which frames do that, and the
decoders of a single frame take those keys as ``ref_keys``.

With ``bframes`` > 0 a frame between two coded frames may be a B FRAME: predicted from both (``ops.predict_bi``:
the mean of the two one-reference predictions where both references have voxels in the cell, the one that has where only one
has), optionally under one motion field per reference, and never a reference itself -- ``decode_sequence_bytes(blob,
frames=anchors)`` never touches its bytes. ``sequence_plan`` has the structure, ``sequence_refs`` reads it back.

    RAHTB001 | int64 ref_back (>= 1) | int64 ref_fwd (>= 1: reference 1 is ref_fwd frames LATER) | int64 up | int64 block_log2
    (0: no fields) | int64 n_blocks (0 iff block_log2 == 0) | with fields: int8 mv0[n_blocks][3], zero bytes up to a multiple of 8,
    int8 mv1[n_blocks][3], padded likewise | a whole RAHTF001 frame

With ``block_modes`` every occupied block of a B frame picks its own predictor (``ops.mode_search``): 0 the rule
above, 1 reference 0 alone, 2 reference 1 alone, 3 none. A frame in which some block chooses another mode than 0 is written with
its modes (``sequence_modes`` reads them back); one in which none does stays an RAHTB001 frame.

    RAHTB002 | int64 ref_back | int64 ref_fwd | int64 up | int64 block_log2 (1 .. J) | int64 n_blocks (>= 1) | int64 flags (bit 0:
    two motion fields follow; all other bits 0) | with bit 0: int8 mv0[n_blocks][3], zero bytes up to a multiple of 8, int8 mv1
    likewise | uint8 mode[n_blocks] (0 .. 3), zero bytes up to a multiple of 8 | a whole RAHTF001 frame

``n_wide = 0``: ``forward_quant`` / ``dequant_inverse`` (float32; the float64 steps of the header are cast to float32 on both
sides, as ``ops._step_array`` does). ``n_wide = 3``: ``forward_quant_mixed`` / ``dequant_inverse_mixed`` (float64 steps), for 59-column
frames whose first three columns are xyz. ``vmin`` / ``width`` are metadata (the voxel grid's box; 0 when not given).
"""
import itertools
import math

import numpy as np

from . import ops
from .geometry import MAX_J, OctreeCoder
from .ops import step_list
from .rlgr import SegmentedCoder

MAGIC = b"RAHTF001"
SEQ_MAGIC = b"RAHTS001"
P_MAGIC = b"RAHTP001"
P_HEAD = len(P_MAGIC) + 16                                     # what a predicted frame's wrapper adds to its inner frame
M_MAGIC = b"RAHTM001"
M_HEAD = len(M_MAGIC) + 32                                     # ... and a motion-compensated frame's, before its motion field
B_MAGIC = b"RAHTB001"
B_HEAD = len(B_MAGIC) + 40                                     # ... and a B frame's, before its two motion fields
B2_MAGIC = b"RAHTB002"
B2_HEAD = len(B2_MAGIC) + 48                                   # ... and that of a B frame with block modes, before its fields and modes
MIN_FRAME_BYTES = len(MAGIC) + 40 + 8 * 5 + 2 * (8 + 48)      # header, one step + box, two sections of 48 bytes at least


def _step_list(step, D):
    steps = step_list(step)
    if len(steps) not in (1, D):
        raise ValueError("step must be a scalar or have one entry per attribute column")
    if any(not (math.isfinite(s) and s > 0) for s in steps):
        raise ValueError("steps must be finite and positive")
    return steps


def _frame_input(who, V_int, attributes, J, n_wide, dev):
    """What an encoder is handed for a frame, checked -> (V (N, 3) int64, A (N, D) float32) on ``dev``. ``who``: the function, and
    the frame where there are several."""
    import torch
    V = torch.as_tensor(V_int).to(dev, torch.int64)
    A = torch.as_tensor(attributes).to(dev, torch.float32)
    if V.dim() != 2 or V.shape[1] != 3 or A.dim() != 2 or A.shape[0] != V.shape[0] or V.shape[0] < 1:
        raise ValueError(f"{who}: expected (N, 3) coordinates and (N, D) attributes, N >= 1")
    if not 1 <= J <= MAX_J:
        raise ValueError(f"{who}: J outside 1 .. 21")
    if not 0 <= n_wide <= A.shape[1]:
        raise ValueError(f"{who}: n_wide outside 0 .. D")
    return V, A


def _keys_geometry_plan(V, J, geometry):
    """sorted voxel coordinates -> (their keys, geometry section, plan over the keys)"""
    keys = ops.get_morton_code(V, J)
    geo = OctreeCoder.encode(keys, J, entropy=geometry)                   # (also refuses rows that are not sorted and unique)
    return keys, geo, ops.RahtPlan.from_keys(keys, 3 * J)


def _quantize(plans, As, steps, n_wide):
    """[plan], [A] -> [Q]: transform + quantization in float32 or, with ``n_wide``, mixed precision; one frame through its plan,
    several in one set of launches"""
    if len(plans) == 1:
        return [plans[0].forward_quant_mixed(As[0], steps, n_wide) if n_wide else plans[0].forward_quant(As[0], steps)]
    return ops.forward_quant_mixed_batch(plans, As, steps, n_wide) if n_wide else ops.forward_quant_batch(plans, As, steps)


def _reconstruct(plans, Qs, steps, n_wide, roots=None, roots_wide=None):
    """[plan], [Q] -> [C_rec]: the inverse of ``_quantize``; one frame (of a truncated plan: with the ``roots`` of its cells, and
    ``roots_wide`` for the wide columns) through its plan, several in one set of launches"""
    if len(plans) == 1 and n_wide:
        return [plans[0].dequant_inverse_mixed(Qs[0], steps, n_wide, roots=roots, roots_wide=roots_wide)]
    if len(plans) == 1:
        return [plans[0].dequant_inverse(Qs[0], steps, roots=roots)]
    return ops.dequant_inverse_mixed_batch(plans, Qs, steps, n_wide) if n_wide else ops.dequant_inverse_batch(plans, Qs, steps)


def _attribute_parts(Qs, seg_len, dev):
    """quantized (N_i, D) matrices -> every frame's attribute container in pieces (header, length table, payload). One frame goes
    through ``SegmentedCoder.encode``; so does, among several, a frame that needs 64-bit offsets (it fills the chip by itself) and a
    frame of exactly D voxels (``encode`` reads a square matrix as (D, N): the same call for the same bytes whatever its company);
    the others share one set of launches (``encode_ragged`` on the row-major integers)."""
    coders = [SegmentedCoder(Q.shape[0], Q.shape[1], seg_len, 1, dev) for Q in Qs]
    rest = []
    for c, Q in zip(coders, Qs):
        if len(Qs) == 1 or c.wide or c.N == c.D:
            c.encode(Q)
        else:
            rest.append((c, Q))
    if rest:
        SegmentedCoder.encode_ragged([c for c, _ in rest], [Q for _, Q in rest], row_major=True)
    out = []
    for c in coders:
        hdr, lens, payload = c.container_parts()
        out.append([hdr, lens.tobytes(), payload.tobytes()])
    return out


def _refuse_outside(bad, who=""):
    """bad: a coder's ``bad`` word is set -- a table entry reached outside the payload, and that segment decoded as zeros"""
    if bad:
        raise ValueError(f"{who}frame container: an attribute segment reaches outside its payload")


def encode_frame_bytes(V_int, attributes, J, step, device="cuda", n_wide=0, seg_len=2048, geometry="rlgr", vmin=None, width=None):
    """V_int: (N, 3) integer voxel coordinates in Morton order, no voxel twice (what the voxelizer yields); attributes: (N, D)
    float32; numpy arrays or tensors. -> bytes. Raises RahtError when the rows are not in strictly ascending Morton order."""
    import torch
    dev = torch.device(device)
    J, n_wide = int(J), int(n_wide)
    V, A = _frame_input("encode_frame_bytes", V_int, attributes, J, n_wide, dev)
    N, D = A.shape
    steps = _step_list(step, D)
    with torch.cuda.device(dev):
        _, geo, plan = _keys_geometry_plan(V, J, geometry)
        att = _attribute_parts(_quantize([plan], [A], steps, n_wide), seg_len, dev)[0]
    return b"".join(_frame_parts(J, N, D, n_wide, steps, vmin, width, geo, att))


def _frame_parts(J, N, D, n_wide, steps, vmin, width, geo, att_parts):
    """the pieces of a frame container, in order; att_parts: the attribute container, whole or in pieces"""
    box = [0.0, 0.0, 0.0] if vmin is None else [float(x) for x in vmin]
    if len(box) != 3:
        raise ValueError("encode_frame_bytes: vmin must have 3 entries")
    box.append(0.0 if width is None else float(width))
    return [MAGIC + np.array([J, N, D, n_wide, len(steps)], np.int64).tobytes() + np.array(steps + box, np.float64).tobytes()
            + np.array([len(geo)], np.int64).tobytes(), geo, np.array([sum(len(a) for a in att_parts)], np.int64).tobytes(), *att_parts]


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
    dev = torch.device(device)
    J, n_wide = int(J), int(n_wide)
    target = int(target_bytes)
    V, A = _frame_input("encode_frame_bytes_target", V_int, attributes, J, n_wide, dev)
    N, D = A.shape
    base = _step_list(step, D)
    lo, hi = float(scale_range[0]), float(scale_range[1])
    if not (math.isfinite(lo) and math.isfinite(hi) and 0 < lo <= hi) or int(rounds) < 1:
        raise ValueError("encode_frame_bytes_target: scale_range must be 0 < lo <= hi, rounds >= 1")
    K = SegmentedCoder.RATE_MAX
    with torch.cuda.device(dev):
        _, geo, plan = _keys_geometry_plan(V, J, geometry)
        # the frame around the attribute container: header, steps + box, the geometry section and the two length words
        budget = target - (len(MAGIC) + 40 + 8 * (len(base) + 4)) - (8 + len(geo)) - 8
        if budget < 0:
            raise ValueError(f"encode_frame_bytes_target: the geometry section and the header alone take {target - budget} bytes, target {target}")
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
            att = _attribute_parts(_quantize([plan], [A], steps, n_wide), seg_len, dev)[0]
            blob = b"".join(_frame_parts(J, N, D, n_wide, steps, vmin, width, geo, att))
            if len(blob) <= target:
                info = dict(multiplier=m, steps=steps, predicted_attribute_bytes=predicted[m], attribute_bytes=sum(len(a) for a in att),
                            tried=tried, sse=sse_of[m])
                return blob, info
    raise ValueError("encode_frame_bytes_target: no candidate that was predicted to fit did fit")


def parse_frame(blob, max_voxels=None):
    """The header of a frame container, checked against the blob (pure Python, nothing allocated on a device) -> dict: J, N, D,
    n_wide, steps, vmin, width, geometry (offset, length), attributes (offset, length), geometry_ref (None, or the voxel count of
    the frame a predicted geometry section is coded against). ``ValueError`` when it does not add up."""
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
                geometry=(go, gl), attributes=(ao, al), geometry_ref=g.get("N_ref"))


def decode_frame_bytes(blob, device="cuda", max_voxels=None, ref_keys=None):
    """-> (V_int (N, 3) int64, C_rec (N, D) float32), CUDA tensors on ``device``, from the bytes alone. ``max_voxels``: refuse
    frames that announce more voxels than this before anything is allocated for them. ``ref_keys``: the keys of the reference
    frame, for the inner frame of a sequence's predicted frame whose geometry is predicted too (``sequence_geometry``); without
    them such a frame is refused before any device work. ``ValueError`` for a corrupt frame."""
    import torch
    h = parse_frame(blob, max_voxels)
    _need_ref_keys("decode_frame_bytes", blob, h, ref_keys)
    return _decode_group([("", blob, h, ref_keys)], torch.device(device), max_voxels)[0][:2]


def _need_ref_keys(who, blob, h, ref_keys):
    """a frame whose geometry is predicted from another frame's is refused here when the keys of that frame are not at hand"""
    if h["geometry_ref"] is not None:
        go, gl = h["geometry"]
        OctreeCoder.check_ref_keys(OctreeCoder.parse(blob[go: go + gl]), ref_keys, who)


def _attribute_matrices(coders):
    """coders with their containers uploaded -> ([Q (N_i, D) int32], failed): ``_attribute_parts`` read backwards. One frame, and
    every frame of a group in which one needs 64-bit offsets, goes through ``SegmentedCoder.decode``; the others share one launch.
    ``failed()`` -> the frames whose tables reached outside their payload (it synchronises: for after the inverse is enqueued)."""
    if len(coders) == 1 or any(c.wide for c in coders):
        return [c.decode(row_major=True) for c in coders], lambda: [j for j, c in enumerate(coders) if int(c.bad.item())]
    return SegmentedCoder.decode_ragged(coders, row_major=True), lambda: SegmentedCoder.roundtrip_failed(coders)


def _decode_group(group, dev, max_voxels):
    """group: [(who, frame container, its parsed header, ref)], one frame at least, all of one (D, n_wide, steps) -> [(V_int,
    C_rec, keys)]: the geometry frame by frame, the entropy decode and the inverse transform of all frames together
    (``_attribute_matrices``, ``_reconstruct``). ``who`` opens what a refusal of that frame says ("" for a frame that stands alone).
    ``ref``: for a frame with a predicted geometry section the keys of its reference frame, or the position in this group of that
    frame (an earlier one)."""
    import torch
    keys, coders, Vs, plans = [], [], [], []
    with torch.cuda.device(dev):
        for who, fb, h, ref in group:
            (go, gl), (ao, al) = h["geometry"], h["attributes"]
            try:
                keys.append(OctreeCoder.decode(fb[go: go + gl], dev, max_voxels, keys[ref] if isinstance(ref, int) else ref))
                coders.append(SegmentedCoder.from_container(fb[ao: ao + al], dev, max_symbols=h["N"] * h["D"]))
            except ValueError as e:
                raise ValueError(f"{who}{e}") from None
            Vs.append(ops.demorton(keys[-1], h["J"]))
            plans.append(ops.RahtPlan.from_keys(keys[-1], 3 * h["J"]))
        Qs, failed = _attribute_matrices(coders)
        Cs = _reconstruct(plans, Qs, group[0][2]["steps"], group[0][2]["n_wide"])
        for j in failed():
            _refuse_outside(True, group[j][0])
    return list(zip(Vs, Cs, keys))


def region_runs(table, J, depth, n_roots):
    """Where a region lies in the coded order of its frame, from the three bucket histograms of ``ops.region_layout`` (host
    integers, (3, 22): whole frame, rows before the region, rows inside it) -> (n_top, runs). The first ``n_top`` coded rows are the
    tree above ``depth`` (row 0 and every row of a bucket >= J - depth); ``runs`` holds one (coded row, row of the region's own coded
    matrix, count) per finer bucket that has rows in the region, coarse to fine. The region's matrix starts with its ``n_roots``
    root slots (one per occupied cell)."""
    return region_runs_set(table, J, depth, n_roots)


def region_runs_set(table, J, depth, n_roots):
    """``region_runs`` for a region of R row ranges (ascending, disjoint runs of depth-``depth`` cells, concatenated), from the
    table of ``ops.region_layout_set`` (host integers, (1 + 2 R, 22): whole frame, then per range the rows before it and inside
    it) -> (n_top, runs). The tree above ``depth`` is the same first ``n_top`` coded rows. The region's own plan
    (``RahtPlan.from_keys`` of the concatenated keys, truncated at the cells) keeps every cell's first row among its ``n_roots``
    root slots, and in a finer bucket holds range 0's rows of the bucket, then range 1's, and so on: one run per (bucket, range),
    buckets coarse to fine. Destinations ascend."""
    whole, cut, R = table[0], int(J) - int(depth), (len(table) - 1) // 2
    n_top = int(sum(whole[cut:]))
    coded, dst, runs = n_top, int(n_roots), []
    for beta in range(cut - 1, -1, -1):
        for r in range(R):
            before, inside = int(table[1 + 2 * r][beta]), int(table[2 + 2 * r][beta])
            if inside:
                runs.append((coded + before, dst, inside))
            dst += inside
        coded += int(whole[beta])
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


def decode_region_bytes(blob, depth, cells, device="cuda", max_voxels=None, keys=None, ref_keys=None):
    """The voxels of the octree cells ``cells = (c0, c1)`` (Morton indices at ``depth``, 1 <= depth <= J - 1, 0 <= c0 < c1 <=
    8^depth) of a frame, from the geometry and the attribute segments they depend on -> (V_int (n, 3) int64, C_rec (n, D) float32,
    info): rows [a, b) of what ``decode_frame_bytes`` returns, up to the rounding of the tree above ``depth``, which the two
    decoders compute in different launches. ``keys``: ``info["keys"]`` of an earlier call on the same frame; the geometry is then
    not decoded again. info: rows (a, b), n_cells (occupied cells in the range), segments_decoded / segments_total (per channel),
    byte_ranges ((offset, length) within ``blob``: everything outside them may be missing) and bytes_needed, geometry_decoded,
    keys. No N x D matrix is allocated: the only full-length arrays are the keys and the cell search's flags. ``ref_keys``: the
    reference frame's keys, for a frame whose geometry section is predicted (``decode_frame_bytes``); ``keys`` makes them needless.
    ``ValueError`` for a corrupt frame or arguments outside the ranges above. The one-range call of ``decode_cells_bytes``' core."""
    import torch
    who = "decode_region_bytes"
    h = parse_frame(blob, max_voxels)
    try:
        depth, (c0, c1) = int(depth), (int(c) for c in cells)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: depth is an integer, cells a pair of integers") from None
    _region_depth(who, h, depth)
    if not 0 <= c0 < c1 <= 8 ** depth:
        raise ValueError(f"{who}: cells must satisfy 0 <= c0 < c1 <= 8^depth = {8 ** depth}")
    V, C_rec, info, _ = _decode_cells(who, blob, h, depth, [(c0, c1)], torch.device(device), max_voxels, keys, ref_keys)
    info["rows"] = info["rows"][0]
    return V, C_rec, info


def decode_cells_bytes(blob, depth, ranges, device="cuda", max_voxels=None, keys=None, ref_keys=None):
    """``decode_region_bytes`` for a SET of cell ranges. ranges: a non-empty ascending list of disjoint pairs
    ``(c0, c1)`` of depth-``depth`` cell indices (0 <= c0 < c1 <= 8^depth, every c0 at or above the c1 before it), 512 at most ->
    (V_int, C_rec, info) for the concatenation of the ranges' rows: bit for bit the concatenation of ``decode_region_bytes`` over
    each range. The geometry is decoded once, the tree above ``depth`` once, and one plan over the concatenated keys serves all
    ranges. info: as ``decode_region_bytes``', with rows a list of (a, b), one per range."""
    import torch
    who = "decode_cells_bytes"
    h = parse_frame(blob, max_voxels)
    try:
        depth, ranges = int(depth), [(int(c0), int(c1)) for c0, c1 in ranges]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: depth is an integer, ranges a list of pairs of integers") from None
    _region_depth(who, h, depth)
    _region_ranges(who, ranges, depth)
    return _decode_cells(who, blob, h, depth, ranges, torch.device(device), max_voxels, keys, ref_keys)[:3]


def _region_depth(who, h, depth):
    if not 1 <= depth <= h["J"] - 1:
        raise ValueError(f"{who}: depth must be 1 .. J - 1 = {h['J'] - 1}")


def _region_ranges(who, ranges, depth):
    """the rules of a set of cell ranges (a list of pairs of integers) at ``depth``"""
    if not 1 <= len(ranges) <= ops.REGION_MAX_RANGES:
        raise ValueError(f"{who}: 1 .. {ops.REGION_MAX_RANGES} ranges")
    if any(not c0 < c1 for c0, c1 in ranges) or any(p[1] > q[0] for p, q in zip(ranges, ranges[1:])) or ranges[0][0] < 0 or ranges[-1][1] > 8 ** depth:
        raise ValueError(f"{who}: ranges must be ascending, disjoint pairs 0 <= c0 < c1 <= 8^depth = {8 ** depth}")


def _decode_cells(who, blob, h, depth, ranges, dev, max_voxels, keys, ref_keys=None):
    """THE region decoder: the frame ``blob`` with its parsed header ``h``, checked ``depth`` and cell ``ranges`` -> (V_int, C_rec,
    info, the region's keys), the rows of the ranges concatenated. ``who`` opens a refusal."""
    import torch
    if keys is None:
        _need_ref_keys(who, blob, h, ref_keys)
    J, N, D, n_wide, steps = h["J"], h["N"], h["D"], h["n_wide"], h["steps"]
    (go, gl), (ao, al) = h["geometry"], h["attributes"]
    view = memoryview(blob)
    n_d = OctreeCoder.parse(view[go: go + gl], max_voxels)["counts"][depth]
    att = view[ao: ao + al]
    _, _, S, _, _, _, pay = SegmentedCoder._parse(att, N * D)
    nseg = (N + S - 1) // S
    byte_ranges = [(0, ao + pay)]                                         # frame header, geometry section, attribute header + table
    if keys is not None:
        if not isinstance(keys, torch.Tensor) or not keys.is_cuda or keys.dtype != torch.int64 or tuple(keys.shape) != (N,):
            raise ValueError(f"{who}: keys must be the ({N},) int64 CUDA tensor an earlier call returned")
        keys = keys.contiguous()
    tl, R = 3 * (J - depth), len(ranges)
    with torch.cuda.device(dev):
        decoded = keys is None
        if decoded:
            keys = OctreeCoder.decode(view[go: go + gl], dev, max_voxels, ref_keys)
        try:
            cell_keys, cell_first = ops.region_cells(keys, 3 * J, tl, n_d)
        except ops.RahtError as e:
            raise ValueError(f"{who}: the keys are not this frame's ({e})") from None
        j = torch.searchsorted(cell_keys, torch.tensor([c for r in ranges for c in r], dtype=torch.int64, device=dev))
        bounds = cell_first[j]                                               # lo_0, hi_0, lo_1, ...: the rows of every range
        host = torch.cat([j, bounds]).tolist()
        js, rows = list(zip(host[0: 2 * R: 2], host[1: 2 * R: 2])), list(zip(host[2 * R:: 2], host[2 * R + 1:: 2]))
        n_roots, n = sum(j1 - j0 for j0, j1 in js), sum(b - a for a, b in rows)
        info = dict(rows=rows, n_cells=n_roots, segments_decoded=0, segments_total=nseg, byte_ranges=byte_ranges,
                    bytes_needed=byte_ranges[0][1], geometry_decoded=decoded, keys=keys)
        if n_roots == 0:
            return (torch.empty((0, 3), dtype=torch.int64, device=dev), torch.empty((0, D), dtype=torch.float32, device=dev), info,
                    torch.empty(0, dtype=torch.int64, device=dev))
        n_top, runs = region_runs_set(ops.region_layout_set(keys, 3 * J, bounds).tolist(), J, depth, n_roots)
        if n_top != n_d:
            raise ValueError(f"{who}: the keys are not this frame's")
        seg_ids, compact = region_segments(n_top, runs, S)
        sc, att_ranges = SegmentedCoder.from_container_segments(att, seg_ids, dev, max_symbols=N * D)
        Qc = sc.decode(row_major=True)
        # the tree above `depth`: a weighted plan over the occupied cells; its inverse gives every cell's low-pass row
        top = ops.RahtPlan.from_keys(cell_keys, 3 * depth, leaf_weights=cell_first[1:] - cell_first[:-1])
        if R == 1:
            pick = slice(*js[0])
            kr = keys[rows[0][0]: rows[0][1]]
        else:                                                                # the selected cells' rows of the top plan's inverse, gathered
            pick = torch.cat([torch.arange(j0, j1, device=dev) for j0, j1 in js])
            kr = torch.cat([keys[a:b] for a, b in rows])
        roots = top.dequant_inverse(Qc[:n_top], steps)[pick]
        # the region: a plan truncated at the cells over its own rows, its coded matrix put together from the decoded runs
        plan = ops.RahtPlan.from_keys(kr, 3 * J, top_level=tl)
        Qr = ops.region_assemble_set(Qc, [(compact(r), d, c) for r, d, c in runs], n)
        wide = top.dequant_inverse(Qc[:n_top, :n_wide], steps[:n_wide], dtype=torch.float64)[pick].contiguous() if n_wide else None
        C_rec = _reconstruct([plan], [Qr], steps, n_wide, roots=roots.contiguous(), roots_wide=wide)[0]
        V = ops.demorton(kr, J)
        _refuse_outside(int(sc.bad.item()))
    byte_ranges = [(0, ao)]                                               # frame header, geometry section, the attributes' length word
    for off, ln in att_ranges:                                            # the first: header + table (+ the slots that follow them)
        if byte_ranges[-1][0] + byte_ranges[-1][1] == ao + off:
            byte_ranges[-1] = (byte_ranges[-1][0], byte_ranges[-1][1] + ln)
        else:
            byte_ranges.append((ao + off, ln))
    info.update(segments_decoded=len(seg_ids), byte_ranges=byte_ranges, bytes_needed=sum(ln for _, ln in byte_ranges))
    return V, C_rec, info, kr


def pack_sequence(frame_blobs):
    """frames (bytes-like, each a RAHTF001 container) -> the sequence container (pure host code)"""
    blobs = [bytes(b) for b in frame_blobs]
    if not blobs:
        raise ValueError("pack_sequence: a sequence has one frame at least")
    if any(len(b) < MIN_FRAME_BYTES for b in blobs):
        raise ValueError(f"pack_sequence: no frame container is shorter than {MIN_FRAME_BYTES} bytes")
    return _pack_parts([[b] for b in blobs])


def _pack_parts(frames):
    """frames: every frame container as a list of its pieces -> the sequence container, every byte copied once"""
    head = len(SEQ_MAGIC) + 8 * (len(frames) + 2)
    off = head + np.concatenate([[0], np.cumsum([sum(len(p) for p in f) for f in frames], dtype=np.int64)]).astype(np.int64)
    return b"".join([SEQ_MAGIC, np.array([len(frames)], np.int64).tobytes(), off.tobytes()] + [p for f in frames for p in f])


def parse_sequence(blob, max_frames=None):
    """The header of a sequence container, checked against the blob before anything is allocated from its numbers (pure host code)
    -> offsets: a list of n_frames + 1 integers, frame i is blob[offsets[i]: offsets[i + 1]]. ``ValueError`` when it does not add up:
    wrong magic, a truncated header, an implausible frame count (or more than ``max_frames``), offsets that do not ascend by at least
    the smallest frame, a first offset that is not the header's size, a last one that is not the blob's length."""
    m = len(SEQ_MAGIC)
    if bytes(blob[:m]) != SEQ_MAGIC:
        raise ValueError("not a RAHT sequence container")
    if len(blob) < m + 8:
        raise ValueError("sequence container: truncated header")
    n = int(np.frombuffer(blob, np.int64, 1, m)[0])
    if n < 1 or n > (len(blob) - m - 16) // (8 + MIN_FRAME_BYTES):      # (every frame costs its offset and its smallest container)
        raise ValueError("sequence container: implausible frame count")
    if max_frames is not None and n > int(max_frames):
        raise ValueError(f"sequence container: {n} frames, more than the caller allows ({max_frames})")
    head = m + 8 * (n + 2)
    off = np.frombuffer(blob, np.int64, n + 1, m + 8)
    if int(off[0]) != head or int(off[-1]) != len(blob) or bool(np.any(off[1:] - off[:-1] < MIN_FRAME_BYTES)) or bool(np.any(off < 0)):
        raise ValueError("sequence container: the offset table does not match the blob")
    return [int(x) for x in off]


def sequence_frame(blob, i, offsets=None):
    """frame i of a sequence container as a memoryview of its RAHTF001 container (no copy). ``offsets``: what ``parse_sequence``
    returned for this blob (parsed here otherwise)."""
    off = parse_sequence(blob) if offsets is None else offsets
    i = int(i)
    if not 0 <= i < len(off) - 1:
        raise ValueError(f"sequence_frame: frame index outside 0 .. {len(off) - 2}")
    return memoryview(blob)[off[i]: off[i + 1]]


_WRAPPERS = {P_MAGIC: ("predicted frame", P_HEAD), M_MAGIC: ("motion-compensated frame", M_HEAD),      # what a refusal says, the fixed part
             B_MAGIC: ("B frame", B_HEAD), B2_MAGIC: ("B frame", B2_HEAD)}


def _motion_field_bytes(n_blocks):
    """the bytes of a motion field in its wrapper: three per block, zero-padded to a multiple of 8"""
    return (3 * n_blocks + 7) // 8 * 8


def _mode_bytes(n_blocks):
    """the bytes of the block modes in their wrapper: one per block, zero-padded to a multiple of 8"""
    return (n_blocks + 7) // 8 * 8


def _parse_wrapper(fb, only=None):
    """The wrapper of a predicted frame of any kind, checked as ``parse_pframe``, ``parse_mframe``, ``parse_bframe`` and
    ``parse_bframe2`` say -> (ref_back, up, motion: None or (block_log2, mv (n_blocks, 3) int8 numpy) -- (block_log2, mv0, mv1) in a
    B frame --, the inner RAHTF001 container as a memoryview, ref_fwd: None but in a B frame, modes: None but in an RAHTB002 frame,
    there (block_log2, mode (n_blocks,) uint8 numpy)). None when ``fb`` opens with no wrapper's magic (with ``only``: with another
    magic than that one)."""
    magic = bytes(fb[:len(P_MAGIC)])
    if magic not in _WRAPPERS or only not in (None, magic):
        return None
    what, head = _WRAPPERS[magic]
    if len(fb) < head + MIN_FRAME_BYTES:
        raise ValueError(f"{what}: truncated wrapper")
    ref_fwd, modes = None, None
    if magic in (B_MAGIC, B2_MAGIC):
        ref_back, ref_fwd, up = [int(x) for x in np.frombuffer(fb, np.int64, 3, len(magic))]
        if ref_fwd < 1:
            raise ValueError(f"{what}: ref_fwd = {ref_fwd}, must be at least 1")
    else:
        ref_back, up = [int(x) for x in np.frombuffer(fb, np.int64, 2, len(magic))]
    if ref_back < 1:
        raise ValueError(f"{what}: ref_back = {ref_back}, must be at least 1")
    if not 0 <= up <= 3:
        raise ValueError(f"{what}: up = {up} outside 0 .. 3")
    motion = None
    if magic == B2_MAGIC:
        block_log2, n_blocks, flags = [int(x) for x in np.frombuffer(fb, np.int64, 3, len(magic) + 24)]
        if not 1 <= block_log2 <= MAX_J:
            raise ValueError(f"{what}: block_log2 = {block_log2} outside 1 .. {MAX_J}")
        if flags & ~1:
            raise ValueError(f"{what}: unknown flag bits ({flags:#x})")
        n_fields = 2 * (flags & 1)
        if n_blocks < 1 or n_blocks >= 2 ** 31 or len(fb) < head + n_fields * _motion_field_bytes(n_blocks) + _mode_bytes(n_blocks) + MIN_FRAME_BYTES:
            raise ValueError(f"{what}: too short for {n_fields} motion fields and the modes of {n_blocks} blocks and a frame")
        if n_fields:
            fields = np.frombuffer(fb, np.int8, 2 * _motion_field_bytes(n_blocks), head).reshape(2, -1)
            if fields[:, 3 * n_blocks:].any():
                raise ValueError(f"{what}: the padding behind a motion field is not zero")
            motion = (block_log2, fields[0, :3 * n_blocks].reshape(n_blocks, 3), fields[1, :3 * n_blocks].reshape(n_blocks, 3))
            head += fields.size
        mode = np.frombuffer(fb, np.uint8, _mode_bytes(n_blocks), head)
        if mode[n_blocks:].any():
            raise ValueError(f"{what}: the padding behind the block modes is not zero")
        if mode[:n_blocks].max() > 3:
            raise ValueError(f"{what}: a block mode of {int(mode[:n_blocks].max())}, outside 0 .. 3")
        modes = (block_log2, mode[:n_blocks])
        head += len(mode)
    elif magic == B_MAGIC:
        block_log2, n_blocks = [int(x) for x in np.frombuffer(fb, np.int64, 2, len(magic) + 24)]
        if (block_log2 == 0) != (n_blocks == 0):
            raise ValueError(f"{what}: block_log2 = {block_log2} with n_blocks = {n_blocks} (both 0 without motion fields, neither with)")
        if block_log2:
            if not 1 <= block_log2 <= MAX_J:
                raise ValueError(f"{what}: block_log2 = {block_log2} outside 1 .. {MAX_J}")
            if n_blocks < 1 or n_blocks >= 2 ** 31 or len(fb) < head + 2 * _motion_field_bytes(n_blocks) + MIN_FRAME_BYTES:
                raise ValueError(f"{what}: too short for two motion fields of {n_blocks} blocks and a frame")
            fields = np.frombuffer(fb, np.int8, 2 * _motion_field_bytes(n_blocks), head).reshape(2, -1)
            if fields[:, 3 * n_blocks:].any():
                raise ValueError(f"{what}: the padding behind a motion field is not zero")
            motion = (block_log2, fields[0, :3 * n_blocks].reshape(n_blocks, 3), fields[1, :3 * n_blocks].reshape(n_blocks, 3))
            head += fields.size
    elif magic == M_MAGIC:
        block_log2, n_blocks = [int(x) for x in np.frombuffer(fb, np.int64, 2, len(magic) + 16)]
        if not 1 <= block_log2 <= MAX_J:
            raise ValueError(f"{what}: block_log2 = {block_log2} outside 1 .. {MAX_J}")
        if n_blocks < 1 or n_blocks >= 2 ** 31 or len(fb) < head + _motion_field_bytes(n_blocks) + MIN_FRAME_BYTES:
            raise ValueError(f"{what}: too short for a motion field of {n_blocks} blocks and a frame")
        field = np.frombuffer(fb, np.int8, _motion_field_bytes(n_blocks), head)
        if field[3 * n_blocks:].any():
            raise ValueError(f"{what}: the padding behind the motion field is not zero")
        motion = (block_log2, field[:3 * n_blocks].reshape(n_blocks, 3))
        head += len(field)
    return ref_back, up, motion, memoryview(fb)[head:], ref_fwd, modes


def parse_pframe(fb):
    """The wrapper of a predicted frame, checked (pure host code) -> (ref_back, up, the inner RAHTF001 container as a memoryview).
    ``ValueError`` for another magic, a wrapper too short to hold a frame, ``ref_back < 1`` or ``up`` outside 0 .. 3; the inner
    frame is ``parse_frame``'s to judge."""
    w = _parse_wrapper(fb, P_MAGIC)
    if w is None:
        raise ValueError("not a RAHT predicted-frame wrapper")
    return w[0], w[1], w[3]


def parse_mframe(fb):
    """The wrapper of a motion-compensated frame, checked (pure host code) -> (ref_back, up, block_log2, mv (n_blocks, 3) int8 numpy,
    the inner RAHTF001 container as a memoryview). ``ValueError`` for another magic, ``ref_back < 1``, ``up`` outside 0 .. 3,
    ``block_log2`` outside 1 .. 21, a wrapper too short for its motion field plus a frame, padding that is not zero. Every int8
    vector is legal. Whether ``block_log2`` and ``n_blocks`` go with the inner frame is for the sequence's checks (``_frame_head``)."""
    w = _parse_wrapper(fb, M_MAGIC)
    if w is None:
        raise ValueError("not a RAHT motion-compensated frame wrapper")
    return w[0], w[1], *w[2], w[3]


def parse_bframe(fb):
    """The wrapper of a B frame, checked (pure host code) -> (ref_back, ref_fwd, up, block_log2, mv0, mv1, the inner RAHTF001
    container as a memoryview); block_log2 is 0 and mv0, mv1 are None without motion fields, (n_blocks, 3) int8 numpy with them.
    ``ValueError`` for another magic, ``ref_back`` or ``ref_fwd`` below 1, ``up`` outside 0 .. 3, ``block_log2`` and ``n_blocks`` of
    which one is 0 and the other not, ``block_log2`` outside 1 .. 21, a wrapper too short for its fields plus a frame, padding that
    is not zero. What depends on the sequence or on the inner frame is for the sequence's checks (``_frame_head``)."""
    w = _parse_wrapper(fb, B_MAGIC)
    if w is None:
        raise ValueError("not a RAHT B-frame wrapper")
    return w[0], w[4], w[1], *(w[2] or (0, None, None)), w[3]


def parse_bframe2(fb):
    """The wrapper of a B frame with block modes (RAHTB002), checked (pure host code) -> (ref_back, ref_fwd, up,
    block_log2, mv0, mv1, modes (n_blocks,) uint8 numpy, the inner RAHTF001 container as a memoryview); mv0, mv1 are None without
    motion fields (flag bit 0), (n_blocks, 3) int8 numpy with them. ``ValueError`` for another magic, ``ref_back`` or ``ref_fwd``
    below 1, ``up`` outside 0 .. 3, ``block_log2`` outside 1 .. 21, an unknown flag bit, ``n_blocks`` below 1, a wrapper too short for
    its fields and modes plus a frame, padding that is not zero, a mode above 3. What depends on the sequence or on the inner frame
    is for the sequence's checks (``_frame_head``)."""
    w = _parse_wrapper(fb, B2_MAGIC)
    if w is None:
        raise ValueError("not a RAHT B-frame wrapper with block modes")
    mv0, mv1 = w[2][1:] if w[2] else (None, None)
    return w[0], w[4], w[1], w[5][0], mv0, mv1, w[5][1], w[3]


def _frame_head(view, off, i, max_voxels):
    """frame i of a sequence from its headers alone -> dict: kind ("I" / "P" / "B"), ref (the frame it is predicted from -- a B
    frame's reference 0 --, or None), ref1 (a B frame's reference 1, or None), up, motion (None, (block_log2, mv) of a
    motion-compensated frame, (block_log2, mv0, mv1) of a B frame with fields), fb (its RAHTF001 container: the inner one of a
    predicted frame), h (``parse_frame`` of it), seg_len. ``ValueError`` naming i."""
    fb = view[off[i]: off[i + 1]]
    kind, ref, ref1, up, motion, modes = "I", None, None, 0, None, None
    try:
        w = _parse_wrapper(fb)
        if w is not None:
            ref_back, up, motion, fb, ref_fwd, modes = w
            what = "predicted frame" if ref_fwd is None else "B frame"
            if i == 0:
                raise ValueError(f"a {what} cannot open a sequence")
            if ref_back > i:
                raise ValueError(f"{what}: ref_back = {ref_back} reaches before frame 0")
            kind, ref = "P", i - ref_back
            if ref_fwd is not None:
                if i + ref_fwd > len(off) - 2:
                    raise ValueError(f"{what}: ref_fwd = {ref_fwd} reaches past the last frame")
                kind, ref1 = "B", i + ref_fwd
        h = parse_frame(fb, max_voxels)
        if h["geometry_ref"] is not None and ref is None:
            raise ValueError("a geometry section predicted from another frame in a frame without a wrapper")
        for blocks, of in ((motion, "a motion field"), (modes, "block modes")):
            if blocks is None:
                continue
            what = "B frame" if kind == "B" else "motion-compensated frame"
            if blocks[0] > h["J"]:
                raise ValueError(f"{what}: block_log2 = {blocks[0]} outside 1 .. J = {h['J']}")
            go, gl = h["geometry"]
            n_level = OctreeCoder.parse(fb[go: go + gl], max_voxels)["counts"][h["J"] - blocks[0]]
            if len(blocks[1]) != n_level:
                raise ValueError(f"{what}: {of} of {len(blocks[1])} blocks, the geometry has {n_level}")
        ao, al = h["attributes"]
        S = SegmentedCoder._parse(fb[ao: ao + al], h["N"] * h["D"])[2]
    except ValueError as e:
        raise ValueError(f"sequence container: frame {i}: {e}") from None
    return dict(kind=kind, ref=ref, ref1=ref1, up=up, motion=motion, modes=modes, fb=fb, h=h, seg_len=S)


def _frame_heads(view, off, idx, max_voxels):
    """the heads of the frames ``idx`` and of every frame they depend on -- under both references of a B frame --, back to the
    nearest intra frames -> {i: head}; a predicted frame whose J or D is not its reference's, whose reference is a B frame, or whose
    geometry is predicted from another voxel count than its reference's (a B frame's: reference 0's), is refused here, before any
    device work"""
    heads = {}
    for i in idx:                                                            # (in the order asked for: the first bad frame is the one named)
        todo = [i]
        while todo:
            i = todo.pop()
            if i is not None and i not in heads:
                heads[i] = _frame_head(view, off, i, max_voxels)
                todo += [heads[i]["ref1"], heads[i]["ref"]]                  # (reference 0's chain first)
    for i in sorted(heads):
        hd = heads[i]
        for g in (hd["ref"], hd["ref1"]):
            if g is None:
                continue
            h, r = hd["h"], heads[g]["h"]
            if heads[g]["kind"] == "B":
                raise ValueError(f"sequence container: frame {i}: its reference (frame {g}) is a B frame, which is no frame's reference")
            if (h["J"], h["D"]) != (r["J"], r["D"]):
                raise ValueError(f"sequence container: frame {i}: a predicted frame of J = {h['J']}, D = {h['D']} against a reference "
                                 f"(frame {g}) of J = {r['J']}, D = {r['D']}")
        if hd["ref"] is not None:
            h, r = hd["h"], heads[hd["ref"]]["h"]
            if h["geometry_ref"] not in (None, r["N"]):
                raise ValueError(f"sequence container: frame {i}: a geometry section predicted from {h['geometry_ref']} voxels, the "
                                 f"reference (frame {hd['ref']}) has {r['N']}")
    return heads


def _sequence_heads(blob, max_voxels, max_frames):
    """-> the head of every frame of a sequence container, in order"""
    off = parse_sequence(blob, max_frames)
    heads = _frame_heads(memoryview(blob), off, range(len(off) - 1), max_voxels)
    return [heads[i] for i in range(len(off) - 1)]


def sequence_kinds(blob, max_voxels=None, max_frames=None):
    """-> ["I" | "P" | "B"] per frame of a sequence container, from the headers alone (pure host code). Every frame's headers are checked
    on the way as ``decode_sequence_bytes`` checks them: ``ValueError`` naming the frame for a predicted frame at index 0, a
    ``ref_back`` below 1 or reaching before frame 0, ``up`` outside 0 .. 3, a truncated wrapper, a frame ``parse_frame`` refuses, a
    predicted frame whose J or D differs from its reference's; for a B frame (RAHTB001) also a ``ref_fwd`` below 1 or reaching past
    the last frame, ``block_log2`` / ``n_blocks`` that do not go together or with the inner frame, and a reference that is a B frame."""
    return [hd["kind"] for hd in _sequence_heads(blob, max_voxels, max_frames)]


def sequence_refs(blob, max_voxels=None, max_frames=None):
    """-> per frame of a sequence container the tuple of the frame indices it is predicted from: () for an intra frame, (r,) for a
    predicted one, (r0, r1) for a B frame; from the headers alone (pure host code), with the checks of ``sequence_kinds``."""
    return [tuple(r for r in (hd["ref"], hd["ref1"]) if r is not None) for hd in _sequence_heads(blob, max_voxels, max_frames)]


def sequence_motion(blob, max_voxels=None, max_frames=None):
    """-> per frame of a sequence container None, (block_log2, mv (n_blocks, 3) int8 numpy) for a motion-compensated frame, or
    (block_log2, mv0, mv1) for a B frame with motion fields, from the headers alone (pure host code), with the checks of
    ``sequence_kinds``."""
    return [hd["motion"] for hd in _sequence_heads(blob, max_voxels, max_frames)]


def sequence_modes(blob, max_voxels=None, max_frames=None):
    """-> per frame of a sequence container None, or the block modes (n_blocks,) uint8 numpy of a B frame that carries them
    (RAHTB002) -- over the blocks of the wrapper's ``block_log2``, which ``parse_bframe2`` returns --, from the
    headers alone (pure host code), with the checks of ``sequence_kinds`` and those of the modes: a mode above 3, an unknown flag
    bit, padding that is not zero, a block count that is not the inner frame's."""
    return [None if hd["modes"] is None else hd["modes"][1] for hd in _sequence_heads(blob, max_voxels, max_frames)]


def sequence_geometry(blob, max_voxels=None, max_frames=None):
    """-> ["intra" | "predicted"] per frame of a sequence container: how its geometry section is coded, from the headers alone
    (pure host code), with the checks of ``sequence_kinds`` and two more: a predicted geometry section in a frame without a
    wrapper, or one predicted from another voxel count than its reference frame's, is refused, the frame named."""
    return ["intra" if hd["h"]["geometry_ref"] is None else "predicted" for hd in _sequence_heads(blob, max_voxels, max_frames)]


class _Predictor:
    """"This frame is predicted from that one": the frame's ``keys``, its reference ``ref`` = (keys, reconstruction), ``J``, ``up``
    and ``motion`` -- None, or (block_log2, mv (n_blocks, 3) int8 on the device, block_first) of a motion-compensated frame. The
    encoder's closed loop and the decoder add the prediction through the one ``restore``, with one argument list: that is what
    keeps the loop free of drift. ``overhead``: the bytes of ``wrapper()``."""

    def __init__(self, keys, ref, J, up, motion=None, back=1, ref1=None, fwd=None, modes=None):
        """back: how many frames earlier ``ref`` lies. A B frame has a second reference ``ref1``, ``fwd`` frames later; its ``motion``
        is None or (block_log2, mv0, mv1, block_first), and its ``modes`` None or (block_log2, mode (n_blocks,) uint8 on the device,
        block_first) over the same blocks."""
        self.keys, self.ref, self.J, self.up, self.motion, self.back, self.ref1, self.fwd = keys, ref, J, up, motion, back, ref1, fwd
        self.modes = modes
        if modes is not None:
            self.overhead = B2_HEAD + (0 if motion is None else 2 * _motion_field_bytes(len(modes[1]))) + _mode_bytes(len(modes[1]))
        elif ref1 is not None:
            self.overhead = B_HEAD + (0 if motion is None else 2 * _motion_field_bytes(len(motion[1])))
        else:
            self.overhead = P_HEAD if motion is None else M_HEAD + _motion_field_bytes(len(motion[1]))

    def _apply(self, X, add):
        """X - P into a fresh matrix, or with ``add`` X + P in place"""
        kw = dict(X=X, up=self.up, add=add, out=X if add else None)
        if self.ref1 is not None:
            if self.motion is not None:
                block_log2, mv0, mv1, block_first = self.motion
                kw.update(J=self.J, block_log2=block_log2, block_first=block_first, mv0=mv0, mv1=mv1)
            if self.modes is not None:
                block_log2, mode, block_first = self.modes
                kw.update(J=self.J, block_log2=block_log2, block_first=block_first, modes=mode)
            return ops.predict_bi(self.keys, self.ref, self.ref1, **kw)
        if self.motion is None:
            return ops.predict(self.keys, *self.ref, **kw)
        block_log2, mv, block_first = self.motion
        return ops.predict_mc(self.keys, *self.ref, mv, block_first, self.J, block_log2, **kw)

    def residual(self, A):
        return self._apply(A, False)

    def restore(self, C):
        return self._apply(C, True)

    def wrapper(self):
        """the bytes in front of the inner frame (a motion field and the block modes come to the host here)"""
        if self.ref1 is not None:
            fields, n_blocks = b"", 0
            if self.motion is not None:
                n_blocks = len(self.motion[1])
                pad = bytes(_motion_field_bytes(n_blocks) - 3 * n_blocks)
                fields = b"".join(mv.cpu().numpy().tobytes() + pad for mv in self.motion[1:3])
            if self.modes is not None:
                block_log2, n_blocks = self.modes[0], len(self.modes[1])
                mode = self.modes[1].cpu().numpy().tobytes() + bytes(_mode_bytes(n_blocks) - n_blocks)
                head = np.array([self.back, self.fwd, self.up, block_log2, n_blocks, int(self.motion is not None)], np.int64)
                return B2_MAGIC + head.tobytes() + fields + mode
            block_log2 = 0 if self.motion is None else self.motion[0]
            return B_MAGIC + np.array([self.back, self.fwd, self.up, block_log2, n_blocks], np.int64).tobytes() + fields
        if self.motion is None:
            return P_MAGIC + np.array([self.back, self.up], np.int64).tobytes()
        field = self.motion[1].cpu().numpy().tobytes()
        return (M_MAGIC + np.array([self.back, self.up, self.motion[0], len(field) // 3], np.int64).tobytes() + field
                + bytes(self.overhead - M_HEAD - len(field)))


SEQ_CHUNK = SegmentedCoder.BATCH_MAX                                     # frames whose transform and entropy stages share launches


def sequence_plan(n, gop, bframes=0):
    """The structure ``encode_sequence_bytes(..., gop, bframes)`` gives a sequence of ``n`` frames (pure host code) -> per frame
    ("I" | "P" | "B", refs): what the frame may be coded as at most, and the frames it is then predicted from. A GOP covers the
    frames g0 .. g1 - 1, g1 = min(g0 + gop, n); its ANCHORS are g0 + k (bframes + 1) and its last frame: g0 is "I" with no
    reference, every other anchor "P" from the anchor before it; every other frame is a "B" candidate between its neighbouring
    anchors (a, c), a < i < c."""
    n, gop, b = int(n), int(gop), int(bframes)
    if n < 1 or gop < 1 or b < 0:
        raise ValueError("sequence_plan: n >= 1, gop >= 1, bframes >= 0")
    plan = []
    for g0 in range(0, n, gop):
        g1 = min(g0 + gop, n)
        anchors = sorted(set(range(g0, g1, b + 1)) | {g1 - 1})
        for a, c in zip([None] + anchors, anchors):
            plan += [("B", (a, c))] * (0 if a is None else c - a - 1) + [("I", ()) if a is None else ("P", (a,))]
    return plan


def encode_sequence_bytes(frames, J, step, device="cuda", n_wide=0, seg_len=2048, geometry="rlgr", vmin=None, width=None, gop=1, up=0,
                          inter="auto", motion=0, block_log2=4, motion_weights=None, geometry_inter="off", bframes=0, motion_levels=0,
                          block_modes=False):
    """frames: a list of (V_int, attributes) as ``encode_frame_bytes`` takes them, any voxel count per frame, one D -> the sequence
    container; frame i of it is ``encode_frame_bytes(*frames[i], J, step, ...)`` byte for byte. Keys, geometry section and plan
    frame by frame; the transform + quantization of up to ``SEQ_CHUNK`` frames in one set of launches (``forward_quant_mixed_batch``
    when ``n_wide`` is set, ``forward_quant_batch`` otherwise) and their entropy stage in another
    (``SegmentedCoder.encode_ragged`` on the row-major integers). Device memory: the quantized matrices and the coders' buffers
    of a whole chunk are alive together, about 8 N D bytes per frame beside its attributes (12 frames of 1 M x 59: 5.7 GB).

    ``gop`` > 1: inter-frame prediction. Frame i with i % gop == 0 is intra; every other frame is a candidate for
    prediction from frame i - 1's RECONSTRUCTION (closed loop: the encoder predicts from what the decoder will have, so nothing
    drifts): R = A - P with P = ``ops.predict(keys_i, keys_(i-1), C_rec_(i-1), up=up)``. ``inter="always"`` codes R as an RAHTP001
    frame; ``inter="auto"`` asks ``RahtPlan.rate_curve`` for the exact attribute bytes of A and of R at the frame's steps and codes R
    iff bytes_R + 24 < bytes_A (the wrapper costs 24 bytes; a tie goes to intra). The chain is a true dependency -- frame i's residual
    needs frame i - 1's reconstruction, which needs its integers -- so with ``gop`` > 1 the transform + quantization (and, where a
    frame is predicted from, the inverse) run frame by frame, for I and P frames alike; the entropy stage still goes through one
    set of launches per ``SEQ_CHUNK`` frames. With the default ``gop=1`` the result is byte for byte what it was without these
    arguments.

    ``motion`` = r > 0 (with ``gop`` > 1): motion compensation. For a candidate frame ``ops.motion_search`` finds, for
    every occupied block of 2^``block_log2`` voxels a side (1 <= block_log2 <= J), the vector of [-r, r]^3 (r <= 3,
    ``ops.motion_candidates``) under which frame i - 1's reconstruction predicts A best; the cost of a column is weighted by
    ``motion_weights`` (D numbers >= 0; default 1 / step of the column as float32, so that cost counts quantization steps; 0 leaves
    a column out). If every vector is zero the frame goes the way of ``motion=0``, byte for byte. Otherwise Rmc = A -
    ``ops.predict_mc`` is a third candidate: ``inter="always"`` codes it as an RAHTM001 frame, ``inter="auto"`` codes the smallest of
    bytes_A, bytes_R + 24 and bytes_Rmc + 40 + the field's bytes (3 per block, padded to 8), a tie going to the earlier of the
    three. ``motion=0`` (the default) is byte for byte what it was without these arguments.

    ``geometry_inter`` (with ``gop`` > 1): "always" -- a frame that is coded as a predicted frame of either kind carries
    a predicted geometry section (``OctreeCoder.encode(keys, J, ref_keys=the keys of frame i - 1)``, the frame its wrapper names;
    under a motion field too: the reference is not shifted); "auto" -- both sections are coded and the smaller is kept, a tie going
    to the intra one. Frames coded intra never carry one. Under ``inter="auto"`` the cost of a way to code the frame is then its
    attribute bytes + its wrapper + the geometry section it would carry. "off" (the default) is byte for byte what it was without
    this argument.

    ``bframes`` = b > 0 (with ``gop`` > 1): B frames (``sequence_plan`` has the structure). The anchors of a GOP --
    every (b + 1)-th frame and its last -- are coded as above, each from the anchor BEFORE it (its wrapper carries that
    ``ref_back``). A frame between two anchors a < i < c is coded after both are reconstructed and is no frame's reference: the
    ways are intra, predicted from a, that under a motion field, B from (a, c) -- R = A - ``ops.predict_bi`` of the two
    reconstructions, an RAHTB001 frame -- and B under two fields (two independent ``ops.motion_search`` calls, one per reference;
    taken when either field is not all zero). ``inter="always"`` takes the last way, ``inter="auto"`` the fewest bytes (attribute
    bytes + wrapper + geometry section), the earliest among equals. A predicted geometry section of such a frame is coded against
    a's keys. No reconstruction is formed for these frames, and the transform + quantization of the ones between two anchors go
    through one set of launches. ``bframes=0`` (the default) is byte for byte what it was without this argument.

    ``motion_levels`` = L > 0 (with ``motion`` = r > 0): every motion search -- against reference 0 and, for a B
    candidate, against reference 1 -- is the coarse-to-fine ``ops.motion_search_hier(levels=L, radius=r)``: vectors of up to
    r 2^L + 2^L - 1 voxels a component at the cost of a few radius-1 searches. L <= min(3, block_log2 - 1) and J - L >= 1. The
    coarse levels of a reconstruction are built once and kept beside it for every frame that is searched against it. The format
    and the decoders are the same: a field is a field. ``motion_levels=0`` (the default) is byte for byte what it was without
    this argument.

    ``block_modes=True`` (with ``bframes`` > 0 and ``gop`` > 1): every occupied block of 2^``block_log2`` voxels a side
    of a B candidate picks its own predictor. After the B ways above, ``ops.mode_search`` is run on the last of them -- the one under
    two fields if there is one, else the one without -- with ``motion_weights`` (default 1 / step per column): mode 0 is that way's
    own rule, 1 reference 0 alone, 2 reference 1 alone, 3 no prediction. If any block chooses another mode than 0, a further way
    is added whose predictor carries the modes; it is written as an RAHTB002 frame, and its overhead is that wrapper, the padded
    mode bytes included. ``inter="always"`` takes this last way, ``inter="auto"`` the fewest bytes as above. Where every block
    chooses 0 nothing is added. ``block_modes=False`` (the default) is byte for byte what it was without this argument."""
    import torch
    dev = torch.device(device)
    J, n_wide, gop, up, motion, block_log2, bframes = int(J), int(n_wide), int(gop), int(up), int(motion), int(block_log2), int(bframes)
    motion_levels, block_modes = int(motion_levels), bool(block_modes)
    if not frames:
        raise ValueError("encode_sequence_bytes: a sequence has one frame at least")
    if gop < 1 or not 0 <= up <= 3 or inter not in ("auto", "always") or bframes < 0:
        raise ValueError('encode_sequence_bytes: gop >= 1, up in 0 .. 3, inter "auto" or "always", bframes >= 0')
    if not 0 <= motion <= 3 or (motion and not 1 <= block_log2 <= J):
        raise ValueError("encode_sequence_bytes: motion in 0 .. 3, block_log2 in 1 .. J")
    if motion_levels < 0 or (motion_levels and (not motion or motion_levels > min(3, block_log2 - 1) or J - motion_levels < 1)):
        raise ValueError("encode_sequence_bytes: motion_levels in 0 .. min(3, block_log2 - 1) with J - motion_levels >= 1, and only with motion")
    if geometry_inter not in ("off", "always", "auto"):
        raise ValueError('encode_sequence_bytes: geometry_inter "off", "always" or "auto"')
    if block_modes and (bframes < 1 or gop < 2 or not 1 <= block_log2 <= J):
        raise ValueError("encode_sequence_bytes: block_modes needs bframes > 0, gop > 1 and block_log2 in 1 .. J")
    VA = []
    for i, (V_int, attributes) in enumerate(frames):
        V, A = _frame_input(f"encode_sequence_bytes: frame {i}", V_int, attributes, J, n_wide, dev)
        if VA and A.shape[1] != VA[0][1].shape[1]:
            raise ValueError(f"encode_sequence_bytes: frame {i} has {A.shape[1]} attribute columns, frame 0 has {VA[0][1].shape[1]}")
        VA.append((V, A))
    D = int(VA[0][1].shape[1])
    steps = _step_list(step, D)
    if motion and gop > 1:
        cands = ops.motion_candidates(motion)
    if (motion or block_modes) and gop > 1 and motion_weights is None:
        motion_weights = (1.0 / np.asarray(steps * (D if len(steps) == 1 else 1), np.float64)).astype(np.float32)
    n = len(VA)
    parts = []                                                               # (the pieces of every frame: joined once, at the end)
    coded = {}                                                               # frame -> (geometry section, Q, wrapper) until its entropy stage

    def flush():
        # the entropy stage of the next SEQ_CHUNK frames in display order (of the rest at the end), once all of them are coded
        while len(parts) < n and all(i in coded for i in range(len(parts), min(len(parts) + SEQ_CHUNK, n))):
            idx = range(len(parts), min(len(parts) + SEQ_CHUNK, n))
            geos, Qs, wraps = zip(*[coded.pop(i) for i in idx])
            atts = _attribute_parts(list(Qs), seg_len, dev)
            parts.extend([w] + _frame_parts(J, VA[i][1].shape[0], D, n_wide, steps, vmin, width, geo, att)
                         for i, geo, att, w in zip(idx, geos, atts, wraps))

    def search(keys, counts, r, A, block_first):
        """the motion field of a frame against the reconstruction of frame ``r``: exhaustive, or coarse to fine with the coarse
        levels of that reconstruction built at their first use and kept until it is dropped"""
        ref = recon[r]
        if not motion_levels:
            return ops.motion_search(keys, ref[0], ref[1], A, J, block_log2, block_first, cands, motion_weights, up=up)[0]
        mv, _, info = ops.motion_search_hier(keys, ref[0], ref[1], A, J, block_log2, block_first, motion_levels, motion, motion_weights, up=up,
                                             counts=counts, ref_counts=level_counts[r], ref_pyramid=pyramids.get(r))
        pyramids[r] = info["ref_pyramid"]
        return mv

    def choose(i, A, a, c=None):
        """How frame i is coded, its reference 0 frame ``a`` (None: intra only) and, for a B candidate, its reference 1 frame ``c``
        -> (plan, source of the transform, geometry section, wrapper, predictor or None). The ways, each by its predictor: intra
        (None), predicted from a's reconstruction, that under a motion field that is not all zero, from both references, and
        that under two fields of which one is not all zero."""
        keys, geo, plan = _keys_geometry_plan(VA[i][0], J, geometry)
        ways, geo_p = [None], geo                                            # geo_p: the section of a frame that is coded predicted
        counts = OctreeCoder.parse(geo)["counts"] if motion_levels else None
        if motion_levels and i in last_use:                                  # a reference to be: its coarse levels need their counts
            level_counts[i] = counts
        if a is not None:
            ref, ref1 = recon[a], None if c is None else recon[c]
            if geometry_inter != "off":
                geo_p = OctreeCoder.encode(keys, J, entropy=geometry, ref_keys=ref[0])
                if geometry_inter == "auto" and len(geo_p) >= len(geo):
                    geo_p = geo
            ways.append(_Predictor(keys, ref, J, up, back=i - a))
            if motion:
                n_blocks = OctreeCoder.parse(geo)["counts"][J - block_log2]
                block_first = ops.motion_blocks(keys, J, block_log2, n_blocks)
                mv = search(keys, counts, a, A, block_first)
                moved = bool(mv.any())
                if moved:
                    ways.append(_Predictor(keys, ref, J, up, (block_log2, mv, block_first), back=i - a))
            if ref1 is not None:
                ways.append(_Predictor(keys, ref, J, up, back=i - a, ref1=ref1, fwd=c - i))
                if motion:                                                   # (two independent searches, one per reference)
                    mv1 = search(keys, counts, c, A, block_first)
                    if moved or bool(mv1.any()):
                        ways.append(_Predictor(keys, ref, J, up, (block_log2, mv, mv1, block_first), back=i - a, ref1=ref1, fwd=c - i))
                if block_modes:                                              # the blocks of the last B way choose among its predictors
                    last = ways[-1]
                    if not motion:
                        n_blocks = OctreeCoder.parse(geo)["counts"][J - block_log2]
                        block_first = ops.motion_blocks(keys, J, block_log2, n_blocks)
                    mv0, mv1 = (None, None) if last.motion is None else last.motion[1:3]
                    mode = ops.mode_search(keys, ref, ref1, A, J, block_log2, block_first, motion_weights, up=up, mv0=mv0, mv1=mv1)[0]
                    if bool(mode.any()):
                        ways.append(_Predictor(keys, ref, J, up, last.motion, back=i - a, ref1=ref1, fwd=c - i,
                                               modes=(block_log2, mode, block_first)))
        if inter == "always" or len(ways) == 1:                              # the last way; its source alone is formed
            pred = ways[-1]
            src = A if pred is None else pred.residual(A)
        else:                                                                # the fewest bytes, wrapper included; the earliest among equals
            srcs = [A] + [p.residual(A) for p in ways[1:]]
            cost = [int(plan.rate_curve(X, [steps], n_wide, seg_len)["bytes"][0]) + (p.overhead + len(geo_p) if p else len(geo))
                    for p, X in zip(ways, srcs)]
            pred, src = min(zip(ways, srcs, cost), key=lambda w: w[2])[:2]
        return keys, plan, src, geo if pred is None else geo_p, b"" if pred is None else pred.wrapper(), pred

    with torch.cuda.device(dev):
        if gop == 1:
            for lo in range(0, n, SEQ_CHUNK):
                chunk = VA[lo: lo + SEQ_CHUNK]
                _, geos, plans = zip(*[_keys_geometry_plan(V, J, geometry) for V, _ in chunk])
                Qs = _quantize(list(plans), [A for _, A in chunk], steps, n_wide)
                coded.update({lo + k: (geo, Q, b"") for k, (geo, Q) in enumerate(zip(geos, Qs))})
                flush()
        else:
            # anchors in display order, each predicted from the anchor before it in its GOP; the B candidates between two anchors
            # after the second of them. recon: anchor -> (keys, reconstruction), kept while a frame to come is predicted from it.
            order = sequence_plan(n, gop, bframes)
            last_use = {r: i for i, (_, refs) in enumerate(order) for r in refs}
            recon, prev = {}, None                                           # prev: the anchor before this one
            level_counts, pyramids = {}, {}                                  # (motion_levels) anchor -> its level counts, its coarse levels
            for i, (kind, refs) in enumerate(order):
                if kind == "B":
                    continue
                keys, plan, src, geo, wrap, pred = choose(i, VA[i][1], refs[0] if refs else None)
                Q = _quantize([plan], [src], steps, n_wide)[0]
                if i in last_use:                                            # a frame to come is predicted from this one
                    C = _reconstruct([plan], [Q], steps, n_wide)[0]
                    recon[i] = (keys, C if pred is None else pred.restore(C))
                coded[i] = (geo, Q, wrap)
                between = [] if prev is None else [j for j in range(prev + 1, i) if order[j][0] == "B"]
                if between:                                                  # no frame is predicted from these: one set of transform launches
                    ways = [choose(j, VA[j][1], *order[j][1]) for j in between]
                    Qs = _quantize([w[1] for w in ways], [w[2] for w in ways], steps, n_wide)
                    coded.update({j: (w[3], Q, w[4]) for j, w, Q in zip(between, ways, Qs)})
                for r in [r for r in recon if last_use[r] <= i]:             # (a B candidate lies before its second anchor)
                    del recon[r]
                    level_counts.pop(r, None)
                    pyramids.pop(r, None)
                prev = i
                flush()
    return _pack_parts(parts)


def decode_sequence_bytes(blob, frames=None, device="cuda", max_voxels=None, max_frames=None):
    """-> [(V_int (N_i, 3) int64, C_rec (N_i, D) float32)] for the frame indices ``frames`` (default: all, in order), each what
    ``decode_frame_bytes(sequence_frame(blob, i))`` returns, bit for bit. The requested indices are closed under dependencies, back
    to the nearest intra frame, and that set is decoded once, in ascending order; the requested frames are returned in the order
    asked. The geometry is decoded frame by frame (a predicted geometry section against the keys of the frame's reference, which is
    decoded before it); consecutive frames of the set with the same (D, seg_len, n_wide, steps) share one
    entropy launch (``SegmentedCoder.decode_ragged``) and one set of inverse transform launches (a frame of exactly D voxels goes
    alone). ``max_voxels`` per frame and ``max_frames`` are checked before anything is allocated from the numbers of the blob.
    ``ValueError`` for a corrupt container; a corrupt frame is named by its index -- for a header or an attribute length table that
    does not add up before any device work, for a corrupt geometry section or a segment outside its payload when that frame's
    group is decoded.

    A predicted frame (RAHTP001) comes back as (V_int, fl(R_rec + P)): R_rec is what ``decode_frame_bytes`` returns for its inner
    frame, P is ``ops.predict`` of its reference's decoded attributes (``ops.predict_mc`` under the frame's motion field for an
    RAHTM001 frame, whose ``block_log2`` and block count are checked against the inner frame's geometry header with the rest).
    R_rec does not depend on the prediction, so the entropy decode and the inverse transform of a group stay batched, for I and P
    frames alike; only the additions run in frame order. A predicted frame at index 0, a ``ref_back`` below 1 or reaching before
    frame 0, ``up`` outside 0 .. 3, a truncated wrapper, an inner frame ``parse_frame`` refuses or one whose J or D is not its
    reference's are refused from the headers, before any device work."""
    import torch
    off = parse_sequence(blob, max_frames)
    n = len(off) - 1
    if frames is None:
        frames = range(n)
    try:
        idx = [int(i) for i in frames]
    except (TypeError, ValueError):
        raise ValueError("decode_sequence_bytes: frames is a list of frame indices") from None
    if any(not 0 <= i < n for i in idx):
        raise ValueError(f"decode_sequence_bytes: frame indices must be in 0 .. {n - 1}")
    dev = torch.device(device)
    heads = _frame_heads(memoryview(blob), off, idx, max_voxels)

    def same(i):
        # (a frame of exactly D voxels is a group of its own: decode_frame_bytes reads its square matrix as the encoder wrote it)
        h = heads[i]["h"]
        return (h["D"], heads[i]["seg_len"], h["n_wide"], tuple(h["steps"])) + ((i,) if h["N"] == h["D"] else ())
    done = {}                                                                # frame -> (V, C_rec or R_rec, keys)

    def geo_ref(i, group):
        # what a predicted geometry section is decoded against: the reference's keys, or its place in the group it shares with i
        r = heads[i]["ref"]
        if heads[i]["h"]["geometry_ref"] is None:
            return None
        return group.index(r) if r in group else done[r][2]
    for _, run in itertools.groupby(sorted(heads), key=same):
        run = list(run)
        for group in (run[lo: lo + SEQ_CHUNK] for lo in range(0, len(run), SEQ_CHUNK)):
            named = [(f"sequence container: frame {i}: ", heads[i]["fb"], heads[i]["h"], geo_ref(i, group)) for i in group]
            done.update(zip(group, _decode_group(named, dev, max_voxels)))
    with torch.cuda.device(dev):
        # a reference is whole before it is used: the anchors ascending, then the B frames, which are no frame's reference
        for i in sorted(done, key=lambda i: (heads[i]["kind"] == "B", i)):
            hd = heads[i]
            if hd["kind"] != "I":
                (_, C, keys), (_, C_ref, ref_keys) = done[i], done[hd["ref"]]
                motion, J = hd["motion"], hd["h"]["J"]
                if motion is not None:
                    block_first = ops.motion_blocks(keys, J, motion[0], len(motion[1]))
                    motion = (motion[0], *(torch.from_numpy(mv.copy()).to(dev) for mv in motion[1:]), block_first)
                ref1 = done[hd["ref1"]][2:0:-1] if hd["kind"] == "B" else None
                modes = hd["modes"]
                if modes is not None:                                        # (an RAHTB002 frame: the modes lie over the fields' blocks)
                    block_first = motion[-1] if motion is not None else ops.motion_blocks(keys, J, modes[0], len(modes[1]))
                    modes = (modes[0], torch.from_numpy(modes[1].copy()).to(dev), block_first)
                _Predictor(keys, (ref_keys, C_ref), J, hd["up"], motion, ref1=ref1, modes=modes).restore(C)
    return [done[i][:2] for i in idx]



def _merge_cells(cells, group, limit=ops.REGION_MAX_RANGES):
    """ascending, duplicate-free first cells of aligned groups of ``group`` cells (a device tensor) -> the ascending list of
    disjoint ranges (c0, c1) they cover, neighbours merged. More than ``limit`` ranges are brought down to it by closing the
    narrowest gaps between them: a needed set may hold more cells than it must, never fewer."""
    import torch
    if cells.shape[0] == 0:
        return []
    brk = cells[1:] != cells[:-1] + group
    one = torch.ones(1, dtype=torch.bool, device=cells.device)
    lo, hi = cells[torch.cat([one, brk])].tolist(), (cells[torch.cat([brk, one])] + group).tolist()
    if len(lo) > limit:
        gaps = np.asarray(lo[1:]) - np.asarray(hi[:-1])
        keep = np.sort(np.argsort(gaps, kind="stable")[len(gaps) - (limit - 1):])      # the limit - 1 widest gaps stay open
        lo, hi = [lo[0]] + [lo[g + 1] for g in keep], [hi[g] for g in keep] + [hi[-1]]
    return list(zip(lo, hi))


def _unite_ranges(range_lists, limit=ops.REGION_MAX_RANGES):
    """ascending lists of disjoint cell ranges -> the ascending list of disjoint ranges that covers them all, overlapping and
    touching ranges merged; more than ``limit`` ranges are brought down to it as ``_merge_cells`` does, by closing the narrowest
    gaps. One list is what it is: nothing is merged in it."""
    lists = [r for r in range_lists if r]
    if len(lists) <= 1:
        return list(lists[0]) if lists else []
    out = []
    for c0, c1 in sorted(r for rs in lists for r in rs):
        if out and c0 <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], c1))
        else:
            out.append((c0, c1))
    if len(out) > limit:
        lo, hi = [r[0] for r in out], [r[1] for r in out]
        gaps = np.asarray(lo[1:]) - np.asarray(hi[:-1])
        keep = np.sort(np.argsort(gaps, kind="stable")[len(gaps) - (limit - 1):])      # the limit - 1 widest gaps stay open
        out = list(zip([lo[0]] + [lo[g + 1] for g in keep], [hi[g] for g in keep] + [hi[-1]]))
    return out


def _region_motion(block_first, mv, rows, dev):
    """The motion field of a region: ``_region_blocks`` for one field -> (block_first, mv) as ``ops.predict_mc`` takes them."""
    first, (field,) = _region_blocks(block_first, rows, dev, mv)
    return first, field


def _region_blocks(block_first, rows, dev, *per_block):
    """The blocks of a region: ``block_first`` (n_blocks + 1 rows of the whole frame), ``rows`` = [(a, b)] of the region's ranges,
    ascending, and any number of ``per_block`` tensors of a frame (a motion field (n_blocks, 3), the block modes (n_blocks,); None
    stays None) -> (block_first over the rows of the region matrix (the ranges concatenated), [every tensor over the same blocks]),
    as ``ops.predict_mc`` and ``ops.predict_bi`` take them: the blocks that have rows in a range, range by range, each with its
    first row in the region. A block that two ranges cut is listed once per range. One selection serves every tensor."""
    import torch
    lo = torch.tensor([a for a, _ in rows], dtype=torch.int64, device=dev)
    hi = torch.tensor([b for _, b in rows], dtype=torch.int64, device=dev)
    k0 = torch.searchsorted(block_first, lo, right=True) - 1                 # the block of row a; the first block that starts at b or later
    k1 = torch.searchsorted(block_first[:-1], hi, right=False)
    idx, first, base = [], [], 0
    for (a, b), b0, b1 in zip(rows, k0.tolist(), k1.tolist()):
        if b > a:
            idx.append(torch.arange(b0, b1, device=dev))
            first.append(torch.clamp(block_first[b0:b1] - a, min=0) + base)
            base += b - a
    first.append(torch.tensor([base], dtype=torch.int64, device=dev))
    pick = torch.cat(idx)
    return torch.cat(first), [None if t is None else t[pick].contiguous() for t in per_block]


def decode_sequence_region(blob, i, depth, cells, device="cuda", max_voxels=None, max_frames=None, keys=None):
    """The voxels of the depth-``depth`` cells ``cells = (c0, c1)`` of frame ``i`` of a sequence container, whatever its kind, from
    the bytes they depend on -> (V_int (n, 3) int64, C_rec (n, D) float32, info): rows [a, b) of
    ``decode_sequence_bytes(blob, [i])[0]``, bit for bit. The argument rules are ``decode_region_bytes``'; for an intra frame so is
    the work.

    A predicted frame is resolved along its chain i -> ref(i) -> ... -> the intra frame (``ref_back`` of every wrapper is
    honoured). Every chain frame f has a NEEDED SET S_f, an ascending list of disjoint ranges of depth-``depth`` cells: S_i =
    [cells]; for f predicted from g, S_g holds every cell with a reference voxel that the predictor of f can resolve for a row of f
    inside S_f (``ops.region_needs``: the cell of the row's key, shifted by its block's vector under a motion field; a row whose
    shifted voxel leaves the cube asks for nothing), widened to the aligned group of cells an ``up``-cell covers where ``up > J -
    depth``, neighbours merged. The geometry of a chain frame is decoded whole, its attributes for S_f only
    (``decode_cells_bytes``' core); then the chain is replayed from the intra frame on with the one predictor on the region
    matrices -- the keys and the reconstruction of S_g as the reference, and under a motion field the blocks that have rows in S_f.

    A chain frame whose geometry section is predicted needs the WHOLE keys of its reference before its own can be
    decoded: the reference's geometry is then decoded (and ``geometry_decoded`` set) even where nothing else is needed of that
    frame -- its section lies inside the bytes listed for it either way -- unless ``keys`` holds the predicted frame already.

    ``keys``: {frame index: keys} as an earlier call returned in ``info["keys"]``; the frames in it skip the geometry decode.
    info: chain (the frame indices, intra first), frames ({f: ranges (S_f), rows, n_cells, segments_decoded, segments_total,
    byte_ranges ((offset, length) within the SEQUENCE blob), bytes_needed, geometry_decoded}; a frame nothing is needed of has no
    ranges and the bytes of an empty region: its headers, which the walk along the chain reads), bytes_needed (the sum over the
    chain), byte_ranges (the sequence header's bytes, then every chain frame's: everything outside them may be missing), keys.
    ``ValueError`` as ``decode_sequence_bytes`` raises it, a frame named by its index; what the headers show is refused before any
    device work. This is the one-range call of ``decode_sequence_cells``' core for I, P and motion-compensated frames; a B frame is
    refused here and goes through ``decode_sequence_cells``."""
    import torch
    who = "decode_sequence_region"
    off = parse_sequence(blob, max_frames)
    n = len(off) - 1
    try:
        i, depth, (c0, c1) = int(i), int(depth), (int(c) for c in cells)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: i and depth are integers, cells a pair of integers") from None
    if not 0 <= i < n:
        raise ValueError(f"{who}: the frame index must be in 0 .. {n - 1}")
    heads = _frame_heads(memoryview(blob), off, [i], max_voxels)
    if heads[i]["kind"] == "B":
        raise ValueError(f"{who}: frame {i} is a B frame: a region of a frame with two references is not supported, decode it whole "
                         "or through decode_sequence_cells")
    _region_depth(who, heads[i]["h"], depth)                                 # (a chain has one J: _frame_heads)
    if not 0 <= c0 < c1 <= 8 ** depth:
        raise ValueError(f"{who}: cells must satisfy 0 <= c0 < c1 <= 8^depth = {8 ** depth}")
    if keys is not None and not isinstance(keys, dict):
        raise ValueError(f'{who}: keys is the dict an earlier call returned in info["keys"]')
    return _decode_sequence_cells(who, blob, off, heads, i, depth, [(c0, c1)], torch.device(device), max_voxels, keys)


def decode_sequence_cells(blob, i, depth, ranges, device="cuda", max_voxels=None, max_frames=None, keys=None):
    """``decode_sequence_region`` for a SET of cell ranges and for a frame of ANY kind, B frames (RAHTB001, RAHTB002) included
     -> (V_int, C_rec, info): the rows of the ranges of ``decode_sequence_bytes(blob, [i])[0]``, concatenated, bit for
    bit. ``ranges``: as ``decode_cells_bytes`` takes them, an ascending list of 1 .. 512 disjoint pairs of depth-``depth`` cells.

    The dependencies of a B frame are a small DAG, i -> (a, c), c -> a, a -> ... -> the intra frame: frame i is walked first, then
    every other frame of the closure in descending index, so that a frame is visited after every frame that needs it. A frame's
    needed set is the UNION of what its dependants ask of it (each dependant's cells as ranges under its own ``up`` group, the lists
    united on the host, brought down to 512 ranges by closing the narrowest gaps: a needed set may hold more than it must, never
    less). A B frame asks both references in one pass over the region's keys (``ops.region_needs_bi``) under the region's blocks, both
    fields and the block modes: a block in mode 1 asks nothing of reference 1, one in mode 2 nothing of reference 0. A frame nothing
    is needed of is an empty region: its headers only. The replay runs in ascending order, frame i last, through the one predictor
    on the region matrices; a reference whose needed rows are empty is taken out through the modes (with reference 1 empty 0 -> 1
    and 2 -> 3, with reference 0 empty 0 -> 2 and 1 -> 3), which gives the predictor's bits: for a row whose cell is empty in one
    reference the two-reference prediction is the one-reference prediction of the other.

    info: ``decode_sequence_region``'s, with chain the ascending list of the frames of the closure and frames[f]["ranges"]
    possibly a union; ``keys`` as there. ``ValueError`` as ``decode_sequence_bytes`` and ``decode_cells_bytes`` raise it."""
    import torch
    who = "decode_sequence_cells"
    off = parse_sequence(blob, max_frames)
    n = len(off) - 1
    try:
        i, depth, ranges = int(i), int(depth), [(int(c0), int(c1)) for c0, c1 in ranges]
    except (TypeError, ValueError):
        raise ValueError(f"{who}: i and depth are integers, ranges a list of pairs of integers") from None
    if not 0 <= i < n:
        raise ValueError(f"{who}: the frame index must be in 0 .. {n - 1}")
    heads = _frame_heads(memoryview(blob), off, [i], max_voxels)
    _region_depth(who, heads[i]["h"], depth)                                 # (a closure has one J: _frame_heads)
    _region_ranges(who, ranges, depth)
    if keys is not None and not isinstance(keys, dict):
        raise ValueError(f'{who}: keys is the dict an earlier call returned in info["keys"]')
    return _decode_sequence_cells(who, blob, off, heads, i, depth, ranges, torch.device(device), max_voxels, keys)


def _decode_sequence_cells(who, blob, off, heads, i, depth, ranges, dev, max_voxels, keys):
    """THE region decoder of a sequence, for checked arguments: ``heads`` is ``_frame_heads``' closure of frame ``i``."""
    import torch
    chain = sorted(heads)
    J = heads[i]["h"]["J"]
    tl = 3 * (J - depth)
    part, frames, keys_out = {}, {}, {}                                      # part: frame -> (V, C, region keys, region blocks)
    asked = {f: [] for f in chain}                                           # frame -> the range lists its dependants ask of it
    given, decoded = keys or {}, set()                                       # decoded: the frames whose geometry this call decodes

    def whole_keys(f):
        # the keys of chain frame f: handed in, decoded before, or decoded here -- a predicted section after its reference's
        todo = [f]
        while todo[-1] not in keys_out and given.get(todo[-1]) is None and heads[todo[-1]]["h"]["geometry_ref"] is not None:
            todo.append(heads[todo[-1]]["ref"])
        for g in reversed(todo):
            if g not in keys_out:
                if given.get(g) is not None:
                    keys_out[g] = given[g]
                    continue
                (go, gl), fb = heads[g]["h"]["geometry"], heads[g]["fb"]
                rk = keys_out[heads[g]["ref"]] if heads[g]["h"]["geometry_ref"] is not None else None
                try:
                    keys_out[g] = OctreeCoder.decode(fb[go: go + gl], dev, max_voxels, rk)
                except ValueError as e:
                    raise ValueError(f"sequence container: frame {g}: {e}") from None
                decoded.add(g)
        return keys_out[f]

    with torch.cuda.device(dev):
        # frame i, then down the other frames: a B frame is no frame's reference and every other reference points backwards, so
        # every frame comes after all frames that need it
        for f in [i] + [g for g in reversed(chain) if g != i]:
            hd = heads[f]
            h, fb = hd["h"], hd["fb"]
            base = off[f + 1] - len(fb)                                      # where the inner frame starts in the sequence blob
            S = ranges if f == i else _unite_ranges(asked[f])
            if not S:                                                        # nothing but what the walk along the chain reads: as an empty region
                ao, al = h["attributes"]
                head = base - off[f] + ao + SegmentedCoder._parse(fb[ao: ao + al], h["N"] * h["D"])[6]
                frames[f] = dict(ranges=[], rows=0, n_cells=0, segments_decoded=0,
                                 segments_total=(h["N"] + hd["seg_len"] - 1) // hd["seg_len"], byte_ranges=[(off[f], head)],
                                 bytes_needed=head, geometry_decoded=False)
                continue
            kf = whole_keys(f)
            try:
                V, C, info, kr = _decode_cells(who, fb, h, depth, S, dev, max_voxels, kf)
            except ValueError as e:
                raise ValueError(f"sequence container: frame {f}: {e}") from None
            spans = [(base + o, ln) for o, ln in info["byte_ranges"]]
            spans[0] = (off[f], spans[0][1] + base - off[f])                 # (the wrapper of a predicted frame lies in front)
            frames[f] = dict(ranges=S, rows=int(kr.shape[0]), n_cells=info["n_cells"], segments_decoded=info["segments_decoded"],
                             segments_total=info["segments_total"], byte_ranges=spans, bytes_needed=sum(ln for _, ln in spans),
                             geometry_decoded=False)
            motion, group = None, 8 ** max(hd["up"] - (J - depth), 0)
            if hd["kind"] == "P" and kr.shape[0]:
                if hd["motion"] is not None:
                    m, mv = hd["motion"]
                    motion = (m,) + _region_motion(ops.motion_blocks(info["keys"], J, m, len(mv)), torch.from_numpy(mv.copy()).to(dev),
                                                   info["rows"], dev)[::-1]
                need = ops.region_needs(kr, J, tl, hd["up"], *((None, None, 0) if motion is None else (motion[2], motion[1], motion[0])))
                asked[hd["ref"]].append(_merge_cells(need, group))
            elif hd["kind"] == "B" and kr.shape[0]:
                # the region's blocks, once for both fields and the modes: (block_log2, block_first, mv0, mv1, mode), or None
                blocks = hd["motion"] or hd["modes"]
                if blocks is not None:
                    per_block = (*(hd["motion"][1:] if hd["motion"] else (None, None)), hd["modes"][1] if hd["modes"] else None)
                    per_block = [None if t is None else torch.from_numpy(t.copy()).to(dev) for t in per_block]
                    bf = ops.motion_blocks(info["keys"], J, blocks[0], len(blocks[1]))
                    bf, per_block = _region_blocks(bf, info["rows"], dev, *per_block)
                    motion = (blocks[0], bf, *per_block)
                need = ops.region_needs_bi(kr, J, tl, hd["up"], *(() if motion is None else (motion[1], *motion[2:], motion[0])))
                for g, cells in zip((hd["ref"], hd["ref1"]), need):
                    asked[g].append(_merge_cells(cells, group))
            part[f] = (V, C, kr, motion)
        # and up again, frame i last: a reference is whole before it is used
        for f in [g for g in chain if g != i] + [i]:
            hd = heads[f]
            if f not in part or not part[f][2].shape[0]:
                continue
            _, C, kr, motion = part[f]
            refs = [(part[g][2], part[g][1]) if g in part and part[g][2].shape[0] else None for g in (hd["ref"], hd["ref1"])]
            if hd["kind"] == "P" and refs[0] is not None:
                _Predictor(kr, refs[0], J, hd["up"], motion).restore(C)
            elif hd["kind"] == "B" and (refs[0] is not None or refs[1] is not None):
                fields = modes = None
                if motion is not None:
                    m, bf, mv0, mv1, mode = motion
                    fields = None if mv0 is None else (m, mv0, mv1, bf)
                    modes = None if mode is None else (m, mode, bf)
                if refs[0] is None or refs[1] is None:
                    # a reference without needed rows goes out through the modes (the ops take no empty reference); the other one
                    # stands in for it and is never read in its place
                    if modes is None:
                        m, bf = (motion[0], motion[1]) if motion is not None else (J, torch.tensor([0, kr.shape[0]], dtype=torch.int64, device=dev))
                        modes = (m, torch.zeros(bf.shape[0] - 1, dtype=torch.uint8, device=dev), bf)
                    table = [1, 1, 3, 3] if refs[1] is None else [2, 3, 2, 3]
                    modes = (modes[0], torch.tensor(table, dtype=torch.uint8, device=dev)[modes[1].long()], modes[2])
                    refs = [refs[0] or refs[1], refs[1] or refs[0]]
                _Predictor(kr, refs[0], J, hd["up"], fields, ref1=refs[1], modes=modes).restore(C)
    for f in decoded:
        frames[f]["geometry_decoded"] = True
    byte_ranges = [(0, off[0])] + [r for f in chain for r in frames[f]["byte_ranges"]]
    info = dict(chain=chain, frames=frames, bytes_needed=sum(fr["bytes_needed"] for fr in frames.values()), byte_ranges=byte_ranges,
                keys=keys_out)
    return part[i][0], part[i][1], info
