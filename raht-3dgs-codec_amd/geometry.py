"""Lossless geometry: the breadth-first octree occupancy code of a frame's occupied voxels (include/raht.h, "Octree geometry";
csrc/octree.hip), optionally entropy-coded with the segmented RLGR coder fed the frequency rank of every occupancy byte.

    blob = OctreeCoder.encode(keys_sorted, J)            # strictly ascending Morton keys (CUDA int64 / uint64) -> bytes
    keys = OctreeCoder.decode(blob, "cuda")              # the same keys, from the bytes alone

The section on the wire: ``OCTG0001`` | int64 J, N, mode, n_nodes, seg_len | int64 n_0 ... n_J | body. Mode 0: the occupancy
bytes. Mode 1: the 256-byte table ``byte_of_rank``, the uint32 length of every RLGR segment, the streams in 4-byte slots.
The header comes off the wire: ``parse`` checks every size against the blob and the caller's cap before anything is
allocated from it, and the kernels bound every store by the header's counts, so a corrupt section raises ``ValueError``.

A frame of a sequence may code its geometry against the keys of a REFERENCE frame (include/raht.h, "Predicted octree geometry";
csrc/octree_inter.hip): every occupancy byte XORed with the reference's occupancy byte of the same cell.

    blob = OctreeCoder.encode(keys_sorted, J, ref_keys=ref)      # ``OCTP0001`` | int64 J, N, mode, n_nodes, seg_len, N_ref, n_used |
    keys = OctreeCoder.decode(blob, "cuda", ref_keys=ref)        # int64 n_0 ... n_J | body laid out as above

Byte 0 is an ordinary residual value (normally the most frequent one), so the header's ``n_used`` -- the number of byte values
that occur -- bounds the symbols of mode 1 (mode 0 writes 0 there).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .rlgr import SegmentedCoder, to_host

MAGIC = b"OCTG0001"
P_MAGIC = b"OCTP0001"                                          # a section predicted from a reference frame's keys
MODES = {"raw": 0, "rlgr": 1}
MAX_J = 21
# Segment length of the entropy-coded occupancy stream. Not the attribute coder's 2048: the coder runs one lane per segment,
# and ONE channel of n_nodes symbols at 2048 is a sixteenth of the lanes an attribute frame has ("Octree geometry").
DEFAULT_SEG_LEN = 256


def _stream(device):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _check_keys(keys, what):
    import torch
    if not isinstance(keys, torch.Tensor) or not keys.is_cuda:
        raise RuntimeError(f"OctreeCoder.{what}: keys must be a CUDA (HIP) tensor; there is no CPU path")
    if keys.dtype not in (torch.int64, torch.uint64) or keys.dim() != 1 or keys.shape[0] < 1:
        raise ValueError(f"OctreeCoder.{what}: keys must be a non-empty 1-D int64/uint64 tensor")
    return keys.contiguous()


def _counts_array(counts, J):
    if len(counts) != J + 1:
        raise ValueError("counts must hold n_0 ... n_J")
    return (C.c_int64 * (J + 1))(*[int(c) for c in counts])


class OctreeCoder:
    """The geometry stage. Stateless: static methods only."""

    # -- the device stages, one entry point each (tools/time_geometry.py times them one by one) -------------------------------
    @staticmethod
    def counts(keys_sorted, J):
        """-> [n_0, ..., n_J]: nodes per octree level. Also the input check: raises RahtError when the keys are not strictly
        ascending or not below 8^J. Synchronises."""
        import torch
        k = _check_keys(keys_sorted, "counts")
        out = (C.c_int64 * (int(J) + 1))() if 1 <= int(J) <= MAX_J else (C.c_int64 * 1)()
        with torch.cuda.device(k.device):
            check(_lib.lib().raht_octree_counts(C.c_void_p(k.data_ptr()), k.shape[0], int(J), out, _stream(k.device)))
        return [int(x) for x in out]

    @staticmethod
    def occupancy(keys_sorted, J, counts, out=None):
        """-> the occupancy stream, (n_nodes,) uint8 on the keys' device; enqueued only"""
        import torch
        k = _check_keys(keys_sorted, "occupancy")
        n_nodes = int(sum(counts[:-1]))
        if out is None:
            out = torch.empty(max(n_nodes, 1), dtype=torch.uint8, device=k.device)
        with torch.cuda.device(k.device):
            check(_lib.lib().raht_octree_encode(C.c_void_p(k.data_ptr()), k.shape[0], int(J), _counts_array(counts, int(J)),
                                                C.c_void_p(out.data_ptr()), _stream(k.device)))
        return out[:n_nodes]

    @staticmethod
    def keys_from_occupancy(occ, counts, J, bad, out=None):
        """occupancy stream + header counts -> (N,) int64 keys; ``bad`` (int32 CUDA tensor, one element) is raised for a stream
        that does not go with the counts. Enqueued only."""
        import torch
        if not occ.is_cuda or occ.dtype != torch.uint8 or occ.dim() != 1 or not occ.is_contiguous() or occ.shape[0] != sum(counts[:-1]):
            raise ValueError("OctreeCoder.keys_from_occupancy: expected the n_nodes occupancy bytes as a contiguous uint8 CUDA tensor")
        if out is None:
            out = torch.empty(int(counts[-1]), dtype=torch.int64, device=occ.device)
        with torch.cuda.device(occ.device):
            check(_lib.lib().raht_octree_decode(C.c_void_p(occ.data_ptr()), _counts_array(counts, int(J)), int(J),
                                                C.c_void_p(out.data_ptr()), C.c_void_p(bad.data_ptr()), _stream(occ.device)))
        return out

    @staticmethod
    def residual(keys_sorted, J, counts, ref_keys, out=None):
        """-> the residual stream against the reference's keys (occupancy ^ the reference's occupancy of the same cells),
        (n_nodes,) uint8; enqueued only"""
        import torch
        k, r = _check_keys(keys_sorted, "residual"), _check_keys(ref_keys, "residual")
        n_nodes = int(sum(counts[:-1]))
        if out is None:
            out = torch.empty(max(n_nodes, 1), dtype=torch.uint8, device=k.device)
        with torch.cuda.device(k.device):
            check(_lib.lib().raht_octree_encode_inter(C.c_void_p(k.data_ptr()), k.shape[0], int(J), _counts_array(counts, int(J)),
                                                      C.c_void_p(r.data_ptr()), r.shape[0], C.c_void_p(out.data_ptr()), _stream(k.device)))
        return out[:n_nodes]

    @staticmethod
    def keys_from_residual(res, counts, J, ref_keys, bad, out=None):
        """``keys_from_occupancy`` for a residual stream and the reference's keys. Enqueued only."""
        import torch
        if not res.is_cuda or res.dtype != torch.uint8 or res.dim() != 1 or not res.is_contiguous() or res.shape[0] != sum(counts[:-1]):
            raise ValueError("OctreeCoder.keys_from_residual: expected the n_nodes residual bytes as a contiguous uint8 CUDA tensor")
        r = _check_keys(ref_keys, "keys_from_residual")
        if out is None:
            out = torch.empty(int(counts[-1]), dtype=torch.int64, device=res.device)
        with torch.cuda.device(res.device):
            check(_lib.lib().raht_octree_decode_inter(C.c_void_p(res.data_ptr()), _counts_array(counts, int(J)), int(J),
                                                      C.c_void_p(r.data_ptr()), r.shape[0], C.c_void_p(out.data_ptr()),
                                                      C.c_void_p(bad.data_ptr()), _stream(res.device)))
        return out

    @staticmethod
    def symbols(occ, out=None):
        """occupancy bytes -> ((1, n_nodes) int32 ranks on the device, byte_of_rank (256,) uint8 numpy). Synchronises."""
        import torch
        n = occ.shape[0]
        if out is None:
            out = torch.empty((1, n), dtype=torch.int32, device=occ.device)
        table = np.zeros(256, np.uint8)
        with torch.cuda.device(occ.device):
            check(_lib.lib().raht_octree_symbols(C.c_void_p(occ.data_ptr()), n, table.ctypes.data_as(C.c_void_p),
                                                 C.c_void_p(out.data_ptr()), _stream(occ.device)))
        return out, table

    @staticmethod
    def bytes_from_symbols(sym, table, bad, out=None, n_used=None):
        """ranks + table -> occupancy bytes; a rank outside the table's used part raises ``bad``. ``n_used``: the number of ranks
        in use, for the residual bytes of a predicted section (default: they end where byte 0 stands). Enqueued only."""
        import torch
        n = sym.numel()
        if out is None:
            out = torch.empty(n, dtype=torch.uint8, device=sym.device)
        table = np.ascontiguousarray(table, dtype=np.uint8)
        args = (C.c_void_p(out.data_ptr()), C.c_void_p(bad.data_ptr()), _stream(sym.device))
        with torch.cuda.device(sym.device):
            if n_used is None:
                check(_lib.lib().raht_octree_bytes(C.c_void_p(sym.data_ptr()), n, table.ctypes.data_as(C.c_void_p), *args))
            else:
                check(_lib.lib().raht_octree_bytes_used(C.c_void_p(sym.data_ptr()), n, table.ctypes.data_as(C.c_void_p), int(n_used), *args))
        return out

    # -- the section ----------------------------------------------------------------------------------------------------------
    @staticmethod
    def encode(keys_sorted, J, entropy="rlgr", seg_len=None, ref_keys=None):
        """Strictly ascending Morton keys < 8^J on the GPU -> the geometry section (bytes). ``entropy``: "rlgr" (mode 1) or "raw"
        (mode 0). ``seg_len``: symbols per RLGR segment (default ``DEFAULT_SEG_LEN``); it travels in the header. ``ref_keys``: the
        keys of a reference frame of the same J (strictly ascending, on the GPU) -- the section is then a predicted one
        (``OCTP0001``) that decodes with the same keys only."""
        if entropy not in MODES:
            raise ValueError('OctreeCoder.encode: entropy must be "rlgr" or "raw"')
        J = int(J)
        k = _check_keys(keys_sorted, "encode")
        r = None if ref_keys is None else _check_keys(ref_keys, "encode")
        counts = OctreeCoder.counts(k, J)
        n_nodes = sum(counts[:-1])
        occ = OctreeCoder.occupancy(k, J, counts) if r is None else OctreeCoder.residual(k, J, counts, r)
        S, n_used = 0, 0
        if entropy == "rlgr":
            S = DEFAULT_SEG_LEN if seg_len is None else int(seg_len)
            sym, table = OctreeCoder.symbols(occ)
            if r is not None:
                n_used = int(sym.max().item()) + 1                           # ranks ascend without gaps over the values that occur
            sc = SegmentedCoder(n_nodes, 1, S, 0, k.device)
            sc.encode(sym)
            _, lens, payload = sc.container_parts()
            body = table.tobytes() + lens.tobytes() + payload.tobytes()
        else:
            body = to_host(occ).tobytes()
        head = [J, k.shape[0], MODES[entropy], n_nodes, S]
        if r is None:
            return MAGIC + np.array(head + counts, np.int64).tobytes() + body
        return P_MAGIC + np.array(head + [r.shape[0], n_used] + counts, np.int64).tobytes() + body

    @staticmethod
    def parse(blob, max_voxels=None):
        """The header of a geometry section, checked against the blob and the caller's cap (pure Python, nothing allocated on a
        device) -> dict: J, N, mode, n_nodes, seg_len, counts, body (offset of the body), length (bytes of the whole section),
        predicted (an ``OCTP0001`` section; then also N_ref and n_used); mode 1 also: table, nseg, lens_off, payload_off,
        payload_bytes. ``ValueError`` on anything that does not add up."""
        m = len(MAGIC)
        if bytes(blob[:m]) not in (MAGIC, P_MAGIC):
            raise ValueError("not an octree geometry section")
        predicted = bytes(blob[:m]) == P_MAGIC
        words = 7 if predicted else 5
        if len(blob) < m + 8 * words:
            raise ValueError("octree geometry: truncated header")
        J, N, mode, n_nodes, S, N_ref, n_used = ([int(x) for x in np.frombuffer(blob, np.int64, words, m)] + [None, None])[:7]
        if not 1 <= J <= MAX_J:
            raise ValueError("octree geometry: J outside 1 .. 21")
        body = m + 8 * words + 8 * (J + 1)
        if len(blob) < body:
            raise ValueError("octree geometry: truncated level counts")
        counts = [int(x) for x in np.frombuffer(blob, np.int64, J + 1, m + 8 * words)]
        if not 1 <= N < 2 ** 31 or mode not in (0, 1):
            raise ValueError("octree geometry: implausible header")
        if predicted and not 1 <= N_ref < 2 ** 31:
            raise ValueError("octree geometry: N_ref outside 1 .. 2^31 - 1")
        if predicted and not (1 <= n_used <= 256 if mode else n_used == 0):
            raise ValueError("octree geometry: n_used outside 1 .. 256 (mode 0: not 0)")
        if max_voxels is not None and N > int(max_voxels):
            raise ValueError(f"octree geometry: {N} voxels, more than the caller allows ({max_voxels})")
        if counts[0] != 1 or counts[J] != N:
            raise ValueError("octree geometry: the level counts do not start at the root or do not end at N")
        if any(not counts[g] <= counts[g + 1] <= 8 * counts[g] for g in range(J)):
            raise ValueError("octree geometry: implausible level counts")
        if n_nodes != sum(counts[:-1]):
            raise ValueError("octree geometry: n_nodes is not the sum of the internal levels")
        h = dict(J=J, N=N, mode=mode, n_nodes=n_nodes, seg_len=S, counts=counts, body=body, predicted=predicted)
        if predicted:
            h.update(N_ref=N_ref, n_used=n_used)
        if mode == 0:
            h["length"] = body + n_nodes
        else:
            if not 64 <= S < 2 ** 31:
                raise ValueError("octree geometry: implausible segment length")
            nseg = (n_nodes + S - 1) // S
            if len(blob) < body + 256 + 4 * nseg:
                raise ValueError("octree geometry: shorter than its header says")
            table = np.frombuffer(blob, np.uint8, 256, body)
            if not np.array_equal(np.sort(table), np.arange(256, dtype=np.uint8)):
                raise ValueError("octree geometry: the rank table is not a permutation of the byte values")
            lens = np.frombuffer(blob, np.uint32, nseg, body + 256).astype(np.int64)
            h.update(table=table, nseg=nseg, lens_off=body + 256, payload_off=body + 256 + 4 * nseg,
                     payload_bytes=int(((lens + 3) // 4 * 4).sum()))
            h["length"] = h["payload_off"] + h["payload_bytes"]
        if len(blob) < h["length"]:
            raise ValueError("octree geometry: shorter than its header says")
        return h

    @staticmethod
    def check_ref_keys(h, ref_keys, who="octree geometry"):
        """what a decoder is handed for the parsed section ``h``, before any device work: ``ValueError`` for a predicted section
        without its reference's keys, or with keys that are not N_ref of them"""
        if not h["predicted"]:
            return
        if ref_keys is None:
            raise ValueError(f"{who}: the geometry is predicted from another frame: its keys are needed (ref_keys)")
        if getattr(ref_keys, "ndim", None) != 1 or int(ref_keys.shape[0]) != h["N_ref"]:
            raise ValueError(f"{who}: the geometry is predicted from a frame of {h['N_ref']} voxels: ref_keys must be its keys")

    @staticmethod
    def decode(blob, device="cuda", max_voxels=None, ref_keys=None):
        """A geometry section -> the (N,) int64 Morton keys on ``device``. ``ref_keys``: the reference frame's keys, for a
        predicted section (ignored by an intra one). ``ValueError`` for a section that does not decode to what its header
        announces (reading that flag is the decoder's one synchronisation), and, before any device work, for a predicted section
        without ``ref_keys`` or with a number of them that is not the header's N_ref."""
        import torch
        h = OctreeCoder.parse(blob, max_voxels)
        OctreeCoder.check_ref_keys(h, ref_keys)
        dev = torch.device(device)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        if h["mode"] == 0:
            occ = torch.from_numpy(np.frombuffer(blob, np.uint8, h["n_nodes"], h["body"]).copy()).to(dev)
            flags = bad
        else:
            inner = (SegmentedCoder.MAGIC + np.array([h["n_nodes"], 1, h["seg_len"], 0, h["payload_bytes"]], np.int64).tobytes()
                     + bytes(blob[h["lens_off"]: h["length"]]))
            sc = SegmentedCoder.from_container(inner, dev, max_symbols=h["n_nodes"])
            occ = OctreeCoder.bytes_from_symbols(sc.decode(), h["table"], bad, n_used=h.get("n_used"))
            flags = sc.bad
        if h["predicted"]:
            keys = OctreeCoder.keys_from_residual(occ, h["counts"], h["J"], ref_keys, bad)
        else:
            keys = OctreeCoder.keys_from_occupancy(occ, h["counts"], h["J"], bad)
        if int((bad | flags).item()) != 0:
            raise ValueError("octree geometry: the section does not decode to what its header announces")
        return keys
