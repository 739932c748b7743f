"""RLGR entropy stage: drop-in for the reference's ``rlgr`` pybind module (vendored PyRLGR,
reference python/PyRLGR/src/libs/rlgr/bindings.cpp:34-57; call sites python/encode_3dgs.py:229-245),
backed by the byte-exact host coder in libraht_hip.so (csrc/rlgr.hip).

    m = membuf(); ns = m.rlgrWrite(seq, 1); m.close(); buf = m.get_buffer()
    ns, out = membuf(buf).rlgrRead(N, 1)

``seq`` may be a Python list (as in the reference) or -- much faster -- a numpy int32/int64 array.
``encode_channels`` / ``decode_channels`` code all columns of an (N, D) int32 matrix at once on host
threads, without the per-channel tensor -> list -> vector copies of the reference driver.
"""
import ctypes as C
import functools
import operator
import time

import numpy as np

_STAGING = {}

from . import _lib
from ._lib import check
from .ops import step_list


def _as_i32(seq):
    a = np.asarray(seq)
    if a.dtype != np.int32:
        if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 32 - 1):
            raise OverflowError("RLGR symbols must fit 32 bits")
        a = a.astype(np.int64).astype(np.uint32).view(np.int32) if a.size and a.max() > 2 ** 31 - 1 else a.astype(np.int32)
    return np.ascontiguousarray(a)


class membuf:
    """Same methods as the reference's ``rlgr.membuf``."""

    def __init__(self, in_buf=None):
        self._write = in_buf is None
        self._buf = np.zeros(0, np.uint8) if in_buf is None else np.ascontiguousarray(np.asarray(in_buf, dtype=np.uint8))

    def rlgrWrite(self, seq, flagSigned=1):
        a = _as_i32(seq)
        cap = int(_lib.lib().raht_rlgr_bound(a.shape[0]))
        out = np.empty(cap, np.uint8)
        n = C.c_int64()
        t0 = time.perf_counter_ns()
        check(_lib.lib().raht_rlgr_encode(a.ctypes.data_as(C.c_void_p), a.shape[0], 1, int(flagSigned),
                                          out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        ns = time.perf_counter_ns() - t0
        self._buf = out[: n.value].copy()
        return ns

    def rlgrRead(self, N, flagSigned=1):
        out = np.empty(int(N), np.int32)
        t0 = time.perf_counter_ns()
        check(_lib.lib().raht_rlgr_decode(self._buf.ctypes.data_as(C.c_void_p), self._buf.shape[0], int(N),
                                          int(flagSigned), out.ctypes.data_as(C.c_void_p), 1))
        ns = time.perf_counter_ns() - t0
        if not flagSigned:
            return ns, out.view(np.uint32).astype(np.int64).tolist()
        return ns, out.tolist()

    def close(self):
        pass                                   # the stream is padded to a byte boundary by rlgrWrite

    def get_buffer(self):
        return self._buf.tolist()              # the reference returns a Python list of ints

    def get_array(self):
        return self._buf                       # numpy view (no copy) for callers that can use it

    def buffer_size(self):
        return int(self._buf.shape[0])


def encode_channels(Q, flag_signed=1, nthreads=0, channel_major=False):
    """Q: (N, D) int32 numpy array, or (D, N) when channel_major (what ``transpose_on_device`` yields)
    -> (list of D uint8 arrays, seconds)."""
    Q = np.asarray(Q)
    if Q.dtype != np.int32 or Q.ndim != 2 or Q.strides[1] != 4:
        Q = np.ascontiguousarray(Q, dtype=np.int32)
    if channel_major:
        D, N = Q.shape
        ss, cs = 1, Q.strides[0] // 4
    else:
        N, D = Q.shape
        ss, cs = Q.strides[0] // 4, 1
    cap = int(_lib.lib().raht_rlgr_bound(N))
    out = np.empty((D, cap), np.uint8)
    nb = np.empty(D, np.int64)
    t0 = time.perf_counter()
    check(_lib.lib().raht_rlgr_encode_channels(Q.ctypes.data_as(C.c_void_p), N, D, ss, cs, int(flag_signed),
                                               out.ctypes.data_as(C.c_void_p), cap, nb.ctypes.data_as(C.c_void_p),
                                               int(nthreads)))
    dt = time.perf_counter() - t0
    return [out[c, : nb[c]].copy() for c in range(D)], dt


def decode_channels(streams, N, flag_signed=1, nthreads=0, channel_major=False):
    """streams: list of D uint8 arrays -> ((N, D) int32 array, or (D, N) when channel_major; seconds)."""
    D = len(streams)
    cap = max(1, max(int(np.asarray(s).shape[0]) for s in streams))
    bufs = np.zeros((D, cap), np.uint8)
    nb = np.empty(D, np.int64)
    for c, s in enumerate(streams):
        s = np.asarray(s, dtype=np.uint8)
        bufs[c, : s.shape[0]] = s
        nb[c] = s.shape[0]
    Q = np.empty((D, int(N)) if channel_major else (int(N), D), np.int32)
    ss, cs = (1, int(N)) if channel_major else (D, 1)
    t0 = time.perf_counter()
    check(_lib.lib().raht_rlgr_decode_channels(bufs.ctypes.data_as(C.c_void_p), cap, nb.ctypes.data_as(C.c_void_p), int(N), D,
                                               int(flag_signed), Q.ctypes.data_as(C.c_void_p), ss, cs, int(nthreads)))
    return Q, time.perf_counter() - t0


class ChannelCoder:
    """All channels of a frame through the host coder WITHOUT per-call glue: one arena for the D streams, kept across
    calls (worst case 13 bytes per symbol: virtual memory -- only what a stream really takes is ever touched), streams
    handed out as views, decoding straight from the arena into a caller-supplied (e.g. page-locked) array, and a threaded
    round-trip check. On the MI355X box the coder itself takes ~25 ms per direction for 3 M x 56 symbols; the per-call
    numpy allocations / copies / array_equal of encode_channels + decode_channels were another 110 ms."""

    def __init__(self, N, D, flag_signed=1, nthreads=0):
        self.N, self.D, self.flag, self.nthreads = int(N), int(D), int(flag_signed), int(nthreads)
        self.cap = int(_lib.lib().raht_rlgr_bound(self.N))
        self.arena = np.empty((self.D, self.cap), np.uint8)
        self.nb = np.zeros(self.D, np.int64)

    def encode(self, Qcm):
        """Qcm: (D, N) int32, channel-major contiguous -> seconds; streams in self.arena / self.nb"""
        if Qcm.dtype != np.int32 or Qcm.shape != (self.D, self.N) or not Qcm.flags.c_contiguous:
            raise ValueError("ChannelCoder.encode: expected a contiguous (D, N) int32 array")
        t0 = time.perf_counter()
        check(_lib.lib().raht_rlgr_encode_channels(Qcm.ctypes.data_as(C.c_void_p), self.N, self.D, 1, self.N, self.flag,
                                                   self.arena.ctypes.data_as(C.c_void_p), self.cap, self.nb.ctypes.data_as(C.c_void_p), self.nthreads))
        return time.perf_counter() - t0

    @property
    def size_bytes(self):
        return int(self.nb.sum())

    def streams(self):
        return [self.arena[c, : self.nb[c]] for c in range(self.D)]

    def decode(self, out):
        """-> seconds; out: (D, N) int32 contiguous (filled)"""
        if out.dtype != np.int32 or out.shape != (self.D, self.N) or not out.flags.c_contiguous:
            raise ValueError("ChannelCoder.decode: expected a contiguous (D, N) int32 array")
        t0 = time.perf_counter()
        check(_lib.lib().raht_rlgr_decode_channels(self.arena.ctypes.data_as(C.c_void_p), self.cap, self.nb.ctypes.data_as(C.c_void_p), self.N, self.D,
                                                   self.flag, out.ctypes.data_as(C.c_void_p), 1, self.N, self.nthreads))
        return time.perf_counter() - t0


def arrays_equal(a, b, nthreads=0):
    """threaded equality of two contiguous int32 arrays (the drivers' round-trip assertion, encode_3dgs.py:242-245)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != np.int32 or b.dtype != np.int32 or not a.flags.c_contiguous or not b.flags.c_contiguous:
        return bool(np.array_equal(a, b))
    first = C.c_int64()
    check(_lib.lib().raht_i32_equal(a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), a.size, int(nthreads), C.byref(first)))
    return first.value < 0


def pinned_like(shape, dtype, key):
    """a cached page-locked host tensor of at least this size (the codec's staging buffers), viewed as `shape`"""
    import torch
    n = int(np.prod(shape))
    buf = _STAGING.get(key)
    if buf is None or buf.numel() < n or buf.dtype != dtype:
        buf = torch.empty(max(n, 1), dtype=dtype, pin_memory=True)
        _STAGING[key] = buf
    return buf[:n].view(shape)


class SegmentedCoder:
    """The RLGR stage on the GPU (include/raht.h: raht_rlgr_seg_*): every channel in segments of ``seg_len`` symbols, every
    segment an independent RLGR stream -- byte-identical to the reference coder's output for that slice -- one lane per
    segment. ``encode`` takes the channel-major (D, N) int32 device tensor (``transpose_on_device`` of the quantized
    coefficients) and leaves the streams on the device; ``container()`` is what goes on the wire; ``decode`` rebuilds the
    (D, N) tensor on the device. Nothing but the compressed bytes ever crosses PCIe.

    ``wide``: the width of the device-side offset table. ``None`` (default) asks ``raht_rlgr_seg_offsets_width``: 32-bit offsets
    (``seg_off`` is ``torch.int32``) for every shape whose worst case stays below 4 GiB, 64-bit ones (``torch.int64``, the
    ``raht_rlgr_seg_*64`` entry points) above -- at ``seg_len = 2048`` from 330 M symbols per frame, e.g. 6 M x 56. ``True``
    forces the 64-bit table on any shape (same bytes), ``False`` the 32-bit one (which refuses the large shapes). The
    container on the wire holds no offsets and is the same either way."""
    MAGIC = b"RLGS0001"

    def __init__(self, N, D, seg_len=2048, flag_signed=1, device="cuda", payload_cap=None, wide=None):
        import torch
        self.N, self.D, self.S, self.flag = int(N), int(D), int(seg_len), int(flag_signed)
        self.nseg = (self.N + self.S - 1) // self.S
        self.G = self.nseg * self.D
        self.device = torch.device(device)
        if wide is None:
            width = _lib.lib().raht_rlgr_seg_offsets_width(self.N, self.D, self.S)
            if width < 0:
                check(width)
            wide = width == 64
        self.wide = bool(wide)
        self.seg_bytes = torch.empty(self.G, dtype=torch.int32, device=self.device)
        self.seg_off = torch.empty(self.G + 1, dtype=torch.int64 if self.wide else torch.int32, device=self.device)
        # encoder: what a raw dump would take, + slack (grown on demand); decoder (from_container): the payload it was handed
        self.cap = 4 * self.N * self.D + 64 * self.G if payload_cap is None else max(16, int(payload_cap))
        self.out = torch.empty(self.cap, dtype=torch.uint8, device=self.device)
        self.bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.total = 0

    def _stream(self):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _strides(self, Q, what):
        """(sym_stride, chan_stride) of a channel-major (D, N) or a row-major (N, D) int32 CUDA tensor"""
        import torch
        if not Q.is_cuda or Q.dtype != torch.int32 or Q.dim() != 2 or Q.stride(1) != 1:
            raise ValueError(f"SegmentedCoder.{what}: expected a 2-D int32 CUDA tensor with unit column stride")
        if tuple(Q.shape) == (self.D, self.N) and (self.D != self.N or Q.stride(0) >= self.N):
            return 1, Q.stride(0)
        if tuple(Q.shape) == (self.N, self.D):
            return Q.stride(0), 1
        raise ValueError(f"SegmentedCoder.{what}: expected a (D, N) channel-major or an (N, D) row-major tensor")

    def encode(self, Q):
        """Q: (D, N) channel-major OR (N, D) row-major int32 CUDA tensor (the latter: the quantized coefficients as forward_quant
        returns them, no transpose) -> total container payload bytes (synchronises: it returns a size). Same container either way."""
        self._encode_core("one", [self], [Q], [self._strides(Q, "encode")])
        return self.total

    @property
    def size_bytes(self):
        """bytes of the container: header + length table + streams"""
        return len(self.MAGIC) + 5 * 8 + 4 * self.G + self.total

    def container_parts(self):
        """-> (header bytes, uint32 lengths (G,), payload uint8 (total,)): the container without joining it. The payload comes down
        through the cached page-locked staging buffer (57 GB/s) and aliases it until the next ``to_host`` of a uint8 tensor."""
        hdr = self.MAGIC + np.array([self.N, self.D, self.S, self.flag, self.total], np.int64).tobytes()
        lens = to_host(self.seg_bytes).view(np.uint32).copy()
        return hdr, lens, to_host(self.out[: self.total])

    def container(self):
        """-> bytes: magic | N, D, seg_len, flag, payload bytes (int64 each) | uint32 length of every segment | the streams, each in
        a 4-byte slot. Only the compressed bytes come down from the device."""
        hdr, lens, payload = self.container_parts()
        return hdr + lens.tobytes() + payload.tobytes()

    @classmethod
    def _parse(cls, blob, max_symbols=None):
        """The header and the WHOLE length table of a container, checked against the blob before anything is allocated from them
        (pure host code) -> (N, D, seg_len, flag, total, lens int64 (G,), payload offset). ``ValueError`` when they do not add up."""
        m = len(cls.MAGIC)
        if bytes(blob[:m]) != cls.MAGIC:
            raise ValueError("not a segmented RLGR container")
        if len(blob) < m + 40:
            raise ValueError("segmented RLGR container: truncated header")
        N, D, S, flag, total = [int(x) for x in np.frombuffer(blob, np.int64, 5, m)]
        # the header comes off the wire: sizes are checked against the blob BEFORE anything is allocated from them
        if not (1 <= N < 2 ** 31 and 1 <= D <= 65536 and 64 <= S < 2 ** 31 and flag in (0, 1) and 0 <= total <= len(blob)):
            raise ValueError("segmented RLGR container: implausible header")
        G = ((N + S - 1) // S) * D
        if len(blob) < m + 40 + 4 * G + total:
            raise ValueError("segmented RLGR container: shorter than its header says")
        if max_symbols is not None and N * D > int(max_symbols):
            raise ValueError(f"segmented RLGR container: {N} x {D} symbols, more than the caller allows ({max_symbols})")
        lens = np.frombuffer(blob, np.uint32, G, m + 40).astype(np.int64)
        if total % 4 or total > len(blob) - (m + 40 + 4 * G) or int(((lens + 3) // 4 * 4).sum()) != total:
            raise ValueError("segmented RLGR container: inconsistent length table")
        return N, D, S, flag, total, lens, m + 40 + 4 * G

    def _upload(self, lens, payload):
        """length table (int64 numpy) and padded payload (uint8 numpy) of a decoder -> the device"""
        import torch
        total = int(payload.shape[0])
        off = np.concatenate([[0], np.cumsum((lens + 3) // 4 * 4)])
        self.seg_bytes.copy_(torch.from_numpy(lens.astype(np.int32)))
        self.seg_off.copy_(torch.from_numpy(off.astype(np.int64) if self.wide else off.astype(np.int64).astype(np.int32)))
        if total > self.cap:
            self.cap, self.out = total, torch.empty(total, dtype=torch.uint8, device=self.device)
        self.out[:total].copy_(torch.from_numpy(payload))
        self.total = total

    @classmethod
    def from_container(cls, blob, device="cuda", max_symbols=None, wide=None):
        """wide: as in the constructor; the default also takes the 64-bit table when the payload itself is 4 GiB or more.
        max_symbols: refuse containers whose header announces more than this many symbols (N x D): decode() allocates
        4 N D bytes for them, and the header comes off the wire."""
        N, D, S, flag, total, lens, pay = cls._parse(blob, max_symbols)
        if wide is None and total >= 2 ** 32:
            wide = True
        sc = cls(N, D, S, flag, device, payload_cap=total, wide=wide)     # (the payload only: a decoder never needs the encoder's raw-size buffer)
        sc._upload(lens, np.frombuffer(blob, np.uint8, total, pay).copy())
        return sc

    @classmethod
    def select_segments(cls, blob, seg_ids):
        """The container of a few segments of every channel, cut out of a whole one (pure host code, no device).
        seg_ids: ascending, distinct segment indices in 0 .. nseg - 1, the same for every channel. The header and the WHOLE length
        table are checked as ``from_container`` checks them. -> ((N', lens', payload'), byte_ranges): the pseudo-frame whose
        segment k of channel c is segment seg_ids[k] of channel c -- N' = (n_sel - 1) seg_len + symbols of the last selected
        segment (the frame's last segment may be short), lens' int64 (D n_sel,), payload' uint8: their 4-byte slots, concatenated --
        and the merged (offset, length) ranges of ``blob`` that were read: header + table, then one per channel and run of
        consecutive segments."""
        N, D, S, flag, total, lens, pay = cls._parse(blob)
        nseg = (N + S - 1) // S
        ids = np.asarray(seg_ids, dtype=np.int64).reshape(-1)
        if ids.size < 1 or ids[0] < 0 or ids[-1] >= nseg or np.any(ids[1:] <= ids[:-1]):
            raise ValueError(f"SegmentedCoder.select_segments: segment ids must be ascending, distinct and in 0 .. {nseg - 1}")
        off = np.concatenate([[0], np.cumsum((lens + 3) // 4 * 4)])
        cut = np.nonzero(ids[1:] != ids[:-1] + 1)[0] + 1                   # runs of consecutive ids: [first[r], last[r]]
        first, last = ids[np.concatenate([[0], cut])], ids[np.concatenate([cut - 1, [ids.size - 1]])]
        view = np.frombuffer(blob, np.uint8, total, pay)
        pieces, ranges = [], [(0, pay)]
        for c in range(D):
            for f, l in zip(first, last):
                lo, hi = int(off[c * nseg + f]), int(off[c * nseg + l + 1])
                pieces.append(view[lo:hi])
                if hi > lo:
                    if ranges[-1][0] + ranges[-1][1] == pay + lo:
                        ranges[-1] = (ranges[-1][0], ranges[-1][1] + hi - lo)
                    else:
                        ranges.append((pay + lo, hi - lo))
        n_last = N - (nseg - 1) * S if ids[-1] == nseg - 1 else S
        lens_sel = lens.reshape(D, nseg)[:, ids].reshape(-1)
        return ((ids.size - 1) * S + n_last, lens_sel, np.concatenate(pieces)), ranges

    @classmethod
    def from_container_segments(cls, blob, seg_ids, device="cuda", max_symbols=None):
        """A decoder for the segments ``seg_ids`` of every channel only (``select_segments``): -> (coder, byte_ranges). The coder is
        an ordinary ``SegmentedCoder(N', D, seg_len)`` that was handed nothing but those segments' lengths and bytes; its
        ``decode(row_major=True)`` gives the (N', D) rows the selected segments cover, in segment order. ``max_symbols``: refuse
        more than this many symbols (N' x D)."""
        (Np, lens, payload), ranges = cls.select_segments(blob, seg_ids)
        m = len(cls.MAGIC)
        _, D, S, flag, _ = [int(x) for x in np.frombuffer(blob, np.int64, 5, m)]
        if max_symbols is not None and Np * D > int(max_symbols):
            raise ValueError(f"segmented RLGR container: {Np} x {D} symbols selected, more than the caller allows ({max_symbols})")
        sc = cls(Np, D, S, flag, device, payload_cap=int(payload.shape[0]))
        sc._upload(lens, payload)
        return sc, ranges

    def decode(self, out=None, row_major=False):
        """-> (D, N) int32 CUDA tensor, or (N, D) with ``row_major=True`` (what dequant_inverse takes: no transpose behind the
        decoder); enqueued on the current stream, no synchronisation"""
        import torch
        if out is None:
            out = torch.empty((self.N, self.D) if row_major else (self.D, self.N), dtype=torch.int32, device=self.device)
        return self._decode_core("one", [self], [out], [self._strides(out, "decode")])[0]

    BATCH_MAX = 12                                            # RAHT_RLGR_BATCH_MAX

    # (direction, form of the call: "one" frame, a "batch" of one shape, a "ragged" batch) -> the entry point with 32-bit and the one
    # with 64-bit offset tables, each with whether it has an expect[] argument. A 32-bit batch has two decoders: the one that
    # compares takes expect[], the plain one has no such argument. A ragged batch has 32-bit tables only (``_same_kind``).
    _ENTRY = {("encode", "one"): (("raht_rlgr_seg_encode_strided", False), ("raht_rlgr_seg_encode64", False)),
              ("encode", "batch"): (("raht_rlgr_seg_encode_batch", False), ("raht_rlgr_seg_encode_batch64", False)),
              ("encode", "ragged"): (("raht_rlgr_seg_encode_ragged", False), None),
              ("decode", "one"): (("raht_rlgr_seg_decode_strided", False), ("raht_rlgr_seg_decode64", False)),
              ("decode", "batch"): (("raht_rlgr_seg_decode_batch", False), ("raht_rlgr_seg_decode_batch64", True)),
              ("decode", "batch", "expect"): (("raht_rlgr_seg_decode_batch_check", True), ("raht_rlgr_seg_decode_batch64", True)),
              ("decode", "ragged"): (("raht_rlgr_seg_decode_ragged", True), None)}

    @staticmethod
    @functools.lru_cache(maxsize=None)
    def _marshal(form, k):
        """How an entry point of ``form`` takes the k frames of a call -> (head, ptrs, ints, shape, I64). head: the leading k (the
        one-frame entry points have none). ptrs / ints: what every frame has of its own -- a table of pointers / of int64, or the
        value itself for one frame. shape: N and the two strides -- a table in a ragged call, the value all frames share otherwise.
        I64: the type of a table of k int64. Cached: a one-frame call costs no more than its ctypes arguments."""
        VP, I64 = C.c_void_p * k, C.c_int64 * k
        first = operator.itemgetter(0)
        if form == "one":
            return (), first, first, first, I64
        return (k,), (lambda xs: VP(*xs)), (lambda xs: I64(*xs)), ((lambda xs: I64(*xs)) if form == "ragged" else first), I64

    @classmethod
    def _encode_core(cls, form, coders, Qs, st):
        """``coders[j].encode(Qs[j])`` (strides ``st[j]``) through the entry point of ``form``, in chunks of ``BATCH_MAX``: the tables
        of a chunk, one call, and when a container turns out too small larger ones and ONE more call; leaves every ``total``."""
        import torch
        c0 = coders[0]
        fn = getattr(_lib.lib(), cls._ENTRY["encode", form][c0.wide][0])
        for lo in range(0, len(coders), cls.BATCH_MAX):
            cs, qs, ss = coders[lo: lo + cls.BATCH_MAX], Qs[lo: lo + cls.BATCH_MAX], st[lo: lo + cls.BATCH_MAX]
            k = len(cs)
            head, ptrs, ints, shape, I64 = cls._marshal(form, k)
            tot = I64()
            for attempt in (0, 1):
                with torch.cuda.device(c0.device):
                    rc = fn(*head, ptrs([q.data_ptr() for q in qs]), shape([c.N for c in cs]), c0.D, shape([s[0] for s in ss]), shape([s[1] for s in ss]),
                            c0.S, c0.flag, ptrs([c.seg_bytes.data_ptr() for c in cs]), ptrs([c.seg_off.data_ptr() for c in cs]),
                            ptrs([c.out.data_ptr() for c in cs]), ints([c.cap for c in cs]), tot, c0._stream())
                if rc == _lib.RAHT_OK or attempt == 1 or all(int(tot[j]) <= cs[j].cap for j in range(k)):
                    check(rc)
                    break
                for j, c in enumerate(cs):                    # incompressible data: the exact sizes are known now
                    if int(tot[j]) > c.cap:
                        c.cap = int(tot[j]) + 64
                        c.out = torch.empty(c.cap, dtype=torch.uint8, device=c.device)
            for j, c in enumerate(cs):
                c.total = int(tot[j])

    @classmethod
    def _decode_core(cls, form, coders, outs, st, expect=None):
        """``coders[j].decode(outs[j])`` (strides ``st[j]``) through the entry point of ``form``, one launch per chunk of ``BATCH_MAX``,
        compared with ``expect[j]`` on the way when given; every chunk reports into its own first coder's ``bad``. -> outs"""
        import torch
        c0 = coders[0]
        name, has_expect = cls._ENTRY[("decode", form) + (("expect",) if form == "batch" and expect is not None else ())][c0.wide]
        fn = getattr(_lib.lib(), name)
        for lo in range(0, len(coders), cls.BATCH_MAX):
            cs, os_, ss = coders[lo: lo + cls.BATCH_MAX], outs[lo: lo + cls.BATCH_MAX], st[lo: lo + cls.BATCH_MAX]
            k = len(cs)
            head, ptrs, ints, shape, _ = cls._marshal(form, k)
            ex = ((None if expect is None else ptrs([e.data_ptr() for e in expect[lo: lo + cls.BATCH_MAX]])),) if has_expect else ()
            with torch.cuda.device(c0.device):
                check(fn(*head, ptrs([c.out.data_ptr() for c in cs]), ints([(c.total + 3) // 4 * 4 for c in cs]),
                         ptrs([c.seg_off.data_ptr() for c in cs]), ptrs([c.seg_bytes.data_ptr() for c in cs]), shape([c.N for c in cs]), c0.D, c0.S, c0.flag,
                         ptrs([o.data_ptr() for o in os_]), *ex, shape([s[0] for s in ss]), shape([s[1] for s in ss]),
                         C.c_void_p(cs[0].bad.data_ptr()), c0._stream()))
        return outs

    @staticmethod
    def _same_kind(coders, what, ragged=False):
        """the coders of one call: they share D, seg_len, flag and device, and N and the offset width (a batch of one shape) or
        32-bit offsets (a ragged batch) -> the first"""
        c0 = coders[0]
        for c in coders:
            if (c.D, c.S, c.flag, c.device) != (c0.D, c0.S, c0.flag, c0.device) or (not ragged and (c.N, c.wide) != (c0.N, c0.wide)):
                raise ValueError(f"SegmentedCoder.{what}: the coders of a ragged batch share D, seg_len, flag and device" if ragged else
                                 f"SegmentedCoder.{what}: the coders of a batch share N, D, seg_len, flag, device and offset width")
            if ragged and c.wide:
                raise ValueError(f"SegmentedCoder.{what}: a ragged batch takes 32-bit offset tables only (a {c.N} x {c.D} frame goes alone)")
        return c0

    @classmethod
    def encode_batch(cls, coders, Qs):
        """The quantization steps of a frame coded together (raht_rlgr_seg_encode_batch): ``coders[j].encode(Qs[j])`` for every j,
        in ONE set of launches -- k times the independent streams of one frame, which is what the coder's speed depends on. Same
        containers, byte for byte. All Qs in the same layout ((N, D) row-major or (D, N) channel-major) with the same strides.
        -> list of container payload sizes (synchronises)."""
        if len(coders) != len(Qs) or not coders:
            raise ValueError("SegmentedCoder.encode_batch: one input per coder")
        cls._same_kind(coders, "encode_batch")
        st = [c._strides(Q, "encode_batch") for c, Q in zip(coders, Qs)]
        if any(x != st[0] for x in st):
            raise ValueError("SegmentedCoder.encode_batch: the inputs of a batch share their layout and strides")
        cls._encode_core("batch", coders, Qs, st)
        return [c.total for c in coders]

    @classmethod
    def decode_batch(cls, coders, outs=None, row_major=False, expect=None):
        """``coders[j].decode()`` for every j in ONE launch (raht_rlgr_seg_decode_batch) -> list of (D, N) int32 CUDA tensors ((N, D)
        with ``row_major=True``); enqueued on the current stream, no synchronisation. ``coders[0].bad`` collects the frames whose
        tables reached outside their payload (bit j of a chunk of 12).
        ``expect`` (row-major only): one (N, D) tensor per coder, what the frame should decode to -- compared inside the decoder
        (raht_rlgr_seg_decode_batch_check: the drivers' round-trip assertion without a pass of its own); bit 16 + j of
        ``coders[0].bad`` reports frame j of a chunk; ``roundtrip_failed(coders)`` reads it."""
        import torch
        if not coders:
            return []
        c0 = cls._same_kind(coders, "decode_batch")
        if outs is None:
            outs = [torch.empty((c0.N, c0.D) if row_major else (c0.D, c0.N), dtype=torch.int32, device=c0.device) for _ in coders]
        st = [c._strides(o, "decode_batch") for c, o in zip(coders, outs)]
        if len(outs) != len(coders) or any(x != st[0] for x in st):
            raise ValueError("SegmentedCoder.decode_batch: one output per coder, all in the same layout")
        if expect is not None:
            if not row_major and st[0][1] != 1:
                raise ValueError("SegmentedCoder.decode_batch: expect= goes with row-major frames")
            if len(expect) != len(coders) or any(c._strides(e, "decode_batch") != st[0] for c, e in zip(coders, expect)):
                raise ValueError("SegmentedCoder.decode_batch: one expected frame per coder, in the layout and strides of the outputs")
        return cls._decode_core("batch", coders, outs, st, expect)

    @staticmethod
    def _one_layout(coders, mats, what, row_major=None):
        """[(sym_stride, chan_stride)] of the matrices of a ragged call, all (N_j, D) row-major or all (D, N_j) channel-major.
        ``row_major`` True / False SAYS which; None reads it off the shapes, and a SQUARE matrix (N_j == D) is then channel-major,
        whatever its company: that is how ``_strides`` -- ``encode`` / ``decode`` of that coder alone -- reads it, and the bytes of a
        frame cannot depend on the other frames of the call. A square matrix among row-major ones therefore needs
        ``row_major=True``."""
        if len(mats) != len(coders):
            raise ValueError(f"SegmentedCoder.{what}: one matrix per coder")
        for c, m in zip(coders, mats):
            c._strides(m, what)                                   # (dtype, device, shape)
        rows = [tuple(m.shape) == (c.N, c.D) and (c.N == 1 or m.stride(0) >= c.D) for c, m in zip(coders, mats)]
        chans = [tuple(m.shape) == (c.D, c.N) and (c.D == 1 or m.stride(0) >= c.N) for c, m in zip(coders, mats)]
        if row_major is None:
            rows = [r and c.N != c.D for r, c in zip(rows, coders)]
        if all(rows) and row_major is not False:
            return [(m.stride(0) if c.N > 1 else c.D, 1) for c, m in zip(coders, mats)]
        if all(chans) and not row_major:
            return [(1, m.stride(0) if c.D > 1 else c.N) for c, m in zip(coders, mats)]
        if row_major is None and any(c.N == c.D for c in coders):
            raise ValueError(f"SegmentedCoder.{what}: a square matrix (N == D) is read as (D, N) channel-major, as encode / decode of one "
                             "frame read it; among (N, D) row-major matrices say row_major=True")
        raise ValueError(f"SegmentedCoder.{what}: the matrices of a ragged batch are all (N, D) row-major or all (D, N) channel-major")

    @classmethod
    def encode_ragged(cls, coders, Qs, row_major=None):
        """The frames of a sequence coded together (raht_rlgr_seg_encode_ragged): ``coders[j].encode(Qs[j])`` for every j in ONE set
        of launches, for coders that share D, seg_len, flag, device and 32-bit offsets and differ in N. Same containers, byte for
        byte. All Qs row-major (N_j, D) or all channel-major (D, N_j); strides may differ. ``row_major``: None reads the layout off
        the shapes, with a square Q (N_j == D) channel-major as ``encode`` reads it; True / False say it (``_one_layout``).
        -> list of container payload sizes (synchronises)."""
        if len(coders) != len(Qs) or not coders:
            raise ValueError("SegmentedCoder.encode_ragged: one input per coder")
        cls._same_kind(coders, "encode_ragged", ragged=True)
        cls._encode_core("ragged", coders, Qs, cls._one_layout(coders, Qs, "encode_ragged", row_major))
        return [c.total for c in coders]

    @classmethod
    def decode_ragged(cls, coders, outs=None, row_major=False, expect=None):
        """``coders[j].decode()`` for every j in ONE launch (raht_rlgr_seg_decode_ragged), for coders as ``encode_ragged`` takes them
        -> list of (D, N_j) int32 CUDA tensors ((N_j, D) with ``row_major=True``); enqueued on the current stream, no
        synchronisation. Given ``outs``, their layout is read off their shapes unless ``row_major=True`` says it; a square out
        (N_j == D) is channel-major otherwise, as ``decode`` reads it (``_one_layout``). ``coders[0].bad`` and ``expect`` (row-major
        only) as in ``decode_batch``; ``roundtrip_failed(coders)`` reads the result."""
        import torch
        if not coders:
            return []
        cls._same_kind(coders, "decode_ragged", ragged=True)
        fresh = outs is None
        if fresh:
            outs = [torch.empty((c.N, c.D) if row_major else (c.D, c.N), dtype=torch.int32, device=c.device) for c in coders]
        kind = bool(row_major) if fresh else (True if row_major else None)
        st = cls._one_layout(coders, outs, "decode_ragged", kind)
        if expect is not None:
            if any(chan != 1 for _, chan in st):
                raise ValueError("SegmentedCoder.decode_ragged: expect= goes with row-major frames")
            if len(expect) != len(coders) or cls._one_layout(coders, expect, "decode_ragged", True) != st:
                raise ValueError("SegmentedCoder.decode_ragged: one expected frame per coder, in the layout and strides of the outputs")
        return cls._decode_core("ragged", coders, outs, st, expect)

    @classmethod
    def roundtrip_failed(cls, coders):
        """after ``decode_batch(..., expect=...)``: -> list of the indices of the frames that did not decode to what was expected, or
        whose tables reached outside their payload (synchronises)"""
        out = []
        for lo in range(0, len(coders), cls.BATCH_MAX):
            w = int(coders[lo].bad.item()) & 0xffffffff
            out += [lo + j for j in range(min(cls.BATCH_MAX, len(coders) - lo)) if (w >> j) & 1 or (w >> (16 + j)) & 1]
        return out

    RATE_MAX = 8                                              # RAHT_RLGR_RATE_MAX: steps walked per pass over the coefficients

    @staticmethod
    def rate(T, steps, seg_len=2048, flag_signed=1, want_sse=True):
        """How many bytes the container takes at every one of k quantization steps, WITHOUT quantizing or coding anything
        (raht_rlgr_seg_rate): one read of the coefficients, k coder states per lane that only count their bits.
        T: (N, D) float32 or float64 CUDA tensor with unit column stride, rows in coded order (row i is row i of the quantized
        matrix); steps: k scalars or k tables of D entries, in T's precision.
        -> (container_bytes int64 numpy [k], seg_bytes (k, G) int32 CUDA tensor, sse (k, D) float64 CUDA tensor or None):
        ``container_bytes[j]`` is ``size_bytes`` of a coder that encoded floor(T / steps[j] + 0.5), ``seg_bytes[j]`` its length table,
        ``sse[j, c]`` the sum over channel c of (T - q * step)^2 in float64. Synchronises (it returns sizes)."""
        import torch
        if not isinstance(T, torch.Tensor) or not T.is_cuda or T.dim() != 2 or T.dtype not in (torch.float32, torch.float64) or \
                (T.shape[1] > 1 and T.stride(1) != 1) or T.shape[0] < 1 or T.shape[1] < 1 or (T.shape[0] > 1 and T.stride(0) < T.shape[1]):
            raise ValueError("SegmentedCoder.rate: expected an (N, D) float32 or float64 CUDA tensor with unit column stride")
        N, D = int(T.shape[0]), int(T.shape[1])
        f64 = T.dtype == torch.float64
        rows = [step_list(st) for st in steps]
        k = len(rows)
        if k < 1 or any(len(r) != len(rows[0]) for r in rows) or len(rows[0]) not in (1, D):
            raise ValueError("SegmentedCoder.rate: steps must be k scalars or k tables of D entries")
        n_steps = len(rows[0])
        flat = [x for r in rows for x in r]
        st = ((C.c_double if f64 else C.c_float) * len(flat))(*flat)
        S = int(seg_len)
        G = ((N + S - 1) // S) * D if S > 0 else 0
        seg_bytes = torch.empty((k, max(G, 1)), dtype=torch.int32, device=T.device)
        seg_sse = torch.empty((k, max(G, 1)), dtype=torch.float64, device=T.device) if want_sse else None
        with torch.cuda.device(T.device):
            check(_lib.lib().raht_rlgr_seg_rate(C.c_void_p(T.data_ptr()), _lib.RAHT_F64 if f64 else _lib.RAHT_F32, T.stride(0) if N > 1 else D,
                                                N, D, st, k, n_steps, S, int(flag_signed), C.c_void_p(seg_bytes.data_ptr()),
                                                C.c_void_p(seg_sse.data_ptr()) if want_sse else None,
                                                C.c_void_p(torch.cuda.current_stream(T.device).cuda_stream)))
        sse = seg_sse.view(k, D, G // D).sum(dim=2) if want_sse else None          # (segments of a channel in segment order)
        padded = (seg_bytes.to(torch.int64) + 3) // 4 * 4
        container = SegmentedCoder.container_size(G, padded.sum(dim=1).cpu().numpy())
        return container, seg_bytes, sse

    step_row = staticmethod(step_list)                        # (one quantization step as a list of floats: ops.step_list)

    @staticmethod
    def container_size(G, payload):
        """``size_bytes`` of a container of G segments whose padded streams take ``payload`` bytes (number or array); with
        ``payload`` 0 what the container takes besides its streams"""
        return len(SegmentedCoder.MAGIC) + 5 * 8 + 4 * int(G) + np.asarray(payload, np.int64)

    def segment(self, c, s):
        """the bytes of segment s of channel c (host copy; tests)"""
        g = c * self.nseg + s
        off, nb = int(self.seg_off[g].item()), int(self.seg_bytes[g].item())
        return self.out[off: off + nb].cpu().numpy()


def transpose_on_device(Q):
    """(rows, cols) int32 CUDA tensor -> (cols, rows) contiguous, with the HIP LDS-tile transpose
    (row-major N x D quantized coefficients -> channel-major D x N for the entropy stage, or back)."""
    import torch
    if not Q.is_cuda or Q.dtype != torch.int32 or Q.dim() != 2 or Q.stride(1) != 1:
        raise ValueError("expected a 2-D int32 CUDA tensor with unit column stride")
    rows, cols = Q.shape
    out = torch.empty((cols, rows), dtype=torch.int32, device=Q.device)
    with torch.cuda.device(Q.device):
        check(_lib.lib().raht_transpose_i32(C.c_void_p(Q.data_ptr()), Q.stride(0), rows, cols, C.c_void_p(out.data_ptr()),
                                            rows, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def to_host(t):
    """Device tensor -> numpy array through a cached page-locked staging buffer: 57 GB/s instead of the
    6.7 GB/s of a pageable ``.cpu()`` on the MI355X box (708 MB of quantized coefficients: 12 ms
    instead of 106 ms; tools/probe_d2h.py). The array aliases the staging buffer of its dtype and stays
    valid until the next ``to_host`` call with that dtype."""
    import torch
    if not t.is_cuda:
        return t.contiguous().numpy()
    t = t.contiguous()
    n = t.numel()
    buf = _STAGING.get(t.dtype)
    if buf is None or buf.numel() < n:
        buf = torch.empty(max(n, 1), dtype=t.dtype, pin_memory=True)
        _STAGING[t.dtype] = buf
    out = buf[:n].view(t.shape)
    out.copy_(t, non_blocking=True)
    torch.cuda.current_stream(t.device).synchronize()
    return out.numpy()
