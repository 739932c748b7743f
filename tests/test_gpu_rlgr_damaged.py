"""The segmented RLGR decoders (csrc/rlgr_seg.hip) on payloads whose BYTES are wrong -- a truncated download, a flipped bit -- with
the tables intact. What include/raht.h promises for them and this file holds every decoder to:

  bounds      every store lands in the damaged segment's own symbols: sentinels around and between the output rows survive, every
              other segment holds the clean symbols, and the `bad` word stays 0 (it speaks of tables, and the tables are fine);
  the model   while the decoder's state fits 32 bits the symbols are those of the reference decoder on the zero-extended bytes
              (tests/numpy_rlgr_damaged.py, itself held to the oracle, the host coder and the reference's build by
              tests/test_rlgr_damaged_model.py on these same cases);
  one answer  every entry point and every way through the kernels -- per-lane and symbol-synchronous decoder, the three bit readers
              (plain words, LDS pieces, the ring), both payload alignments, 32- and 64-bit tables, batch and ragged launches --
              gives the same symbols for the same damaged container, the saturating cases included;
  expect      the comparison inside the decoder reports exactly the frames a damaged segment changed.

The cases come from tests/rlgr_damage_cases.py (seed 0); every decode here takes milliseconds."""
import ctypes as C

import numpy as np
import pytest

from . import numpy_rlgr_damaged as M
from . import rlgr_damage_cases as DC

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A                                                      # no clean symbol of these frames, and it fits int32
FILL = 4096                                                            # zero bytes on either side of a container
_PREP = {}


class _Frame:
    """a clean frame, coded once: its container and tables on the host, the damage cases with what the model says of each, and two
    companions of other N (its first N - 7 and its first seg_len + 1 symbols) for the ragged launch"""

    def __init__(self, name):
        import torch
        from raht_3dgs_codec_amd import rlgr
        self.name = name
        self.N, self.D, self.S, self.Q = DC.frame(name)
        self.nseg = (self.N + self.S - 1) // self.S
        self.Qd = torch.from_numpy(self.Q).cuda()
        sc = rlgr.SegmentedCoder(self.N, self.D, self.S)
        self.total = sc.encode(self.Qd)
        segs = DC.host_segments(self.Q, self.S)
        self.blob, self.offs, self.lens = DC.container(segs)
        # the GPU encoder's container is the host coder's segments: the cases built from those apply to it
        assert self.total == len(self.blob) and self.total % 4 == 0
        assert np.array_equal(sc.out[: self.total].cpu().numpy(), self.blob)
        assert np.array_equal(sc.seg_bytes.cpu().numpy(), self.lens) and np.array_equal(sc.seg_off.cpu().numpy(), self.offs)
        self.cases = []
        for cname, g, damage in DC.build(segs, 0, DC.fragile_segments(name, self.N, self.D, self.S)):
            n = DC.symbols_of(self.N, self.S, g)
            seq, info = M.decode(DC.seen_bytes(self.blob, self.offs, self.lens, g, damage), n)
            in_domain = not DC.is_saturating(cname) and not info["left_domain"]
            self.cases.append((cname, g, damage, np.array(seq, np.int64).astype(np.int32) if in_domain else None))
        self.mates = []
        for n in (self.N - 7, self.S + 1):
            Qm = self.Qd[:, :n].contiguous()
            c = rlgr.SegmentedCoder(n, self.D, self.S)
            c.encode(Qm)
            self.mates.append((n, Qm, c))
        self.clean = self.upload(self.blob, 0)

    @staticmethod
    def upload(blob, shift):
        """the container in the middle of a zero-filled device buffer, FILL bytes and more on both sides, starting on a 32-byte
        boundary (shift 0) or 4 bytes behind one -> (tensor, address of the container)"""
        import torch
        host = np.zeros(FILL + 32 + len(blob) + FILL, np.uint8)
        host[FILL + shift: FILL + shift + len(blob)] = blob
        buf = torch.from_numpy(host).cuda()
        assert buf.data_ptr() % 32 == 0
        return buf, buf.data_ptr() + FILL + shift

    def segment_slice(self, g):
        c, s = divmod(g, self.nseg)
        return c, slice(s * self.S, min(self.N, (s + 1) * self.S))


def _frame(name):
    if name not in _PREP:
        _PREP[name] = _Frame(name)
    return _PREP[name]


class _Out:
    """an output matrix inside sentinels: one row of them before and after, and a padded row stride whose padding holds them"""

    def __init__(self, N, D, row_major):
        import torch
        self.rm = row_major
        rows, cols = (N, D) if row_major else (D, N)
        ld = cols + 3 if row_major else (cols + 3) // 4 * 4 + 8          # (channel-major: 16-byte aligned rows, as the LDS columns need)
        self.buf = torch.full((rows + 2, ld), SENT, dtype=torch.int32, device="cuda")
        self.view = self.buf[1: rows + 1, :cols]
        self.strides = (ld, 1) if row_major else (1, ld)                 # (sym_stride, chan_stride)
        assert row_major or self.view.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.view.data_ptr()

    def symbols(self):
        """(D, N), whatever the layout"""
        return self.view.t() if self.rm else self.view

    def sentinels_intact(self):
        rows, cols = self.view.shape
        b = self.buf == SENT
        return b[0].all() & b[-1].all() & b[1: rows + 1, cols:].all()


def _vp(t):
    return C.c_void_p(t.data_ptr() if hasattr(t, "data_ptr") else int(t))


def _decode_every_way(F, L, ins, tables, clean_tables):
    """ins: the damaged container's address at the aligned and at the shifted start; tables: (seg_off int32, seg_off int64, seg_bytes)
    on the device for it, clean_tables the same for the clean container -> ([(label, _Out)] that must all hold the same symbols,
    [(label, _Out, clean (D, n) tensor)] for the ragged launches' companions, the two `bad` words: of every plain call together, and
    of the launch that compares with the clean frame)"""
    import torch
    N, D, S = F.N, F.D, F.S
    off32, off64, lens = tables
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    bad_x = torch.zeros(1, dtype=torch.int32, device="cuda")
    outs, mates = [], []
    VP3, I3 = C.c_void_p * 3, C.c_int64 * 3

    def ok(rc):
        assert rc == 0, L.raht_last_error()

    def one(label, fn, inp, off, row_major):
        o = _Out(N, D, row_major)
        ok(fn(C.c_void_p(inp), F.total, _vp(off), _vp(lens), N, D, S, 1, C.c_void_p(o.ptr), o.strides[0], o.strides[1], _vp(bad), None))
        outs.append((label, o))

    def three(label, row_major, expect=None):
        """k = 3 of one shape: the damaged container at both alignments, and between them the clean one (when compared) or the
        aligned damaged one again"""
        os_ = [_Out(N, D, row_major) for _ in range(3)]
        mid = F.clean[1] if expect is not None else ins[0]
        mid_t = clean_tables if expect is not None else tables
        args = (3, VP3(ins[0], mid, ins[1]), I3(F.total, F.total, F.total), VP3(*[t[0].data_ptr() for t in (tables, mid_t, tables)]),
                VP3(*[t[2].data_ptr() for t in (tables, mid_t, tables)]), N, D, S, 1, VP3(*[o.ptr for o in os_]))
        st = os_[0].strides
        if expect is None:
            ok(L.raht_rlgr_seg_decode_batch(*args, st[0], st[1], _vp(bad), None))
        else:
            ok(L.raht_rlgr_seg_decode_batch_check(*args, VP3(*[expect.ptr] * 3), st[0], st[1], _vp(bad_x), None))
        for j, o in enumerate(os_):
            if expect is None or j != 1:
                outs.append((f"{label}[{j}]", o))
            else:
                mates.append((f"{label}[1]", o, F.Qd))

    def ragged(label, row_major):
        """three different N in one launch: the damaged frame between its two companions"""
        (n1, Q1, c1), (n2, Q2, c2) = F.mates
        os_ = [_Out(n1, D, row_major), _Out(N, D, row_major), _Out(n2, D, row_major)]
        ok(L.raht_rlgr_seg_decode_ragged(3, VP3(c1.out.data_ptr(), ins[1], c2.out.data_ptr()), I3(c1.total, F.total, c2.total),
                                         VP3(c1.seg_off.data_ptr(), off32.data_ptr(), c2.seg_off.data_ptr()),
                                         VP3(c1.seg_bytes.data_ptr(), lens.data_ptr(), c2.seg_bytes.data_ptr()), I3(n1, N, n2), D, S, 1,
                                         VP3(*[o.ptr for o in os_]), None, I3(*[o.strides[0] for o in os_]), I3(*[o.strides[1] for o in os_]),
                                         _vp(bad), None))
        outs.append((label, os_[1]))
        mates.extend([(f"{label} N={n1}", os_[0], Q1), (f"{label} N={n2}", os_[2], Q2)])

    prev = L.raht_debug_rlgr_decode_out(0)                                # channel-major output as single words
    try:
        for a, inp in zip(("aligned", "shifted"), ins):
            one(f"one frame, words, {a}", L.raht_rlgr_seg_decode_strided, inp, off32, False)
            one(f"one frame, words, 64-bit offsets, {a}", L.raht_rlgr_seg_decode64, inp, off64, False)
        three("batch, words", False)
        L.raht_debug_rlgr_decode_out(2)                                   # ... as LDS columns
        for a, inp in zip(("aligned", "shifted"), ins):
            one(f"one frame, LDS columns, {a}", L.raht_rlgr_seg_decode_strided, inp, off32, False)
        three("batch, LDS columns (LDS pieces in, [1]: word by word)", False)
        ragged("ragged, LDS columns", False)
        L.raht_debug_rlgr_decode_out(3)                                   # row-major output: the symbol-synchronous decoder (the ring)
        for a, inp in zip(("aligned", "shifted"), ins):
            one(f"one frame, rows, symbol-synchronous, {a}", L.raht_rlgr_seg_decode_strided, inp, off32, True)
        one("one frame, rows, symbol-synchronous, 64-bit offsets", L.raht_rlgr_seg_decode64, ins[1], off64, True)
        three("batch, rows, the ring", True)
        ragged("ragged, rows", True)
        expect = _Out(N, D, True)
        expect.view.copy_(F.Qd.t())
        three("batch, rows, compared with the clean frame", True, expect)
        L.raht_debug_rlgr_decode_out(4)                                   # row-major output from the per-lane decoder
        for a, inp in zip(("aligned", "shifted"), ins):
            one(f"one frame, rows, per lane, {a}", L.raht_rlgr_seg_decode_strided, inp, off32, True)
        three("batch, rows, per lane", True)
    finally:
        L.raht_debug_rlgr_decode_out(-1)                                  # (also takes back 3 / 4)
        L.raht_debug_rlgr_decode_out(prev)
    return outs, mates, bad, bad_x


def _apply(F, L, damages):
    """damages: [(case name, g, damage, the model's symbols or None)] on distinct segments, applied to one container together"""
    import torch
    assert len({g for _, g, _, _ in damages}) == len(damages)
    blob, lens = F.blob.copy(), F.lens.copy()
    want = F.Q.copy()                                                    # what the model says the frame decodes to ...
    judged = np.ones(F.Q.shape, bool)                                    # ... where it says anything
    for _, g, damage, seq in damages:
        c, sl = F.segment_slice(g)
        if isinstance(damage, int):
            lens[g] = damage
        else:
            blob[int(F.offs[g]): int(F.offs[g]) + len(damage)] = np.frombuffer(damage, np.uint8)
        if seq is None:
            judged[c, sl] = False
        else:
            want[c, sl] = seq
    names = "+".join(n for n, _, _, _ in damages)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).cuda()            # noqa: E731
    tables = (dev(F.offs, np.int32), dev(F.offs, np.int64), dev(lens, np.int32))
    clean_tables = (tables[0], tables[1], dev(F.lens, np.int32))
    bufs = [F.upload(blob, shift) for shift in (0, 4)]
    outs, mates, bad, bad_x = _decode_every_way(F, L, [p for _, p in bufs], tables, clean_tables)
    want_d, judged_d = torch.from_numpy(want).cuda(), torch.from_numpy(judged).cuda()
    first = outs[0][1].symbols()
    labels, flags = [], []
    labels.append(f"{outs[0][0]}: the model's symbols in the damaged segments, the clean ones everywhere else")
    flags.append(((first == want_d) | ~judged_d).all())
    for label, o in outs:
        labels.append(f"{label}: sentinels")
        flags.append(o.sentinels_intact())
        labels.append(f"{label}: the same symbols as '{outs[0][0]}'")
        flags.append((o.symbols() == first).all())
    for label, o, clean in mates:
        labels.append(f"{label}: a clean frame of the same launch")
        flags.append(o.sentinels_intact() & (o.symbols() == clean).all())
    changed = (first != F.Qd).any()
    labels.append("bad: no table bit after any plain decode")
    flags.append(bad[0] == 0)
    labels.append("bad: bits 16 and 18 (the damaged frames) iff a damaged segment decodes differently, never bit 17 (the clean one) or a table bit")
    flags.append(bad_x[0] == torch.where(changed, (1 << 16) | (1 << 18), 0))
    got = torch.stack(flags).cpu().numpy()
    assert got.all(), (F.name, names, [lab for lab, f in zip(labels, got) if not f][:6])
    return bool(changed.item())


@pytest.mark.parametrize("name", [s[0] for s in DC.SHAPES])
def test_one_damaged_segment_at_a_time(name):
    from raht_3dgs_codec_amd import _lib
    F, L = _frame(name), _lib.lib()
    assert _apply(F, L, []) is False                                     # the clean container, through the same paths
    changed = {}
    for case in F.cases:
        changed[case[0]] = _apply(F, L, [case])
    assert changed["longer"] is False                                    # a decoder stops at symbol n wherever the table says the bytes end
    assert changed["all_zero"] and changed["random_bytes"] and changed["sat_all_ff"], changed
    # the all-zero segment is the pattern the kernel's own comment speaks of (an empty stream is not zeros)
    (_, g, _, seq), = [c for c in F.cases if c[0] == "all_zero"]
    assert seq.tolist() == M.empty_stream_pattern(len(seq))
    assert sum(seq is not None for _, _, _, seq in F.cases) >= len(F.cases) - 2 - 1      # (the two saturating kinds; the cap of the model's test)


@pytest.mark.parametrize("name", [s[0] for s in DC.SHAPES])
def test_every_case_at_once_on_different_segments(name):
    from raht_3dgs_codec_amd import _lib
    F, L = _frame(name), _lib.lib()
    rounds = []
    for case in F.cases:                                                 # into the first round whose segment g is still free
        for r in rounds:
            if all(case[1] != other[1] for other in r):
                r.append(case)
                break
        else:
            rounds.append([case])
    assert sum(len(r) for r in rounds) == len(F.cases) and max(len(r) for r in rounds) >= 5
    assert [_apply(F, L, r) for r in rounds][0] is True


def test_the_frames_reach_the_reader_edges_they_were_chosen_for():
    """what the shapes are for, checked on the clean containers: a last segment of one symbol; more channels than a wave has lanes;
    streams of more than the ring's 16 words and of many 32-byte pieces; a lane that needs more than 16 words within 32 symbols;
    a container that ends inside a 32-byte piece (the LDS reader's word-by-word edge)"""
    Fs = {s[0]: _frame(s[0]) for s in DC.SHAPES}
    assert Fs["last_of_one"].N % Fs["last_of_one"].S == 1 and Fs["pieces"].N % Fs["pieces"].S == 1
    assert Fs["wide"].D > 64
    assert Fs["pieces"].lens.max() > 20 * 32
    noise = Fs["noise"].lens[DC.NOISE_CHANNEL * Fs["noise"].nseg]
    assert noise > 1024 // 32 * 16 * 4 * 2                               # twice 16 words per 32 symbols, on average
    assert any(F.total % 32 for F in Fs.values())


def test_a_flipped_payload_bit_in_a_frame_and_in_a_p_frame_decodes_to_something():
    """through bitstream.py: a coded frame, and the P frame of a two-frame sequence, each with one flipped bit in its attribute
    payload. Both decode without raising: the keys exact, the attributes of the right shape and finite, the same on two calls."""
    import torch
    from raht_3dgs_codec_amd import bitstream, synth
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    J, D = 8, 8
    V0, _, A0 = synth.scene(3000, J, D, seed=5)
    V1, _, A1 = synth.scene(3000, J, D, seed=6)

    def flipped(blob, frame_at, frame):
        """one bit of the attribute payload of `frame` (a RAHTF001 container that begins at frame_at of blob)"""
        ao, al = bitstream.parse_frame(frame)["attributes"]
        *_, lens, pay = SegmentedCoder._parse(bytes(frame[ao: ao + al]))
        g = len(lens) // 3
        assert lens[g] >= 2
        at = int(((lens[:g] + 3) // 4 * 4).sum()) + int(lens[g]) // 2     # the middle of segment g: a byte the decoder reads
        b = bytearray(blob)
        b[frame_at + ao + pay + at] ^= 0x10
        return bytes(b)

    one = bitstream.encode_frame_bytes(V0, A0, J, 0.05, "cuda", seg_len=256)
    bad1 = flipped(one, 0, one)
    outs = [bitstream.decode_frame_bytes(bad1, "cuda") for _ in range(2)]
    clean = bitstream.decode_frame_bytes(one, "cuda")
    for V, Cr in outs:
        assert np.array_equal(V.cpu().numpy(), V0) and tuple(Cr.shape) == A0.shape and bool(torch.isfinite(Cr).all())
    assert torch.equal(outs[0][1].view(torch.int32), outs[1][1].view(torch.int32))
    assert not torch.equal(outs[0][1], clean[1])                          # (the bit was one the decoder reads)

    seq = bitstream.encode_sequence_bytes([(V0, A0), (V1, A1)], J, 0.05, "cuda", seg_len=256, gop=2, inter="always")
    assert bitstream.sequence_kinds(seq) == ["I", "P"]
    off = bitstream.parse_sequence(seq)
    inner = bitstream.parse_pframe(bitstream.sequence_frame(seq, 1, off))[2]
    inner_at = off[2] - len(inner)                                        # (the inner frame is the wrapper's tail)
    bad2 = flipped(seq, inner_at, inner)
    outs = [bitstream.decode_sequence_bytes(bad2, device="cuda") for _ in range(2)]
    clean = bitstream.decode_sequence_bytes(seq, device="cuda")
    for dec in outs:
        assert len(dec) == 2
        for (V, Cr), (Vw, Aw) in zip(dec, ((V0, A0), (V1, A1))):
            assert np.array_equal(V.cpu().numpy(), Vw) and tuple(Cr.shape) == Aw.shape and bool(torch.isfinite(Cr).all())
        assert torch.equal(dec[0][1], clean[0][1])                        # the I frame is untouched
    assert torch.equal(outs[0][1][1].view(torch.int32), outs[1][1][1].view(torch.int32))
    assert not torch.equal(outs[0][1][1], clean[1][1])
