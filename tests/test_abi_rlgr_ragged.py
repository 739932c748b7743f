"""CPU-only checks of the ragged-batch entry points of the segmented RLGR coder at the C-ABI boundary
(raht_rlgr_seg_encode_ragged / raht_rlgr_seg_decode_ragged): declared, exported and bound, and every argument rule refused with
RAHT_ERR_INVALID and the function's name before any HIP call. No compute calls: the "device pointers" are addresses that must
never be read, and no entry point is called with them in a case that would get as far as a launch."""
import ctypes
import os
import re

import pytest

INVALID = -1
BATCH_MAX = 12                                                        # RAHT_RLGR_BATCH_MAX
ENC, DEC = "raht_rlgr_seg_encode_ragged", "raht_rlgr_seg_decode_ragged"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# never dereferenced: every call below is refused before its first HIP call
A, B, Cc, Dd, E = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
D, S = 8, 64


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def _vp(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _i64(*vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def test_the_two_symbols_are_declared_exported_and_bound(L):
    from raht_3dgs_codec_amd import _lib
    header = open(os.path.join(ROOT, "include", "raht.h")).read()
    for name in (ENC, DEC):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
    assert len(L.raht_rlgr_seg_encode_ragged.argtypes) == 14
    assert len(L.raht_rlgr_seg_decode_ragged.argtypes) == 15


def _enc(L, k, N, sym, chan, Q=None, seg_bytes=None, seg_off=None, out=None, cap=None, tot=True, d=D, s=S):
    """k frames at fake addresses 64 bytes apart; a table given as False is passed as NULL"""
    def tab(given, base):
        return None if given is False else (given if given is not None else _vp(*[base + 64 * j for j in range(max(k, 1))]))
    n = max(k, 1)
    return L.raht_rlgr_seg_encode_ragged(k, tab(Q, A), None if N is None else _i64(*N), d, None if sym is None else _i64(*sym),
                                         None if chan is None else _i64(*chan), s, 1, tab(seg_bytes, B), tab(seg_off, Cc), tab(out, Dd),
                                         _i64(*[1 << 20] * n) if cap is None else cap, _i64(*[0] * n) if tot else None, None)


def _dec(L, k, N, sym, chan, inp=None, in_bytes=None, seg_off=None, seg_bytes=None, Q=None, expect=None, bad=E, d=D, s=S):
    def tab(given, base):
        return None if given is False else (given if given is not None else _vp(*[base + 64 * j for j in range(max(k, 1))]))
    n = max(k, 1)
    return L.raht_rlgr_seg_decode_ragged(k, tab(inp, A), _i64(*[1 << 12] * n) if in_bytes is None else in_bytes, tab(seg_off, Cc), tab(seg_bytes, B),
                                         None if N is None else _i64(*N), d, s, 1, tab(Q, Dd), expect, None if sym is None else _i64(*sym),
                                         None if chan is None else _i64(*chan), bad, None)


def _refused(L, rc, name, what):
    assert rc == INVALID, (what, rc)
    assert name.encode() in L.raht_last_error(), (what, L.raht_last_error())


def test_encoder_argument_rules(L):
    N = [100, 7]
    rm = ([D, D + 3], [1, 1])                                           # row-major strides
    cm = ([1, 1], [100, 8])                                             # channel-major strides
    _refused(L, _enc(L, 0, [100], [D], [1]), ENC, "k = 0")
    _refused(L, _enc(L, BATCH_MAX + 1, [100] * 13, [D] * 13, [1] * 13), ENC, "k = 13")
    for name in ("Q", "seg_bytes", "seg_off", "out"):
        _refused(L, _enc(L, 2, N, *rm, **{name: False}), ENC, name + " NULL")
    _refused(L, _enc(L, 2, N, *rm, tot=False), ENC, "total_bytes NULL")
    _refused(L, _enc(L, 2, None, *rm), ENC, "N NULL")
    _refused(L, _enc(L, 2, N, None, rm[1]), ENC, "sym_stride NULL")
    _refused(L, _enc(L, 2, N, rm[0], None), ENC, "chan_stride NULL")
    _refused(L, _enc(L, 2, N, *rm, Q=_vp(A, None)), ENC, "Q[1] NULL")
    _refused(L, _enc(L, 2, [100, 0], *rm), ENC, "N[1] = 0")
    _refused(L, _enc(L, 2, [100, -5], *cm), ENC, "N[1] < 0")
    _refused(L, _enc(L, 2, N, [D, 1], [1, 7]), ENC, "mixed layout kinds")
    assert b"all channel-major or all row-major" in L.raht_last_error()
    _refused(L, _enc(L, 2, N, [1, 1], [100, 6]), ENC, "channel-major, chan_stride < N[1]")
    assert b"frame 1" in L.raht_last_error()
    _refused(L, _enc(L, 2, N, [D, D - 1], [1, 1]), ENC, "row-major, sym_stride < D")
    _refused(L, _enc(L, 2, N, *rm, out=_vp(Dd, Dd + 66)), ENC, "out[1] unaligned")
    assert b"frame 1" in L.raht_last_error()
    _refused(L, _enc(L, 2, N, *rm, cap=_i64(1 << 20, 8)), ENC, "cap[1] < 16")
    _refused(L, _enc(L, 2, N, *rm, s=63), ENC, "seg_len < 64")
    _refused(L, _enc(L, 2, N, *rm, d=0), ENC, "D < 1")
    # a frame whose shape needs 64-bit offsets: refused, and the text names it
    wideN = 6_000_000
    assert L.raht_rlgr_seg_offsets_width(wideN, 56, 2048) == 64 and L.raht_rlgr_seg_offsets_width(1000, 56, 2048) == 32
    _refused(L, _enc(L, 3, [1000, 2000, wideN], [56] * 3, [1] * 3, d=56, s=2048), ENC, "frame 2 needs 64-bit offsets")
    assert b"frame 2" in L.raht_last_error() and b"4 GiB" in L.raht_last_error()
    _refused(L, _enc(L, 2, [2 ** 40, 10], [1, 1], [2 ** 40, 10], d=1), ENC, "frame 0: too many segments")
    assert b"frame 0" in L.raht_last_error()


def test_decoder_argument_rules(L):
    N = [100, 7]
    rm = ([D, D + 3], [1, 1])
    cm = ([1, 1], [100, 8])
    _refused(L, _dec(L, 0, [100], [D], [1]), DEC, "k = 0")
    _refused(L, _dec(L, BATCH_MAX + 1, [100] * 13, [D] * 13, [1] * 13), DEC, "k = 13")
    for name in ("inp", "seg_off", "seg_bytes", "Q"):
        _refused(L, _dec(L, 2, N, *rm, **{name: False}), DEC, name + " NULL")
    _refused(L, _dec(L, 2, None, *rm), DEC, "N NULL")
    _refused(L, _dec(L, 2, N, None, rm[1]), DEC, "sym_stride NULL")
    _refused(L, _dec(L, 2, N, *rm, seg_off=_vp(Cc, None)), DEC, "seg_off[1] NULL")
    _refused(L, _dec(L, 2, [100, 0], *rm), DEC, "N[1] = 0")
    _refused(L, _dec(L, 2, N, [D, 1], [1, 7]), DEC, "mixed layout kinds")
    _refused(L, _dec(L, 2, N, [1, 1], [100, 6]), DEC, "channel-major, chan_stride < N[1]")
    _refused(L, _dec(L, 2, N, *rm, inp=_vp(A, A + 66)), DEC, "in[1] unaligned")
    _refused(L, _dec(L, 2, N, *rm, in_bytes=_i64(4096, 4098)), DEC, "in_bytes[1] not a multiple of 4")
    _refused(L, _dec(L, 2, N, *rm, in_bytes=_i64(4096, -4)), DEC, "in_bytes[1] < 0")
    _refused(L, _dec(L, 2, N, *rm, s=63), DEC, "seg_len < 64")
    _refused(L, _dec(L, 3, [1000, 2000, 6_000_000], [56] * 3, [1] * 3, d=56, s=2048), DEC, "frame 2 needs 64-bit offsets")
    assert b"frame 2" in L.raht_last_error()
    # expect: row-major frames only, bad_dev required, every expect[j] set
    _refused(L, _dec(L, 2, N, *cm, expect=_vp(E, E + 64)), DEC, "expect with channel-major frames")
    assert b"row-major" in L.raht_last_error()
    _refused(L, _dec(L, 2, N, *rm, expect=_vp(E, E + 64), bad=None), DEC, "expect without bad_dev")
    _refused(L, _dec(L, 2, N, *rm, expect=_vp(E, None)), DEC, "expect[1] NULL")
