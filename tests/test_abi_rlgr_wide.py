"""CPU-only checks of the segmented RLGR coder's 64-bit-offset entry points at the C-ABI boundary (raht_rlgr_seg_offsets_width,
raht_rlgr_seg_encode64 / _decode64 / _encode_batch64 / _decode_batch64): exported and bound; the width rule (the one place that
decides which shapes the 32-bit tables take) against the formula it stands for; the 32-bit entry points still refuse what the rule
sends to the 64-bit ones; and every argument rule of the 64-bit entry points and of their seven 32-bit twins (the same tables, on a
shape the 32-bit tables take) is refused with RAHT_ERR_INVALID and the name the entry point reports under before any HIP call. No
compute calls: the "device pointers" are addresses that must never be read, and no entry point is
called with them in a case that would get as far as a launch."""
import ctypes
import os
import random

import pytest

INVALID = -1
NAMES = ("raht_rlgr_seg_offsets_width", "raht_rlgr_seg_encode64", "raht_rlgr_seg_decode64", "raht_rlgr_seg_encode_batch64",
         "raht_rlgr_seg_decode_batch64")
BATCH_MAX = 12                                                        # RAHT_RLGR_BATCH_MAX
# shapes at seg_len = 2048 (and one at 1024) on either side of the 32-bit rule
NARROW = ((3_000_000, 59, 2048), (5_894_144, 56, 2048))
WIDE = ((5_894_145, 56, 2048), (5_595_137, 59, 2048), (6_000_000, 56, 2048), (6_000_000, 59, 2048), (50_000_000, 59, 2048),
        (6_000_000, 56, 1024))


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def test_the_five_symbols_are_exported_and_bound(L):
    from raht_3dgs_codec_amd import _lib
    for name in NAMES:
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
        assert getattr(L, name).argtypes is not None, name
    assert len(L.raht_rlgr_seg_offsets_width.argtypes) == 3
    assert len(L.raht_rlgr_seg_encode64.argtypes) == 13
    assert len(L.raht_rlgr_seg_decode64.argtypes) == 13
    assert len(L.raht_rlgr_seg_encode_batch64.argtypes) == 14
    assert len(L.raht_rlgr_seg_decode_batch64.argtypes) == 15


def _model(L, N, D, S):
    """the rule as the issue states it, from raht_rlgr_bound"""
    G = -(-N // S) * D
    return 64 if (L.raht_rlgr_bound(S) + 4) * G >= 2 ** 32 else 32


def test_offsets_width_at_the_named_shapes(L):
    for N, D, S in NARROW:
        assert L.raht_rlgr_seg_offsets_width(N, D, S) == 32, (N, D, S)
    for N, D, S in WIDE:
        assert L.raht_rlgr_seg_offsets_width(N, D, S) == 64, (N, D, S)


def test_offsets_width_equals_the_formula_on_a_sweep(L):
    rng = random.Random(20261016)
    shapes = [(N, D, S) for (N, D, S) in NARROW + WIDE]
    for _ in range(400):
        S = rng.choice((64, 100, 1000, 1024, 2048, 4096, 100000, rng.randrange(64, 1 << 20)))
        D = rng.choice((1, 3, 4, 56, 59, 64, rng.randrange(1, 300)))
        # around the boundary of this (D, seg_len) as well as anywhere
        per_seg = L.raht_rlgr_bound(S) + 4
        nseg_edge = max(1, (2 ** 32) // (per_seg * D))
        N = rng.choice((rng.randrange(1, 400_000_000), max(1, nseg_edge * S + rng.randrange(-2 * S, 2 * S))))
        if -(-N // S) * D < 2 ** 31:
            shapes.append((N, D, S))
    assert len(shapes) > 300
    seen = set()
    for N, D, S in shapes:
        w = L.raht_rlgr_seg_offsets_width(N, D, S)
        assert w == _model(L, N, D, S), (N, D, S, w)
        seen.add(w)
    assert seen == {32, 64}


def test_offsets_width_refuses_what_nobody_accepts(L):
    for what, (N, D, S) in {"N = 0": (0, 56, 2048), "D = 0": (1000, 0, 2048), "seg_len = 63": (1000, 56, 63),
                            "G >= 2^31": (2 ** 31, 64, 64), "nseg >= 2^31": (2 ** 37, 1, 64),
                            "a segment longer than uint32": (10 ** 9, 1, 400_000_000)}.items():
        assert L.raht_rlgr_seg_offsets_width(N, D, S) == INVALID, what
        assert b"raht_rlgr_seg_offsets_width" in L.raht_last_error(), (what, L.raht_last_error())


def _vp(*vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def _i64(*vals):
    return (ctypes.c_int64 * len(vals))(*vals)


# never dereferenced: every call below is refused before its first HIP call
A, B, Cc, Dd, E = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000


def test_the_32_bit_entry_points_still_refuse_the_wide_shapes(L):
    tot = ctypes.c_int64(0)
    for N, D, S in WIDE:
        for sym, chan in ((1, N), (D, 1)):
            rc = L.raht_rlgr_seg_encode_strided(A, N, D, sym, chan, S, 1, B, Cc, Dd, 1 << 20, ctypes.byref(tot), None)
            assert rc == INVALID and b"4 GiB" in L.raht_last_error(), (N, D, S, rc, L.raht_last_error())
            assert b"raht_rlgr_seg_encode" in L.raht_last_error()
            rc = L.raht_rlgr_seg_encode_batch(2, _vp(A, A + 64), N, D, sym, chan, S, 1, _vp(B, B + 64), _vp(Cc, Cc + 64), _vp(Dd, Dd + 64),
                                              _i64(1 << 20, 1 << 20), _i64(0, 0), None)
            assert rc == INVALID and b"4 GiB" in L.raht_last_error(), (N, D, S, rc, L.raht_last_error())
            assert b"raht_rlgr_seg_encode_batch" in L.raht_last_error()


def _refused(L, name, rc, what):
    assert rc == INVALID, (name, what, rc)
    assert (name + ":").encode() in L.raht_last_error(), (name, what, L.raht_last_error())


# the shape the broken-rule tables below start from, by the width of the offset tables that take it
SHAPES = {32: (3_000_000, 56, 2048), 64: (6_000_000, 56, 2048)}


# (entry point, width, the name its errors carry, channel-major only: no sym_stride argument)
@pytest.mark.parametrize("entry,width,name,cm_only", [("raht_rlgr_seg_encode64", 64, "raht_rlgr_seg_encode64", False),
                                                      ("raht_rlgr_seg_encode_strided", 32, "raht_rlgr_seg_encode", False),
                                                      ("raht_rlgr_seg_encode", 32, "raht_rlgr_seg_encode", True)])
def test_encode_argument_validation(L, entry, width, name, cm_only):
    N0, D0, S0 = SHAPES[width]
    tot = ctypes.c_int64(0)

    def call(Q=A, N=N0, D=D0, sym=1, chan=N0, S=S0, sb=B, so=Cc, out=Dd, cap=1 << 20, tb=ctypes.byref(tot)):
        if cm_only:
            assert sym == 1
            return L.raht_rlgr_seg_encode(Q, N, D, chan, S, 1, sb, so, out, cap, tb, None)
        return getattr(L, entry)(Q, N, D, sym, chan, S, 1, sb, so, out, cap, tb, None)

    cases = {
        "NULL Q": dict(Q=None), "NULL seg_bytes": dict(sb=None), "NULL seg_off": dict(so=None), "NULL out": dict(out=None),
        "NULL total_bytes": dict(tb=None), "N = 0": dict(N=0, chan=1), "N < 0": dict(N=-5), "D = 0": dict(D=0), "seg_len = 63": dict(S=63),
        "seg_len = 0": dict(S=0), "channel-major with chan_stride < N": dict(chan=N0 - 1), "row-major with sym_stride < D": dict(sym=D0 - 1, chan=1),
        "neither layout": dict(sym=2, chan=2), "sym_stride = 0": dict(sym=0), "chan_stride = 0": dict(sym=D0, chan=0), "cap = 15": dict(cap=15),
        "cap < 0": dict(cap=-1), "out not 4-byte aligned": dict(out=Dd + 2), "too many segments": dict(N=2 ** 31, D=64, S=64, chan=2 ** 31),
        "a segment longer than uint32": dict(N=10 ** 9, D=1, S=400_000_000, chan=10 ** 9),
    }
    if cm_only:
        cases = {what: cases[what] for what in ("NULL Q", "NULL seg_bytes", "NULL seg_off", "NULL out", "NULL total_bytes", "D = 0", "seg_len = 63",
                                                "channel-major with chan_stride < N", "cap = 15")}
    for what, kw in cases.items():
        _refused(L, name, call(**kw), what)
    if not cm_only:
        assert call(N=2 ** 31, D=64, S=64, chan=2 ** 31) == INVALID and b"too many segments" in L.raht_last_error()


@pytest.mark.parametrize("entry,width,name,cm_only", [("raht_rlgr_seg_decode64", 64, "raht_rlgr_seg_decode64", False),
                                                      ("raht_rlgr_seg_decode_strided", 32, "raht_rlgr_seg_decode", False),
                                                      ("raht_rlgr_seg_decode", 32, "raht_rlgr_seg_decode", True)])
def test_decode_argument_validation(L, entry, width, name, cm_only):
    N0, D0, S0 = SHAPES[width]
    sym0, chan0 = (1, N0) if cm_only else (D0, 1)

    def call(inp=A, nbytes=1 << 20, so=B, sb=Cc, N=N0, D=D0, S=S0, Q=Dd, sym=sym0, chan=chan0, bad=E):
        if cm_only:
            assert sym == 1
            return L.raht_rlgr_seg_decode(inp, nbytes, so, sb, N, D, S, 1, Q, chan, bad, None)
        return getattr(L, entry)(inp, nbytes, so, sb, N, D, S, 1, Q, sym, chan, bad, None)

    cases = {
        "NULL in": dict(inp=None), "NULL seg_off": dict(so=None), "NULL seg_bytes": dict(sb=None), "NULL Q": dict(Q=None),
        "N = 0": dict(N=0), "D = 0": dict(D=0), "seg_len = 63": dict(S=63), "in_bytes < 0": dict(nbytes=-4),
        "in_bytes not a multiple of 4": dict(nbytes=(1 << 20) + 2), "in not 4-byte aligned": dict(inp=A + 1),
        "row-major with sym_stride < D": dict(sym=D0 - 1), "channel-major with chan_stride < N": dict(sym=1, chan=N0 - 1),
        "neither layout": dict(sym=3, chan=3), "too many segments": dict(N=2 ** 31, D=64, S=64, sym=64),
    }
    if cm_only:
        cases = {what: cases[what] for what in ("NULL in", "NULL seg_off", "NULL seg_bytes", "NULL Q", "D = 0", "seg_len = 63",
                                                "channel-major with chan_stride < N")}
    for what, kw in cases.items():
        _refused(L, name, call(**kw), what)


@pytest.mark.parametrize("entry,width", [("raht_rlgr_seg_encode_batch64", 64), ("raht_rlgr_seg_encode_batch", 32)])
def test_encode_batch_argument_validation(L, entry, width):
    N0, D0, S0 = SHAPES[width]

    def call(k=3, Q=_vp(A, A + 64, A + 128), N=N0, D=D0, sym=D0, chan=1, S=S0, sb=_vp(B, B + 64, B + 128), so=_vp(Cc, Cc + 64, Cc + 128),
             out=_vp(Dd, Dd + 64, Dd + 128), cap=_i64(1 << 20, 1 << 20, 1 << 20), tb=_i64(0, 0, 0)):
        return getattr(L, entry)(k, Q, N, D, sym, chan, S, 1, sb, so, out, cap, tb, None)

    many = BATCH_MAX + 1
    cases = {
        "k = 0": dict(k=0), "k < 0": dict(k=-1),
        "k = RAHT_RLGR_BATCH_MAX + 1": dict(k=many, Q=_vp(*[A] * many), sb=_vp(*[B] * many), so=_vp(*[Cc] * many), out=_vp(*[Dd] * many),
                                            cap=_i64(*[1 << 20] * many), tb=_i64(*[0] * many)),
        "NULL Q": dict(Q=None), "NULL seg_bytes": dict(sb=None), "NULL seg_off": dict(so=None), "NULL out": dict(out=None), "NULL cap": dict(cap=None),
        "NULL total_bytes": dict(tb=None), "NULL Q[1]": dict(Q=_vp(A, None, A + 128)), "NULL seg_bytes[2]": dict(sb=_vp(B, B + 64, None)),
        "NULL seg_off[0]": dict(so=_vp(None, Cc + 64, Cc + 128)), "NULL out[1]": dict(out=_vp(Dd, None, Dd + 128)),
        "out[2] not 4-byte aligned": dict(out=_vp(Dd, Dd + 64, Dd + 130)), "cap[1] = 15": dict(cap=_i64(1 << 20, 15, 1 << 20)),
        "N = 0": dict(N=0), "D = 0": dict(D=0), "seg_len = 63": dict(S=63), "row-major with sym_stride < D": dict(sym=D0 - 1),
        "channel-major with chan_stride < N": dict(sym=1, chan=N0 - 1), "neither layout": dict(sym=2, chan=2),
        "too many segments": dict(N=2 ** 31, D=64, S=64, sym=64),
    }
    for what, kw in cases.items():
        _refused(L, entry, call(**kw), what)
    assert call(Q=_vp(A, None, A + 128)) == INVALID and b"frame 1" in L.raht_last_error()


# (entry point, width, how it takes expect[]: "optional" argument, "none" at all, "required": the faults of expect[] then carry
# the entry point's own name and every other fault raht_rlgr_seg_decode_batch's)
@pytest.mark.parametrize("entry,width,expects", [("raht_rlgr_seg_decode_batch64", 64, "optional"), ("raht_rlgr_seg_decode_batch", 32, "none"),
                                                 ("raht_rlgr_seg_decode_batch_check", 32, "required")])
def test_decode_batch_argument_validation(L, entry, width, expects):
    N0, D0, S0 = SHAPES[width]
    many = BATCH_MAX + 1
    EX = _vp(E + 64, E + 128, E + 192)
    UNSET = object()

    def call(k=3, inp=_vp(A, A + 64, A + 128), nbytes=_i64(1 << 20, 1 << 20, 1 << 20), so=_vp(B, B + 64, B + 128), sb=_vp(Cc, Cc + 64, Cc + 128),
             N=N0, D=D0, S=S0, Q=_vp(Dd, Dd + 64, Dd + 128), expect=UNSET, sym=D0, chan=1, bad=E):
        if expects == "none":
            assert expect is UNSET
            return L.raht_rlgr_seg_decode_batch(k, inp, nbytes, so, sb, N, D, S, 1, Q, sym, chan, bad, None)
        if expect is UNSET:                                           # (k = 13: as many entries as the call may look at)
            expect = _vp(*[E + 64] * k) if expects == "required" and k > 3 else EX if expects == "required" else None
        return getattr(L, entry)(k, inp, nbytes, so, sb, N, D, S, 1, Q, expect, sym, chan, bad, None)

    general = {
        "k = 0": dict(k=0),
        "k = RAHT_RLGR_BATCH_MAX + 1": dict(k=many, inp=_vp(*[A] * many), nbytes=_i64(*[1 << 20] * many), so=_vp(*[B] * many), sb=_vp(*[Cc] * many),
                                            Q=_vp(*[Dd] * many)),
        "NULL in": dict(inp=None), "NULL in_bytes": dict(nbytes=None), "NULL seg_off": dict(so=None), "NULL seg_bytes": dict(sb=None), "NULL Q": dict(Q=None),
        "NULL in[0]": dict(inp=_vp(None, A + 64, A + 128)), "NULL seg_off[1]": dict(so=_vp(B, None, B + 128)), "NULL seg_bytes[2]": dict(sb=_vp(Cc, Cc + 64, None)),
        "NULL Q[1]": dict(Q=_vp(Dd, None, Dd + 128)), "in[1] not 4-byte aligned": dict(inp=_vp(A, A + 66, A + 128)),
        "in_bytes[2] < 0": dict(nbytes=_i64(1 << 20, 1 << 20, -4)), "in_bytes[0] not a multiple of 4": dict(nbytes=_i64(1001, 1 << 20, 1 << 20)),
        "N = 0": dict(N=0), "D = 0": dict(D=0), "seg_len = 63": dict(S=63), "row-major with sym_stride < D": dict(sym=D0 - 1),
        "neither layout": dict(sym=2, chan=2), "too many segments": dict(N=2 ** 31, D=64, S=64, sym=64),
        "channel-major with chan_stride < N": dict(sym=1, chan=N0 - 1), "expect and k = 0": dict(expect=EX, k=0),
    }
    of_expect = {
        "expect with a NULL inside": dict(expect=_vp(E + 64, None, E + 192)), "expect without bad_dev": dict(expect=EX, bad=None),
        "expect with channel-major frames": dict(expect=EX, sym=1, chan=N0),
    }
    if expects == "required":
        of_expect["NULL expect"] = dict(expect=None)
        for what in ("channel-major with chan_stride < N", "neither layout"):
            # (chan_stride != 1 breaks the layout rule AND the row-major rule of expect[]: either name may report it)
            assert call(**general.pop(what)) == INVALID and b"raht_rlgr_seg_decode_batch" in L.raht_last_error(), what
    for what, kw in general.items():
        if expects == "none" and "expect" in kw:
            continue
        _refused(L, "raht_rlgr_seg_decode_batch" if expects == "required" else entry, call(**kw), what)
    if expects != "none":
        for what, kw in of_expect.items():
            _refused(L, entry, call(**kw), what)
