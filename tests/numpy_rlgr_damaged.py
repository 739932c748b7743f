"""The reference RLGR decoder loop (python/PyRLGR membuf.cpp:258-338, as oracle/raht_oracle.c:587-621 restates it) on ARBITRARY
bytes, in plain Python integers with no width limit: what a segment of the GPU entropy stage (csrc/rlgr_seg.hip) must decode to
when its bytes are not what an encoder wrote -- a truncated download, a flipped bit.

Two things are made definite that the reference leaves to chance on such input: bits past the end of the stream read as
zeros (the reference's bit counter underflows there), and a run of zeros stops at symbol n (the reference writes on).

The kernels carry their state in 32 bits; a 64-bit decoder and this one part ways with them only where that state overflows.
``left_domain`` reports it: a decoded value that does not fit int32, a Golomb-Rice value of 2^32 or more, or a run header that
is asked for one more doubling at k >= 31. While it stays False the kernels must give exactly these symbols.
"""

L, U0, D0, U1, D1 = 4, 3, 1, 2, 1                                      # membuf.h:18-22


class _Bits:
    """MSB-first reader over bytes, zero-extended without end"""

    def __init__(self, buf):
        buf = bytes(buf)
        self.val = int.from_bytes(buf, "big")
        self.total = 8 * len(buf)
        self.pos = 0

    def read(self, bits):
        if bits == 0:
            return 0
        end = self.pos + bits
        if end <= self.total:
            v = (self.val >> (self.total - end)) & ((1 << bits) - 1)
        else:
            have = max(self.total - self.pos, 0)
            v = (self.val & ((1 << have) - 1)) << (bits - have)
        self.pos = end
        return v

    def golomb_rice(self, k):                                          # membuf.cpp:228-240
        p = 0
        while self.read(1):
            p += 1
            if p >= 32:
                return self.read(32)
        return (p << k) + self.read(k)


def _u2s(v):                                                           # membuf.cpp:16-23
    return -(v >> 1) - 1 if v & 1 else v >> 1


def decode(buf, n, flag_signed=1):
    """-> (the n symbols as Python ints, info). info["left_domain"]: see the module's text. info["overshoot"]: some run header
    announced more zeros than there were symbols left (the reference's own loop writes past its output there: its build must
    not be handed such bytes). info["bits"]: the bits consumed, past the end included."""
    r = _Bits(buf)
    seq = []
    k_P, k_RP = 0, 2 * L
    left = overshoot = False

    def emit(v):
        nonlocal left
        if not -2 ** 31 <= v <= 2 ** 31 - 1:
            left = True
        seq.append(v)

    def adapt(u, k_R):
        nonlocal k_RP
        p = u >> k_R
        if p:
            k_RP = min(k_RP + p - 1, 32 * L)
        else:
            k_RP = 0 if k_RP < 2 else k_RP - 2

    while len(seq) < n:
        k, k_R = k_P // L, k_RP // L
        if k:                                                          # run mode, membuf.cpp:274-309
            m = 0
            while r.read(1):
                if k >= 31:
                    left = True
                m += 1 << k
                k_P += U1
                k = k_P // L
            m += r.read(k)
            room = n - len(seq)
            if m > room:
                overshoot = True
            seq.extend([0] * min(m, room))
            if len(seq) >= n:
                break
            u = r.golomb_rice(k_R)
            if u >= 2 ** 32:
                left = True
            emit(_u2s(u + 1) if flag_signed else u + 1)
            adapt(u, k_R)
            k_P = 0 if k_P < D1 else k_P - D1
        else:                                                          # no-run mode, membuf.cpp:310-333
            u = r.golomb_rice(k_R)
            if u >= 2 ** 32:
                left = True
            emit(_u2s(u) if flag_signed else u)
            adapt(u, k_R)
            if u:
                k_P = 0 if k_P < D0 else k_P - D0
            else:
                k_P += U0
    return seq, {"left_domain": left, "overshoot": overshoot, "bits": r.pos}


def empty_stream_pattern(n):
    """what no bits at all decode to (every bit a zero): 0, 0, then a run header of length 0 and a closing symbol coded as 0 -- that
    is -1 -- while k_P steps down 6, 5, 4: 0, 0, -1, -1, -1, 0, -1, -1, -1, 0, ...  Worked out by hand from the loop, to hold the
    model to it:
      k_P 0 -> symbol 0, k_P 3;  k_P 3 -> symbol 0, k_P 6;  k_P 6 (k 1): empty run, closing -1, k_P 5;  5 -> -1, 4;  4 -> -1, 3;
      k_P 3 (k 0): symbol 0, k_P 6;  and from here the period (-1, -1, -1, 0) repeats. k_RP falls meanwhile, 8, 6, 4, 2, 0, which
      changes no symbol (every remainder is read as zeros)."""
    out, k_P = [], 0
    while len(out) < n:
        if k_P // L:
            out.append(-1)
            k_P -= 1
        else:
            out.append(0)
            k_P += U0
    return out
