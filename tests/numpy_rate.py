"""A numpy / plain Python model of raht_rlgr_seg_rate, independent of the library: the quantizer in the matrix's own precision,
the LENGTH of the RLGR stream of a sequence (the coder of python/PyRLGR/src/libs/rlgr/membuf.cpp:340-423 with every write
replaced by its bit count), the size of the segmented container, and the squared quantization error in float64."""
import numpy as np

L, U0, D0, U1, D1 = 4, 3, 1, 2, 1            # membuf.h:18-22
MAGIC_LEN = 8                                # len(b"RLGS0001")


def quantize(x, step):
    """floor(x / step + 0.5) in x's own dtype (float32 or float64) -> int64"""
    x = np.asarray(x)
    st = np.asarray(step, dtype=x.dtype)
    return np.floor(x / st + x.dtype.type(0.5)).astype(np.int64)


def rlgr_bits(seq, flag_signed=1):
    """bits membuf::rlgrWrite emits for seq (before the padding to a byte)"""
    bits = 0
    u = 0
    k = 0
    k_P, k_RP, m = 0, 2 * L, 0
    for v in (int(x) for x in seq):
        if flag_signed:
            u = 2 * v if v >= 0 else -2 * v - 1                          # _s2u, membuf.cpp:4-13
        else:
            u = v & 0xffffffff
        k, k_R = k_P // L, k_RP // L
        if k:
            if u:
                u -= 1
                bits += 1 + k                                           # write(0); write(m, k)
                m = 0
                coded = True
            else:
                coded = False
                m += 1
                if m == 1 << k:
                    bits += 1                                           # write(1)
                    k_P += U1
                    m = 0
        else:
            coded = True
        if coded:
            p = u >> k_R
            bits += p + 1 + k_R if p < 32 else 64                       # grWrite, membuf.cpp:242-256
            if p:
                k_RP = min(k_RP + p - 1, 32 * L)
            else:
                k_RP = max(k_RP - 2, 0)
            if k:                                                      # run mode: always down by D1
                k_P = max(k_P - D1, 0)
            elif u:
                k_P = max(k_P - D0, 0)
            else:
                k_P += U0
            m = 0
    if len(seq) and k and not u:                                        # membuf.cpp:416-419: the open run
        bits += 1 + k_P // L
    return bits


def rlgr_len(seq, flag_signed=1):
    """bytes of the closed stream"""
    return (rlgr_bits(seq, flag_signed) + 7) // 8


def container_bytes(seg_lens):
    """size of the segmented container whose segments have these unpadded lengths: magic, five int64, a uint32 length per
    segment, every stream in a 4-byte slot"""
    seg_lens = np.asarray(seg_lens, np.int64).reshape(-1)
    return MAGIC_LEN + 40 + 4 * seg_lens.size + int(((seg_lens + 3) // 4 * 4).sum())


def segment_table(Q, seg_len, flag_signed=1):
    """lengths of all segments of an (N, D) integer matrix, g = c * nseg + s"""
    N, D = Q.shape
    nseg = -(-N // seg_len)
    out = np.zeros(D * nseg, np.int64)
    for c in range(D):
        for s in range(nseg):
            out[c * nseg + s] = rlgr_len(Q[s * seg_len: (s + 1) * seg_len, c], flag_signed)
    return out


def sse(T, q, step):
    """per-column sum of ((double)T - (double)q * (double)step)^2"""
    e = np.asarray(T, np.float64) - np.asarray(q, np.float64) * np.asarray(np.asarray(step, dtype=np.asarray(T).dtype), np.float64)
    return (e * e).sum(axis=0)
