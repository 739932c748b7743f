"""Damaged segments for the segmented RLGR decoders: the frames, and ONE seeded builder of damage cases, shared by the model's
own test (tests/test_rlgr_damaged_model.py, no GPU) and the GPU decoders' test (tests/test_gpu_rlgr_damaged.py).

A frame's segments are taken from the HOST coder here (segment g = c * nseg + s is the stream of Q[c, s * S: (s + 1) * S]); the GPU
encoder's are the same bytes (tests/test_gpu_rlgr_seg.py pins that, and the GPU test asserts it again for its frames).

A case is ``(name, g, damage)``: segment g of the frame gets ``damage`` --
  bytes  the segment's bytes are replaced (same length: the tables stay as they are);
  int    the segment's entry in the length table is replaced (the payload stays as it is).
Names that begin with ``sat_`` are the saturating kinds: they drive the decoders' 32-bit state over its edge on purpose and the
model is not asked about them. Every other kind must stay inside the model's domain.
"""
import numpy as np

# (name, N, D, seg_len): the smallest shapes that reach every edge of the decoders' bit readers --
#   last_of_one   a last segment of one symbol
#   wide          more channels than a wave has lanes
#   pieces        streams of many 32-byte pieces and several rounds of the ring's top-up (every 32 symbols)
#   noise         the same with 32-bit noise in channel 2: more than 16 words per 32 symbols, so that lane drains its ring of 16
#                 words between two top-ups and reads ahead of it word by word
SHAPES = (("last_of_one", 129, 3, 64), ("wide", 70, 65, 64), ("pieces", 2049, 5, 1024), ("noise", 2049, 5, 1024))
NOISE_CHANNEL = 2


def frame(name):
    """-> (N, D, seg_len, Q): Q (D, N) int32, Laplacian with a zero mask; channel scales from runs of zeros to several bytes a symbol"""
    (N, D, S), = [s[1:] for s in SHAPES if s[0] == name]
    rng = np.random.default_rng([17, N, D, S])
    scale = 10.0 ** rng.uniform(-0.5, 3.5, size=(D, 1))
    Q = (np.rint(rng.laplace(0, 1.0, size=(D, N)) * scale) * (rng.random((D, N)) < 0.6)).astype(np.int32)
    if name == "noise":
        Q[NOISE_CHANNEL] = rng.integers(-2 ** 31, 2 ** 31 - 1, size=N, endpoint=True).astype(np.int32)
    return N, D, S, Q


def symbols_of(N, S, g):
    """how many symbols segment g holds"""
    nseg = (N + S - 1) // S
    s = g % nseg
    return min(S, N - s * S)


def host_segments(Q, S, flag_signed=1):
    """the host coder's stream for every segment, in container order -> list of bytes"""
    from raht_3dgs_codec_amd import rlgr
    D, N = Q.shape
    out = []
    for c in range(D):
        for s0 in range(0, N, S):
            m = rlgr.membuf()
            m.rlgrWrite(Q[c, s0: s0 + S], flag_signed)
            out.append(m.get_array().tobytes())
    return out


def container(segs):
    """the payload as the encoder lays it out: every segment in a 4-byte slot -> (uint8 array, offsets (G + 1,), lengths (G,))"""
    lens = np.array([len(s) for s in segs], np.int64)
    offs = np.concatenate([[0], np.cumsum((lens + 3) // 4 * 4)])
    blob = np.zeros(int(offs[-1]), np.uint8)
    for s, o in zip(segs, offs):
        blob[o: o + len(s)] = np.frombuffer(s, np.uint8)
    return blob, offs, lens


def fragile_segments(name, N, D, S):
    """segments in which a lost bit position cannot stay inside the model's domain: the noise channel's. Its codes are 33 bits with
    k_R = 32 -- one bit read out of step and the next prefix is random bits: p >= 1 with k_R = 32 is a value of 2^32 and more.
    They get the cuts only (zeros behind the cut keep every prefix empty)."""
    nseg = (N + S - 1) // S
    return set(range(NOISE_CHANNEL * nseg, (NOISE_CHANNEL + 1) * nseg)) if name == "noise" else set()


CUTS = ("0", "1", "3", "4", "5", "half", "last")


def _cut_at(kind, nb):
    return {"0": 0, "1": 1, "3": 3, "4": 4, "5": 5, "half": nb // 2, "last": nb - 1}[kind]


def is_saturating(name):
    return name.startswith("sat_")


def build(segs, seed, fragile=()):
    """segs: the clean frame's segments (list of bytes, container order) -> [(name, g, damage)], see the module's text.
    Segments are dealt out from a seeded shuffle that goes round and round, so every segment of a small frame is damaged by
    several kinds; a kind that cannot apply to the segment it was dealt (a cut at or past its length, a longer length on the last
    segment, anything but a cut on a fragile segment) moves on to the next."""
    G = len(segs)
    rng = np.random.default_rng([23, seed, G])
    order = [int(g) for g in rng.permutation(G)]
    cursor = [0]

    def deal(ok):
        for _ in range(G):
            g = order[cursor[0] % G]
            cursor[0] += 1
            if ok(g):
                return g
        return None

    free = lambda g: g not in fragile and len(segs[g]) >= 1                                    # noqa: E731
    cases = []

    def add(name, g, damage):
        if g is None:
            return
        if isinstance(damage, (bytes, bytearray)):
            assert len(damage) == len(segs[g])
        cases.append((name, g, bytes(damage) if not isinstance(damage, int) else int(damage)))

    # in-domain kinds
    for kind in CUTS:                                                # the table says shorter, the payload is untouched ...
        g = deal(lambda g: 0 <= _cut_at(kind, len(segs[g])) < len(segs[g]))
        if g is not None:
            add(f"cut_table_{kind}", g, _cut_at(kind, len(segs[g])))
    for kind in CUTS:                                                # ... and the same cuts by zeroing the tail
        g = deal(lambda g: 0 <= _cut_at(kind, len(segs[g])) < len(segs[g]))
        if g is not None:
            c = _cut_at(kind, len(segs[g]))
            add(f"cut_zeros_{kind}", g, segs[g][:c] + bytes(len(segs[g]) - c))
    for g in sorted(fragile)[:2]:                                    # the fragile segments get cuts of their own
        nb = len(segs[g])
        add(f"cut_table_half_fragile{g}", g, nb // 2)
        add(f"cut_zeros_5_fragile{g}", g, segs[g][:5] + bytes(nb - 5))
        add(f"cut_table_last_fragile{g}", g, nb - 1)
    for where in ("first", "last", "random"):                        # one flipped bit
        g = deal(free)
        if g is None:
            continue
        b = bytearray(segs[g])
        at = {"first": 0, "last": len(b) - 1, "random": int(rng.integers(0, len(b)))}[where]
        b[at] ^= 1 << int(rng.integers(0, 8))
        add(f"flip_{where}", g, b)
    g = deal(free)
    if g is not None:
        add("random_bytes", g, rng.integers(0, 256, size=len(segs[g]), dtype=np.uint8).tobytes())
    g = deal(free)
    if g is not None:
        add("all_zero", g, bytes(len(segs[g])))
    g = deal(lambda g: free(g) and (g + 1) % G not in fragile and G > 1)
    if g is not None:                                                # the neighbour's bytes, cut or zero-extended to this segment's length
        nbr = segs[(g + 1) % G]
        add("neighbour", g, (nbr + bytes(len(segs[g])))[: len(segs[g])])
    g = deal(lambda g: g < G - 1)                                    # a longer length, inside the container: into the next slot
    if g is not None:
        add("longer", g, (len(segs[g]) + 3) // 4 * 4 + 3)
    # saturating kinds
    g = deal(free)
    if g is not None:
        add("sat_all_ff", g, b"\xff" * len(segs[g]))
    g = deal(lambda g: free(g) and len(segs[g]) >= 7)
    if g is None:
        g = deal(free)
    if g is not None:
        nb = len(segs[g])
        add("sat_zeros_then_ff", g, (bytes(6) + b"\xff" * nb)[:nb])
    return cases


def seen_bytes(blob, offs, lens, g, damage):
    """the bytes a decoder reads for segment g under a case: the replaced bytes, or the container's from the segment's start to
    its new length"""
    if isinstance(damage, int):
        assert int(offs[g]) + (damage + 3) // 4 * 4 <= len(blob), "a longer length must stay inside the container"
        return blob[int(offs[g]): int(offs[g]) + damage].tobytes()
    return damage
