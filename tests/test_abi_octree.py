"""CPU-only checks of the octree geometry coder: its six entry points at the C-ABI boundary (exported, bound, every argument rule
refused with RAHT_ERR_INVALID and the function's name before any HIP call -- the "device pointers" below are addresses that must
never be read), the pure-Python header parsers of the geometry section and the frame container, and the numpy model the GPU
tests compare against (tests/numpy_octree.py): against the set-of-prefixes definition, against the known node counts of the two
benchmark scenes, and through its own decoder."""
import ctypes
import os

import numpy as np
import pytest

from . import numpy_octree as M
from .conftest import golden_names, load_golden

INVALID = -1
NAMES = {"raht_octree_counts": 5, "raht_octree_encode": 6, "raht_octree_decode": 6, "raht_octree_symbols": 5, "raht_octree_bytes": 6,
         "raht_demorton": 5}
CFG2_COUNTS = [1, 8, 64, 375, 2110, 11618, 60854, 263126, 702599, 948501, 993262]
CFG3_COUNTS = [1, 8, 62, 401, 2257, 13034, 73716, 370027, 1360959, 2579895, 2939680, 2992251, 2999072]
A, B, Cc, Dd = 0x10000, 0x20000, 0x30000, 0x40000          # never dereferenced


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def _i64(*vals):
    return (ctypes.c_int64 * len(vals))(*vals)


def _refused(L, name, rc, what):
    assert rc == INVALID, (name, what, rc)
    assert name.encode() in L.raht_last_error(), (name, what, L.raht_last_error())


def test_the_six_symbols_are_exported_and_bound(L):
    from raht_3dgs_codec_amd import _lib
    for name, arity in NAMES.items():
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == arity, name
    assert L.raht_version() == 300


def test_counts_argument_validation(L):
    out = _i64(*[0] * 22)

    def call(keys=A, N=1000, J=10, counts=out):
        return L.raht_octree_counts(keys, N, J, counts, None)

    for what, kw in {"NULL keys": dict(keys=None), "NULL counts": dict(counts=None), "N = 0": dict(N=0), "N < 0": dict(N=-3),
                     "N = 2^31": dict(N=2 ** 31), "J = 0": dict(J=0), "J = 22": dict(J=22)}.items():
        _refused(L, "raht_octree_counts", call(**kw), what)


GOOD = (1, 8, 20, 100)                                       # J = 3, N = 100


def _bad_count_lists():
    return {"n_0 = 2": (2, 8, 20, 100), "n_0 = 0": (0, 0, 0, 0), "a level shrinks": (1, 8, 7, 56), "more than 8 children per node": (1, 9, 20, 100),
            "a level of 2^31": (1, 8, 64, 512, 4096, 32768, 262144, 2097152, 16777216, 134217728, 1073741824, 2 ** 31)}


def test_encode_argument_validation(L):
    def call(keys=A, N=100, J=3, counts=GOOD, occ=B):
        return L.raht_octree_encode(keys, N, J, None if counts is None else _i64(*counts), occ, None)

    cases = {"NULL keys": dict(keys=None), "NULL occ": dict(occ=None), "NULL counts": dict(counts=None), "N = 0": dict(N=0),
             "N = 2^31": dict(N=2 ** 31), "J = 0": dict(J=0), "J = 22": dict(J=22), "counts[J] != N": dict(N=99)}
    for what, cl in _bad_count_lists().items():
        cases[what] = dict(counts=cl, J=len(cl) - 1, N=cl[-1] if 0 < cl[-1] < 2 ** 31 else 100)
    for what, kw in cases.items():
        _refused(L, "raht_octree_encode", call(**kw), what)


def test_decode_argument_validation(L):
    def call(occ=A, counts=GOOD, J=3, keys=B, bad=Cc):
        return L.raht_octree_decode(occ, None if counts is None else _i64(*counts), J, keys, bad, None)

    cases = {"NULL occ": dict(occ=None), "NULL keys": dict(keys=None), "NULL bad": dict(bad=None), "NULL counts": dict(counts=None),
             "J = 0": dict(J=0), "J = 22": dict(J=22)}
    for what, cl in _bad_count_lists().items():
        cases[what] = dict(counts=cl, J=len(cl) - 1)
    for what, kw in cases.items():
        _refused(L, "raht_octree_decode", call(**kw), what)


def test_symbols_and_bytes_argument_validation(L):
    table = (ctypes.c_uint8 * 256)(*range(256))

    def sym(occ=A, n=1000, tab=table, s=B):
        return L.raht_octree_symbols(occ, n, tab, s, None)

    for what, kw in {"NULL occ": dict(occ=None), "NULL table": dict(tab=None), "NULL sym": dict(s=None), "n_nodes = 0": dict(n=0),
                     "n_nodes = 2^31": dict(n=2 ** 31), "sym not 4-byte aligned": dict(s=B + 2)}.items():
        _refused(L, "raht_octree_symbols", sym(**kw), what)

    twice = (ctypes.c_uint8 * 256)(*([1, 1] + list(range(2, 256))))

    def byt(s=A, n=1000, tab=table, occ=B, bad=Cc):
        return L.raht_octree_bytes(s, n, tab, occ, bad, None)

    for what, kw in {"NULL sym": dict(s=None), "NULL table": dict(tab=None), "NULL occ": dict(occ=None), "NULL bad": dict(bad=None),
                     "n_nodes = 0": dict(n=0), "n_nodes < 0": dict(n=-1), "sym not 4-byte aligned": dict(s=A + 1),
                     "a table that is no permutation": dict(tab=twice)}.items():
        _refused(L, "raht_octree_bytes", byt(**kw), what)


def test_demorton_argument_validation(L):
    for what, (keys, N, J, V) in {"NULL keys": (None, 10, 5, B), "NULL V": (A, 10, 5, None), "N < 0": (A, -1, 5, B), "J = 0": (A, 10, 0, B),
                                  "J = 22": (A, 10, 22, B)}.items():
        _refused(L, "raht_demorton", L.raht_demorton(keys, N, J, V, None), what)
    assert L.raht_demorton(None, 0, 5, None, None) == 0              # nothing to do, as raht_morton


# ---- the model -------------------------------------------------------------------------------------------------------------------
def _golden_key_sets():
    out = []
    for name in golden_names():
        g = load_golden(name)
        if all(f in g for f in ("V", "J", "morton")):
            out.append((name, np.unique(g["morton"].astype(np.uint64)), int(g["J"])))
    return out


def _random_key_sets():
    rng = np.random.default_rng(20261016)
    sets = [("one voxel", np.array([5], np.uint64), 1), ("one voxel deep", np.array([8 ** 21 - 1], np.uint64), 21),
            ("full cube", np.arange(8 ** 3, dtype=np.uint64), 3)]
    for J in (1, 2, 3, 5, 8):
        for n in (1, 2, 7, 60, 400):
            k = np.unique(rng.integers(0, 8 ** J, size=n, dtype=np.uint64))
            sets.append((f"random J={J} n={n}", k, J))
    return sets


def test_the_fixtures_offer_the_corner_cases():
    sets = _golden_key_sets()
    assert len(sets) >= 10
    assert {1, 20} <= {J for _, _, J in sets} and 1 in {len(k) for _, k, _ in sets}


def test_model_equals_the_set_of_prefixes_definition():
    for name, keys, J in _random_key_sets() + [s for s in _golden_key_sets() if len(s[1]) <= 3000]:
        counts, levels = M.occ_encode(keys, J)
        bc, bl = M.occ_brute_force(keys, J)
        assert counts == bc, name
        assert all(np.array_equal(a, b) for a, b in zip(levels, bl)), name
        assert counts[0] == 1 and counts[-1] == len(keys) and len(np.concatenate(levels)) == sum(counts[:-1]), name
        assert all(lv.min() > 0 for lv in levels), name


def test_model_round_trip():
    for name, keys, J in _random_key_sets() + _golden_key_sets():
        assert np.array_equal(M.occ_decode(M.occ_encode(keys, J)[1], J), keys), name


@pytest.mark.parametrize("cfg, expect", [("cfg2", CFG2_COUNTS), ("cfg3", CFG3_COUNTS)])
def test_model_known_node_counts(cfg, expect):
    from raht_3dgs_codec_amd import synth
    n, J, _, seed = synth.CONFIGS[cfg]
    keys = synth.sorted_unique_keys(n, J, seed)
    counts, levels = M.occ_encode(keys, J)
    assert counts == expect
    assert np.array_equal(M.occ_decode(levels, J), keys)


def test_rank_table_rule():
    stream = np.array([4, 4, 4, 9, 9, 2, 2, 200], np.uint8)
    t = M.rank_table(stream)
    assert list(t[:5]) == [4, 2, 9, 200, 0] and sorted(t) == list(range(256))     # ties by byte value; byte 0 leads the unused ones


# ---- the parsers -----------------------------------------------------------------------------------------------------------------
def _host_rlgr(L):
    from raht_3dgs_codec_amd import rlgr

    def enc(sym):
        m = rlgr.membuf()
        m.rlgrWrite(np.ascontiguousarray(sym, np.int32), 0)
        return m.get_array()
    return enc


def _sections(L):
    from raht_3dgs_codec_amd import synth
    keys = synth.sorted_unique_keys(3000, 6, 11)
    return keys, M.geometry_section(keys, 6, 0), M.geometry_section(keys, 6, 1, 256, _host_rlgr(L))


def _patched(blob, word, value, base=8):
    b = bytearray(blob)
    b[base + 8 * word: base + 8 * word + 8] = np.array([value], np.int64).tobytes()
    return bytes(b)


def test_geometry_parse_accepts_the_model_and_refuses_malformed_headers(L):
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    keys, raw, coded = _sections(L)
    counts, stream = M.occ_stream(keys, 6)
    for blob, mode in ((raw, 0), (coded, 1)):
        h = OctreeCoder.parse(blob)
        assert (h["J"], h["N"], h["mode"], h["n_nodes"], h["counts"], h["length"]) == (6, len(keys), mode, len(stream), counts, len(blob))
        assert OctreeCoder.parse(blob + b"trailing")["length"] == len(blob)
        bad = {
            "magic": b"OCTG0002" + blob[8:], "J = 0": _patched(blob, 0, 0), "J = 22": _patched(blob, 0, 22), "N = 0": _patched(blob, 1, 0),
            "N != n_J": _patched(blob, 1, len(keys) + 1), "mode 2": _patched(blob, 2, 2), "n_nodes off by one": _patched(blob, 3, len(stream) + 1),
            "n_0 = 2": _patched(blob, 5, 2), "a level shrinks": _patched(blob, 5 + 3, counts[2] - 1),
            "more than 8 children per node": _patched(blob, 5 + 2, 8 * counts[1] + 1), "truncated header": blob[:40],
            "truncated counts": blob[:8 + 40 + 8 * 3], "shorter than its header says": blob[:-1], "body missing": blob[:8 + 40 + 8 * 7],
        }
        for what, b in bad.items():
            with pytest.raises(ValueError):
                OctreeCoder.parse(b)
                pytest.fail(what)
        with pytest.raises(ValueError, match="more than the caller allows"):
            OctreeCoder.parse(blob, max_voxels=len(keys) - 1)
        assert OctreeCoder.parse(blob, max_voxels=len(keys))["N"] == len(keys)
    body = 8 + 40 + 8 * 7
    for what, b in {"seg_len = 63": _patched(coded, 4, 63), "seg_len = 2^31": _patched(coded, 4, 2 ** 31),
                    "a table that is no permutation": coded[:body] + coded[body + 1: body + 2] + coded[body + 1:],
                    "a segment longer than the blob": coded[:body + 256] + np.array([2 ** 31], np.uint32).tobytes() + coded[body + 260:]}.items():
        with pytest.raises(ValueError):
            OctreeCoder.parse(b)
            pytest.fail(what)


def test_frame_parse_accepts_the_model_and_refuses_malformed_headers(L):
    from raht_3dgs_codec_amd import bitstream
    keys, raw, coded = _sections(L)
    N, D = len(keys), 56

    def att(n=N, d=D):
        return b"RLGS0001" + np.array([n, d, 2048, 1, 0], np.int64).tobytes()

    steps = [0.01 * (1 + c % 5) for c in range(D)]
    for geo, st, nw in ((raw, [0.02], 0), (coded, steps, 3)):
        blob = M.frame_container(6, N, D, nw, st, geo, att(), (1.0, 2.0, 3.0), 64.0)
        h = bitstream.parse_frame(blob)
        assert (h["J"], h["N"], h["D"], h["n_wide"], h["steps"], h["vmin"], h["width"]) == (6, N, D, nw, st, [1.0, 2.0, 3.0], 64.0)
        go, gl = h["geometry"]
        ao, al = h["attributes"]
        assert blob[go: go + gl] == geo and blob[ao: ao + al] == att() and ao + al == len(blob)
        glen_at = 8 + 40 + 8 * (len(st) + 4)
        bad = {
            "magic": b"RAHTF002" + blob[8:], "J = 0": _patched(blob, 0, 0), "J = 22": _patched(blob, 0, 22), "N = 0": _patched(blob, 1, 0),
            "N that is not the geometry's": _patched(blob, 1, N + 1), "D = 0": _patched(blob, 2, 0), "n_wide > D": _patched(blob, 3, D + 1),
            "n_wide < 0": _patched(blob, 3, -1), "n_steps = 2": _patched(blob, 4, 2), "truncated header": blob[:30],
            "steps missing": blob[:8 + 40 + 8], "geometry longer than the blob": _patched(blob, 0, len(blob), glen_at),
            "geometry length too short": _patched(blob, 0, gl - 8, glen_at), "negative geometry length": _patched(blob, 0, -1, glen_at),
            "attribute container cut": blob[:-1], "attribute container missing": blob[:ao - 8],
            "a zero step": blob[:8 + 40] + np.array([0.0]).tobytes() + blob[8 + 48:],
            "a NaN step": blob[:8 + 40] + np.array([np.nan]).tobytes() + blob[8 + 48:],
            "attributes of another frame": M.frame_container(6, N, D, nw, st, geo, att(N, D + 1)),
            "attributes without magic": M.frame_container(6, N, D, nw, st, geo, b"x" * 48),
            "another J": M.frame_container(7, N, D, nw, st, geo, att()),
        }
        for what, b in bad.items():
            with pytest.raises(ValueError):
                bitstream.parse_frame(b)
                pytest.fail(what)
        with pytest.raises(ValueError, match="more than the caller allows"):
            bitstream.parse_frame(blob, max_voxels=N - 1)


def test_decoders_refuse_before_touching_a_device(L):
    """a malformed blob never gets as far as the first tensor: these run without a GPU"""
    from raht_3dgs_codec_amd import bitstream
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    _, raw, _ = _sections(L)
    with pytest.raises(ValueError):
        OctreeCoder.decode(raw[:-1], "cuda")
    with pytest.raises(ValueError):
        OctreeCoder.decode(raw, "cuda", max_voxels=10)
    with pytest.raises(ValueError):
        bitstream.decode_frame_bytes(b"RAHTF001" + raw, "cuda")
