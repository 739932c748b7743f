"""The predicted octree geometry on the GPU (csrc/octree_inter.hip, geometry.OctreeCoder with ``ref_keys``) against the numpy model
of tests/numpy_octree_inter.py: the residual stream byte for byte, the whole ``OCTP0001`` section in both modes (mode 1: model +
host RLGR coder), exact round trips, and the decoder's behaviour on residuals that are built to be refused: a flag and keys
inside the buffer, never a store behind it. Every key set of tests/test_gpu_octree.py (level sizes on both sides of every launch
border, J = 21 with its 63-bit shifts at the root) meets six kinds of reference frame."""
import numpy as np
import pytest

from . import numpy_octree as M
from . import numpy_octree_inter as MI
from . import test_gpu_octree as T

pytestmark = pytest.mark.gpu

SENTINEL = T.SENTINEL
KINDS = ["identical", "every other key", "a superset", "one voxel", "independent", "a tenth jittered"]
_MODEL = {}


def _reference(kind, keys, J, rng):
    from raht_3dgs_codec_amd import synth
    if kind == "identical":
        return keys.copy()
    if kind == "every other key":
        return keys[::2].copy()
    if kind == "one voxel":
        return keys[len(keys) // 2: len(keys) // 2 + 1].copy()
    if kind in ("a superset", "independent"):
        n = len(keys) if kind == "independent" else max(len(keys) // 4, 1)
        extra = np.unique(rng.integers(0, 8 ** J, size=n, dtype=np.uint64))
        return extra if kind == "independent" else np.unique(np.concatenate([keys, extra]))
    V = synth.keys_to_coords(keys, J)                                        # a tenth of the voxels moved by one along every axis
    move = rng.random(len(keys)) < 0.1
    move[0] = True
    V[move] = np.clip(V[move] + rng.choice(np.array([-1, 1]), size=(int(move.sum()), 3)), 0, (1 << J) - 1)
    return np.unique(synth.morton_keys(V, J))


def _cases(kind):
    """{name: (keys, J, reference keys, counts, the model's residual stream)}, computed once and left unchanged"""
    if kind not in _MODEL:
        rng = np.random.default_rng(KINDS.index(kind) + 77)
        out = {}
        for name, (keys, J) in T._key_sets().items():
            ref = _reference(kind, keys, J, rng)
            out[name] = (keys, J, ref) + MI.res_stream(keys, ref, J)
        _MODEL[kind] = out
    return _MODEL[kind]


@pytest.fixture(scope="module")
def rt():
    import torch
    import raht_3dgs_codec_amd as R
    assert torch.cuda.is_available()
    return R


@pytest.mark.parametrize("kind", KINDS)
def test_residual_stream_equals_the_model(rt, kind):
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    cases = _cases(kind)
    assert len(cases) > 50
    for name, (keys, J, ref, counts, res) in cases.items():
        got = OctreeCoder.residual(T._dev_keys(keys), J, counts, T._dev_keys(ref)).cpu().numpy()
        assert np.array_equal(got, res), (name, int(np.flatnonzero(got != res)[0]) if len(got) == len(res) else "length")
        if kind == "identical":
            assert not got.any(), name


@pytest.mark.parametrize("kind", KINDS)
def test_sections_equal_the_model_and_round_trip_in_both_modes(rt, kind):
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    for name, (keys, J, ref, counts, res) in _cases(kind).items():
        kd, rd = T._dev_keys(keys), T._dev_keys(ref)
        for entropy, seg_len in (("raw", None), ("rlgr", 64), ("rlgr", 256), ("rlgr", 1000)):
            blob = OctreeCoder.encode(kd, J, entropy=entropy, seg_len=seg_len, ref_keys=rd)
            want = MI.section(keys, ref, J, 0) if entropy == "raw" else MI.section(keys, ref, J, 1, seg_len, T._host_rlgr)
            assert blob == want, (name, entropy, seg_len, len(blob), len(want))
            h = OctreeCoder.parse(blob)
            assert h["predicted"] and h["N_ref"] == len(ref) and h["n_used"] == (len(np.unique(res)) if entropy == "rlgr" else 0), name
            assert np.array_equal(T._back(OctreeCoder.decode(blob, "cuda", ref_keys=rd)), keys), (name, entropy, seg_len)
        if kind == "identical":                                              # header + table + 8 bytes per segment of zeros
            assert len(blob) == MI.header_bytes(J) + 256 + 8 * ((len(res) + 999) // 1000), name


def test_the_default_segment_length_and_an_intra_section_with_ref_keys(rt):
    from raht_3dgs_codec_amd.geometry import DEFAULT_SEG_LEN, OctreeCoder
    keys, J, ref, counts, res = _cases("a tenth jittered")["200 k scene"]
    kd, rd = T._dev_keys(keys), T._dev_keys(ref)
    blob = OctreeCoder.encode(kd, J, ref_keys=rd)
    assert blob == MI.section(keys, ref, J, 1, DEFAULT_SEG_LEN, T._host_rlgr)
    intra = OctreeCoder.encode(kd, J)
    assert len(blob) < len(intra)                                            # nine tenths of the scene stand still
    assert np.array_equal(T._back(OctreeCoder.decode(intra, "cuda", ref_keys=rd)), keys)       # an intra section ignores them


# ---- hardening: residuals the decoder is built to refuse -------------------------------------------------------------------------
def _decode_guarded(counts, J, res, ref):
    """raht_octree_decode_inter into a buffer with sentinel regions around keys[0 .. N) -> (bad flag, keys, sentinels intact)"""
    import torch
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    N, G = counts[-1], 4096
    buf = torch.full((N + 2 * G,), SENTINEL, dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    OctreeCoder.keys_from_residual(torch.from_numpy(res).cuda(), counts, J, T._dev_keys(ref), bad, out=buf[G: G + N])
    torch.cuda.synchronize()
    return int(bad.item()), T._back(buf[G: G + N]), bool((buf[:G] == SENTINEL).all().item() and (buf[G + N:] == SENTINEL).all().item())


@pytest.mark.parametrize("name", ["200 k scene", "sparse n=2049", "dense n=16391", "prefix shard"])
def test_corrupt_residuals_raise_the_flag_and_stay_inside_the_buffer(rt, name):
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    keys, J, ref, counts, res = _cases("a tenth jittered")[name]
    flag, got, intact = _decode_guarded(counts, J, res, ref)
    assert flag == 0 and intact and np.array_equal(got, keys)
    occ = M.occ_stream(keys, J)[1]
    off = np.concatenate([[0], np.cumsum(counts[:-1])])
    rng = np.random.default_rng(1)
    cases = {}
    for g in sorted({0, J // 2, J - 1}):
        at = int(off[g] + rng.integers(0, counts[g]))
        z = res.copy()
        z[at] ^= occ[at]                                                  # res = pred: the reconstructed byte is 0
        cases[f"a byte that makes the occupancy 0 at level {g}"] = (counts, z)
        free = np.flatnonzero((occ[off[g]: off[g + 1] if g + 1 < J else len(occ)] != 0xff))
        if len(free):
            at = int(off[g] + free[0])
            x = res.copy()
            x[at] ^= np.uint8(1 << int(np.flatnonzero(np.unpackbits(occ[at: at + 1], bitorder="little") == 0)[0]))
            cases[f"popcounts one too many at level {g}"] = (counts, x)
            if bin(int(occ[at])).count("1") > 1:
                y = res.copy()
                y[at] ^= np.uint8(1 << int(np.flatnonzero(np.unpackbits(occ[at: at + 1], bitorder="little"))[0]))
                cases[f"popcounts one too few at level {g}"] = (counts, y)
    cases["every residual 0xff"] = (counts, np.full_like(res, 0xff))
    cases["the residuals of another reference"] = (counts, MI.res_stream(keys, keys[::3], J)[1])
    if counts[-1] > 1 and counts[-2] < counts[-1]:
        lie = list(counts)
        lie[-1] -= 1
        cases["N one too small"] = (lie, res)
    assert len(cases) >= 6
    for what, (cn, s) in cases.items():
        flag, _, intact = _decode_guarded(cn, J, s, ref)
        assert intact, what
        assert flag != 0, what
        blob = MI.MAGIC + np.array([J, cn[-1], 0, len(s), 0, len(ref), 0] + list(cn), np.int64).tobytes() + s.tobytes()
        with pytest.raises(ValueError, match="does not decode"):
            OctreeCoder.decode(blob, "cuda", ref_keys=T._dev_keys(ref))


def test_a_symbol_at_or_above_n_used_is_refused(rt):
    import torch
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    keys, J, ref, counts, res = _cases("a tenth jittered")["sparse n=2049"]
    table = M.rank_table(res)
    used = len(np.unique(res))
    assert 1 < used < 255 and table[0] == 0                                  # byte 0 is in use: the intra rule would stop at rank 0
    rank_of = np.zeros(256, np.int32)
    rank_of[table] = np.arange(256)
    n = len(res)
    good = torch.from_numpy(rank_of[res]).cuda().view(1, n)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert np.array_equal(OctreeCoder.bytes_from_symbols(good, table, bad, n_used=used).cpu().numpy(), res) and int(bad.item()) == 0
    for wrong in (used, 255, 256, -1, 2 ** 31 - 1):
        sym = rank_of[res].copy()
        sym[n // 2] = wrong
        buf = torch.full((n + 1024,), 0xA5, dtype=torch.uint8, device="cuda")
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        OctreeCoder.bytes_from_symbols(torch.from_numpy(sym).cuda().view(1, n), table, bad, out=buf[:n], n_used=used)
        assert int(bad.item()) != 0, wrong
        assert bool((buf[n:] == 0xA5).all().item()), wrong
        got = buf[:n].cpu().numpy()
        assert got[n // 2] == 0 and np.array_equal(np.delete(got, n // 2), np.delete(res, n // 2)), wrong
    # through the section: the symbol `used` coded by the real coder
    sym = rank_of[res].copy()
    sym[n // 2] = used
    sc = SegmentedCoder(n, 1, 256, 0, "cuda")
    sc.encode(torch.from_numpy(sym).cuda().view(1, n))
    _, lens, payload = sc.container_parts()
    blob = (MI.MAGIC + np.array([J, len(keys), 1, n, 256, len(ref), used] + counts, np.int64).tobytes() + table.tobytes() + lens.tobytes()
            + payload.tobytes())
    OctreeCoder.parse(blob)
    with pytest.raises(ValueError, match="does not decode"):
        OctreeCoder.decode(blob, "cuda", ref_keys=T._dev_keys(ref))


def test_a_wrong_number_of_reference_keys_is_refused(rt):
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    keys, J, ref, counts, res = _cases("a superset")["dense n=513"]
    kd, rd = T._dev_keys(keys), T._dev_keys(ref)
    blob = OctreeCoder.encode(kd, J, ref_keys=rd)
    assert np.array_equal(T._back(OctreeCoder.decode(blob, "cuda", ref_keys=rd)), keys)
    for wrong in (rd[:-1], kd, None, rd.view(1, -1)):
        with pytest.raises(ValueError, match="predicted from"):
            OctreeCoder.decode(blob, "cuda", ref_keys=wrong)
