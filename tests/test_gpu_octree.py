"""The octree geometry coder on the GPU (csrc/octree.hip, geometry.OctreeCoder) against the numpy model of tests/numpy_octree.py:
node counts and occupancy stream byte for byte, the rank table, the whole section in both modes (mode 1: model + host RLGR
coder), exact round trips, the input check of raht_octree_counts, demorton, and the decoder's behaviour on sections that are
built to be refused: a flag and keys inside the buffer, never a store behind it."""

import numpy as np
import pytest

from . import numpy_octree as M
from .conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu

CHUNK = 2048                       # OCT_CHUNK: nodes per workgroup step; levels up to one chunk go through the single-workgroup kernels
CFG2_COUNTS = [1, 8, 64, 375, 2110, 11618, 60854, 263126, 702599, 948501, 993262]
CFG3_COUNTS = [1, 8, 62, 401, 2257, 13034, 73716, 370027, 1360959, 2579895, 2939680, 2992251, 2999072]
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _host_rlgr(sym):
    from raht_3dgs_codec_amd import rlgr
    m = rlgr.membuf()
    m.rlgrWrite(np.ascontiguousarray(sym, np.int32), 0)
    return m.get_array()


def _key_sets():
    from raht_3dgs_codec_amd import synth
    rng = np.random.default_rng(4242)
    sets = {}
    for name in golden_names():
        g = load_golden(name)
        if all(f in g for f in ("V", "J", "morton")):
            sets["golden " + name] = (np.unique(g["morton"].astype(np.uint64)), int(g["J"]))
    sets["one voxel"] = (np.array([3], np.uint64), 1)
    sets["one voxel, J = 21"] = (np.array([8 ** 21 - 1], np.uint64), 21)
    for J in (3, 4, 5):
        sets[f"full cube J={J}"] = (np.arange(8 ** J, dtype=np.uint64), J)
    sets["J = 21 scene"] = (np.unique(rng.integers(0, 8 ** 21, size=30000, dtype=np.uint64)), 21)
    sets["200 k scene"] = (synth.sorted_unique_keys(200_000, 10, 5), 10)
    sets["prefix shard"] = (synth.sorted_unique_keys(100_000, 10, 7, prefix_range=(3, 5, 6)), 10)
    # level sizes on both sides of every launch-geometry border: one node, a thread's 8 items, one wave, one workgroup step
    # (2048 nodes: single-workgroup kernel / chunked launches), one more, several chunks. Dense: consecutive keys, the levels
    # shrink by 8; sparse: random keys at J = 21, (nearly) every level has the leaf count.
    for n in (2, 8, 9, 63, 64, 65, 511, 512, 513, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK, 2 * CHUNK + 1, 8 * CHUNK + 7):
        sets[f"dense n={n}"] = (np.arange(n, dtype=np.uint64) + np.uint64(8 ** 5 - n if n % 2 else 0), 6)
        k = np.unique(rng.integers(0, 8 ** 21, size=n + 8, dtype=np.uint64))[:n]
        sets[f"sparse n={n}"] = (k, 21)
    return sets


@pytest.fixture(scope="module")
def rt():
    import torch
    import raht_3dgs_codec_amd as R
    assert torch.cuda.is_available()
    return R


def _dev_keys(keys):
    import torch
    return torch.from_numpy(keys.view(np.int64).copy()).cuda()


def _back(t):
    return t.cpu().numpy().view(np.uint64)


def test_counts_and_occupancy_stream_equal_the_model(rt):
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    sets = _key_sets()
    assert len(sets) > 50
    for name, (keys, J) in sets.items():
        counts, stream = M.occ_stream(keys, J)
        kd = _dev_keys(keys)
        got = OctreeCoder.counts(kd, J)
        assert got == counts, name
        occ = OctreeCoder.occupancy(kd, J, got).cpu().numpy()
        assert np.array_equal(occ, stream), (name, int(np.flatnonzero(occ != stream)[0]) if len(occ) == len(stream) else "length")


def test_sections_equal_the_model_and_round_trip_in_both_modes(rt):
    from raht_3dgs_codec_amd.geometry import DEFAULT_SEG_LEN, OctreeCoder
    for name, (keys, J) in _key_sets().items():
        kd = _dev_keys(keys)
        for entropy, seg_len in (("raw", None), ("rlgr", None), ("rlgr", 64), ("rlgr", 1000)):
            blob = OctreeCoder.encode(kd, J, entropy=entropy, seg_len=seg_len)
            if entropy == "raw":
                want = M.geometry_section(keys, J, 0)
            else:
                want = M.geometry_section(keys, J, 1, seg_len or DEFAULT_SEG_LEN, _host_rlgr)
                h = OctreeCoder.parse(blob)
                assert np.array_equal(h["table"], M.rank_table(M.occ_stream(keys, J)[1])), name
            assert blob == want, (name, entropy, seg_len, len(blob), len(want))           # the whole container
            assert np.array_equal(_back(OctreeCoder.decode(blob, "cuda")), keys), (name, entropy, seg_len)


def test_unaligned_streams_take_the_scalar_kernels(rt):
    """the byte <-> rank kernels read 4 nodes per thread when the buffers are aligned for it, one by one otherwise: same result"""
    import torch
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    keys, J = _key_sets()["200 k scene"]
    counts, stream = M.occ_stream(keys, J)
    n = len(stream)
    table = M.rank_table(stream)
    rank_of = np.zeros(256, np.int32)
    rank_of[table] = np.arange(256)
    for shift in (0, 1, 2, 3):
        buf = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
        occ = buf[shift: shift + n]
        occ.copy_(torch.from_numpy(stream))
        symbuf = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
        sym = symbuf[shift: shift + n].view(1, n)
        _, tab = OctreeCoder.symbols(occ, out=sym)
        assert np.array_equal(tab, table)
        assert np.array_equal(sym.cpu().numpy()[0], rank_of[stream])
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        back = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
        OctreeCoder.bytes_from_symbols(sym, tab, bad, out=back[shift: shift + n])
        assert np.array_equal(back.cpu().numpy()[shift: shift + n], stream) and int(bad.item()) == 0
        assert int(back[:shift].sum()) == 0 and int(back[shift + n:].sum()) == 0


def test_counts_refuses_unsorted_duplicate_and_out_of_range_keys(rt):
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    keys, J = _key_sets()["200 k scene"]
    OctreeCoder.counts(_dev_keys(keys), J)
    swapped, dup, far = keys.copy(), keys.copy(), keys.copy()
    swapped[[70000, 70001]] = swapped[[70001, 70000]]
    dup[123456] = dup[123455]
    far[-1] = np.uint64(8 ** J)
    first = keys.copy()
    first[0], first[1] = keys[1], keys[0]
    for what, k in {"two rows swapped": swapped, "a duplicate": dup, "a key of 8^J": far, "the first two rows swapped": first,
                    "one key out of range": np.array([8 ** 4], np.uint64)}.items():
        with pytest.raises(rt.RahtError) as e:
            OctreeCoder.counts(_dev_keys(k), J if len(k) > 1 else 4)
        assert e.value.code == -1 and "raht_octree_counts" in str(e.value), what


def test_demorton_is_the_inverse_of_morton(rt):
    from raht_3dgs_codec_amd import ops, synth
    for name in ("200 k scene", "J = 21 scene", "one voxel, J = 21", "full cube J=4", "golden maxcoord_j6"):
        keys, J = _key_sets()[name]
        kd = _dev_keys(keys)
        V = ops.demorton(kd, J)
        assert np.array_equal(V.cpu().numpy(), synth.keys_to_coords(keys, J)), name
        assert np.array_equal(_back(ops.get_morton_code(V, J)), keys), name


# ---- hardening: sections the decoder is built to refuse --------------------------------------------------------------------------
def _decode_guarded(counts, J, stream):
    """raht_octree_decode into a buffer with a sentinel region behind keys[N] -> (bad flag, keys, sentinel region intact)"""
    import torch
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    N = counts[-1]
    buf = torch.full((N + 4096,), SENTINEL, dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    OctreeCoder.keys_from_occupancy(torch.from_numpy(stream).cuda(), counts, J, bad, out=buf[:N])
    torch.cuda.synchronize()
    return int(bad.item()), _back(buf[:N]), bool((buf[N:] == SENTINEL).all().item())


@pytest.mark.parametrize("name", ["200 k scene", "sparse n=2049", "dense n=16391", "prefix shard"])
def test_corrupt_streams_raise_the_flag_and_stay_inside_the_buffer(rt, name):
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    keys, J = _key_sets()[name]
    counts, stream = M.occ_stream(keys, J)
    flag, got, intact = _decode_guarded(counts, J, stream)
    assert flag == 0 and intact and np.array_equal(got, keys)
    off = np.concatenate([[0], np.cumsum(counts[:-1])])
    rng = np.random.default_rng(1)
    cases = {}
    for g in sorted({0, J // 2, J - 1}):
        at = int(off[g] + rng.integers(0, counts[g]))
        z = stream.copy()
        z[at] = 0
        cases[f"a zeroed byte at level {g}"] = (counts, z)
        x = stream.copy()
        x[at] = 0xff if x[at] != 0xff else 0x7f
        cases[f"a byte with other bits at level {g}"] = (counts, x)
    every = stream.copy()
    every[:] = 0xff                                                   # every level overflows its count eight-fold at most
    cases["every byte 0xff"] = (counts, every)
    for g in range(1, J):                                             # header counts that lie within the plausibility rules
        lie = list(counts)
        lie[g] += 1
        if all(lie[i] <= lie[i + 1] <= 8 * lie[i] for i in range(J)):
            cases[f"n_{g} one too large"] = (lie, np.concatenate([stream, stream[-1:]]))
            break
    if counts[-1] > 1 and counts[-2] < counts[-1]:
        lie = list(counts)
        lie[-1] -= 1
        cases["N one too small"] = (lie, stream)
    assert len(cases) >= 4
    for what, (cn, s) in cases.items():
        flag, _, intact = _decode_guarded(cn, J, s)
        assert intact, what
        assert flag != 0, what
        # the same through the section: ValueError
        blob = M.GEOMETRY_MAGIC + np.array([J, cn[-1], 0, len(s), 0] + list(cn), np.int64).tobytes() + s.tobytes()
        with pytest.raises(ValueError):
            OctreeCoder.decode(blob, "cuda")


def test_out_of_table_symbol_is_refused(rt):
    import torch
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    keys, J = _key_sets()["sparse n=2049"]
    counts, stream = M.occ_stream(keys, J)
    table = M.rank_table(stream)
    used = int(np.flatnonzero(table == 0)[0])
    assert 0 < used < 255
    rank_of = np.zeros(256, np.int32)
    rank_of[table] = np.arange(256)
    n = len(stream)
    for wrong in (used, 255, 256, -1, 2 ** 31 - 1):
        sym = rank_of[stream].copy()
        sym[n // 2] = wrong
        buf = torch.full((n + 1024,), 0xA5, dtype=torch.uint8, device="cuda")
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        OctreeCoder.bytes_from_symbols(torch.from_numpy(sym).cuda().view(1, n), table, bad, out=buf[:n])
        assert int(bad.item()) != 0, wrong
        assert bool((buf[n:] == 0xA5).all().item()), wrong
        got = buf[:n].cpu().numpy()
        assert got[n // 2] == 0 and np.array_equal(np.delete(got, n // 2), np.delete(stream, n // 2)), wrong
    # through the section: the symbol `used` coded by the real coder
    sym = rank_of[stream].copy()
    sym[n // 2] = used
    sc = SegmentedCoder(n, 1, 256, 0, "cuda")
    sc.encode(torch.from_numpy(sym).cuda().view(1, n))
    _, lens, payload = sc.container_parts()
    blob = (M.GEOMETRY_MAGIC + np.array([J, len(keys), 1, n, 256] + counts, np.int64).tobytes() + table.tobytes() + lens.tobytes()
            + payload.tobytes())
    OctreeCoder.parse(blob)
    with pytest.raises(ValueError):
        OctreeCoder.decode(blob, "cuda")
    good = OctreeCoder.encode(_dev_keys(keys), J, seg_len=256)
    assert np.array_equal(_back(OctreeCoder.decode(good, "cuda")), keys)


# ---- the benchmark scenes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg, expect", [("cfg2", CFG2_COUNTS), ("cfg3", CFG3_COUNTS)])
def test_benchmark_scenes_known_counts_round_trip_and_size(rt, cfg, expect):
    from raht_3dgs_codec_amd import _lib, synth
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    n, J, _, seed = synth.CONFIGS[cfg]
    keys = synth.sorted_unique_keys(n, J, seed)
    before = _lib.lib().raht_sort_fallbacks()
    kd = _dev_keys(keys)
    counts = OctreeCoder.counts(kd, J)
    assert counts == expect
    mcounts, stream = M.occ_stream(keys, J)
    assert np.array_equal(OctreeCoder.occupancy(kd, J, counts).cpu().numpy(), stream)
    raw = OctreeCoder.encode(kd, J, entropy="raw")
    coded = OctreeCoder.encode(kd, J)
    for blob in (raw, coded):
        assert np.array_equal(_back(OctreeCoder.decode(blob, "cuda", max_voxels=len(keys))), keys)
    assert len(coded) < len(raw)
    print(f"{cfg}: raw {len(raw)} B, rank + RLGR {len(coded)} B ({len(coded) / len(raw):.3f}), {8 * len(coded) / len(keys):.2f} bits/voxel")
    if cfg == "cfg2":                                                  # the exact size comes from the model (host coder, segment by segment)
        from raht_3dgs_codec_amd.geometry import DEFAULT_SEG_LEN
        assert coded == M.geometry_section(keys, J, 1, DEFAULT_SEG_LEN, _host_rlgr)
    assert _lib.lib().raht_sort_fallbacks() == before


def test_mode_1_is_smaller_than_mode_0_at_the_default_segment_length(rt):
    from raht_3dgs_codec_amd.geometry import DEFAULT_SEG_LEN, OctreeCoder
    keys, J = _key_sets()["200 k scene"]
    kd = _dev_keys(keys)
    raw, coded = OctreeCoder.encode(kd, J, entropy="raw"), OctreeCoder.encode(kd, J)
    want = M.geometry_section(keys, J, 1, DEFAULT_SEG_LEN, _host_rlgr)
    assert len(coded) == len(want) and len(coded) < len(raw), (len(coded), len(want), len(raw))


def test_more_chunks_than_the_grid_cap(rt):
    """a level of more than 2048 chunks (4.2 M nodes): grid-strided chunks and the scanned chunk offsets"""
    import torch
    from raht_3dgs_codec_amd.geometry import OctreeCoder
    J = 21
    k = torch.unique(torch.randint(0, 8 ** 21 - 1, (4_600_000,), dtype=torch.int64, device="cuda", generator=torch.Generator("cuda").manual_seed(3)))
    keys = k.cpu().numpy().view(np.uint64)
    assert len(keys) > 2048 * CHUNK + CHUNK
    counts, stream = M.occ_stream(keys, J)
    got = OctreeCoder.counts(k, J)
    assert got == counts
    occ = OctreeCoder.occupancy(k, J, got)
    assert np.array_equal(occ.cpu().numpy(), stream)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert torch.equal(OctreeCoder.keys_from_occupancy(occ, got, J, bad), k) and int(bad.item()) == 0
