"""bitstream.decode_region_bytes and the pieces under it on the GPU: the layout kernels (raht_region_layout, raht_region_cells,
raht_region_assemble) against the numpy model (tests/numpy_region.py), a decoder of selected segments against the whole one, and
the region decoder against decode_frame_bytes on the same blob.

The two decoders are two float32 paths that round the tree above the cells in different launches, so the attribute check was to
be a measured one: both compared, per column, with the float64 model on rows [a, b), the region decoder allowed twice the
whole-frame decoder's largest error there plus one float32 ulp of the column's largest magnitude (the triangle inequality, as in
tests/test_gpu_parity.py). Measured on the MI355X, the two turned out BIT-IDENTICAL on every column of every case below (and on
one depth-2 cell of the 3 M x 59 benchmark frame, tools/time_region.py): a butterfly is the same float32 (float64 on the wide
columns) expression of the same two rows and weights whichever launch performs it. So the test asserts torch.equal, which implies
the bound; both errors against the model are still printed (run with -s) and listed in DESIGN.md 16: a few float32 ulp of the
column's largest magnitude, the same figure for both decoders."""
import functools

import numpy as np
import pytest

from . import numpy_region as M

pytestmark = pytest.mark.gpu

# (draws, J, D, n_wide, seg_len, per-channel steps)
SHAPES = [(3000, 6, 5, 0, 64, False), (3000, 6, 59, 3, 64, False), (20000, 10, 14, 0, 256, True), (400, 5, 3, 0, 64, False)]
CASES = [(i, d) for i, s in enumerate(SHAPES) for d in sorted({1, 2, 3, s[1] - 1}) if d <= s[1] - 1]


@functools.lru_cache(maxsize=None)
def _frame(i):
    """everything about shape i that is computed once and only read afterwards"""
    import torch
    from raht_3dgs_codec_amd import bitstream, synth
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    draws, J, D, n_wide, S, per_channel = SHAPES[i]
    V, keys, C = synth.scene(draws, J, D, seed=70 + i)
    steps = [0.004 * (1 + (c % 7)) for c in range(D)] if per_channel else 0.01
    blob = bitstream.encode_frame_bytes(V, C, J, steps, "cuda", n_wide=n_wide, seg_len=S)
    h = bitstream.parse_frame(blob)
    ao, al = h["attributes"]
    att = blob[ao: ao + al]
    Vw, Cw = bitstream.decode_frame_bytes(blob, "cuda")
    Q = SegmentedCoder.from_container(att, "cuda").decode(row_major=True)
    # the steps as the kernels use them: float64 on the wide columns, cast to float32 everywhere else
    st = np.array(h["steps"] * (D if len(h["steps"]) == 1 else 1), np.float64)
    st[n_wide:] = st[n_wide:].astype(np.float32).astype(np.float64)
    model = M.decode_frame(keys, J, Q.cpu().numpy(), st)
    assert np.array_equal(Vw.cpu().numpy(), V)
    return dict(J=J, D=D, S=S, N=len(keys), keys=keys, keys_dev=torch.from_numpy(keys.view(np.int64)).cuda(), V=Vw, C=Cw, Q=Q, blob=blob,
                ao=ao, att=att, model=model)


@pytest.mark.parametrize("i, depth", CASES)
def test_layout_and_cells_equal_the_model(i, depth):
    import torch
    from raht_3dgs_codec_amd import ops
    f = _frame(i)
    J, N, keys, kd = f["J"], f["N"], f["keys"], f["keys_dev"]
    tl = 3 * (J - depth)
    ck, cf = M.cells(keys, tl)
    gk, gf = ops.region_cells(kd, 3 * J, tl, len(ck))
    assert gk.dtype == torch.int64 and np.array_equal(gk.cpu().numpy().view(np.uint64), ck) and np.array_equal(gf.cpu().numpy(), cf)
    for wrong in {max(len(ck) - 1, 1), min(len(ck) + 1, N)} - {len(ck)}:
        with pytest.raises(ops.RahtError, match="RAHT_ERR_INVALID"):
            ops.region_cells(kd, 3 * J, tl, wrong)
    ranges = [M.region_rows(keys, J, depth, c0, c1) for c0, c1 in M.regions(keys, J, depth).values()] + [(0, N), (0, 0), (N, N), (N // 2, N // 2)]
    for a, b in ranges:
        got = ops.region_layout(kd, 3 * J, a, b)
        assert got.dtype == torch.int64 and np.array_equal(got.cpu().numpy(), M.layout(keys, a, b)), (a, b)


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_assemble_equals_the_model(i):
    import torch
    from raht_3dgs_codec_amd import ops
    f = _frame(i)
    Q = f["Q"]
    n = Q.shape[0]
    wide = torch.zeros((n, Q.shape[1] + 3), dtype=torch.int32, device="cuda")
    wide[:, : Q.shape[1]] = Q
    for runs, rows in (([(0, 2, 5), (n - 70, 70, 70), (n // 2, 141, 1)], 200), ([], 3), ([(0, 0, n)], n), ([(n - 1, 64, 1)], 65)):
        want = np.zeros((rows, Q.shape[1]), np.int32)
        for s, d, c in runs:
            want[d: d + c] = Q[s: s + c].cpu().numpy()
        for src in (Q, wide[:, : Q.shape[1]]):                            # (a row stride above D too)
            assert np.array_equal(ops.region_assemble(src, runs, rows).cpu().numpy(), want), runs
    with pytest.raises(ops.RahtError, match="RAHT_ERR_INVALID"):
        ops.region_assemble(Q, [(n - 1, 0, 2)], 4)


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_decoder_of_selected_segments_equals_the_whole_one(i):
    import torch
    from raht_3dgs_codec_amd.rlgr import SegmentedCoder
    f = _frame(i)
    N, S, D, Q = f["N"], f["S"], f["D"], f["Q"]
    nseg = -(-N // S)
    picks = {(0,), (nseg - 1,), (0, nseg - 1), tuple(range(nseg // 3, nseg // 3 + min(3, nseg - nseg // 3))), tuple(range(nseg))}
    for ids in sorted(picks):
        sc, ranges = SegmentedCoder.from_container_segments(f["att"], list(ids), "cuda", max_symbols=N * D)
        rows = M.covered_rows(ids, S, N)
        assert (sc.N, sc.D, sc.S, sc.nseg) == (len(rows), D, S, len(ids))
        got = sc.decode(row_major=True)
        assert got.dtype == torch.int32 and torch.equal(got, Q[torch.from_numpy(rows).cuda()]), ids
        assert int(sc.bad.item()) == 0 and sum(ln for _, ln in ranges) == M.attribute_bytes(f["att"], ids)
    with pytest.raises(ValueError, match="more than the caller allows"):
        SegmentedCoder.from_container_segments(f["att"], [0], "cuda", max_symbols=D)


def _scrambled(blob, ranges):
    keep = np.zeros(len(blob), bool)
    for o, ln in ranges:
        keep[o: o + ln] = True
    return np.where(keep, np.frombuffer(blob, np.uint8), 0xFF).astype(np.uint8).tobytes(), int(keep.sum())


@pytest.mark.parametrize("i, depth", CASES)
def test_region_decoder_against_the_whole_frame_decoder(i, depth):
    import torch
    from raht_3dgs_codec_amd import bitstream
    f = _frame(i)
    J, N, D, S, keys, blob = f["J"], f["N"], f["D"], f["S"], f["keys"], f["blob"]
    worst = (0.0, 0.0)
    for name, cells in M.regions(keys, J, depth).items():
        a, b = M.region_rows(keys, J, depth, *cells)
        V, C, info = bitstream.decode_region_bytes(blob, depth, cells, "cuda", max_voxels=N)
        assert V.dtype == torch.int64 and C.dtype == torch.float32 and tuple(V.shape) == (b - a, 3) and tuple(C.shape) == (b - a, D), name
        assert info["rows"] == (a, b) and info["geometry_decoded"] is True and info["segments_total"] == -(-N // S), name
        assert info["n_cells"] == len(np.unique(keys[a:b] >> np.uint64(3 * (J - depth)))), name
        assert torch.equal(info["keys"], f["keys_dev"]), name
        ids = M.segments(*M.coded_runs(keys, J, depth, a, b), S) if b > a else []
        assert info["segments_decoded"] == len(ids), name
        assert info["bytes_needed"] == sum(ln for _, ln in info["byte_ranges"]) == f["ao"] + M.attribute_bytes(f["att"], ids), name
        assert torch.equal(V, f["V"][a:b]), name
        if b > a:
            ref = f["model"][a:b]
            ew = np.abs(f["C"][a:b].cpu().numpy().astype(np.float64) - ref).max(axis=0)
            er = np.abs(C.cpu().numpy().astype(np.float64) - ref).max(axis=0)
            ulp = np.spacing(np.abs(ref).max(axis=0).astype(np.float32)).astype(np.float64)
            same = int((C.view(torch.int32) == f["C"][a:b].view(torch.int32)).sum().item())
            print(f"shape {SHAPES[i]} depth {depth} region {name}: rows [{a}, {b}), {len(ids)} of {info['segments_total']} segments, "
                  f"{info['bytes_needed']} of {len(blob)} bytes; max over columns of error / ulp: whole {np.max(ew / ulp):.3f}, "
                  f"region {np.max(er / ulp):.3f}; bit-identical elements {same} of {C.numel()}")
            worst = (max(worst[0], float(np.max(ew / ulp))), max(worst[1], float(np.max(er / ulp))))
            assert torch.equal(C, f["C"][a:b]), (name, np.max(er / ulp), np.max(ew / ulp))
        # every byte outside the ranges may be anything (the geometry section is inside them)
        other, kept = _scrambled(blob, info["byte_ranges"])
        assert kept == info["bytes_needed"] <= len(blob) and (name != "all" or kept == len(blob)), name
        V2, C2, info2 = bitstream.decode_region_bytes(other, depth, cells, "cuda")
        assert torch.equal(V2, V) and torch.equal(C2, C) and info2["byte_ranges"] == info["byte_ranges"], name
        # the keys of the first call spare the second one the geometry
        V3, C3, info3 = bitstream.decode_region_bytes(blob, depth, cells, "cuda", keys=info["keys"])
        assert torch.equal(V3, V) and torch.equal(C3, C) and info3["geometry_decoded"] is False, name
        assert {k: v for k, v in info3.items() if k not in ("keys", "geometry_decoded")} == {k: v for k, v in info.items() if k not in ("keys", "geometry_decoded")}
    print(f"shape {SHAPES[i]} depth {depth}: worst error / ulp over the regions: whole-frame decoder {worst[0]:.3f}, region decoder {worst[1]:.3f}")


def test_refusals():
    import torch
    from raht_3dgs_codec_amd import bitstream
    f = _frame(3)
    J, N, blob = f["J"], f["N"], f["blob"]
    _, _, info = bitstream.decode_region_bytes(blob, 1, (0, 1), "cuda")
    bad = {"depth = 0": dict(depth=0), "depth = J": dict(depth=J), "depth no number": dict(depth="x"), "c0 = c1": dict(cells=(3, 3)),
           "c0 > c1": dict(cells=(4, 3)), "c0 < 0": dict(cells=(-1, 3)), "c1 > 8^depth": dict(cells=(0, 9)), "three cells": dict(cells=(0, 1, 2)),
           "keys too short": dict(keys=info["keys"][:-1]), "keys too long": dict(keys=torch.cat([info["keys"], info["keys"][-1:] + 1])),
           "keys on the host": dict(keys=info["keys"].cpu()), "keys of another type": dict(keys=info["keys"].to(torch.int32)),
           "keys of another frame": dict(keys=torch.arange(N, dtype=torch.int64, device="cuda")),
           "more voxels than the caller allows": dict(max_voxels=N - 1), "a truncated blob": dict(blob=blob[:-1])}
    for what, kw in bad.items():
        args = dict(blob=blob, depth=1, cells=(0, 8), device="cuda")
        args.update(kw)
        with pytest.raises(ValueError):
            bitstream.decode_region_bytes(**args)
            pytest.fail(what)
    V = np.array([[0, 0, 0], [1, 1, 1]], np.int64)
    flat = bitstream.encode_frame_bytes(V, np.ones((2, 3), np.float32), 1, 0.01, "cuda", seg_len=64)
    for depth in (0, 1, 2):
        with pytest.raises(ValueError, match="depth"):
            bitstream.decode_region_bytes(flat, depth, (0, 1), "cuda")
