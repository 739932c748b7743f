"""CPU-only checks of the region entry points at the C-ABI boundary: exported, bound, and every argument rule refused with
RAHT_ERR_INVALID and the function's name before any HIP call -- the "device pointers" below are addresses that must never be
read."""
import ctypes
import os

import pytest

INVALID = -1
NAMES = {"raht_region_layout": 7, "raht_region_cells": 8, "raht_region_assemble": 10}
A, B, Cc = 0x10000, 0x20000, 0x30000                        # never dereferenced


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def _refused(L, name, rc, what):
    assert rc == INVALID, (name, what, rc)
    assert name.encode() in L.raht_last_error(), (name, what, L.raht_last_error())


def test_the_three_symbols_are_exported_and_bound(L):
    from raht_3dgs_codec_amd import _lib, ops
    for name, arity in NAMES.items():
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == arity, name
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "raht.h")).read()
    assert "#define RAHT_REGION_BUCKETS 22" in header and ops.REGION_BUCKETS == 22


def test_layout_argument_validation(L):
    def call(keys=A, N=1000, nbits=30, lo=10, hi=20, table=B):
        return L.raht_region_layout(keys, N, nbits, lo, hi, table, None)

    for what, kw in {"NULL keys": dict(keys=None), "NULL table": dict(table=None), "N = 0": dict(N=0), "N < 0": dict(N=-5),
                     "N = 2^31": dict(N=2 ** 31), "row_lo > row_hi": dict(lo=21), "row_hi > N": dict(hi=1001), "row_lo < 0": dict(lo=-1),
                     "nbits = 0": dict(nbits=0), "nbits = 64": dict(nbits=64)}.items():
        _refused(L, "raht_region_layout", call(**kw), what)


def test_cells_argument_validation(L):
    def call(keys=A, N=1000, nbits=30, tl=12, n=50, ck=B, cf=Cc):
        return L.raht_region_cells(keys, N, nbits, tl, n, ck, cf, None)

    for what, kw in {"NULL keys": dict(keys=None), "NULL cell_keys": dict(ck=None), "NULL cell_first": dict(cf=None), "N = 0": dict(N=0),
                     "nbits = 0": dict(nbits=0), "nbits = 64": dict(nbits=64), "top_level no multiple of 3": dict(tl=13),
                     "top_level = 0": dict(tl=0), "top_level = nbits": dict(tl=30), "top_level above nbits - 3": dict(nbits=12, tl=12),
                     "n_cells = 0": dict(n=0), "n_cells > N": dict(n=1001)}.items():
        _refused(L, "raht_region_cells", call(**kw), what)


def test_assemble_argument_validation(L):
    def call(src=A, ld_src=8, n_src=100, dst=B, ld_dst=8, n_dst=50, D=8, runs=((0, 5, 10), (40, 15, 35)), n_runs=None):
        flat = [x for r in runs for x in r]
        arr = None if runs is None else (ctypes.c_int64 * max(len(flat), 1))(*flat)
        return L.raht_region_assemble(src, ld_src, n_src, dst, ld_dst, n_dst, D, arr, len(flat) // 3 if n_runs is None else n_runs, None)

    cases = {"NULL src": dict(src=None), "NULL dst": dict(dst=None), "D = 0": dict(D=0), "ld_src < D": dict(ld_src=7), "ld_dst < D": dict(ld_dst=7),
             "no source rows": dict(n_src=0), "no destination rows": dict(n_dst=0), "23 runs": dict(runs=tuple((i, i, 1) for i in range(23))),
             "n_runs < 0": dict(n_runs=-1), "a run past the end of src": dict(runs=((91, 0, 10),)), "a run before src": dict(runs=((-1, 0, 10),)),
             "a run past the end of dst": dict(runs=((0, 41, 10),)), "a run before dst": dict(runs=((0, -1, 10),)),
             "a negative count": dict(runs=((0, 0, -1),)), "runs that overlap in dst": dict(runs=((0, 5, 10), (40, 14, 5))),
             "destinations not ascending": dict(runs=((40, 15, 35), (0, 5, 10)))}
    for what, kw in cases.items():
        _refused(L, "raht_region_assemble", call(**kw), what)


def test_python_wrappers_refuse_host_tensors():
    import torch
    from raht_3dgs_codec_amd import bitstream, ops
    k = torch.arange(10, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.region_layout(k, 12, 0, 10)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.region_cells(k, 12, 3, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.region_assemble(torch.zeros((4, 2), dtype=torch.int32), [(0, 0, 1)], 4)
    with pytest.raises(ValueError):
        bitstream.decode_region_bytes(b"RAHTF001 but nothing else", 1, (0, 1))


def test_region_runs_and_segments_of_the_decoder_equal_the_model():
    import numpy as np
    from raht_3dgs_codec_amd import bitstream, synth
    from . import numpy_region as M
    keys = synth.sorted_unique_keys(3000, 6, 11)
    for depth in (1, 2, 5):
        for name, (c0, c1) in M.regions(keys, 6, depth).items():
            a, b = M.region_rows(keys, 6, depth, c0, c1)
            if a == b:
                continue
            n_top, runs = M.coded_runs(keys, 6, depth, a, b)
            n_roots = len(np.unique(keys[a:b] >> np.uint64(3 * (6 - depth))))
            assert bitstream.region_runs(M.layout(keys, a, b).tolist(), 6, depth, n_roots) == (n_top, runs), (depth, name)
            ids, compact = bitstream.region_segments(n_top, runs, 64)
            assert list(ids) == M.segments(n_top, runs, 64), (depth, name)
            rows = M.covered_rows(list(ids), 64, len(keys))
            assert all(rows[compact(r)] == r and rows[compact(r + n - 1)] == r + n - 1 for r, _, n in runs), (depth, name)
