"""CPU-only checks of the entry points of a region made of several ranges at the C-ABI boundary (include/raht.h, "A SET of row
ranges"): exported, bound with the header's prototypes, and every argument rule refused with RAHT_ERR_INVALID and the function's
name before any HIP call -- the "device pointers" below are addresses that must never be read."""
import ctypes
import os
import re

import pytest

INVALID = -1
NAMES = {"raht_region_layout_set": 7, "raht_region_assemble_set": 11, "raht_region_needs": 13}
A, B, Cc, Dd = 0x10000, 0x20000, 0x30000, 0x40000            # never dereferenced
CTYPE = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "raht_stream_t": ctypes.c_void_p}


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


def _prototype(header, name):
    """the argument types of a prototype of the header as ctypes: any pointer but a HOST int64 one is a void pointer"""
    args = re.search(r"\bint " + name + r"\(([^;]*)\);", header).group(1)
    out = []
    for arg in (a.strip() for a in args.replace("\n", " ").split(",")):
        kind, arg_name = arg.rsplit(" ", 1)
        if "*" in arg:
            out.append(ctypes.POINTER(ctypes.c_int64) if arg_name.lstrip("*") in ("runs_host", "n_cells") else ctypes.c_void_p)
        else:
            out.append(CTYPE[kind.replace("const ", "").strip()])
    return out


def test_the_three_symbols_are_exported_and_bound_as_the_header_declares_them(L):
    from raht_3dgs_codec_amd import _lib, ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "raht.h")).read()
    for name, arity in NAMES.items():
        assert name in _lib.EXPORTS, name
        assert hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == arity, name
        assert list(getattr(L, name).argtypes) == _prototype(header, name), name
    assert "#define RAHT_REGION_MAX_RANGES 512" in header and ops.REGION_MAX_RANGES == 512


def test_layout_set_argument_validation(L):
    def call(keys=A, N=1000, nbits=30, bounds=B, R=3, table=Cc):
        return L.raht_region_layout_set(keys, N, nbits, bounds, R, table, None)

    for what, kw in {"NULL keys": dict(keys=None), "NULL bounds": dict(bounds=None), "NULL table": dict(table=None), "N = 0": dict(N=0),
                     "N = 2^31": dict(N=2 ** 31), "nbits = 0": dict(nbits=0), "nbits = 64": dict(nbits=64), "R = 0": dict(R=0), "R < 0": dict(R=-1),
                     "R = 513": dict(R=513)}.items():
        _refused(L, "raht_region_layout_set", call(**kw), what)


def test_assemble_set_argument_validation(L):
    def call(src=A, ld_src=8, n_src=100, dst=B, ld_dst=8, n_dst=50, D=8, runs=Cc, host=((0, 5, 10), (40, 15, 35)), n_runs=None):
        flat = [x for r in host or () for x in r]
        arr = None if host is None else (ctypes.c_int64 * max(len(flat), 1))(*flat)
        return L.raht_region_assemble_set(src, ld_src, n_src, dst, ld_dst, n_dst, D, runs, arr, len(flat) // 3 if n_runs is None else n_runs, None)

    cases = {"NULL src": dict(src=None), "NULL dst": dict(dst=None), "runs without a device table": dict(runs=None), "D = 0": dict(D=0),
             "ld_src < D": dict(ld_src=7), "ld_dst < D": dict(ld_dst=7), "no source rows": dict(n_src=0), "no destination rows": dict(n_dst=0),
             "n_runs < 0": dict(n_runs=-1), "more than 22 * 512 runs": dict(host=None, n_runs=22 * 512 + 1),
             "a run past the end of src": dict(host=((91, 0, 10),)), "a run before src": dict(host=((-1, 0, 10),)),
             "a run past the end of dst": dict(host=((0, 41, 10),)), "a run before dst": dict(host=((0, -1, 10),)),
             "a negative count": dict(host=((0, 0, -1),)), "runs that overlap in dst": dict(host=((0, 5, 10), (40, 14, 5))),
             "destinations not ascending": dict(host=((40, 15, 35), (0, 5, 10)))}
    for what, kw in cases.items():
        _refused(L, "raht_region_assemble_set", call(**kw), what)


def test_needs_argument_validation(L):
    n = ctypes.c_int64(-7)

    def call(keys=A, N=1000, J=10, tl=12, up=0, bf=None, nb=0, mv=None, m=0, cells=B, cap=100, count=ctypes.byref(n)):
        return L.raht_region_needs(keys, N, J, tl, up, bf, nb, mv, m, cells, cap, count, None)

    field = dict(bf=Cc, nb=10, mv=Dd, m=4)
    cases = {"NULL keys": dict(keys=None), "NULL cells": dict(cells=None), "NULL count": dict(count=None), "N = 0": dict(N=0), "N = 2^31": dict(N=2 ** 31),
             "J = 0": dict(J=0), "J = 22": dict(J=22), "top_level no multiple of 3": dict(tl=13), "top_level = 0": dict(tl=0),
             "top_level = 3 J": dict(tl=30), "up = 4": dict(up=4), "up < 0": dict(up=-1), "capacity = 0": dict(cap=0),
             "a field without block_first": dict(field, bf=None), "a field of no blocks": dict(field, nb=0),
             "more blocks than rows": dict(field, nb=1001), "block_log2 = 0": dict(field, m=0), "block_log2 > J": dict(field, m=11)}
    for what, kw in cases.items():
        _refused(L, "raht_region_needs", call(**kw), what)
    assert n.value == -7                                                 # a refused call does not write the count


def test_python_wrappers_refuse_host_tensors_and_bad_shapes():
    import torch
    from raht_3dgs_codec_amd import ops
    k = torch.arange(10, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.region_layout_set(k, 12, torch.tensor([0, 5]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.region_assemble_set(torch.zeros((4, 2), dtype=torch.int32), [(0, 0, 1)], 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.region_needs(k, 4, 3, 0)
