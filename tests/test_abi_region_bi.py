"""CPU-only checks of raht_region_needs_bi at the C-ABI boundary (include/raht.h, "The needed sets of a B frame"):
declared, exported and bound with the header's prototype, no new ABI version, and every argument rule refused with
RAHT_ERR_INVALID and the function's name before any HIP call -- the "device pointers" below are addresses that must never be read."""
import ctypes
import os

import pytest

from .test_abi_region_set import A, B, Cc, Dd, INVALID, _prototype, _refused

NAME = "raht_region_needs_bi"
E, F = 0x50000, 0x60000


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def test_the_symbol_is_exported_and_bound_as_the_header_declares_it(L):
    from raht_3dgs_codec_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "raht.h")).read()
    assert NAME in _lib.EXPORTS and hasattr(L, NAME)
    want = _prototype(header, NAME)
    # keys, N, J, top_level, up | block_first, n_blocks, block_log2 | mv0, mv1, mode | cells0, cells1, capacity, n_cells | stream
    assert len(want) == 16 and list(getattr(L, NAME).argtypes) == want
    assert want[14] == ctypes.POINTER(ctypes.c_int64) and want[7] == ctypes.c_int and want[13] == ctypes.c_int64
    assert L.raht_version() == 300                                       # no new ABI version


def test_argument_validation(L):
    n = (ctypes.c_int64 * 2)(-7, -9)

    def call(keys=A, N=1000, J=10, tl=12, up=0, bf=None, nb=0, m=0, mv0=None, mv1=None, mode=None, c0=B, c1=Cc, cap=100, count=n):
        return L.raht_region_needs_bi(keys, N, J, tl, up, bf, nb, m, mv0, mv1, mode, c0, c1, cap, count, None)

    cases = {"NULL keys": dict(keys=None), "NULL cells0": dict(c0=None), "NULL cells1": dict(c1=None), "NULL n_cells": dict(count=None),
             "N = 0": dict(N=0), "N < 0": dict(N=-1), "N = 2^31": dict(N=2 ** 31), "J = 0": dict(J=0), "J = 22": dict(J=22),
             "top_level no multiple of 3": dict(tl=13), "top_level = 0": dict(tl=0), "top_level = 3 J": dict(tl=30), "up = 4": dict(up=4),
             "up < 0": dict(up=-1), "capacity = 0": dict(cap=0), "capacity < 0": dict(cap=-1)}
    # a field or the modes, each alone and all together, without the blocks they lie over
    for what, given in {"mv0": dict(mv0=Dd), "mv1": dict(mv1=E), "modes": dict(mode=F), "all three": dict(mv0=Dd, mv1=E, mode=F)}.items():
        blocks = dict(given, bf=0x70000, nb=10, m=4)
        cases.update({f"{what} without block_first": dict(blocks, bf=None), f"{what} over no blocks": dict(blocks, nb=0),
                      f"{what} over more blocks than rows": dict(blocks, nb=1001), f"{what} with block_log2 = 0": dict(blocks, m=0),
                      f"{what} with block_log2 > J": dict(blocks, m=11)})
    for what, kw in cases.items():
        _refused(L, NAME, call(**kw), what)
    assert (n[0], n[1]) == (-7, -9)                                      # a refused call does not write the counts
    assert INVALID == -1


def test_the_python_wrapper_refuses_host_tensors_and_bad_shapes(monkeypatch):
    import torch
    from raht_3dgs_codec_amd import ops
    k = torch.arange(10, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.region_needs_bi(k, 4, 3, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.region_needs_bi(k, 4, 3, 0, torch.tensor([0, 10]), modes=torch.zeros(1, dtype=torch.uint8), block_log2=2)
    # shapes and dtypes are judged before any call: with the device check out of the way, host tensors show it
    monkeypatch.setattr(ops, "_need_cuda", lambda t, name: None)
    bf, mv, md = torch.tensor([0, 4, 10]), torch.zeros((2, 3), dtype=torch.int8), torch.zeros(2, dtype=torch.uint8)
    bad = {"keys of another dtype": dict(keys=k.float()), "keys that are no vector": dict(keys=k.reshape(2, 5)), "no keys": dict(keys=k[:0]),
           "a field without block_first": dict(block_first=None), "J = 22": dict(J=22), "block_log2 = 0": dict(block_log2=0),
           "block_log2 > J": dict(block_log2=5), "block_first of another dtype": dict(block_first=bf.int()),
           "block_first of one entry": dict(block_first=bf[:1]), "more blocks than rows": dict(block_first=torch.arange(12)),
           "mv0 of another dtype": dict(mv0=mv.short()), "mv0 of another block count": dict(mv0=mv[:1]), "mv1 of two columns": dict(mv1=mv[:, :2]),
           "modes of another dtype": dict(modes=md.char()), "modes of another block count": dict(modes=md[:1]),
           "modes as a matrix": dict(modes=md.reshape(2, 1)), "capacity = 0": dict(capacity=0)}
    for what, kw in bad.items():
        args = dict(keys=k, J=4, top_level=3, up=0, block_first=bf, mv0=mv, mv1=mv, modes=md, block_log2=2)
        args.update(kw)
        with pytest.raises(ValueError, match="region_needs_bi"):
            ops.region_needs_bi(**args)
            pytest.fail(what)
