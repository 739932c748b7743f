"""CPU-only check of raht_debug_motion_tile (include/raht.h): the rows of the tile raht_motion_search stages in LDS for rows of D
floats, at both sides of every switch -- 256 | 192 at D = 59 | 60, 192 | 128 at 79 | 80, 128 | 64 at 121 | 122, 64 | unstaged at
243 | 244 -- and never growing with D. The GPU tests of the search's forms (tests/test_gpu_motion_paths.py) rest on these values."""
import os

import pytest

WANT = {1: 256, 59: 256, 60: 192, 79: 192, 80: 128, 121: 128, 122: 64, 243: 64, 244: 0, 5000: 0}


@pytest.fixture(scope="module")
def L():
    import raht_3dgs_codec_amd as R
    from raht_3dgs_codec_amd import _lib
    if not os.path.exists(R.SO_PATH):
        R.build()
    return _lib.lib()


def test_the_symbol_is_exported_and_bound(L):
    from raht_3dgs_codec_amd import _lib
    assert "raht_debug_motion_tile" in _lib.EXPORTS and hasattr(L, "raht_debug_motion_tile")
    assert len(L.raht_debug_motion_tile.argtypes) == 1


@pytest.mark.parametrize("D", sorted(WANT))
def test_the_tile_at_both_sides_of_every_switch(L, D):
    assert L.raht_debug_motion_tile(D) == WANT[D]


def test_the_tile_never_grows_with_D(L):
    tiles = [L.raht_debug_motion_tile(D) for D in range(1, 301)]
    assert all(a >= b for a, b in zip(tiles, tiles[1:]))
    assert sorted(set(tiles)) == [0, 64, 128, 192, 256]                  # every form occurs below D = 300
    assert L.raht_debug_motion_tile(0) == 0 and L.raht_debug_motion_tile(-3) == 0      # no D at all: nothing to stage
