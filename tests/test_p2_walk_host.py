"""CPU (no GPU): the persistent tile walk of the P2 conv kernels (csrc/conv_p2.h) visits every tile exactly once.

The launchers of conv_p2 / block / bneck / stem take their grid from ``mval_p2_walk_grid``; the kernels' side of the walk
(``p2_walk_begin``: XCD group, contiguous range per group, step) is restated here in Python.  A grid of 12 workgroups for 12
tiles -- what the fused kernels' launchers used to ask for -- walks its eight groups in steps of 12 // 8 = 1 and computes
four tiles twice; ``walk`` shows that for the old rule as a check of the restatement itself."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def grid():
    from multi_view_active_learning_amd import _lib, build

    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    f = _lib.lib().mval_p2_walk_grid
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int]
    return f


def walk(tiles_total, wgs_x):
    """Tiles each workgroup of one cout group computes, in the kernel's order (p2_walk_begin + the tile loop)."""
    visits = []
    X = 8 if wgs_x >= 8 else 1
    per = (tiles_total + X - 1) // X
    wgx = wgs_x // X
    for b in range(wgs_x):
        xg = b % X
        tile = xg * per + b // X
        tile_end = min(tiles_total, (xg + 1) * per)
        while tile < tile_end:
            visits.append(tile)
            tile += wgx
    return visits


def test_restated_walk_shows_the_old_rule_repeating_tiles():
    v = walk(12, 12)  # `if (wgs >= tiles_total) wgs = tiles_total;`
    assert sorted(set(v)) == list(range(12)) and len(v) == 16


@pytest.mark.parametrize("groups", [1, 2, 3])
@pytest.mark.parametrize("resident", [8, 256, 512, 1024])
def test_every_tile_once(grid, resident, groups):
    for tiles_total in range(1, 601):
        wgs = grid(tiles_total, resident, groups)
        assert wgs >= 1
        if wgs >= 8:
            assert wgs % 8 == 0, (tiles_total, wgs)
        assert wgs <= max(8, (tiles_total + 7) // 8 * 8, resident), (tiles_total, wgs)
        assert sorted(walk(tiles_total, wgs)) == list(range(tiles_total)), (tiles_total, wgs)
