"""Shapes at which csrc/bilateral_grid.hip changes its code path, with the plan lfs_bilateral_slice_plan must report for each, shared by the CPU test of
the plan (tests/test_capi_symbols.py) and the GPU parity cases (tests/test_gpu_bilateral.py). The expected plans are literals worked out outside the library from the
host rule (window_floats / span, LDS_FLOATS = 6144, 64 KB of LDS, 16 * NT_MAX = 64 columns): a threshold change in the library moves a case to another kernel
only by failing here. The numpy helpers restate the DEVICE side (float32 grid_coord, tile_window) so a test can prove which column-tile counts and how many
accumulator flushes a shape really reaches."""
from collections import namedtuple

import numpy as np

Plan = namedtuple("Plan", "fwd_lds fwd_floats bwd_window bwd_lds_bytes col_tiles")
TILE_W, TILE_H, BWD_ROWS, BWD_TILE_H = 64, 4, 8, 32

# (L, H, W, h, w) -> plan, and for the windowed backward: the set of column-tile counts nt and of column counts nx * L over the 64-pixel strips
LimitCase = namedtuple("LimitCase", "dims plan nt cols pins")
LIMIT_CASES = [
    LimitCase((8, 16, 16, 120, 200), Plan(1, 2016, 1, 52736, 4), {1, 3, 4}, {16, 48, 56}, "3 and 4 column tiles; ncols not a multiple of 16"),
    LimitCase((8, 8, 8, 64, 20), Plan(1, 2304, 1, 57344, 4), {4}, {64}, "whole grid in the window; span * L == 64, the column limit exactly"),
    LimitCase((5, 16, 16, 40, 300), Plan(1, 1440, 1, 60800, 2), {2}, {20, 25}, "L not a power of two; partly filled last tile"),
    LimitCase((3, 12, 20, 33, 257), Plan(1, 1008, 1, 44672, 2), {1, 2}, {3, 18, 21}, "H != W; last strip one pixel wide"),
    LimitCase((2, 16, 16, 33, 130), Plan(1, 960, 1, 51200, 2), {1, 2}, {4, 18}, "up to 5 y0 per 8 rows: repeated flushes"),
    LimitCase((2, 16, 16, 8, 80), Plan(1, 3024, 1, 63488, 2), {1, 2}, {8, 26}, "top of the LDS budget (63 488 B); y0 changes on every row"),
    LimitCase((2, 16, 16, 8, 20), Plan(1, 3456, 0, 69632, 2), None, None, "backward LDS just over 64 KB (69 632 B): generic"),
    LimitCase((16, 8, 8, 16, 20), Plan(1, 6144, 0, 118784, 8), None, None, "forward window == LDS_FLOATS exactly: still LDS"),
    LimitCase((4, 16, 16, 8, 20), Plan(0, 6912, 0, 118784, 4), None, None, "forward window just over LDS_FLOATS: generic"),
    # grid extents of 1: every one takes the LDS forward and the windowed backward with one column tile
    LimitCase((3, 1, 5, 4, 70), Plan(1, 180, 1, 21920, 1), {1}, {6, 15}, "H == 1"),
    LimitCase((3, 5, 1, 70, 4), Plan(1, 108, 1, 21632, 1), {1}, {3}, "W == 1"),
    LimitCase((1, 1, 1, 2, 2), Plan(1, 12, 1, 20576, 1), {1}, {1}, "L == H == W == 1 against the smallest image"),
]
# most distinct y0 inside one wavefront's 8 rows (each change flushes the register accumulators)
FLUSHES = {(2, 16, 16, 33, 130): 5, (2, 16, 16, 8, 80): 8}

# the plans of tests/test_gpu_bilateral.py's CASES, in its order
CASES_PLANS = [((8, 16, 16, 270, 480), Plan(1, 1152, 1, 32768, 2)), ((8, 16, 16, 67, 131), Plan(1, 2880, 0, 97280, 5)), ((4, 40, 90, 24, 100), Plan(0, 22656, 0, 926720, 15)),
               ((1, 3, 2, 9, 70), Plan(1, 72, 1, 21056, 1)), ((8, 16, 16, 2, 2), Plan(0, 24576, 0, 217088, 8))]
# the two shapes of the out-of-range colour cases (one windowed, one generic backward)
UNCLAMPED = [(8, 16, 16, 120, 200), (8, 16, 16, 67, 131)]


def grid_coord(i, n, G):
    """grid_coord of the kernels, in float32 as there"""
    return np.asarray(i, np.float32) / np.float32(n - 1) * np.float32(G - 1)


def _extent(first, last, n, G):
    a = np.floor(grid_coord(first, n, G)).astype(np.int64)
    b = np.minimum(np.floor(grid_coord(last, n, G)).astype(np.int64) + 1, G - 1)
    return b - a + 1


def strip_columns(L, W, w):
    """nx * L of tile_window for every 64-pixel strip of an image w pixels wide"""
    px0 = np.arange(0, w, TILE_W)
    return (_extent(px0, np.minimum(px0 + TILE_W, w) - 1, w, W) * L).tolist()


def column_tiles(L, W, w):
    """nt = ceil(nx * L / 16) of slice_bwd_window_kernel for every strip"""
    return [(c + 15) // 16 for c in strip_columns(L, W, w)]


def max_window_cells(L, H, W, h, w, rows):
    """the largest nx * ny * L any tile of 64 x rows pixels stages"""
    px0, py0 = np.arange(0, w, TILE_W), np.arange(0, h, rows)
    nx = _extent(px0, np.minimum(px0 + TILE_W, w) - 1, w, W)
    ny = _extent(py0, np.minimum(py0 + rows, h) - 1, h, H)
    return int(nx.max() * ny.max() * L)


def max_y0_per_wave(H, h):
    y0 = np.floor(grid_coord(np.arange(h), h, H)).astype(np.int64)
    return max(len(set(y0[r:r + BWD_ROWS].tolist())) for r in range(0, h, BWD_ROWS))
