"""The detection grid's sizes as the library states them (no GPU needed): per-cell list capacity for cell sizes 8 .. 64 and the
per-frame detection scratch, unchanged for the sizes accepted before wider cells and larger grids."""
import ctypes as C
import importlib

import pytest


@pytest.fixture(scope="module")
def sdvl():
    return importlib.import_module("slam-sdvl_amd")


def test_cell_kp_cap_bounds_the_survivors_of_the_suppression(sdvl):
    lib = sdvl.load_library()
    # a c x c ROI tests (c - 6)^2 pixels; no two 8-neighbours both survive the strict 3x3 suppression
    for c in range(8, 65):
        bound = ((c - 6 + 1) // 2) ** 2
        cap = lib.sdvl_cell_kp_cap(c)
        assert cap >= bound, c
        assert cap == (176 if c <= 32 else bound), c
    assert lib.sdvl_cell_kp_cap(7) == 0 and lib.sdvl_cell_kp_cap(65) == 0


def scratch(sdvl, w, h, cell):
    lib = sdvl.load_library()
    lib.sdvl_detect_scratch_bytes.restype = C.c_int64
    dp = sdvl.default_detect_params()
    dp.cell_size = cell
    return lib.sdvl_detect_scratch_bytes(w, h, C.byref(dp))


def test_detect_scratch_of_the_default_size_is_unchanged(sdvl):
    # counts | lengths | 300 + 80 + 20 lists of 176 entries | 3 spill areas of 2 x 4096 words, each part 256-byte aligned
    assert scratch(sdvl, 640, 480, 32) == 1792 + 1792 + 281600 + 98304


def test_detect_scratch_grows_with_wide_cells_and_large_grids(sdvl):
    assert scratch(sdvl, 3840, 2160, 64) > 2040 * 841 * 4
    assert scratch(sdvl, 3840, 2160, 32) > 8160 * 176 * 4 + 2 * 65280 * 4
    assert scratch(sdvl, 640, 480, 65) == -1


@pytest.mark.parametrize("w,h,cell,per_level,total,scratch_bytes", [
    (640, 480, 32, (300, 80, 20), 400, 383488),
    (752, 480, 32, (360, 96, 24), 480, 440320),
    (640, 480, 8, (4800, 1200, 300), 6300, 4902656),
    (640, 480, 16, (1200, 300, 80), 1580, 1267456),
    (640, 480, 33, (300, 80, 20), 400, 415488),
    (1920, 1080, 48, (920, 240, 60), 1220, 2286848),
    (1920, 1200, 32, (2280, 570, 150), 3000, 2351616),
    (2560, 1440, 32, (3600, 920, 240), 4760, 3711488),
    (3840, 2160, 32, (8160, 2040, 510), 10710, 8311552),
    (3840, 2160, 64, (2040, 510, 135), 2685, 9250048),
    (4000, 2400, 32, (9375, 2394, 608), 12377, 9529600),     # refused at launch (more than 8192 cells in a level): still counted
    (640, 480, 7, (6348, 1610, 414), 8372, -1),              # refused at launch (cell size): counted, no scratch size
])
def test_grid_sizes_are_pinned(sdvl, w, h, cell, per_level, total, scratch_bytes):
    """sdvl_fast_num_cells and sdvl_detect_scratch_bytes answer for shapes the launches refuse: Context.fast_cells asks for the counts
    before the call that raises the named refusal"""
    lib = sdvl.load_library()
    dp = sdvl.default_detect_params()
    dp.cell_size = cell
    assert dp.max_fast_levels == 3
    cpl, tot = (C.c_int * 4)(), C.c_int()
    assert lib.sdvl_fast_num_cells(w, h, C.byref(dp), cpl, C.byref(tot)) == 0
    assert tuple(cpl[:3]) == per_level and tot.value == total
    assert scratch(sdvl, w, h, cell) == scratch_bytes
