"""k_resize2 on host-built records: a wave reads its strip (rows, column, first / last source row, rounds that load without a test) and each
destination row (second tap, flags, shifted weights) from tables written at orbx_create, walks its source rows with a running scalar pointer, and
takes one of two copies of the walk — one dword store per lane, or the last strip column's (lanes past the width switched off, bytes for the one
lane with fewer than four columns).  Every level of every frame must equal the oracle, on the smallest shapes that reach each of these paths.

check() of test_resize_stream.py does the comparison; parametrised over the emulated build and the product library."""
import ctypes
import re

import numpy as np
import pytest

from devarrays import BACKENDS, lib  # noqa: F401  (lib: the fixture of the tests parametrised over BACKENDS)
from test_resize_stream import MIN_LEVEL, R2_R, SRC, _height_for, check

R2_D = int(re.search(r"^#define R2_D (\d+)", SRC, re.M).group(1))   # the shipped prefetch depth


def _width_for(w1):
    """the image width whose level 1 at scale factor 1.2 is w1 columns wide: the same inverse as _height_for"""
    return _height_for(w1)


# Level-1 widths, height 84 (level 1: 70 rows).  256: one strip column, every lane four columns — the dword-store copy alone.  257 ... 260: a second
# strip column whose first lane holds 1, 2, 3 columns or one full dword (the copy with the byte stores; 260: that copy with no partial lane).
# 513: three strip columns, an interior one between the first and the last.
WIDTHS = [256, 257, 258, 259, 260, 513]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("w1", WIDTHS)
def test_level_widths_around_a_strip_column(lib, backend, w1):
    check(lib, backend, _width_for(w1), 84, 1.2, 2, seed=600 + w1, expect={1: (w1, 70)})


def _last_strip_source_rows(h1):
    """source rows [rlo, rhi] of the last strip of a level of h1 rows built from _height_for(h1) rows, as orbx_create tabulates them (resize_coef)"""
    sh = _height_for(h1)
    scale = 1. / (float(h1) / sh)
    ys = [int(np.floor(np.float32((y + 0.5) * scale - 0.5))) for y in range(h1)]
    clip = lambda r: min(max(r, 0), sh - 1)   # noqa: E731
    y0 = (h1 - 1) // R2_R * R2_R
    return clip(ys[h1 - 1] + 1) - clip(ys[y0]) + 1


def _height_with_last_strip_of(n):
    for h1 in range(MIN_LEVEL, MIN_LEVEL + 4 * R2_R):
        if _last_strip_source_rows(h1) == n:
            return h1
    raise AssertionError(n)


# Source rows of the last strip with the shipped constants: R2_D - 1 (fewer than the prologue asks for: its last row again), R2_D (the prologue alone,
# no round, no tail load), R2_D + 1 (one load in the rows behind the rounds), 2 * R2_D (one full round, then a tail without loads).
TAILS = [R2_D - 1, R2_D, R2_D + 1, 2 * R2_D]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("n", TAILS)
def test_source_rows_of_the_last_strip(lib, backend, n):
    h1 = _height_with_last_strip_of(n)
    check(lib, backend, 100, _height_for(h1), 1.2, 2, seed=700 + n, expect={1: (83, h1)})


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("frames", [2, 9])
def test_batches_with_padding_workgroups_and_the_reversed_walk(lib, backend, frames):
    check(lib, backend, 120, 100, 1.2, 3, n=frames, seed=800 + frames)


@pytest.mark.parametrize("backend", BACKENDS)
def test_the_tail_stays_inside_a_buffer_that_ends_with_its_last_row(lib, backend):
    """row_stride == W and nothing behind the last frame's last row; level 1's last strip asks for one row behind its rounds, the image's last one"""
    h1 = _height_with_last_strip_of(R2_D + 1)
    check(lib, backend, 100, _height_for(h1), 1.2, 2, seed=900, exact=True, expect={1: (83, h1)})


def test_emu_small_strips_shallow_prefetch_one_wave():
    """The emulated build with R2_R = 8, R2_D = 2 and one wave per workgroup: nine strip boundaries in 70 rows, rounds of two rows, both strip
    columns of a 257-wide level."""
    import build_emu
    from orbhip import _lib
    L = _lib.bind(ctypes.CDLL(build_emu.build(defines=("R2_R=8", "R2_D=2", "R2_WAVES=1"), tag="r2_r8_d2_w1")))
    check(L, "emu", _width_for(257), 84, 1.2, 2, seed=1000, expect={1: (257, 70)})
    check(L, "emu", 120, 100, 1.2, 3, n=3, seed=1010)
