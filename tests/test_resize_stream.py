"""k_resize2, the register-streaming pyramid kernel of the batch entry point: every level of every frame bit-identical to the oracle, on the
smallest shapes at which each of its paths can go wrong.  A wave owns a strip of 256 destination columns x R2_R destination rows; a lane owns four
columns, streams the strip's source rows through registers R2_D rows ahead and emits a destination row when its second tap has passed.

Every case calls orbx_extract_batch_dev with two frames or more (one frame takes k_pyramid_chain and would not run this kernel): a seeded
synth_image next to uniform noise, where every tap of every pixel matters.  Parametrised over the emulated build and the product library."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from devarrays import BACKENDS, lib  # noqa: F401  (lib: the fixture of the tests parametrised over BACKENDS)
from orbhip.synth import synth_image
from test_extractor_batch_plans import Handle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = open(os.path.join(ROOT, "awesome-orb-slam3-3dvisioncraft-version_amd", "csrc", "orbx_extractor.hip")).read()
R2_R = int(re.search(r"^#define R2_R (\d+)", SRC, re.M).group(1))   # the shipped strip height
MIN_LEVEL = 62   # orbx_create refuses a level without one 30-px FAST cell inside the 16-px borders


def frames_for(W, H, n, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        out.append(synth_image(seed + i, W, H, n_rect=20, n_disc=10) if i % 2 == 0 else rng.integers(0, 256, (H, W), dtype=np.uint8))
    return out


def check(L, backend, W, H, sf, nl, n=2, seed=300, exact=False, expect=None):
    """n frames of W x H through the batch entry point -> every level of every frame == the oracle's level_image.  exact: the caller's buffer is
    n * H * W bytes, row_stride == W, nothing behind the last row.  expect: {level: (w, h)} the case relies on."""
    cfg = (200, sf, nl, 20, 7)
    frames = frames_for(W, H, n, seed)
    hd = Handle(L, backend, cfg, W, H, n)
    img = (hd.dev.upload(np.stack(frames)), 0, W * H, W) if exact else hd.images(frames, row_stride=(W + 3) & ~3)
    hd.call(img, n, (0, 0))
    o = O.OrbOracle(*cfg)
    for b in range(n):
        o.extract(frames[b])
        for l in range(nl):
            ref = o.level_image(l)
            if expect and l in expect:
                assert ref.shape == (expect[l][1], expect[l][0]), (l, ref.shape, expect[l])
            got = hd.e.pyramid_level(l, b)
            assert got.shape == ref.shape and np.array_equal(got, ref), \
                "%dx%d scale %.2f: level %d of frame %d differs in %d pixels" % (W, H, sf, l, b, int((got != ref).sum()) if got.shape == ref.shape else -1)
            if l >= 1:   # the case runs k_resize2, not k_resize: both axes scale by <= 1.3
                up = o.level_image(l - 1).shape
                assert 1. / (ref.shape[1] / up[1]) <= 1.3 and 1. / (ref.shape[0] / up[0]) <= 1.3, (l, up, ref.shape)


SHAPES = {
    # level 1 is 257 wide: the second strip column has one active lane and the row a bytewise tail; level 2 is 214 wide
    "308x90_l1_257_wide": dict(W=308, H=90, sf=1.2, nl=3, expect={1: (257, 75), 2: (214, 62)}),
    # level 1 is 320 = 5 x 64 wide, its plane has no padding: the right-edge window of the level-2 build clamps
    "384x100_l1_stride_eq_width": dict(W=384, H=100, sf=1.2, nl=3, expect={1: (320, 83)}),
    # the same clamp on level 0: row_stride == W = 320, the batch buffer ends with the last row
    "320x96_exact_buffer": dict(W=320, H=96, sf=1.2, nl=3, exact=True),
    # level 1 is 83 wide: fewer than 21 active lanes in the wave
    "100x84_l1_83_wide": dict(W=100, H=84, sf=1.2, nl=2, expect={1: (83, 70)}),
    # nine frames: padding workgroups of the frame-per-XCD grid, and the reversed frame walk of level 2
    "nine_frames": dict(W=120, H=100, sf=1.2, nl=3, n=9),
    # the largest scale factor the kernel serves (200 / 154 and 122 / 94 are below 1.3; a lane's four columns span five source columns)
    "scale_1.3": dict(W=200, H=122, sf=1.3, nl=2, expect={1: (154, 94)}),
    # nearly every source row emits a destination row
    "scale_1.01": dict(W=100, H=84, sf=1.01, nl=2, expect={1: (99, 83)}),
}


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_streamed_levels_equal_the_oracle(lib, backend, shape):
    check(lib, backend, **SHAPES[shape])


def _height_for(h1):
    """the image height whose level 1 at scale factor 1.2 is h1 rows high (orbx_create: cvRound(H * (1 / 1.2f)))"""
    inv = np.float32(1.0) / np.float32(np.float32(1.0) * 1.2)
    for H in range(h1, 2 * h1 + 4):
        if int(np.rint(np.float32(H) * inv)) == h1:
            return H
    raise AssertionError(h1)


# level-1 heights k * R2_R - 1, k * R2_R, k * R2_R + 1 with the shipped R2_R: a last strip of R2_R - 1 rows, none, and one of a single row — for the two
# smallest k the library accepts.  It refuses a level below 62 rows, so k = 1 and 2 exist only for R2_R >= 63 and 32; with the shipped 16 rows the
# first strip boundaries that can occur are k = 4 and 5 (63 ... 65 and 79 ... 81 rows).
_KS = [k for k in range(1, 70) if k * R2_R - 1 >= MIN_LEVEL][:2]
STRIP_HEIGHTS = [k * R2_R + d for k in _KS for d in (-1, 0, 1)]


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("h1", STRIP_HEIGHTS)
def test_level_heights_around_a_strip_boundary(lib, backend, h1):
    H = _height_for(h1)
    check(lib, backend, 100, H, 1.2, 2, seed=400 + h1, expect={1: (83, h1)})


def test_emu_small_strips_and_prefetch_depth():
    """The emulated build with R2_R = 8 and R2_D = 4: in an 81-row level ten strip boundaries, a last strip of one destination row whose two source
    rows are fewer than the prefetch depth, rounds of R2_D rows followed by one to three left-over rows; with one wave per workgroup too."""
    import build_emu
    from orbhip import _lib
    for defines, tag in ((("R2_R=8", "R2_D=4"), "r2_r8_d4"), (("R2_R=8", "R2_D=2", "R2_WAVES=1"), "r2_r8_d2_w1")):
        L = _lib.bind(ctypes.CDLL(build_emu.build(defines=defines, tag=tag)))
        check(L, "emu", 100, _height_for(81), 1.2, 2, seed=500, expect={1: (83, 81)})
        check(L, "emu", 308, 90, 1.2, 3, seed=510, expect={1: (257, 75), 2: (214, 62)})
