"""The launch plans of orbx_extract_batch_dev on the shipped constants: every case bit-exact against the oracle's single-frame result.

The batch entry point picks its chain of launches from the batch size, the frames' content and what the handle's earlier calls left behind:
frame order (k_frame_order / the bookkeeping workgroup of k_resize2<true>), one- or two-cell-row tiles of k_fast (FAST_TALL_MIN_BATCH = 8), one
FAST pass or two (FAST_TWO_PASS_MIN_BATCH = 64 and the listed-share policy), the octree's LDS key cache or its global-key path (OCT_KEYCAP = 4096,
OCT_CACHE_MAX_BATCH = 48) and the second, 1 024-thread k_octree launch for problems of OCT_HEAVY_MIN = 8 192 candidates.  tests/test_extractor_parity.py
forces these paths on the emulator in builds with other constants; the cases here reach them with the default build, through the C ABI where the
Python wrapper cannot express the arguments (strides, a base that is only 4-byte aligned, a short cap_per_frame, batch < max_batch).

Where a case depends on a path being taken it asserts the precondition from the oracle's candidate counts and from what the product reports
(orbx_last_schedule, orbx_last_fast_passes), never from the result.  Cases 4 and 5 depend on no default constant and also run on the emulator."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fuzz_parity as F  # noqa: E402
import oracle_lib as O  # noqa: E402
import orbhip  # noqa: E402
from devarrays import BACKENDS, lib  # noqa: E402,F401  (lib: the fixture of the tests parametrised over BACKENDS)
from orbhip import _lib  # noqa: E402
from orbhip.synth import flat_image, low_contrast_image, synth_image  # noqa: E402

KP = O.KP_DTYPE
CANARY = 0xA7
TAIL = 256   # canary bytes behind every output allocation


# ---- the oracle, once per distinct (configuration, lapping window, frame) ------------------------------------------------------------------
_ORACLES = {}
_REFS = {}
_LEVELS = {}


def _oracle(cfg):
    if cfg not in _ORACLES:
        _ORACLES[cfg] = O.OrbOracle(*cfg)
    return _ORACLES[cfg]


def _key(cfg, lap, frame):
    return cfg, tuple(lap), frame.shape, hashlib.sha1(np.ascontiguousarray(frame).tobytes()).digest()


def ref(cfg, frame, lap):
    """(monoIndex, key points, descriptors) of the oracle's single-frame run; cfg = (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)"""
    k = _key(cfg, lap, frame)
    if k not in _REFS:
        _REFS[k] = _oracle(cfg).extract(frame, *lap)
    return _REFS[k]


def ref_levels(cfg, frame, lap):
    """per level: (FAST candidates as a set of (x, y, score), the octree's selection in list order as int32 [n, 3])"""
    k = _key(cfg, lap, frame)
    if k not in _LEVELS:
        o = _oracle(cfg)
        o.extract(frame, *lap)
        out = []
        for l in range(cfg[2]):
            ka, _ = o.level_keypoints(l)
            sel = np.stack([ka["x"] - 16, ka["y"] - 16, ka["response"]], 1).astype(np.int32) if len(ka) else np.zeros((0, 3), np.int32)
            out.append((set(map(tuple, o.level_candidates(l).tolist())), sel))
        _LEVELS[k] = out
    return _LEVELS[k]


# ---- device memory of the backend under test: numpy for the emulated build (its device memory is host memory), torch for the product ---------
class Dev:
    def __init__(self, backend):
        self.hip = backend == "hip"
        if self.hip:
            import torch
            self.torch = torch

    def full(self, nbytes, value):
        if self.hip:
            return self.torch.full((nbytes,), value, dtype=self.torch.uint8, device="cuda")
        return np.full(nbytes, value, np.uint8)

    def upload(self, a):
        a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        return self.torch.from_numpy(a.copy()).cuda() if self.hip else a.copy()

    def addr(self, buf, off=0):
        return C.c_void_p((buf.data_ptr() if self.hip else buf.ctypes.data) + off)

    def host(self, buf):
        return buf.cpu().numpy() if self.hip else buf.copy()

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream) if self.hip else None

    def sync(self):
        if self.hip:
            self.torch.cuda.current_stream().synchronize()


class Handle:
    """One extractor handle and its calls through the C ABI.  Every output allocation is filled with CANARY first and ends in TAIL canary bytes."""

    def __init__(self, L, backend, cfg, W, H, max_batch):
        self.L, self.dev, self.cfg, self.W, self.H, self.max_batch = L, Dev(backend), cfg, W, H, max_batch
        self.e = orbhip.ORBextractor(*cfg, lib=L, max_batch=max_batch)
        self.h = self.e._handle(W, H, max_batch=max_batch)
        self.max_kp = L.orbx_max_keypoints(self.h)

    def images(self, frames, row_stride=None, gap=0, lead=0, fill=0, rng=None):
        """the frames in one allocation: base `lead` bytes in, rows `row_stride` apart, frames row_stride * H + gap apart; the padding holds `fill`
        (a byte value, or None: random bytes of `rng`) -> (buffer, lead, frame_stride, row_stride)"""
        B, H, W = len(frames), self.H, self.W
        rs = row_stride or W
        fs = rs * H + gap
        if fill is None:
            host = rng.integers(0, 256, lead + B * fs + 64, dtype=np.uint8)
        else:
            host = np.full(lead + B * fs + 64, fill, np.uint8)
        for b in range(B):
            rows = host[lead + b * fs: lead + b * fs + rs * H].reshape(H, rs)
            rows[:, :W] = frames[b]
        return self.dev.upload(host), lead, fs, rs

    def call_raw(self, img, B, lap, cap, slabs=None, lead_shift=0):
        """orbx_extract_batch_dev on outputs of `slabs` (default B) slabs of `cap` entries -> (rc, kps [slabs, cap], desc [slabs, cap, 32],
        counts [slabs, 2], tails: the bytes behind the three allocations)"""
        buf, lead, fs, rs = img
        slabs = slabs or B
        n = max(cap, 1)
        sizes = (slabs * n * KP.itemsize, slabs * n * 32, slabs * 8)
        out = [self.dev.full(s + TAIL, CANARY) for s in sizes]
        rc = self.L.orbx_extract_batch_dev(self.h, self.dev.addr(buf, lead + lead_shift), B, fs, rs, int(lap[0]), int(lap[1]), self.dev.addr(out[0]),
                                           self.dev.addr(out[1]), cap, self.dev.addr(out[2]), self.dev.stream())
        self.dev.sync()
        host = [self.dev.host(o) for o in out]
        tails = [hh[s:] for hh, s in zip(host, sizes)]
        return (rc, host[0][:sizes[0]].view(KP).reshape(slabs, n), host[1][:sizes[1]].reshape(slabs, n, 32),
                host[2][:sizes[2]].view(np.int32).reshape(slabs, 2), tails)

    def call(self, img, B, lap, cap=None, slabs=None):
        rc, kps, desc, cnt, tails = self.call_raw(img, B, lap, cap or self.max_kp, slabs)
        assert rc == 0, (rc, self.L.orbx_last_error(self.h))
        for t in tails:
            assert (t == CANARY).all(), "bytes behind an output allocation were written"
        return kps, desc, cnt

    def schedule(self):
        a, b = C.c_int(-1), C.c_int(-1)
        assert self.L.orbx_last_schedule(self.h, C.byref(a), C.byref(b)) == 0
        return a.value, b.value

    def fast_passes(self):
        return self.e.last_fast_passes()


def assert_frame(out, b, r, what, cap=None):
    """frame b of a call's outputs against the oracle's (monoIndex, key points, descriptors); cap: the slab's size if it is below the need"""
    kps, desc, cnt = out
    mono, k, d = r
    n = int(cnt[b, 0])
    assert n == len(k) and int(cnt[b, 1]) == mono, (what, b, "n %d oracle %d, monoIndex %d oracle %d" % (n, len(k), cnt[b, 1], mono))
    m = n if cap is None else min(n, cap)
    assert np.array_equal(kps[b, :m].view(np.uint8), k[:m].view(np.uint8)), (what, b, "key points (bitwise)")
    assert np.array_equal(desc[b, :m], d[:m]), (what, b, "descriptors")


def assert_same(o1, o2, what):
    """two calls on the same frames: bitwise equal outputs"""
    assert np.array_equal(o1[2], o2[2]), (what, "counts")
    for b in range(len(o1[2])):
        n = int(o1[2][b, 0])
        assert np.array_equal(o1[0][b, :n].view(np.uint8), o2[0][b, :n].view(np.uint8)) and np.array_equal(o1[1][b, :n], o2[1][b, :n]), (what, b)


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
W0, H0 = 400, 300
# Uniform noise at 400x300 under thresholds 5/3: the oracle finds 10 555 candidates on level 0 (>= OCT_HEAVY_MIN: the heavy launch's problem)
# and 6 673 on level 1 (above OCT_KEYCAP, below OCT_HEAVY_MIN: the global-key path on OCT_T_BATCH threads), 4 180 on level 2 (just above the
# cache's 4 096) and 2 608 on level 3, which fits the LDS cache.
# The tests assert these counts from the oracle before they rely on them.
CFG_MIX = (400, 1.2, 4, 5, 3)
LAP_MIX = (120, 260)
_FRAMES = {}


def mix_frames():
    """noise, flat, textured, sparse, a second noise frame, low contrast: very different weights (10 555 ... 0 candidates on level 0)"""
    if not _FRAMES:
        _FRAMES["noise"] = np.random.default_rng(77).integers(0, 256, (H0, W0), dtype=np.uint8)
        _FRAMES["flat"] = flat_image(W0, H0, 90)
        _FRAMES["textured"] = synth_image(61, W0, H0, n_rect=60, n_disc=30)
        _FRAMES["sparse"] = synth_image(62, W0, H0, n_rect=6, n_disc=3)
        _FRAMES["noise2"] = np.random.default_rng(78).integers(0, 256, (H0, W0), dtype=np.uint8)
        _FRAMES["lowc"] = low_contrast_image(63, W0, H0)
    return _FRAMES


def assert_noise_frame_is_heavy_and_global(cfg, frame, lap):
    lv = ref_levels(cfg, frame, lap)
    n0, n1 = len(lv[0][0]), len(lv[1][0])
    assert n0 >= 8192, "precondition: the noise frame's level 0 is a heavy octree problem (oracle: %d candidates)" % n0
    assert 4096 < n1 < 8192, "precondition: its level 1 takes the global-key path without being heavy (oracle: %d candidates)" % n1
    assert 0 < len(lv[cfg[2] - 1][0]) <= 4096, "precondition: the top level fits the LDS key cache"
    return n0, n1


# ---- case 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mixed_weight_batch_takes_the_heavy_octree_launch(hip_lib):
    """Four frames of very different weight (noise, flat, textured, sparse; 400x300, 4 levels, thresholds 5/3, lapping window 120..260), three
    calls on one handle: identity order on cleared counters, then ordered, then ordered with the 1 024-thread launch for the noise frame's
    level 0 (10 555 candidates) while its level 1 (6 673) reads its keys from global memory on 256 threads and the rest use the LDS cache.  Every
    frame of every call equals the oracle, the stage taps of the heavy call too; a different batch afterwards (stale order and counts) and
    the first one again do as well."""
    fr = mix_frames()
    frames = [fr["noise"], fr["flat"], fr["textured"], fr["sparse"]]
    n0, n1 = assert_noise_frame_is_heavy_and_global(CFG_MIX, frames[0], LAP_MIX)
    hd = Handle(hip_lib, "hip", CFG_MIX, W0, H0, 4)
    img = hd.images(frames)
    plans = []
    for call in range(3):
        out = hd.call(img, 4, LAP_MIX)
        plans.append(hd.schedule())
        for b in range(4):
            assert_frame(out, b, ref(CFG_MIX, frames[b], LAP_MIX), "call %d" % call)
    assert plans[0] == (1, 0) and plans[1][0] == 1, plans
    print("case 1: (frames_ordered, heavy_octree_pass) of the three calls: %s; the noise frame has %d / %d candidates on levels 0 / 1" % (plans, n0, n1))
    assert plans[2] == (1, 1), "the third call reports (frames_ordered, heavy_octree_pass) = %s, expected (1, 1); plans %s" % (plans[2], plans)
    lv = ref_levels(CFG_MIX, frames[0], LAP_MIX)
    for l in (0, 1):
        cand = hd.e.debug_candidates(l, frame=0)
        assert len(cand) == len(lv[l][0]) and set(map(tuple, cand.tolist())) == lv[l][0], "FAST candidates of the noise frame, level %d" % l
        assert np.array_equal(hd.e.debug_selected(l, frame=0), lv[l][1]), "octree selection of the noise frame, level %d (%d candidates)" % (l, (n0, n1)[l])
    rev = frames[::-1][:3]
    out = hd.call(hd.images(rev), 3, LAP_MIX)
    assert hd.schedule()[0] == 1
    for b in range(3):
        assert_frame(out, b, ref(CFG_MIX, rev[b], LAP_MIX), "three frames reversed")
    out = hd.call(img, 4, LAP_MIX)
    for b in range(4):
        assert_frame(out, b, ref(CFG_MIX, frames[b], LAP_MIX), "the first batch again")


# ---- case 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [2, 7, 8, 48, 49, 64])
def test_batch_size_classes_on_mixed_content(hip_lib, B):
    """The six frames of mix_frames(), permuted and cycled, at the batch sizes around every threshold of the plan: 2 (smallest ordered batch),
    7 / 8 (one- / two-cell-row tiles of k_fast), 48 / 49 (with / without the octree's LDS key cache), 64 (two FAST passes).  Three calls: the
    first on cleared counters, the second ordered by weight, the third also with the heavy launch (which at 48 frames runs next to cached
    problems).  All three are bitwise equal; against the oracle every frame for B <= 8, else the first, the last and every noise or flat frame."""
    fr = mix_frames()
    for n in ("noise", "noise2"):
        assert_noise_frame_is_heavy_and_global(CFG_MIX, fr[n], LAP_MIX)
    names = ["textured", "noise", "sparse", "flat", "lowc", "noise2"]
    pick = [names[(5 * i + i // 6) % 6] for i in range(B)]   # every frame kind at changing positions; B = 2: textured, noise2
    frames = [fr[n] for n in pick]
    hd = Handle(hip_lib, "hip", CFG_MIX, W0, H0, B)
    img = hd.images(frames)
    outs, plans, passes = [], [], []
    for call in range(3):
        outs.append(hd.call(img, B, LAP_MIX))
        plans.append(hd.schedule())
        passes.append(hd.fast_passes())
    print("case 2, B = %d: (frames_ordered, heavy_octree_pass) %s, two_pass %s" % (B, plans, [p["two_pass"] for p in passes]))
    assert plans[0] == (1, 0) and plans[1][0] == 1 and plans[2] == (1, 1), "(frames_ordered, heavy_octree_pass) of the three calls: %s" % plans
    if B == 64:
        assert passes[0]["two_pass"] == 1, passes
    else:
        assert all(p["two_pass"] == 0 for p in passes), passes
    assert_same(outs[0], outs[1], "second call")
    assert_same(outs[0], outs[2], "third call")
    check = range(B) if B <= 8 else [b for b in range(B) if b in (0, B - 1) or pick[b] in ("noise", "noise2", "flat")]
    for b in check:
        assert_frame(outs[0], b, ref(CFG_MIX, frames[b], LAP_MIX), "B = %d (%s)" % (B, pick[b]))


# ---- case 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("th", [(20, 7), (40, 5)], ids=lambda t: "%d_%d" % t)
def test_two_fast_passes_list_tiles_next_to_frames_that_list_none(hip_lib, th):
    """64 frames: low-contrast ones, whose cells come back empty at iniThFAST and are listed for the second pass, between noise and textured
    frames that list (almost) nothing.  Four consecutive calls on one handle keep the two-pass form (the product reports it, and listed > 0); from
    the second on, the second pass's grid is sized from the previous call's list.  Then 8 frames on the same handle (another tile count: the
    (listed, tiles) pair of the 64-frame calls does not describe it) and 64 again.  Every checked frame of every call equals the oracle."""
    cfg = (500, 1.2, 4, th[0], th[1])
    lap = (0, 0)
    kinds = {"lowc": [low_contrast_image(70 + i, W0, H0) for i in range(2)],
             "noise": [np.random.default_rng(77).integers(0, 256, (H0, W0), dtype=np.uint8)],
             "textured": [synth_image(80 + i, W0, H0, n_rect=400, n_disc=200) for i in range(3)]}
    # the low-contrast frames really have cells that are empty at ini and not at min: fewer candidates at (ini, ini) than at (ini, min)
    for f in kinds["lowc"]:
        o_hi = O.OrbOracle(500, 1.2, 4, th[0], th[0])
        o_hi.extract(f)
        assert len(o_hi.level_candidates(0)) < len(ref_levels(cfg, f, lap)[0][0]), "precondition: low-contrast cells retry at minThFAST"
    pick = [("lowc", i % 2) if i % 8 == 3 else ("noise", 0) if i % 8 == 6 else ("textured", i % 3) for i in range(64)]   # 8 low-contrast, 8 noise
    frames = [kinds[k][j] for k, j in pick]
    hd = Handle(hip_lib, "hip", cfg, W0, H0, 64)
    img = hd.images(frames)
    check = [0, 3, 6, 11, 59, 63]

    def run(image, B, idx, what):
        out = hd.call(image, B, lap)
        p = hd.fast_passes()   # (hd.call synchronised the stream: the pair is the one of the call just made)
        for b in idx:
            assert_frame(out, b, ref(cfg, frames[b], lap), what)
        return p
    seen = []
    for call in range(4):
        p = run(img, 64, check, "call %d" % call)
        seen.append(p)
        assert p["two_pass"] == 1 and p["tiles"] > 0, "call %d did not run two passes: %s" % (call, seen)
        assert p["listed"] > 0, "call %d: listed = %d of %d tiles, expected > 0 (%s)" % (call, p["listed"], p["tiles"], seen)
    print("case 3, thresholds %d/%d: (two_pass, listed, tiles) of the four calls: %s" % (th[0], th[1], [(q["two_pass"], q["listed"], q["tiles"]) for q in seen]))
    assert seen[0]["listed"] == seen[3]["listed"] and seen[0]["listed"] < seen[0]["tiles"], seen   # the same frames list the same tiles; noise lists none
    p = run(hd.images(frames[:8]), 8, range(8), "8 frames on the same handle")
    assert p["two_pass"] == 0, p
    p = run(img, 64, check, "64 frames again")
    assert p["two_pass"] == 1 and p["listed"] == seen[0]["listed"], (p, seen)


# ---- case 4 ---------------------------------------------------------------------------------------------------------------------------------
def _stride_frames(W, H):
    rng = np.random.default_rng(5)
    return [synth_image(91, W, H, n_rect=8, n_disc=4), flat_image(W, H, 200), rng.integers(0, 256, (H, W), dtype=np.uint8),
            synth_image(92, W, H, n_rect=80, n_disc=40), low_contrast_image(93, W, H), synth_image(94, W, H, n_rect=30, n_disc=10),
            rng.integers(0, 256, (H, W), dtype=np.uint8), synth_image(95, W, H, n_rect=200, n_disc=100)]


def _size(backend, narrow):
    W, H = (400, 300) if backend == "hip" else (240, 200)
    return (W - 2 if narrow else W), H


@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("narrow", [False, True], ids=["w_mult_of_4", "w_even"])
def test_padded_strides_and_a_4_byte_aligned_base(lib, backend, narrow):
    """orbx_extract_batch_dev with what the header allows and the Python wrapper never passes: rows row_stride > width apart, a gap of 64
    bytes between the frames, the base 4 bytes into the allocation (4-byte, not 16-byte aligned).  Widths 400 and 398 on the product (240 and 238
    on the emulator); row strides: the width rounded up to 4, that + 4, and 448 (288).  (The header refuses a row stride that is no multiple of 4,
    so 398 + 4 = 402 is among the refused arguments of the test below, not here.)  The padding holds 0, then 255, then random bytes: the results
    are the same and equal the oracle's on the cropped frames, at 3 frames (one-cell-row tiles) and 8 (two-cell-row tiles; the emulator runs a
    subset of the combinations); the frames differ in
    weight, so every call after a handle's first walks them in another order than they lie in memory."""
    W, H = _size(backend, narrow)
    cfg = (300, 1.2, 4, 20, 7)
    lap = (W // 3, 2 * W // 3)
    frames = _stride_frames(W, H)
    W4 = (W + 3) & ~3
    hd = Handle(lib, backend, cfg, W, H, 8)
    rng = np.random.default_rng(11)
    plan = [(rs, B, (0, 255, None)) for rs in (W4, W4 + 4, 448) for B in (3, 8)]
    if backend == "emu":   # (the emulator pays about a second per frame: every stride, batch class and filling once, not their product)
        plan = [(W4, 3, (255,)), (W4 + 4, 3, (0, 255, None)), (288, 8, (0, None))]
    for rs, B, fills in plan:
        first = None
        for fill in fills:
            out = hd.call(hd.images(frames[:B], row_stride=rs, gap=64, lead=4, fill=fill, rng=rng), B, lap)
            what = "width %d row_stride %d B %d padding %s" % (W, rs, B, "random" if fill is None else fill)
            if first is None:
                first = out
                for b in range(B):
                    assert_frame(out, b, ref(cfg, frames[b], lap), what)
            else:
                assert_same(first, out, what)
    assert hd.schedule()[0] == 1   # (the calls after the first were ordered)


@pytest.mark.parametrize("backend", BACKENDS)
def test_refused_batch_arguments_launch_nothing(lib, backend):
    """row_stride < width, row_stride or base not 4-byte aligned, batch > max_batch, cap_per_frame < 1: ORB_E_INVALID, and no output byte changes."""
    W, H = _size(backend, True)
    cfg = (300, 1.2, 4, 20, 7)
    frames = _stride_frames(W, H)[:3]
    hd = Handle(lib, backend, cfg, W, H, 3)
    W4 = (W + 3) & ~3
    good = hd.images(frames, row_stride=W4 + 4, gap=64, lead=4)
    buf, lead, fs, rs = good
    cases = {"row_stride < width": dict(img=(buf, lead, fs, W - 2)),
             "row_stride = width + 4, no multiple of 4": dict(img=(buf, lead, fs, W + 4)),
             "base 2 bytes off": dict(img=good, lead_shift=2),
             "base 1 byte off": dict(img=good, lead_shift=1),
             "batch > max_batch": dict(img=good, B=4, slabs=4),
             "batch 0": dict(img=good, B=0, slabs=3),
             "cap_per_frame 0": dict(img=good, cap=0),
             "cap_per_frame -1": dict(img=good, cap=-1)}
    for what, kw in cases.items():
        B = kw.get("B", 3)
        rc, kps, desc, cnt, tails = hd.call_raw(kw["img"], B, (0, 0), kw.get("cap", hd.max_kp), slabs=kw.get("slabs"), lead_shift=kw.get("lead_shift", 0))
        assert rc == _lib.ORB_E_INVALID, (what, rc)
        for a in (kps, desc, cnt) + tuple(tails):
            assert (a.view(np.uint8) == CANARY).all(), (what, "an output was written")
    out = hd.call(good, 3, (0, 0))   # the handle is still good
    for b in range(3):
        assert_frame(out, b, ref(cfg, frames[b], (0, 0)), "after the refused calls")


# ---- case 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", BACKENDS)
@pytest.mark.parametrize("lap", ["no_lapping", "lapping_split"])
def test_cap_below_the_need_and_batch_below_max_batch(lib, backend, lap):
    """A handle for 8 frames called with 3, cap_per_frame at 60 % of the smallest frame's n: counts report the oracle's n and monoIndex (those of
    the untruncated output, see orbhip.h), every slab holds entries [0, cap_per_frame) of the oracle's output — with a lapping split the monocular
    key points and then the tail end of the lapping ones, which the reference stores from the back — and nothing else is written: not the slabs
    [3, 8) of an allocation for max_batch frames, not the bytes behind the allocations."""
    W, H = _size(backend, False)
    cfg = (300, 1.2, 4, 20, 7)
    lap = (0, 0) if lap == "no_lapping" else (W // 2, W)
    fr = _stride_frames(W, H)
    frames = [fr[3], fr[2], fr[5]]   # textured, noise, moderately textured
    refs = [ref(cfg, f, lap) for f in frames]
    need = min(len(r[1]) for r in refs)
    assert need > 50, need
    cap = int(0.6 * need)
    if lap != (0, 0):
        assert all(0 < r[0] < len(r[1]) for r in refs), "precondition: a real lapping split in every frame"
        assert any(r[0] < cap for r in refs), "precondition: a slab that holds monocular and lapping key points"
    hd = Handle(lib, backend, cfg, W, H, 8)
    img = hd.images(frames, row_stride=(W + 3) & ~3)
    for call in range(2):   # (the second call runs ordered)
        kps, desc, cnt = hd.call(img, 3, lap, cap=cap, slabs=8)
        for b in range(3):
            assert cnt[b, 0] > cap
            assert_frame((kps, desc, cnt), b, refs[b], "cap %d of %d, call %d" % (cap, len(refs[b][1]), call), cap=cap)
        assert (kps[3:].view(np.uint8) == CANARY).all() and (desc[3:] == CANARY).all() and (cnt[3:].view(np.uint8) == CANARY).all(), \
            "slabs [batch, max_batch) were written"


# ---- case 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_single_frame_handle_reuse_across_content_window_and_entry_point(hip_lib):
    """One ORBextractor: image A, A again (replay of the captured graph), B of the same size, A with another lapping window (the graph is captured
    again), a flat image (replay on zero key points), then a batch call on the same handle and a single frame again — each equals the oracle."""
    cfg = (400, 1.2, 4, 20, 7)
    A = synth_image(101, W0, H0, n_rect=80, n_disc=40)
    Bimg = np.random.default_rng(77).integers(0, 256, (H0, W0), dtype=np.uint8)
    flat = flat_image(W0, H0, 128)
    e = orbhip.ORBextractor(*cfg, lib=hip_lib, max_batch=4)

    def single(img, lap, what):
        mono, k, d = ref(cfg, img, lap)
        m2, k2, d2 = e(img, None, lap)
        assert m2 == mono and len(k2) == len(k), (what, m2, mono, len(k2), len(k))
        assert np.array_equal(k.view(np.uint8), k2.view(np.uint8)) and np.array_equal(d, d2), what
    single(A, (0, 0), "A")
    h0 = e._h.value
    single(A, (0, 0), "A again")
    single(Bimg, (0, 0), "B")
    single(A, (100, 300), "A, lapping window 100..300")
    single(flat, (100, 300), "flat")
    import torch
    frames = [Bimg, flat, A]
    kps, desc, cnt = [t.cpu().numpy() for t in e.extract_batch(torch.from_numpy(np.stack(frames)).cuda(), (100, 300))]
    assert e._h.value == h0, "the batch call ran on the same handle"
    for b in range(3):
        assert_frame((kps.view(np.uint8).reshape(3, -1).view(KP), desc, cnt), b, ref(cfg, frames[b], (100, 300)), "batch of 3 on the single-frame handle")
    single(A, (100, 300), "A after the batch call")
    single(Bimg, (0, 0), "B after the batch call, without lapping")


# ---- case 7 ---------------------------------------------------------------------------------------------------------------------------------
# seeds of tools/fuzz_parity.case with a width that is a multiple of 4: 2001 uniform noise 224 wide; 2003 Gaussian noise, scale 1.25, thresholds 20/3,
# lapping; 2013 speckled scene, 3 levels, lapping; 2014 Gaussian noise, scale 1.1; 2016 thresholds 100/5; 2018 scale 1.4 (k_resize, own k_frame_order)
FUZZ_SEEDS = [2001, 2003, 2013, 2014, 2016, 2018]


def _fuzz_case(seed):
    rng = np.random.default_rng(seed)
    img, nf, sf, nl, ini, mn, lap = F.case(rng)
    img = np.ascontiguousarray(img[:300, :400])
    while nl > 1 and min(img.shape) / sf ** (nl - 1) < 70:
        nl -= 1
    return img, (min(nf, 500), sf, min(nl, 4), ini, mn), lap


@pytest.mark.gpu
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_hip_fuzz_batch_of_64_copies(hip_lib, seed):
    """The batch leg of tools/fuzz_parity.py (64 copies of the case's frame: two-cell-row tiles and, with ini > min, two FAST passes), on the
    case's frame cropped to 400x300 and at most 4 levels / 500 features; thresholds, scale factor and lapping window are the case's."""
    img, cfg, lap = _fuzz_case(seed)
    assert img.shape[1] % 4 == 0
    mono, k, d = ref(cfg, img, lap)
    e = orbhip.ORBextractor(*cfg, lib=hip_lib)
    assert F.batch_leg_matches(e, img, lap, mono, k, d), (seed, cfg, lap)
