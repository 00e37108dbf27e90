"""Host-side mirror of the ORB_SLAM3::Frame constructor steps between the extractor and the matcher (reference src/Frame.cc:
UndistortKeyPoints :874, ComputeImageBounds :926 + grid scalars :394-397, ComputeStereoFromRGBD :1136) above the C ABI.
Arrays are torch CUDA tensors (product path) or numpy arrays (emulated test build only)."""
import ctypes as C

import numpy as np

from . import _lib
from ._abi import GRID_COLS, GRID_ROWS, Camera, FisheyeRig, GridParams  # noqa: F401
from ._lib import OrbHipError, check, ptr, stream, zeros  # noqa: F401


class FrameOps:
    def __init__(self, camera, width, height, *, lib=None):
        self._L = lib if lib is not None else _lib.load()
        self.camera, self.width, self.height = camera, int(width), int(height)
        b, gp = (C.c_float * 4)(), GridParams()
        self._check(self._L.orbf_image_bounds(C.byref(camera), self.width, self.height, C.byref(b), C.byref(gp)))
        self.mnMinX, self.mnMaxX, self.mnMinY, self.mnMaxY = (float(v) for v in b)
        self.grid = (gp.min_x, gp.min_y, gp.grid_w_inv, gp.grid_h_inv)   # argument of ORBmatcher.grid_build

    def _check(self, rc):
        check(rc, "orbf call failed")

    def UndistortKeyPoints(self, kps, counts, count_stride=1, out=None):
        """kps [B, cap, 7] float32 (orb_keypoint), counts int32 -> mvKeysUn, same shape"""
        B, cap = kps.shape[0], kps.shape[1]
        out = zeros(kps, tuple(kps.shape), np.float32) if out is None else out
        self._check(self._L.orbf_undistort_keypoints(ptr(kps), ptr(counts), count_stride, cap, B, C.byref(self.camera), ptr(out), stream(kps)))
        return out

    def UndistortAndGrid(self, kps, counts, count_stride=1, out=None):
        """UndistortKeyPoints + AssignFeaturesToGrid in one launch (orbm_undistort_and_grid_build).
        -> (mvKeysUn [B, cap, 7] f32, grid_start [B, 64*48+1] i32, grid_idx [B, cap] i32), the same arrays as the two separate calls"""
        B, cap = kps.shape[0], kps.shape[1]
        un, gs, gi = out if out is not None else (zeros(kps, tuple(kps.shape), np.float32), zeros(kps, (B, GRID_COLS * GRID_ROWS + 1), np.int32),
                                                  zeros(kps, (B, cap), np.int32))
        gp = GridParams(*self.grid)
        self._check(self._L.orbm_undistort_and_grid_build(ptr(kps), ptr(counts), count_stride, cap, B, C.byref(self.camera), C.byref(gp), ptr(un),
                                                          ptr(gs), ptr(gi), stream(kps)))
        return un, gs, gi

    def ComputeStereoFromRGBD(self, kps, kps_un, counts, depth, mbf, count_stride=1):
        """depth [B, H, W] float32 -> (mvuRight, mvDepth) [B, cap] float32"""
        B, cap = kps.shape[0], kps.shape[1]
        H, W = depth.shape[1], depth.shape[2]
        ur, dz = zeros(kps, (B, cap), np.float32), zeros(kps, (B, cap), np.float32)
        self._check(self._L.orbf_stereo_from_rgbd(ptr(kps), ptr(kps_un), ptr(counts), count_stride, cap, B, ptr(depth), H * W, W, W, H,
                                                  float(mbf), ptr(ur), ptr(dz), stream(kps)))
        return ur, dz


def ComputeStereoFishEyeMatches(kps_l, desc_l, n_l, mono_l, kps_r, desc_r, n_r, mono_r, rig, *, lib=None, count_stride=1):
    """Frame::ComputeStereoFishEyeMatches for a batch of fisheye stereo frames -> (mvLeftToRightMatch [B,capL], mvRightToLeftMatch [B,capR],
    mvDepth [B,capL], mvStereo3Dpoints [B,capL,3], nMatches [B])"""
    L = lib if lib is not None else _lib.load()
    B, capL, capR = kps_l.shape[0], kps_l.shape[1], kps_r.shape[1]
    l2r, r2l = zeros(kps_l, (B, capL), np.int32), zeros(kps_l, (B, capR), np.int32)
    depth, p3d, nm = zeros(kps_l, (B, capL), np.float32), zeros(kps_l, (B, capL, 3), np.float32), zeros(kps_l, (B,), np.int32)
    check(L.orbf_stereo_fisheye_matches(ptr(kps_l), ptr(desc_l), ptr(n_l), ptr(mono_l), ptr(kps_r), ptr(desc_r), ptr(n_r), ptr(mono_r), capL, capR,
                                        count_stride, B, C.byref(rig), ptr(l2r), ptr(r2l), ptr(depth), ptr(p3d), ptr(nm), stream(kps_l)),
          "orbf_stereo_fisheye_matches failed")
    return l2r, r2l, depth, p3d, nm
