"""Host-side wrapper of the device Sim3Solver (reference src/Sim3Solver.cc; include/orbhip.h "Sim3Solver"): a batch of RANSAC Horn alignment
problems in one launch, every hypothesis of every problem evaluated, the reference's serial pick on the device.

Slabs are torch CUDA tensors (product path) or numpy arrays (device=None: only meaningful with the emulated test build, whose "device" is host
memory).  The slabs are allocated once; set_problems rewrites them in place, so a captured graph of launch() sees new problems on replay."""
import numpy as np

from . import _lib
from ._abi import (SIM3_BAD_INDEX, SIM3_BAD_SAMPLE, SIM3_CAM_KB8, SIM3_CAM_PINHOLE, SIM3_CAMERA_DTYPE, SIM3_CORR_DTYPE, SIM3_HYP_DTYPE,  # noqa: F401
                   SIM3_ITS_CLAMPED, SIM3_MAX_N, SIM3_N_CLAMPED, SIM3_PROBLEM_DTYPE, SIM3_RESULT_DTYPE)
from ._lib import OrbHipError, check, ptr, stream, to_host, zeros

CAMERA_DTYPE, CORR_DTYPE, PROBLEM_DTYPE, HYP_DTYPE, RESULT_DTYPE = SIM3_CAMERA_DTYPE, SIM3_CORR_DTYPE, SIM3_PROBLEM_DTYPE, SIM3_HYP_DTYPE, SIM3_RESULT_DTYPE
RAND_MAX = 2147483647   # glibc


def truncated_max_error(sigma2):
    """mvnMaxError*.push_back(9.210*sigmaSquare) (Sim3Solver.cc:99-100): the double product truncated by the conversion to size_t, as the float the
    comparison of CheckInliers converts it to"""
    return np.float32(int(9.210 * float(np.float32(sigma2))))


def draw_samples(n, its, rand_values):
    """The triples the reference's iterations draw from n correspondences (Sim3Solver.cc:175-189): three DUtils::Random::RandomInt(0, size - 1) =
    int((double)r / ((double)RAND_MAX + 1.0) * d) + min each, with the swap-with-back removal.  rand_values: raw rand() outputs, three per
    iteration, in call order.  -> int32 [its, 3]"""
    if n < 3:
        raise OrbHipError(_lib.ORB_E_INVALID, "draw_samples needs at least 3 correspondences")
    r = iter(rand_values)
    out = np.zeros((its, 3), np.int32)
    for h in range(its):
        avail = list(range(n))
        for i in range(3):
            d = (len(avail) - 1) - 0 + 1
            randi = int((float(next(r)) / (float(RAND_MAX) + 1.0)) * d) + 0
            out[h, i] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return out


class Sim3Solver:
    def __init__(self, batch, cap_n, cap_its, cap_n1, device=None, lib=None):
        """device: a torch device for the product library, None for numpy slabs (emulated build)."""
        self._L = lib if lib is not None else _lib.load()
        self.batch, self.cap_n, self.cap_its, self.cap_n1, self.device = int(batch), int(cap_n), int(cap_its), int(cap_n1), device
        if self.batch < 1 or self.cap_n < 1 or self.cap_its < 1 or self.cap_n1 < 1:
            raise OrbHipError(_lib.ORB_E_INVALID, "batch, cap_n, cap_its and cap_n1 are at least 1")
        if self.cap_n > SIM3_MAX_N:
            raise OrbHipError(_lib.ORB_E_CAPACITY, "cap_n = %d exceeds ORBM_SIM3_MAX_N = %d" % (self.cap_n, SIM3_MAX_N))
        self.words = (self.cap_n + 63) // 64
        z, B = self._zeros, self.batch
        self.d = dict(problems=z((B, PROBLEM_DTYPE.itemsize), np.uint8), corr=z((B, self.cap_n, CORR_DTYPE.itemsize), np.uint8), n=z((B,), np.int32),
                      samples=z((B, self.cap_its, 3), np.int32))
        # the mask words as int64 bit patterns (torch has no uint64 arithmetic; nothing here computes with them)
        self.out = dict(hyp=z((B, self.cap_its, HYP_DTYPE.itemsize), np.uint8), hyp_count=z((B, self.cap_its), np.int32),
                        hyp_mask=z((B, self.cap_its, self.words), np.int64), result=z((B, RESULT_DTYPE.itemsize), np.uint8),
                        inliers=z((B, self.cap_n1), np.uint8))
        self._work = z(((int(self._L.orbm_sim3_workspace_bytes(B, self.cap_n, self.cap_its)) + 7) // 8,), np.int64)

    def _zeros(self, shape, dtype):
        return zeros(self.device, shape, dtype)

    def _write(self, dst, src):
        """host numpy -> the leading entries of a slab, in place (the slab's address must not change: captured graphs hold it)"""
        src = np.ascontiguousarray(src)
        flat = src.reshape(-1) if src.dtype == np.int32 else src.view(np.uint8).reshape(-1)
        if self.device is None:
            dst.reshape(-1)[:flat.size] = flat
        else:
            import torch
            dst.view(-1)[:flat.size].copy_(torch.from_numpy(flat.copy()))

    def ransac_iterations(self, probability, min_inliers, max_its, n):
        """mRansacMaxIts after SetRansacParameters(probability, min_inliers, max_its) with n correspondences (Sim3Solver.cc:137-147)"""
        return int(self._L.orbm_sim3_ransac_iterations(float(probability), int(min_inliers), int(max_its), int(n)))

    def set_problems(self, problems, corr, samples):
        """problems: PROBLEM_DTYPE [batch]; corr: one CORR_DTYPE array per problem (its length is N); samples: per problem int32 [max_its, 3]
        (draw_samples).  Host-side checks: min_inliers >= 3, N <= cap_n, max_its <= cap_its, one entry per problem."""
        problems = np.ascontiguousarray(problems, PROBLEM_DTYPE).reshape(-1)
        if len(problems) != self.batch or len(corr) != self.batch or len(samples) != self.batch:
            raise OrbHipError(_lib.ORB_E_INVALID, "one problem, one correspondence list and one sample list per batch entry (%d)" % self.batch)
        if (problems["min_inliers"] < 3).any():
            raise OrbHipError(_lib.ORB_E_INVALID, "min_inliers below 3: a Horn alignment needs three pairs")
        if (problems["max_its"] > self.cap_its).any() or (problems["max_its"] < 1).any():
            raise OrbHipError(_lib.ORB_E_CAPACITY, "max_its outside 1..cap_its = %d" % self.cap_its)
        c = np.zeros((self.batch, self.cap_n), CORR_DTYPE)
        s = np.zeros((self.batch, self.cap_its, 3), np.int32)
        n = np.zeros(self.batch, np.int32)
        for b in range(self.batch):
            if len(corr[b]) > self.cap_n:
                raise OrbHipError(_lib.ORB_E_CAPACITY, "problem %d has %d correspondences, cap_n = %d" % (b, len(corr[b]), self.cap_n))
            sb = np.asarray(samples[b], np.int32).reshape(-1, 3)
            if len(sb) < problems["max_its"][b] and len(corr[b]) >= problems["min_inliers"][b]:
                raise OrbHipError(_lib.ORB_E_INVALID, "problem %d: %d sample triples for max_its = %d" % (b, len(sb), problems["max_its"][b]))
            n[b] = len(corr[b])
            c[b, :n[b]] = corr[b]
            s[b, :min(len(sb), self.cap_its)] = sb[:self.cap_its]
        self._write(self.d["problems"], problems)
        self._write(self.d["corr"], c)
        self._write(self.d["n"], n)
        self._write(self.d["samples"], s)

    def launch(self):
        """orbm_sim3_solve on the slabs as they are: no host read, no allocation, graph-capturable.  -> the dict of device outputs"""
        d, o = self.d, self.out
        check(self._L.orbm_sim3_solve(ptr(d["problems"]), ptr(d["corr"]), ptr(d["n"]), self.cap_n, ptr(d["samples"]), self.cap_its, self.batch,
                                      ptr(o["hyp"]), ptr(o["hyp_count"]), ptr(o["hyp_mask"]), ptr(o["result"]), ptr(o["inliers"]), self.cap_n1,
                                      ptr(self._work), stream(self.device)), "orbm_sim3_solve failed")
        return o

    def solve(self, problems, corr, samples):
        self.set_problems(problems, corr, samples)
        return self.launch()

    def to_host(self, out=None):
        """-> dict(hyp HYP_DTYPE [batch, cap_its], hyp_count, hyp_mask uint64 [batch, cap_its, words], result RESULT_DTYPE [batch], inliers)"""
        o = out if out is not None else self.out
        return dict(hyp=to_host(o["hyp"]).view(HYP_DTYPE).reshape(self.batch, self.cap_its), hyp_count=to_host(o["hyp_count"]),
                    hyp_mask=to_host(o["hyp_mask"]).view(np.uint64), result=to_host(o["result"]).view(RESULT_DTYPE).reshape(self.batch),
                    inliers=to_host(o["inliers"]))
