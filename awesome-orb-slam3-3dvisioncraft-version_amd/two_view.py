"""Host-side wrapper of the device TwoViewReconstruction (reference src/TwoViewReconstruction.cc; include/orbhip.h "TwoViewReconstruction"):
Reconstruct for a batch of frame pairs in one call: every eight-point homography and fundamental hypothesis fitted and scored against all matches,
the best of each model and the choice between them, then the motion hypotheses of the chosen model, CheckRT and the accept logic.

Slabs are torch CUDA tensors (product path) or numpy arrays (device=None: only meaningful with the emulated test build, whose "device" is host
memory).  The slabs are allocated once; set_problems rewrites them in place, so a captured graph of launch() sees new problems on replay."""
import numpy as np

from . import _lib
from ._abi import (KP_DTYPE, TVR_BAD_INDEX, TVR_BAD_SAMPLE, TVR_ITS_CLAMPED, TVR_N_CLAMPED, TVR_NAN_PARALLAX, TVR_PROBLEM_DTYPE,  # noqa: F401
                   TVR_RESULT_DTYPE, TVR_TOO_FEW)
from ._lib import OrbHipError, check, ptr, stream, to_host, zeros

PROBLEM_DTYPE, RESULT_DTYPE = TVR_PROBLEM_DTYPE, TVR_RESULT_DTYPE
RAND_MAX = 2147483647   # glibc


def draw_sets(n, its, rand_values):
    """mvSets of Reconstruct (TwoViewReconstruction.cc:100-127) for n matches: eight DUtils::Random::RandomInt(0, size - 1) =
    int((double)r / ((double)RAND_MAX + 1.0) * d) + min per iteration, with the swap-with-back removal.  rand_values: raw rand() outputs, eight
    per iteration, in call order.  -> int32 [its, 8]"""
    if n < 8:
        raise OrbHipError(_lib.ORB_E_INVALID, "draw_sets needs at least 8 matches")
    r = iter(rand_values)
    out = np.zeros((its, 8), np.int32)
    for it in range(its):
        avail = list(range(n))
        for j in range(8):
            d = (len(avail) - 1) - 0 + 1
            randi = int((float(next(r)) / (float(RAND_MAX) + 1.0)) * d) + 0
            out[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return out


class TwoViewReconstruction:
    def __init__(self, batch, cap_k, cap_its, device=None, lib=None):
        """device: a torch device for the product library, None for numpy slabs (emulated build)."""
        self._L = lib if lib is not None else _lib.load()
        self.batch, self.cap_k, self.cap_its, self.device = int(batch), int(cap_k), int(cap_its), device
        if self.batch < 1 or self.cap_k < 1 or self.cap_its < 1:
            raise OrbHipError(_lib.ORB_E_INVALID, "batch, cap_k and cap_its are at least 1")
        self.words = (self.cap_k + 63) // 64
        z, B = self._zeros, self.batch
        self.d = dict(problems=z((B, PROBLEM_DTYPE.itemsize), np.uint8), keys1=z((B, self.cap_k, KP_DTYPE.itemsize), np.uint8),
                      keys2=z((B, self.cap_k, KP_DTYPE.itemsize), np.uint8), matches12=z((B, self.cap_k), np.int32),
                      sets=z((B, self.cap_its, 8), np.int32))
        # the mask words as int64 bit patterns (torch has no uint64 arithmetic; nothing here computes with them)
        self.out = dict(score=z((B, 2, self.cap_its), np.float32), model=z((B, 2, self.cap_its, 9), np.float32),
                        mask=z((B, 2, self.cap_its, self.words), np.int64), result=z((B, RESULT_DTYPE.itemsize), np.uint8),
                        p3d=z((B, self.cap_k, 3), np.float32), triangulated=z((B, self.cap_k), np.uint8))
        self._work = z(((int(self._L.orbm_two_view_workspace_bytes(B, self.cap_k, self.cap_its)) + 7) // 8,), np.int64)

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

    def set_problems(self, keys1, keys2, matches12, sets, K=(500.0, 500.0, 320.0, 240.0), sigma=1.0, min_parallax=1.0, min_triangulated=50):
        """Per problem: keys1 / keys2 KP_DTYPE arrays (x and y are read), matches12 int32 [len(keys1)] (index into keys2, negative = none), sets
        int32 [max_its, 8] (draw_sets): max_its is the number of sets.  K = (fx, fy, cx, cy); sigma, min_parallax and min_triangulated as the
        reference passes them.  Host-side checks: the capacities, one entry per problem."""
        if not (len(keys1) == len(keys2) == len(matches12) == len(sets) == self.batch):
            raise OrbHipError(_lib.ORB_E_INVALID, "one key list per frame, one match list and one set list per batch entry (%d)" % self.batch)
        P = np.zeros(self.batch, PROBLEM_DTYPE)
        k1 = np.zeros((self.batch, self.cap_k), KP_DTYPE)
        k2 = np.zeros((self.batch, self.cap_k), KP_DTYPE)
        m = np.full((self.batch, self.cap_k), -1, np.int32)
        s = np.zeros((self.batch, self.cap_its, 8), np.int32)
        for b in range(self.batch):
            sb = np.asarray(sets[b], np.int32).reshape(-1, 8)
            if len(keys1[b]) > self.cap_k or len(keys2[b]) > self.cap_k:
                raise OrbHipError(_lib.ORB_E_CAPACITY, "problem %d has %d / %d keys, cap_k = %d" % (b, len(keys1[b]), len(keys2[b]), self.cap_k))
            if len(sb) > self.cap_its:
                raise OrbHipError(_lib.ORB_E_CAPACITY, "problem %d has %d sets, cap_its = %d" % (b, len(sb), self.cap_its))
            if len(matches12[b]) != len(keys1[b]):
                raise OrbHipError(_lib.ORB_E_INVALID, "problem %d: matches12 has %d entries for %d keys" % (b, len(matches12[b]), len(keys1[b])))
            P[b] = (K[0], K[1], K[2], K[3], sigma, len(sb), len(keys1[b]), len(keys2[b]), min_parallax, min_triangulated)
            k1[b, :len(keys1[b])] = keys1[b]
            k2[b, :len(keys2[b])] = keys2[b]
            m[b, :len(matches12[b])] = matches12[b]
            s[b, :len(sb)] = sb
        for name, a in (("problems", P), ("keys1", k1), ("keys2", k2), ("matches12", m), ("sets", s)):
            self._write(self.d[name], a)

    def launch(self):
        """orbm_two_view_reconstruct on the slabs as they are: no host read, no allocation, graph-capturable.  -> the dict of device outputs"""
        d, o = self.d, self.out
        check(self._L.orbm_two_view_reconstruct(ptr(d["problems"]), ptr(d["keys1"]), ptr(d["keys2"]), self.cap_k, ptr(d["matches12"]),
                                                ptr(d["sets"]), self.cap_its, self.batch, ptr(o["score"]), ptr(o["model"]), ptr(o["mask"]),
                                                ptr(o["result"]), ptr(o["p3d"]), ptr(o["triangulated"]), ptr(self._work), stream(self.device)),
              "orbm_two_view_reconstruct failed")
        return o

    def reconstruct(self, keys1, keys2, matches12, sets, **params):
        self.set_problems(keys1, keys2, matches12, sets, **params)
        return self.launch()

    def to_host(self, out=None):
        """-> dict(score [batch, 2, cap_its], model [batch, 2, cap_its, 9], mask uint64 [batch, 2, cap_its, words], result RESULT_DTYPE [batch],
        p3d [batch, cap_k, 3], triangulated [batch, cap_k])"""
        o = out if out is not None else self.out
        return dict(score=to_host(o["score"]), model=to_host(o["model"]), mask=to_host(o["mask"]).view(np.uint64),
                    result=to_host(o["result"]).view(RESULT_DTYPE).reshape(self.batch), p3d=to_host(o["p3d"]), triangulated=to_host(o["triangulated"]))
