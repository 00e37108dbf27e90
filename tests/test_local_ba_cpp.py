"""Builds tests/cpp/local_ba_test.cpp (the header-only adapter orbslam3_hip::LocalBundleAdjustment on a device-resident map against the C++
restatement of tests/cpp/local_ba_host.h: the window as built with the poseFromTcw bytes at the stop-flag exit before the first optimise,
the exit between the two optimisations, the whole chain with the folded map, a window that does not fit as an exception) and runs it: CPU
tier = emulated library, GPU tier = the real liborbhip.so.  tests/cpp/local_ba_host_test.cpp (the restatement alone on a hand-computed map;
links no library) also runs under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU only."""
import pytest

from cpp_harness import CPP, INCLUDE, build_and_run

DIRS = (INCLUDE, CPP)


def _build_and_run(libpath, tag, tmp_path):
    build_and_run(["local_ba_test.cpp"], tag, tmp_path, "local_ba_test OK", libpath=libpath, include_dirs=DIRS, flags=("-ffp-contract=off",))


def test_local_ba_adapter_on_emulated_library(emu_lib, tmp_path):
    import build_emu
    _build_and_run(build_emu.OUT, "emu", tmp_path)


@pytest.mark.gpu
def test_local_ba_adapter_on_hip_library(hip_lib, tmp_path):
    from orbhip import _lib
    _build_and_run(_lib.LIB_PATH, "hip", tmp_path)


def test_host_restatement_hand_computed(tmp_path):
    build_and_run(["local_ba_host_test.cpp"], "plain", tmp_path, "local_ba_host_test OK", include_dirs=DIRS, flags=("-ffp-contract=off", "-Wall", "-Wextra"))


def test_host_restatement_under_asan_ubsan(tmp_path):
    out = build_and_run(["local_ba_host_test.cpp"], "san", tmp_path, "local_ba_host_test OK", include_dirs=DIRS,
                        flags=("-g", "-ffp-contract=off", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
