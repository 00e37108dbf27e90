"""Builds tests/cpp/new_keyframe_test.cpp (the header-only adapters orbslam3_hip::ProcessNewKeyFrame and orbslam3_hip::MapPointCulling against
the host restatement of tests/cpp/new_keyframe_host.h: codes, added and culled points, the recent list, the slabs left on the device, the
hand-over between the two, exceptions) and runs it: CPU tier = emulated library, GPU tier = the real liborbhip.so.
tests/cpp/new_keyframe_host_test.cpp (the host restatement on a hand-made map with a worked-out answer and on random worlds; links no
library) also runs under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU only."""
import pytest

from cpp_harness import build_and_run


def _build_and_run(libpath, tag, tmp_path):
    build_and_run(["new_keyframe_test.cpp"], tag, tmp_path, "new_keyframe_test OK", libpath=libpath, flags=("-Wall", "-Wextra"))


def test_new_keyframe_adapters_on_emulated_library(emu_lib, tmp_path):
    import build_emu
    _build_and_run(build_emu.OUT, "emu", tmp_path)


@pytest.mark.gpu
def test_new_keyframe_adapters_on_hip_library(hip_lib, tmp_path):
    from orbhip import _lib
    _build_and_run(_lib.LIB_PATH, "hip", tmp_path)


def test_host_restatement(tmp_path):
    build_and_run(["new_keyframe_host_test.cpp"], "plain", tmp_path, "new_keyframe_host_test OK", flags=("-Wall", "-Wextra"))


def test_host_restatement_under_asan_ubsan(tmp_path):
    out = build_and_run(["new_keyframe_host_test.cpp"], "san", tmp_path, "new_keyframe_host_test OK",
                        flags=("-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
