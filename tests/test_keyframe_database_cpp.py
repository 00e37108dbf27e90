"""Builds tests/cpp/keyframe_db_test.cpp (the header-only adapter orbslam3_hip::KeyFrameDatabase on a small hand-built database with hand-written
expected candidates: a tie, a stale read, a merge candidate, a bad map; plus the device-pointer overload) and runs it: CPU tier = emulated library,
GPU tier = the real liborbhip.so."""
import pytest

from cpp_harness import build_and_run


def _build_and_run(libpath, tag, tmp_path):
    build_and_run(["keyframe_db_test.cpp"], tag, tmp_path, "keyframe_db_test OK", libpath=libpath, flags=("-ffp-contract=off",))


def test_keyframe_database_adapter_on_emulated_library(emu_lib, tmp_path):
    import build_emu
    _build_and_run(build_emu.OUT, "emu", tmp_path)


@pytest.mark.gpu
def test_keyframe_database_adapter_on_hip_library(hip_lib, tmp_path):
    from orbhip import _lib
    _build_and_run(_lib.LIB_PATH, "hip", tmp_path)
