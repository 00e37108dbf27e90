"""Builds tests/cpp/adapter_test.cpp against the header-only adapters in include/orbslam3_hip/ and runs it:
CPU tier = emulated library, GPU tier = the real liborbhip.so."""
import pytest

from cpp_harness import build_and_run


def _build_and_run(libpath, tag, tmp_path):
    build_and_run(["adapter_test.cpp"], tag, tmp_path, "adapter_test OK", libpath=libpath, oracle=True)


def test_cpp_adapters_on_emulated_library(emu_lib, tmp_path):
    import build_emu
    _build_and_run(build_emu.OUT, "emu", tmp_path)


@pytest.mark.gpu
def test_cpp_adapters_on_hip_library(hip_lib, tmp_path):
    from orbhip import _lib
    _build_and_run(_lib.LIB_PATH, "hip", tmp_path)
