"""Builds tests/cpp/two_view_test.cpp (the header-only adapter orbslam3_hip::TwoViewReconstruction against the plain C++ host loop of rule R7,
tests/cpp/two_view_host.h, on the adapter's own sets: a general scene, a planar one, a pure rotation, too few matches, and the overload on
device pointers) and runs it: CPU tier = emulated library (bit for bit), GPU tier = the real liborbhip.so (the parallax within one float ulp)."""
import pytest

from cpp_harness import build_and_run


def _build_and_run(libpath, tag, tmp_path, flags=()):
    build_and_run(["two_view_test.cpp"], tag, tmp_path, "two_view_test OK", libpath=libpath, flags=("-ffp-contract=off",) + flags)


def test_two_view_adapter_on_emulated_library(emu_lib, tmp_path):
    import build_emu
    _build_and_run(build_emu.OUT, "emu", tmp_path)


@pytest.mark.gpu
def test_two_view_adapter_on_hip_library(hip_lib, tmp_path):
    from orbhip import _lib
    _build_and_run(_lib.LIB_PATH, "hip", tmp_path, ("-DTV_GPU",))
