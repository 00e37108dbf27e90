"""Builds tests/cpp/map_projection_test.cpp (the header-only adapter's SearchByProjectionFromMap against the existing SearchByProjection fed
hand-built queries) and runs it: CPU tier = emulated library, GPU tier = the real liborbhip.so."""
import pytest

from cpp_harness import build_and_run


def _build_and_run(libpath, tag, tmp_path):
    build_and_run(["map_projection_test.cpp"], tag, tmp_path, "map_projection_test OK", libpath=libpath, flags=("-ffp-contract=off",))


def test_map_projection_adapter_on_emulated_library(emu_lib, tmp_path):
    import build_emu
    _build_and_run(build_emu.OUT, "emu", tmp_path)


@pytest.mark.gpu
def test_map_projection_adapter_on_hip_library(hip_lib, tmp_path):
    from orbhip import _lib
    _build_and_run(_lib.LIB_PATH, "hip", tmp_path)
