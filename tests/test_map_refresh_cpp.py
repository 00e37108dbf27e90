"""Builds tests/cpp/map_refresh_test.cpp (the header-only adapter's MapPointRefresh::Refresh on flattened host records and on device pointers,
against hand-built expectations: a tie, a bad key frame, an overflow point) and runs it: CPU tier = emulated library, GPU tier = the real
liborbhip.so."""
import pytest

from cpp_harness import build_and_run


def _build_and_run(libpath, tag, tmp_path):
    build_and_run(["map_refresh_test.cpp"], tag, tmp_path, "map_refresh_test OK", libpath=libpath, flags=("-ffp-contract=off",))


def test_map_refresh_adapter_on_emulated_library(emu_lib, tmp_path):
    import build_emu
    _build_and_run(build_emu.OUT, "emu", tmp_path)


@pytest.mark.gpu
def test_map_refresh_adapter_on_hip_library(hip_lib, tmp_path):
    from orbhip import _lib
    _build_and_run(_lib.LIB_PATH, "hip", tmp_path)
