"""Builds tests/cpp/adapter_transfers_test.cpp (the runtime calls one steady-state call of each adapter entry point makes: one host->device and one
device->host transfer for the packed-block methods, no allocation anywhere; the program counts the calls by interposing the runtime helpers) and
runs it: CPU tier = emulated library, GPU tier = the real liborbhip.so."""
import pytest

from cpp_harness import build_and_run


def _build_and_run(libpath, tag, tmp_path):
    build_and_run(["adapter_transfers_test.cpp"], tag, tmp_path, "adapter_transfers_test OK", libpath=libpath,
                  flags=("-ffp-contract=off", "-Wall", "-Wno-sign-compare"), libs=("-ldl",), timeout=300)


def test_adapter_transfers_on_emulated_library(emu_lib, tmp_path):
    import build_emu
    _build_and_run(build_emu.OUT, "emu", tmp_path)


@pytest.mark.gpu
def test_adapter_transfers_on_hip_library(hip_lib, tmp_path):
    from orbhip import _lib
    _build_and_run(_lib.LIB_PATH, "hip", tmp_path)
