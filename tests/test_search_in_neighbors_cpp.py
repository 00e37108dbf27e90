"""Builds tests/cpp/search_in_neighbors_test.cpp (the header-only adapter orbslam3_hip::SearchInNeighbors against the host restatement of
tests/cpp/search_in_neighbors_host.h: targets, events, candidates, the merged rows, the slabs left on the device, exceptions) and runs it:
CPU tier = emulated library, GPU tier = the real liborbhip.so.  tests/cpp/search_in_neighbors_host_test.cpp (the host restatement on a
hand-made map with a worked-out answer and on random worlds; links no library) also runs under AddressSanitizer + UndefinedBehaviorSanitizer,
on the CPU only."""
import pytest

from cpp_harness import build_and_run


def _build_and_run(libpath, tag, tmp_path):
    build_and_run(["search_in_neighbors_test.cpp"], tag, tmp_path, "search_in_neighbors_test OK", libpath=libpath, flags=("-Wall", "-Wextra"))


def test_search_in_neighbors_adapter_on_emulated_library(emu_lib, tmp_path):
    import build_emu
    _build_and_run(build_emu.OUT, "emu", tmp_path)


@pytest.mark.gpu
def test_search_in_neighbors_adapter_on_hip_library(hip_lib, tmp_path):
    from orbhip import _lib
    _build_and_run(_lib.LIB_PATH, "hip", tmp_path)


def test_host_restatement(tmp_path):
    build_and_run(["search_in_neighbors_host_test.cpp"], "plain", tmp_path, "search_in_neighbors_host_test OK", flags=("-Wall", "-Wextra"))


def test_host_restatement_under_asan_ubsan(tmp_path):
    out = build_and_run(["search_in_neighbors_host_test.cpp"], "san", tmp_path, "search_in_neighbors_host_test OK",
                        flags=("-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
