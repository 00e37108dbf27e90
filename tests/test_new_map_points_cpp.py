"""Builds tests/cpp/new_map_points_test.cpp (the header-only adapter orbslam3_hip::NewMapPoints: search -> create for three neighbours on one
stream with one download, against the existing ORBmatcher adapter plus the host loop of tests/cpp/new_map_points_host.h; the abort predicate, an
empty neighbour list, the capacity error as an exception, a rig refused) and runs it: CPU tier = emulated library, GPU tier = the real
liborbhip.so.  tests/cpp/new_map_points_pair_test.cpp (the adapter's host-only parts and the host loop; links no library) also runs under
AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU only."""
import pytest

from cpp_harness import build_and_run


def _build_and_run(libpath, tag, tmp_path):
    build_and_run(["new_map_points_test.cpp"], tag, tmp_path, "new_map_points_test OK", libpath=libpath, flags=("-ffp-contract=off",))


def test_new_map_points_adapter_on_emulated_library(emu_lib, tmp_path):
    import build_emu
    _build_and_run(build_emu.OUT, "emu", tmp_path)


@pytest.mark.gpu
def test_new_map_points_adapter_on_hip_library(hip_lib, tmp_path):
    from orbhip import _lib
    _build_and_run(_lib.LIB_PATH, "hip", tmp_path)


def test_pair_record_and_host_loop(tmp_path):
    build_and_run(["new_map_points_pair_test.cpp"], "plain", tmp_path, "new_map_points_pair_test OK", flags=("-ffp-contract=off", "-Wall", "-Wextra"))


def test_pair_record_and_host_loop_under_asan_ubsan(tmp_path):
    out = build_and_run(["new_map_points_pair_test.cpp"], "san", tmp_path, "new_map_points_pair_test OK",
                        flags=("-g", "-ffp-contract=off", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
