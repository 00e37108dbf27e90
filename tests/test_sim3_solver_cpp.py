"""Builds tests/cpp/sim3_solver_test.cpp (the header-only adapter orbslam3_hip::Sim3Solver: chunked iterate() with chunks of 1, 20 and
mRansacMaxIts, both overloads, find(), continuation calls after a convergence and after bNoMore, against a serial replay of the reference's
control flow on the adapter's downloaded counts) and runs it: CPU tier = emulated library, GPU tier = the real liborbhip.so."""
import pytest

from cpp_harness import build_and_run


def _build_and_run(libpath, tag, tmp_path):
    build_and_run(["sim3_solver_test.cpp"], tag, tmp_path, "sim3_solver_test OK", libpath=libpath, flags=("-ffp-contract=off",))


def test_sim3_solver_adapter_on_emulated_library(emu_lib, tmp_path):
    import build_emu
    _build_and_run(build_emu.OUT, "emu", tmp_path)


@pytest.mark.gpu
def test_sim3_solver_adapter_on_hip_library(hip_lib, tmp_path):
    from orbhip import _lib
    _build_and_run(_lib.LIB_PATH, "hip", tmp_path)
