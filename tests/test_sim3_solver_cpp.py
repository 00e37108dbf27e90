"""Builds tests/cpp/sim3_solver_test.cpp (the header-only adapter orbslam3_hip::Sim3Solver: chunked iterate() with chunks of 1, 20 and
mRansacMaxIts, both overloads, find(), continuation calls after a convergence and after bNoMore, against a serial replay of the reference's
control flow on the adapter's downloaded counts) and runs it: CPU tier = emulated library, GPU tier = the real liborbhip.so."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_and_run(libpath, tag, tmp_path):
    exe = str(tmp_path / ("sim3_solver_test_" + tag))
    libdir, libname = os.path.dirname(libpath), os.path.basename(libpath)[3:-3]
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "sim3_solver_test.cpp"), "-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-o", exe]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "sim3_solver_test OK" in out.stdout, out.stdout + out.stderr


def test_sim3_solver_adapter_on_emulated_library(emu_lib, tmp_path):
    import build_emu
    _build_and_run(build_emu.OUT, "emu", tmp_path)


@pytest.mark.gpu
def test_sim3_solver_adapter_on_hip_library(hip_lib, tmp_path):
    from orbhip import _lib
    _build_and_run(_lib.LIB_PATH, "hip", tmp_path)
