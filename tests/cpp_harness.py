"""Builds one C++ test program of tests/cpp against the adapters in include/orbslam3_hip/ and runs it.  The wrappers (test_*_cpp.py, test_glue.py,
test_cpp_adapter.py) pass the emulated library on the CPU tier and the real liborbhip.so on the GPU tier."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
MOCK = os.path.join(CPP, "mock_orbslam3")
INCLUDE = os.path.join(ROOT, "include")
ORACLE = os.path.join(ROOT, "oracle")


def build_and_run(sources, tag, tmp_path, ok, libpath=None, include_dirs=(INCLUDE,), flags=(), libs=(), oracle=False, timeout=600):
    """sources: files of tests/cpp (or absolute paths), the first names the program.  libpath: the liborbhip build to link, or None for a program
    that links none.  oracle: also link oracle/liboracle.so (built first).  Asserts return code 0 and the line `ok`; returns the finished run."""
    sources = [s if os.path.isabs(s) else os.path.join(CPP, s) for s in sources]
    exe = str(tmp_path / (os.path.splitext(os.path.basename(sources[0]))[0] + "_" + tag))
    cmd = ["g++", "-std=c++17", "-O1"] + list(flags)
    for d in include_dirs:
        cmd += ["-I", d]
    cmd += sources
    if libpath:
        libdir, libname = os.path.dirname(libpath), os.path.basename(libpath)[3:-3]
        cmd += ["-L", libdir, "-l" + libname, "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"]
    if oracle:
        subprocess.check_call(["make", "-C", ORACLE], stdout=subprocess.DEVNULL)
        cmd += ["-L", ORACLE, "-loracle", "-Wl,-rpath," + ORACLE]
    subprocess.check_call(cmd + list(libs) + ["-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and ok in out.stdout, out.stdout + out.stderr
    return out

