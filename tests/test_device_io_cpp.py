"""Builds tests/cpp/device_io_test.cpp (include/orbslam3_hip/detail/DeviceIO.h alone: layout offsets, the buffers' growth rules, the state after a
failed allocation, the checked download; the program defines the runtime helpers itself over malloc and links no library) and runs it, plain and
under AddressSanitizer + UndefinedBehaviorSanitizer.  CPU tier only."""
from cpp_harness import build_and_run


def test_device_io(tmp_path):
    build_and_run(["device_io_test.cpp"], "plain", tmp_path, "device_io_test OK", flags=("-Wall", "-Wextra"))


def test_device_io_under_asan_ubsan(tmp_path):
    out = build_and_run(["device_io_test.cpp"], "san", tmp_path, "device_io_test OK",
                        flags=("-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
