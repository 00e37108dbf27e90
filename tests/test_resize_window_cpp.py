"""Builds tests/cpp/resize_window_test.cpp and runs it, plain and under AddressSanitizer + UndefinedBehaviorSanitizer: the source window of a
k_resize2 lane (csrc/resize_window.inc, the helper the kernel itself calls) over 3 000 random configurations and widths that are multiples of 64 —
every dword index inside the source row, every tap inside the lane's 8-byte window.  Host code only; the program links no library."""
from cpp_harness import build_and_run


def test_resize_window_plain(tmp_path):
    build_and_run(["resize_window_test.cpp"], "plain", tmp_path, "resize_window_test OK", include_dirs=(), flags=("-Wall", "-Wextra"))


def test_resize_window_under_asan_ubsan(tmp_path):
    out = build_and_run(["resize_window_test.cpp"], "san", tmp_path, "resize_window_test OK", include_dirs=(),
                        flags=("-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
