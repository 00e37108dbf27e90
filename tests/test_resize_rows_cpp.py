"""Builds tests/cpp/resize_rows_test.cpp and runs it, plain and under AddressSanitizer + UndefinedBehaviorSanitizer: the strip and row records of
k_resize2 (csrc/resize_window.inc: resize2_records, the builder orbx_create calls) over image sizes 64 ... 1 300, scale factors 1.01 ... 1.3 and
2 ... 8 levels — every record against its definition from resize_coef, and the kernel's walk of every strip from the records alone: every source
row it asks for inside the strip, every destination row emitted once behind its second tap.  Host code only; the program links no library."""
from cpp_harness import build_and_run


def test_resize_rows_plain(tmp_path):
    build_and_run(["resize_rows_test.cpp"], "plain", tmp_path, "resize_rows_test OK", include_dirs=(), flags=("-Wall", "-Wextra"))


def test_resize_rows_under_asan_ubsan(tmp_path):
    out = build_and_run(["resize_rows_test.cpp"], "san", tmp_path, "resize_rows_test OK", include_dirs=(),
                        flags=("-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    assert "ERROR: AddressSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr
