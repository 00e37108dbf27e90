"""The C-ABI library loads and exports every symbol include/orbhip.h declares (no compute calls, no GPU)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header(name="orbhip.h"):
    """the header without its comments"""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def _declarations(name="orbhip.h", prefixes="orbx|orbm|orbf|lba|liba|orb|pose|bow|bowdb"):
    """{function: parameter count} of every function the header declares"""
    found = re.findall(r"\b((?:%s)_[a-z0-9_]+)\s*\(([^()]*)\)\s*;" % prefixes, _header(name))
    return {fn: 0 if params.strip() == "void" else params.count(",") + 1 for fn, params in found}


def _declared():
    return sorted(_declarations())


def _probe(tmp_path):
    """Compiles a C program generated from the mirrors' own field names (a name the header lacks does not compile) and returns what it prints:
    {struct: [sizeof, offsetof of every field in the mirror's order]}, {macro: value}."""
    from orbhip import _abi
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "orbhip.h"\nint main(void) {\n'
    for s, rec in _abi.RECORDS.items():
        src += 'printf("S %s %%zu", sizeof(%s));' % (s, s) + "".join('printf(" %%zu", offsetof(%s, %s));' % (s, f) for f in _fields(rec)) + \
               'printf("\\n");\n'
    for m in _abi.MACROS:
        src += 'printf("M %s %%lld\\n", (long long)(%s));\n' % (m, m)
    src += "return 0; }\n"
    (tmp_path / "probe.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")])
    structs, macros = {}, {}
    for ln in subprocess.check_output([str(tmp_path / "probe")], text=True).splitlines():
        kind, name, *vals = ln.split()
        (structs if kind == "S" else macros)[name] = [int(v) for v in vals]
    return structs, macros


def _fields(rec):
    return list(rec.names) if isinstance(rec, np.dtype) else [n for n, _ in rec._fields_]


def _layout(rec):
    if isinstance(rec, np.dtype):
        return [rec.itemsize] + [rec.fields[f][1] for f in rec.names]
    return [ctypes.sizeof(rec)] + [getattr(rec, f).offset for f in _fields(rec)]


def test_header_declares_entry_points():
    names = _declared()
    assert "orbx_create" in names and "orbx_extract" in names and "orbx_extract_batch_dev" in names


def test_records_and_macros_match_the_header(tmp_path):
    """every struct of include/orbhip.h has a mirror in _abi.RECORDS with the same size and the same offset of every field, and every macro the
    value _abi.MACROS gives it (sizes, offsets and values from a compiled probe)"""
    from orbhip import _abi
    hdr = _header()
    assert sorted(_abi.RECORDS) == sorted(re.findall(r"typedef\s+struct\s+(\w+)\s*\{", hdr))
    assert sorted(_abi.MACROS) == sorted(m for m in re.findall(r"#define\s+(\w+)\s+\S", hdr) if m != "ORBHIP_H")
    structs, macros = _probe(tmp_path)
    for s, rec in _abi.RECORDS.items():
        assert structs[s] == _layout(rec), s
    for m, value in _abi.MACROS.items():
        assert macros[m] == [value], m
    assert _abi.REFRESH_MAX_OBS >= 1024
    assert [_abi.OBS_RIGHT, _abi.OBS_KF_BAD, _abi.REFRESH_DESCRIPTOR, _abi.REFRESH_NORMAL_DEPTH, _abi.REFRESHED_DESCRIPTOR,
            _abi.REFRESHED_NORMAL_DEPTH, _abi.REFRESH_OVERFLOW, _abi.REFRESH_BAD_RECORD] == [1, 2, 1, 2, 1, 2, 4, 8]


@pytest.mark.parametrize("header, table, prefixes", [("orbhip.h", "PROTOTYPES", "orbx|orbm|orbf|lba|liba|orb|pose|bow|bowdb"),
                                                     ("orbd.h", "ORBD_PROTOTYPES", "orbd")], ids=["orbhip.h", "orbd.h"])
def test_prototypes_match_the_header(header, table, prefixes):
    """every function the header declares has a prototype in the table and the other way round, with the declaration's parameter count"""
    from orbhip import _abi
    declared, protos = _declarations(header, prefixes), getattr(_abi, table)
    assert sorted(protos) == sorted(declared)
    assert {fn: len(argtypes) for fn, (_, argtypes) in protos.items()} == declared


def test_bind_applies_the_prototypes_once():
    """_lib.bind sets every prototype of the table on a library object and leaves an already bound one alone"""
    from orbhip import _abi, _lib

    class Fn:
        restype = argtypes = "unset"

    class Lib:
        def __init__(self):
            for name in _abi.PROTOTYPES:
                setattr(self, name, Fn())
    lib = _lib.bind(Lib())
    assert all((getattr(lib, n).restype, getattr(lib, n).argtypes) == p for n, p in _abi.PROTOTYPES.items())
    lib.orbx_create.argtypes = "mine"
    assert _lib.bind(lib) is lib and lib.orbx_create.argtypes == "mine"


def test_product_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    so = os.path.join(ROOT, "awesome-orb-slam3-3dvisioncraft-version_amd", "liborbhip.so")
    if not os.path.exists(so):
        ge.build()
    lib = ctypes.CDLL(so)  # loads without a GPU (libamdhip64 is in the image)
    missing = [n for n in _declared() if not hasattr(lib, n)]
    assert not missing, missing


def test_hint_entry_points_reject_unknown_bits():
    """lba_build_system_hint / pose_optimize_hint validate the hint word before anything else (argument check only: no GPU work)."""
    lib = ctypes.CDLL(os.path.join(ROOT, "awesome-orb-slam3-3dvisioncraft-version_amd", "liborbhip.so"))
    lib.lba_build_system_hint.restype = ctypes.c_int
    lib.lba_build_system_hint.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]
    assert lib.lba_build_system_hint(None, 1, None, 8, None) == -3          # ORB_E_INVALID: unknown hint bit
    assert lib.lba_build_system_hint(None, 1, None, 1, None) == -3          # known hint, null problem: the ordinary argument check
    lib.pose_optimize_hint.restype = ctypes.c_int
    lib.pose_optimize_hint.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 2 + [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 3 + [ctypes.c_uint, ctypes.c_void_p]
    assert lib.pose_optimize_hint(None, None, None, 1, 1, None, 1, None, None, None, 1, None) == -3   # LBA_HINT_MONO_PINHOLE is not a pose_optimize hint


def test_loader_has_no_cpu_fallback(tmp_path, monkeypatch):
    from orbhip import _lib
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    monkeypatch.setattr(_lib, "_lib", None)
    with pytest.raises(_lib.OrbHipError):
        _lib.load()
