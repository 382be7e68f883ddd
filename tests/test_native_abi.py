"""The C-ABI library builds, loads, and exports every symbol include/vpt_hip.h declares, and _native.py binds each of them with the types
the header gives it -- held to tests/golden/abi_signatures.json (no compute calls: this runs without a GPU)."""
import ctypes
import json
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    import vpt_amd
    from vpt_amd import _native
    return _native.load()


def test_header_symbols_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "vpt_hip.h")).read()
    names = re.findall(r"^(?:int|long|const char\*)\s+(vpt_\w+)\s*\(", hdr, flags=re.M)
    assert len(names) >= 11
    for n in names:
        assert hasattr(lib, n), n


def _fixture():
    with open(os.path.join(ROOT, "tests", "golden", "abi_signatures.json")) as f:
        return json.load(f)


def _native_module():
    import vpt_amd  # noqa: F401
    from vpt_amd import _native
    return _native


def test_parsed_binding_equals_the_recorded_one():
    """What _native.py derives from the header == tests/golden/abi_signatures.json for EVERY declared function, type by type (the file was first
    written from the hand-kept table the parser replaced).  From now on a change detector: a diff that alters an existing line of the JSON
    changes the binary interface and needs a raised VPT_HIP_ABI; a new entry point adds a line (tests/golden/make_golden_abi.py)."""
    from tests.golden.make_golden_abi import signatures
    hdr, fix = _native_module().header(), _fixture()
    parsed = signatures(hdr)
    assert len(parsed) >= 92
    assert sorted(parsed) == sorted(fix["functions"])           # the fixture covers every declared name and no other
    for name, rec in parsed.items():
        assert rec == fix["functions"][name], name
    assert fix["abi"] == hdr.abi == int(re.search(r"#define\s+VPT_HIP_ABI\s+(\d+)", open(os.path.join(ROOT, "include", "vpt_hip.h")).read()).group(1))


def test_both_libraries_carry_the_recorded_types(lib):
    _native, fix = _native_module(), _fixture()
    for handle in (lib, _native.load("fp16")):
        for name, rec in fix["functions"].items():
            fn = getattr(handle, name)
            assert fn.restype.__name__ == rec["restype"], name
            assert [t.__name__ for t in fn.argtypes] == rec["argtypes"], name


def test_no_function_keeps_the_default_restype_unless_the_header_says_int(lib):
    """ctypes' default restype is c_int: a size query left at it would be truncated above 2 GiB."""
    hdr = open(os.path.join(ROOT, "include", "vpt_hip.h")).read()
    declared = dict((n, r) for r, n in re.findall(r"^(int|long|int64_t|const char\*)\s+(vpt_\w+)\s*\(", hdr, flags=re.M))
    _native = _native_module()
    assert sorted(declared) == sorted(_native.header().functions)
    wide = {"long": ctypes.c_long, "int64_t": ctypes.c_int64, "const char*": ctypes.c_char_p}
    for handle in (lib, _native.load("fp16")):
        for name, ret in declared.items():
            fn = getattr(handle, name)
            if ret == "int":
                assert fn.restype is ctypes.c_int, name
            else:
                assert fn.restype is wide[ret] and ctypes.sizeof(fn.restype) == 8, name
    assert sum(r != "int" for r in declared.values()) >= 12


def test_workspace_enum_is_read_from_the_header():
    from vpt_amd import ops
    ws = _native_module().header().workspace_ops
    assert len(ws) == 14 and sorted(ws.values()) == list(range(1, 15))
    for name, value in ws.items():
        assert getattr(ops, name[len("VPT_"):]) == value, name


_ABI = "#define VPT_HIP_ABI 5\n"


def test_parser_reads_multi_line_declarations_and_ignores_comments():
    _native = _native_module()
    text = _ABI + """/* a comment with ; and ( in it: int vpt_not_declared(int x); */
    const char* vpt_name(void);
    int64_t vpt_bytes(int op,
                      int64_t n);
    int vpt_run(const float* x, void* y, /* in between ( ; */ uint8_t* flag,
                long n, float s, double d,
                uint32_t a, uint64_t b, void* stream);
    enum { VPT_WS_A = 1,
           VPT_WS_B = 2 };
    """
    hdr = _native.parse_header(text)
    P = ctypes.c_void_p
    assert hdr.abi == 5 and hdr.workspace_ops == {"VPT_WS_A": 1, "VPT_WS_B": 2}
    assert hdr.functions == {"vpt_name": (ctypes.c_char_p, []), "vpt_bytes": (ctypes.c_int64, [ctypes.c_int, ctypes.c_int64]),
                             "vpt_run": (ctypes.c_int, [P, P, P, ctypes.c_long, ctypes.c_float, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint64, P])}
    with pytest.raises(_native.NativeLibraryError, match="VPT_HIP_ABI"):
        _native.parse_header("int vpt_ok(int x);\n")


@pytest.mark.parametrize("decl, named", [
    ("int vpt_f(short x);", "vpt_f"),                                   # a scalar type outside the closed table
    ("int vpt_f(unsigned x);", "vpt_f"),
    ("int vpt_f(unsigned int x);", "vpt_f"),
    ("size_t vpt_f(int x);", "vpt_f"),                                  # ... as the return type
    ("float* vpt_f(int x);", "vpt_f"),                                  # only `const char*` may be returned by pointer
    ("int vpt_a(int x)\nint vpt_b(int y);", "vpt_a"),                   # a missing `;` must not merge two declarations
    ("int vpt_a(int x);\nint vpt_b(int y)", "vpt_b"),                   # ... nor drop the last one
    ("int vpt_a(int x);\nint vpt_a(long x);", "vpt_a"),
    ("int other_f(int x);", "other_f"),
    ("enum { VPT_WS_A = 1, VPT_WS_B };", "VPT_WS_B"),
])
def test_parser_raises_on_what_it_cannot_read(decl, named):
    _native = _native_module()
    with pytest.raises(_native.NativeLibraryError, match=named):
        _native.parse_header(_ABI + "int vpt_ok(int x);\n" + decl + "\n")


def test_version_and_error_strings(lib):
    assert b"gfx950" in lib.vpt_version()
    assert isinstance(lib.vpt_last_error(), bytes)


def test_abi_number_matches_header_and_binding(lib, monkeypatch):
    """vpt_abi_version() == VPT_HIP_ABI of the header == the number _native.py was written against; a library that reports another
    number (a stale build: argument lists differ) is refused at load time, before any call."""
    from vpt_amd import _native
    hdr = open(os.path.join(ROOT, "include", "vpt_hip.h")).read()
    abi_hdr = int(re.search(r"#define\s+VPT_HIP_ABI\s+(\d+)", hdr).group(1))
    assert lib.vpt_abi_version() == abi_hdr == _native.ABI_VERSION
    monkeypatch.setattr(_native, "_libs", {})
    monkeypatch.setattr(_native, "ABI_VERSION", abi_hdr + 1)
    with pytest.raises(_native.NativeLibraryError, match="C-ABI version"):
        _native.load("bf16")


def test_missing_library_fails_loudly(monkeypatch):
    import vpt_amd  # noqa: F401
    from vpt_amd import _native
    monkeypatch.setattr(_native, "_libs", {})
    monkeypatch.setattr(_native, "_LIB_PATHS", {"bf16": "/nonexistent/libvpt_hip.so", "fp16": "/nonexistent/libvpt_hip_f16.so"})
    for fmt in ("bf16", "fp16"):
        with pytest.raises(_native.NativeLibraryError):
            _native.load(fmt)


def test_both_operand_formats_built_with_the_same_abi(lib):
    """libvpt_hip_f16.so (precision="fp16") is the same sources built with -DVPT_OPERAND_F16: identical export list."""
    from vpt_amd import _native
    f16 = _native.load("fp16")
    assert lib.vpt_operand_format() == b"bf16" and f16.vpt_operand_format() == b"fp16"
    assert len(_native.header().functions) >= 92
    for name in _native.header().functions:
        assert hasattr(f16, name), name
