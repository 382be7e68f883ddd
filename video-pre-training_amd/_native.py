"""ctypes binding of libvpt_hip.so, derived from the header that declares its C ABI.

load() reads include/vpt_hip.h once per process and types EVERY function it declares (argtypes and restype) on both
libraries: there is no second copy of a signature to keep in step.  The parser is strict -- a declaration it cannot read is
an error that names it, never a skipped or guessed binding.  tests/golden/abi_signatures.json pins what was bound.

The library is built in-tree by build.py.  There is NO fallback: if it cannot be loaded every op raises.
"""
import collections
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
_HEADER_PATH = os.path.join(_HERE, "..", "include", "vpt_hip.h")
_LIB_PATH = os.environ.get("VPT_HIP_LIB") or os.path.join(_HERE, "libvpt_hip.so")   # VPT_HIP_LIB: profiling builds (tools/)
# one library per 16-bit operand format (vpt_operand_format()): same sources, same ABI
_LIB_PATHS = {"bf16": _LIB_PATH, "fp16": os.path.join(_HERE, "libvpt_hip_f16.so")}
_libs = {}
_header = None

ABI_VERSION = 5      # VPT_HIP_ABI of the include/vpt_hip.h that ops.py's positional call sites were written against

# the scalar types a declaration may use (closed: anything else is an error); every `*` argument is a c_void_p
_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
            "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
# identification: mandatory even in a VPT_HIP_LIB override build
_IDENTIFICATION = ("vpt_version", "vpt_abi_version", "vpt_operand_format", "vpt_last_error")

Header = collections.namedtuple("Header", "abi functions workspace_ops")   # functions: name -> (restype, [argtypes]); workspace_ops: VPT_WS_* -> int


class NativeLibraryError(RuntimeError):
    pass


def parse_header(text: str) -> Header:
    """The C ABI a header text declares: VPT_HIP_ABI, every `ret vpt_name(args);` and the VPT_WS_* enum."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"^[ \t]*#[ \t]*define[ \t]+VPT_HIP_ABI[ \t]+(\d+)[ \t]*$", text, flags=re.M)
    if not m:
        raise NativeLibraryError("the header does not define VPT_HIP_ABI")
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)                      # preprocessor lines
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    *statements, tail = text.split(";")
    if tail.strip():
        raise NativeLibraryError(f"cannot read the declaration `{' '.join(tail.split())}`: no terminating `;`")
    functions, workspace_ops = {}, {}
    for decl in (" ".join(s.split()) for s in statements):
        enum = re.fullmatch(r"enum \{(.*)\}", decl)
        if enum:
            for item in enum.group(1).split(","):
                m_item = re.fullmatch(r"\s*(VPT_WS_\w+) ?= ?(\d+)\s*", item)
                if not m_item:
                    raise NativeLibraryError(f"cannot read the enumerator `{item.strip()}` of `{decl}`")
                workspace_ops[m_item.group(1)] = int(m_item.group(2))
            continue
        fn = re.fullmatch(r"(const char ?\*|\w+) ?(vpt_\w+) ?\(([^()]*)\)", decl)
        if not fn:
            raise NativeLibraryError(f"cannot read the declaration `{decl}`")
        ret, name, args = fn.groups()
        if name in functions:
            raise NativeLibraryError(f"`{decl}` declares {name} a second time")
        restype = ctypes.c_char_p if "*" in ret else _SCALARS.get(ret)
        argtypes = []
        for arg in ([] if args.strip() in ("", "void") else args.split(",")):
            scalar = re.fullmatch(r"\s*(\w+) \w+\s*", arg)
            argtypes.append(ctypes.c_void_p if "*" in arg else _SCALARS.get(scalar.group(1)) if scalar else None)
        if restype is None or None in argtypes:
            raise NativeLibraryError(f"cannot type the declaration `{decl}`: scalar types are {', '.join(_SCALARS)}")
        functions[name] = (restype, argtypes)
    return Header(int(m.group(1)), functions, workspace_ops)


def header() -> Header:
    """include/vpt_hip.h (it travels with the package tree), parsed once per process."""
    global _header
    if _header is None:
        try:
            with open(_HEADER_PATH) as f:
                text = f.read()
        except OSError as e:
            raise NativeLibraryError(f"{_HEADER_PATH}: the header the binding is derived from cannot be read ({e})")
        _header = parse_header(text)
    return _header


def lib_path():
    return _LIB_PATH


def load(fmt: str = "bf16"):
    """Load (once) and type the shared library for one operand format.  Raises NativeLibraryError if it is missing."""
    if fmt in _libs:
        return _libs[fmt]
    # PyTorch-ROCm ships its own libamdhip64.so; load it FIRST so that libvpt_hip.so binds to the same HIP
    # runtime instance torch uses (two runtimes in one process cannot share streams or device pointers).
    import torch  # noqa: F401
    path = _LIB_PATHS[fmt]
    if not os.path.exists(path):
        raise NativeLibraryError(
            f"{path} is missing: run `python __graft_entry__.py` (build()) first; there is no CPU fallback")
    hdr = header()
    lib = ctypes.CDLL(path)
    try:
        lib.vpt_abi_version.restype = ctypes.c_int
        abi = int(lib.vpt_abi_version())
    except AttributeError:
        abi = None
    if abi != ABI_VERSION:      # a stale .so would take a stream handle for a flag pointer, etc.: refuse before the first call
        raise NativeLibraryError(f"{path} has C-ABI version {abi}, this package binds version {ABI_VERSION}: rebuild it (`python __graft_entry__.py`)")
    if hdr.abi != ABI_VERSION:
        raise NativeLibraryError(f"{_HEADER_PATH} declares C-ABI version {hdr.abi}, this package binds version {ABI_VERSION}")
    override = fmt == "bf16" and bool(os.environ.get("VPT_HIP_LIB"))
    for name, (restype, argtypes) in hdr.functions.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            # only an A/B reference build named by VPT_HIP_LIB (tools/build_ref_lib.sh: an OLDER revision of the same ABI) may lack entry points
            # added since -- calling one raises below; the in-tree library must export every symbol
            if override and name not in _IDENTIFICATION:
                continue
            raise NativeLibraryError(f"{path} does not export {name}: rebuild it (`python __graft_entry__.py`)")
        fn.argtypes, fn.restype = argtypes, restype
    if lib.vpt_operand_format().decode() != fmt:
        raise NativeLibraryError(f"{path} reports operand format {lib.vpt_operand_format().decode()}, expected {fmt}")
    _libs[fmt] = lib
    return lib


def call(name, *args, fmt: str = "bf16"):
    lib = load(fmt)
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed: {lib.vpt_last_error().decode()}")


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())
