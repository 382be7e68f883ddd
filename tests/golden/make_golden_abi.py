"""The ctypes binding of every function include/vpt_hip.h declares, as _native.py derives it from the header (no library and no
GPU needed):   python tests/golden/make_golden_abi.py   -> tests/golden/abi_signatures.json
One line per function, in the header's order: name -> restype and argtypes as ctypes class names, plus "abi" = VPT_HIP_ABI.
tests/test_native_abi.py holds the parsed binding to this file type by type.  The file was first written from what the hand-kept
signature table bound (the four identification functions, whose argtypes it never set, recorded as []), and the parser reproduced it with no
type difference.  Regenerate it after ADDING an entry
point (a new line); a diff that alters or removes an existing line changes the binary interface and needs a raised VPT_HIP_ABI."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
PATH = os.path.join(HERE, "abi_signatures.json")


def signatures(header) -> dict:
    """{name: {"restype": ..., "argtypes": [...]}} of a parsed header (_native.Header), ctypes classes by __name__."""
    return {name: {"restype": restype.__name__, "argtypes": [t.__name__ for t in argtypes]} for name, (restype, argtypes) in header.functions.items()}


def main():
    import vpt_amd  # noqa: F401
    from vpt_amd import _native
    hdr = _native.header()
    lines = ",\n".join(f"  {json.dumps(name)}: {json.dumps(rec)}" for name, rec in signatures(hdr).items())
    with open(PATH, "w") as f:
        f.write("{\n \"abi\": %d,\n \"functions\": {\n%s\n }\n}\n" % (hdr.abi, lines))
    print(f"wrote {os.path.basename(PATH)}: {len(hdr.functions)} functions, ABI {hdr.abi}")


if __name__ == "__main__":
    main()
