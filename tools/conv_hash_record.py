"""Record the expected hashes of tests/test_gpu_conv_fwd_bitwise.py, tests/test_gpu_conv_dgrad_bitwise.py and tests/test_gpu_attention_bitwise.py from a
pair of REFERENCE libraries (the parent commit's builds of libvpt_hip.so and libvpt_hip_f16.so by build.py, copied aside before the kernel is changed;
tools/build_ref_lib.sh serves the convolutions only: it omits the per-source flags the attention backward is built with, and the fp16 library):

    python tools/conv_hash_record.py <reference bf16 .so> <reference fp16 .so> [forward out.json [dgrad out.json [attention out.json]]]

Writes {format: {case: {tag: sha256}}} per test (default: tests/golden/conv3x3_fwd_hashes.json, tests/golden/conv3x3_dgrad_hashes.json,
tests/golden/attention_hashes.json); the tests then hold the working tree's libraries to those bits.  Every case is computed twice and must hash the same both times.  Needs an MI355X."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if len(sys.argv) < 3:
    raise SystemExit(__doc__)
os.environ["VPT_HIP_LIB"] = os.path.abspath(sys.argv[1])     # read when vpt_amd._native is imported
import vpt_amd  # noqa: E402,F401
from vpt_amd import _native  # noqa: E402

_native._LIB_PATHS["fp16"] = os.path.abspath(sys.argv[2])
assert not _native._libs, "a library was loaded before the reference paths were set"
from tests import test_gpu_attention_bitwise as TA  # noqa: E402
from tests import test_gpu_conv_dgrad_bitwise as TD  # noqa: E402
from tests import test_gpu_conv_fwd_bitwise as T  # noqa: E402


def record(mod, path):
    out = {}
    for fmt in ("bf16", "fp16"):
        out[fmt] = {}
        for name in mod.CASES:
            a, b = mod.case_hashes(name, fmt), mod.case_hashes(name, fmt)
            if a != b:
                raise SystemExit(f"{name} {fmt}: two runs of the same library disagree: {[k for k in a if a[k] != b[k]]}")
            out[fmt][name] = a
            print(fmt, name, {k: v[:12] for k, v in a.items()})
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


def main():
    print("reference libraries:", _native._LIB_PATHS)
    record(T, sys.argv[3] if len(sys.argv) > 3 else T.GOLDEN)
    record(TD, sys.argv[4] if len(sys.argv) > 4 else TD.GOLDEN)
    record(TA, sys.argv[5] if len(sys.argv) > 5 else TA.GOLDEN)


if __name__ == "__main__":
    main()
