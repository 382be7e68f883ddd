"""The augmentation's per-pixel code under the host sanitizers (no GPU).

tools/augment_host_check.cpp is a stand-alone program around csrc/vpt_augment_pixel.h -- the very function vpt_augment_frames_kernel runs -- built as plain
C++ with contraction off and the address and undefined-behaviour sanitizers, on the host code only (the sanitizer option sits behind -Xarch_host).
It runs every pixel of four frame sizes, each frame in a heap block of exactly H * W * 3 bytes, under tables holding NaN, +-Inf, +-1e30 and denormals in every position and under random in-range tables.  Held here: the sanitizers report nothing (no
table contents make the code read outside its frame or convert an out-of-range float), and the outputs of the finite tables equal tests/augment_ref.py."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import augment_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc's clang (the build container)")


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("augment_host")
    exe, out = str(tmp / "augment_host_check"), str(tmp / "cases.bin")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "augment_host_check.cpp"), "-o", exe])
    blob = open(exe, "rb").read()
    assert b"__asan_init" in blob and b"__ubsan_handle" in blob          # the program really is instrumented
    p = subprocess.run([exe, out], capture_output=True, text=True, timeout=300)
    return p, out


def test_sanitizers_report_nothing(host_run):
    p, _ = host_run
    assert p.returncode == 0, p.stderr[-2000:]
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-2000:]
    assert "tables run" in p.stdout


def test_finite_tables_equal_the_restatement(host_run):
    p, path = host_run
    assert p.returncode == 0, p.stderr[-2000:]
    data = open(path, "rb").read()
    (count,), pos = struct.unpack_from("<i", data, 0), 4
    assert count >= 4 * (16 * 4 + 8)            # per size: +-1e30 and two denormals in 16 positions, 8 random tables
    sizes, special = set(), 0
    for _ in range(count):
        h, w = struct.unpack_from("<ii", data, pos)
        table = np.frombuffer(data, np.float32, 16, pos + 8)
        n = h * w * 3
        src = np.frombuffer(data, np.uint8, n, pos + 72).reshape(h, w, 3)
        out = np.frombuffer(data, np.uint8, n, pos + 72 + n).reshape(h, w, 3)
        pos += 72 + 2 * n
        assert np.isfinite(table).all()
        special += bool((np.abs(table) > 1e29).any() or ((table != 0) & (np.abs(table) < 1e-38)).any())
        sizes.add((h, w))
        assert np.array_equal(out, R.augment_frame_ref(src, table)), (h, w, table.tolist())
    assert pos == len(data) and sizes == {(5, 7), (16, 16), (33, 20), (128, 128)} and special >= 4 * 16 * 4
