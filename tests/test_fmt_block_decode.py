"""The FMT GEMM's block decode without run-time division (csrc/fmt_decode.hpp) is the same map as the formula with / and % it
replaces, for every workgroup id of every launch shape, and a bijection onto the tiles.  Runs on the CPU: a stand-alone host
program (tests/fmt_block_decode_main.cpp) built with the host compiler, under AddressSanitizer and UBSan where it has them."""
import os
import shutil
import subprocess

import pytest

from tests.util import PKG_DIR, ROOT

SRC = os.path.join(ROOT, "tests", "fmt_block_decode_main.cpp")


def _compiler():
    for c in ("c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    return None


@pytest.fixture(scope="module")
def decode_check(tmp_path_factory):
    cxx = _compiler()
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("fmt_decode") / "decode_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", os.path.join(PKG_DIR, "csrc"), SRC, "-o", exe]
    p = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if p.returncode != 0:  # a compiler without the sanitizer runtimes: the comparison itself still runs
        p = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return exe


def test_block_decode_matches_definition(decode_check):
    """All ids of (column blocks 1..72 and the models' widths, also not a multiple of 8) x (row blocks 1..12 and the stacked
    clips') x (ksplit 1, 2, 3, 4, 8) x (EPI_PARTIAL or not): new decode == old formula, in range, each tile exactly once."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")
    p = subprocess.run([decode_check], capture_output=True, text=True, timeout=300, env=env)
    print(p.stdout)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok: ")
