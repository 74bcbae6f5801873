"""The exact quotients of the chunked engine's walk arithmetic (openwhisk_amd/csrc/owgs_divq.h), checked
on the host: the header is plain C++, so a stand-alone program (its own main, no device, no
library; tests/divq_check.cpp) compares it with the integer / and %.

Capacity: every memory limit in 1..131,071, every multiple boundary (k * mem - 1, k * mem, k * mem + 1, and the middle
of each interval) below 2^22, negative operands, the CAPMAX clamp; operands of 2^22 and more with the clamp (exact up to
a limit of 4,095 MB, not at 4,096); and a counter-example of the bare quotient at 2^23 or above, which documents why the
engine bounds its permits.  Position: every pool size in 2..32,767 at the boundaries of a strided set of multiples with
the first and the last below 2^31, 2^31 - 1 itself, and four million seeded random operands.  About 230 M points, a
second or two.  The same program runs once more under -fsanitize=undefined.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "divq_check.cpp")
INC = os.path.join(ROOT, "openwhisk_amd", "csrc")


def _cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no C++ compiler found for the stand-alone check")


@pytest.fixture(scope="module")
def build_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("divq")


def _run(build_dir, name, flags):
    exe = os.path.join(str(build_dir), name)
    subprocess.run([_cxx(), "-std=c++17", "-Wall", "-I", INC, *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


def test_exact_quotients(build_dir):
    out = _run(build_dir, "divq_check", ["-O2", "-ffp-contract=off"])
    assert out[-1] == "OK"
    cap = next(x for x in out if x.startswith("capacity:"))
    assert cap.endswith("0 mismatches") and int(cap.split()[1]) > 150_000_000  # every boundary below 2^22
    assert any(x.startswith("clamped capacity:") and "exact up to mem 4095, not at 4096" in x for x in out)
    assert any(x.startswith("beyond: first mismatch at x=") for x in out)  # the bare form fails from 2^23 on
    pos = next(x for x in out if x.startswith("position:"))
    assert pos.endswith("0 mismatches") and int(pos.split()[1]) > 10_000_000
    sm = next(x for x in out if x.startswith("small remainder:"))  # (reciprocals up to 2 ulp off)
    assert sm.endswith("0 mismatches") and int(sm.split()[2]) > 5_000_000


def test_exact_quotients_ubsan(build_dir):
    out = _run(build_dir, "divq_check_ub", ["-O1", "-g", "-ffp-contract=off", "-fsanitize=undefined",
                                            "-fno-sanitize-recover=undefined"])
    assert out[-1] == "OK"
