"""CPU: the buffer-argument check of the record-set calls (csrc/operands.h).

tests/operand_check.cpp, a stand-alone program over the header, built plainly and with AddressSanitizer + UndefinedBehaviorSanitizer (an
executable of its own: nothing is preloaded): required, optional, dead and unknown names; every pair of equal names; exact fits and one byte
short at rows of 16, 96 and 1024 bytes; 2^64 - 1 rows; byte-count operands; empty buffers; and that the operand reported is the one made bad.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=("plain", "asan_ubsan"))
def check_program(request, tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no C++ compiler")
    exe = tmp_path_factory.mktemp("operand_check") / "operand_check"
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "asan_ubsan" else []
    cc_ = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", *san, os.path.join(ROOT, "tests", "operand_check.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr[-3000:]
    return str(exe)


def test_the_operand_check(check_program):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([check_program], capture_output=True, text=True, timeout=60, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    m = re.search(r"^(\d+) cases, 0 failed$", r.stdout, re.M)
    assert m and int(m.group(1)) >= 70, r.stdout[-500:]
    assert "FAILED" not in r.stdout
