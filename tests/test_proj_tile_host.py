"""CPU: the integer maps of a wave's stage of projected records (csrc/proj_tile.h).

tests/proj_tile_check.cpp, a stand-alone program over the header's plain part, built plainly and with AddressSanitizer + UndefinedBehaviorSanitizer
(an executable of its own: nothing is preloaded): for have = 0 .. 64 records of a wave and both pitches of the stage (records back to back, and five
pieces apart) the pieces the 64 lanes store are exactly [0, 4 have), each once; every slot read was put by a lane with a record; no two records share
a slot; piece j goes to byte 16 j of the wave's range and is piece j % 4 of record j / 4; wave_have at the ends of a segment and of 32 bits.
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
    exe = tmp_path_factory.mktemp("proj_tile_check") / "proj_tile_check"
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "asan_ubsan" else []
    cc_ = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", *san, os.path.join(ROOT, "tests", "proj_tile_check.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr[-3000:]
    return str(exe)


def test_the_proj_tile_check(check_program):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([check_program], capture_output=True, text=True, timeout=60, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    m = re.search(r"^(\d+) cases, 0 failed$", r.stdout, re.M)
    assert m and int(m.group(1)) >= 2 * 65 * 6, r.stdout[-500:]
    assert "FAILED" not in r.stdout
