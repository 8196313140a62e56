"""CPU: the host loop and the integer maps of the record tile (csrc/record_tile.h).

tests/record_tile_check.cpp, a stand-alone program over the header's plain part, built plainly and with AddressSanitizer +
UndefinedBehaviorSanitizer (an executable of its own: nothing is preloaded): the runs of launch_runs tile [0, groups) in order at max_grid 1 and 4,
at 2^32 - 1 groups and at 2^32 groups with the shipped max_grid; an error of the k-th launch ends the walk there and is returned; the staged walk
visits every piece of a tile of 1, 63, 64, 65, 255 and 256 records once, by a workgroup's threads and by a wave's lanes, and reads only slots that
a put wrote; pose's spans cover every tile once at a walk of 1 and of 4.
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
    exe = tmp_path_factory.mktemp("record_tile_check") / "record_tile_check"
    san = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "asan_ubsan" else []
    cc_ = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", *san, os.path.join(ROOT, "tests", "record_tile_check.cpp"), "-o", str(exe)],
                         capture_output=True, text=True)
    assert cc_.returncode == 0, cc_.stderr[-3000:]
    return str(exe)


def test_the_record_tile_check(check_program):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([check_program], capture_output=True, text=True, timeout=60, env=env)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    m = re.search(r"^(\d+) cases, 0 failed$", r.stdout, re.M)
    assert m and int(m.group(1)) >= 80, r.stdout[-500:]
    assert "FAILED" not in r.stdout
