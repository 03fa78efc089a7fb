"""The launch plan of the BVH8 traversal launches (rtxpt_amd/csrc/pt_trace_plan.h: rays per chunk, the grid bound, a launch's grid, the visibility resolve's grid, two or
four task rounds, and the fused launch's split of its grid between closest-hit and visibility blocks), CPU only: tests/trace_plan_check.cpp includes the header the
launchers call and holds it to its invariants over nineteen extend counts x nineteen shadow counts x eight grid bounds — the fused launch's precondition (a bound of at
least 2) included, counts from 0 to 4 x 10^7 and on both sides of every threshold.

The program is built with g++ twice, plainly and with -fsanitize=address,undefined, and run as a program of its own; nothing is loaded into Python. No GPU."""
import os, subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
COMBOS = 19 * 19 * 8


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("trace_plan") / ("trace_plan_check_" + request.param))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param == "sanitized" else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror"] + flags + [os.path.join(HERE, "trace_plan_check.cpp"), "-o", exe], check=True)
    return exe


def test_launch_plan_holds_its_invariants(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok combos %d" % COMBOS, "exit %d\n%s%s" % (r.returncode, r.stdout, r.stderr)
