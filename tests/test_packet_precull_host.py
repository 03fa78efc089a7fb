"""The packet's interval test of a BVH8 child (rtxpt_amd/csrc/pt_packet_precull.h, what traverse8_packets64 runs before the per-ray slab tests) on the HOST:
tests/packet_precull_check.cpp holds it against a plain restatement of t8_slab + T8_HIT over twelve million seeded (packet, child box) cases — random 8-bit boxes at scales
2^-20 .. 2^20, origins up to 1e6, best t from 0 to kMaxRayTravel, reciprocals that straddle zero or sit at ray_safe_rcp's clamp on one to three axes, origins on a plane of
the box, inverted (empty-slot) boxes, packets of one ray. The property: a child the interval test drops is a child no ray of the packet enters. Zero violations.

The program is built with -fsanitize=address,undefined and -ffp-contract=off and run as a program of its own; nothing is loaded into Python. No GPU."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = 12000000


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("packet_precull") / "packet_precull_check")
    subprocess.run([cxx, "-std=c++17", "-O2", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", os.path.join(HERE, "packet_precull_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(CASES)], capture_output=True, text=True)
    print(r.stdout); print(r.stderr)
    return r


def test_no_dropped_child_is_entered(report):
    assert report.returncode == 0, report.stdout[-2000:] + report.stderr[-2000:]
    m = re.search(r"cases (\d+) tested (\d+) dropped (\d+) violations (\d+) share_kept ([0-9.]+)", report.stdout)
    assert m, report.stdout[-2000:]
    cases, tested, dropped, violations = (int(m.group(k)) for k in range(1, 5))
    assert cases == CASES and cases >= 10 ** 7
    assert violations == 0
    # the property is not held vacuously: most cases have a test, and it drops and keeps children
    assert tested > cases // 3 and 0 < dropped < tested


def test_every_family_is_exercised(report):
    rows = re.findall(r"^(.+?)\s+cases\s+(\d+)\s+no test\s+(\d+)\s+kept\s+(\d+) \(entered by a ray\s+(\d+)\)\s+dropped\s+(\d+)\s+violations (\d+)$", report.stdout, re.M)
    assert len(rows) == 7, report.stdout[-2000:]
    for name, cases, no_test, kept, entered, dropped, violations in rows:
        assert int(violations) == 0, name
        assert int(cases) > 10 ** 6 and int(dropped) > 0 and int(entered) > 0, name      # (kept children that a ray does enter: the test is not dropping everything)
    straddle = [r for r in rows if r[0].startswith("reciprocals straddle zero")][0]
    assert int(straddle[2]) > int(straddle[1]) // 2      # mixed signs: mostly no test at all
