"""The opacity of a byte of an alpha plane (rtxpt_amd/csrc/pt_scene.h unorm8_to_float): k / 255 formed in registers — the product with the rounded reciprocal and one
correction step on the exact residual — must be the correctly rounded quotient (float)k / 255.0f for every byte, bit for bit: it is what the traversal's alpha test compares
with the cutoff, and the texture upload and the oracle form the quotient by division. CPU only: tests/unorm8_exact_check.cpp includes the header itself and walks all 256
bytes; it also counts the bytes for which the uncorrected product is wrong (126), so the correction step is known to be exercised.

The program is built with g++ twice, plainly and with -fsanitize=address,undefined, and run as a program of its own; nothing is loaded into Python. No GPU."""
import os, subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "rtxpt_amd", "csrc")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("unorm8") / ("unorm8_exact_check_" + request.param))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param == "sanitized" else []
    # (the header is written for hipcc: its clang pragmas and vector-type attributes are unknown to g++ and unused here)
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-Wno-attributes", "-Wno-misleading-indentation", "-I" + CSRC] + flags +
                   [os.path.join(HERE, "unorm8_exact_check.cpp"), "-o", exe], check=True)
    return exe


def test_every_byte_gives_the_correctly_rounded_quotient(checker):
    r = subprocess.run([checker], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok bytes 256 plain_product_wrong 126", "exit %d\n%s%s" % (r.returncode, r.stdout, r.stderr)
