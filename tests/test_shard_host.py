"""The host half of the shard exchange (rtxpt_amd/csrc/pt_shard_host.cpp: the shard layout, the schedule of who sends what to whom, and the exchange over host memory and
a caller's transport), CPU only: tests/shard_exchange_check.cpp runs the ranks as threads over a rendezvous transport — a send returns only when the matching receive has
taken the bytes — and checks, for both routes and planes of 4, 8 and 16 bytes per pixel: the planes every rank ends up with, that a rank sends exactly its own bytes once per
receiver, the group calls of rank 0 of a gather, and the schedule's offsets and pairs. A deadlock ends the checker after a fixed wall time with exit code 2."""
import os, subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shard") / "shard_exchange_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", os.path.join(HERE, "shard_exchange_check.cpp"), os.path.join(ROOT, "rtxpt_amd", "csrc", "pt_shard_host.cpp"), "-o", exe], check=True)
    return exe


# partial tiles on both axes; 70 x 45 has six tiles, so two ranks of a world of 8 own nothing
@pytest.mark.parametrize("size", [(70, 45), (97, 61)])
@pytest.mark.parametrize("world", [1, 2, 3, 5, 8])
def test_exchange_over_a_rendezvous_transport(checker, size, world):
    r = subprocess.run([checker, str(size[0]), str(size[1]), str(world)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), "exit %d\n%s%s" % (r.returncode, r.stdout, r.stderr)
    if size == (70, 45) and world == 8:
        assert r.stdout.strip().endswith("2 ranks own nothing")
