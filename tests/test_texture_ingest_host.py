"""The texture ingest's arithmetic without a device: tests/texture_ingest_ref.py (the float32 numpy restatement the GPU tests hold both upload paths to) against the float64
chain of tests/texture_ref.py within that file's derived bound, the claim that every 8-bit opacity makes a byte plane, and rtxpt_amd/csrc/pt_texture_ingest.h itself — the
text both paths run — compiled into a stand-alone host program (tests/texture_ingest_check.cpp, under the address and undefined-behaviour sanitizers) whose digests of every
level, plane and table equal the restatement's."""
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import texture_cases as tc
import texture_ref as tr
import texture_ingest_ref as ti
from test_texture_sampling import dm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def all_textures():
    return list(tc.zoo()[1]) + list(ti.ingest_set().texs)


def test_float32_chain_is_within_the_derived_bound_of_the_float64_chain():
    """texture_ref.py: a texel of level L carries at most 2 L u M of box-filter rounding, the bound grants 3 L u M (u = 2^-24, M = the channel's largest |texel| of level 0).
    Level 0 is the same float32 array in both."""
    pw = dm(5); worst = 0.0
    for t in all_textures():
        l0 = ti.level0(t.pixels, t.upload, pw)
        assert np.array_equal(l0.view(np.uint32), tr.level0(t.pixels, t.upload, pow32=pw).view(np.uint32)), t.name
        m32, m64 = ti.chain(l0), tr.build_mips(l0)
        assert len(m32) == len(m64) == t.levels
        M = np.abs(m64[0]).reshape(-1, 4).max(0)
        for L, (a, b) in enumerate(zip(m32, m64)):
            assert a.shape == b.shape and a.dtype == np.float32
            err = np.abs(a.astype(np.float64) - b).reshape(-1, 4).max(0)
            if L == 0: assert (err == 0).all()
            else:
                assert (err <= 3.0 * L * tr.U24 * M).all(), (t.name, L, err, 3.0 * L * tr.U24 * M)
                worst = max(worst, float((err / (3.0 * L * tr.U24 * M)).max()))
    print("largest error / bound over all levels: %.3f" % worst)


def test_every_8_bit_opacity_makes_a_byte_plane():
    """What lets the device path skip the scan for 8-bit sources: (float)k / 255.0f satisfies the byte-plane predicate and gives k back, for all 256 values."""
    k = np.arange(256); a = (k.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    assert ti.alpha_is_byte(a).all() and np.array_equal(ti.alpha_byte(a), k)
    # and the predicate is no tautology: the neighbours of k / 255 in float32, and values outside [0, 1], fail it
    up, down = np.nextafter(a, np.float32(2.0)), np.nextafter(a, np.float32(-1.0))
    assert not ti.alpha_is_byte(up[1:-1]).any() and not ti.alpha_is_byte(down[1:-1]).any()
    assert not ti.alpha_is_byte(np.float32([-0.25, 1.25, np.nextafter(np.float32(1.0), np.float32(2.0))])).any()
    fmt, plane = ti.alpha_plane(np.dstack([np.zeros((16, 16, 3), np.float32), a.reshape(16, 16)]))
    assert fmt == 0 and np.array_equal(plane, k.astype(np.uint8))


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("texingest") / "texture_ingest_check")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-x", "hip", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "rtxpt_amd", "csrc"),
                    os.path.join(HERE, "texture_ingest_check.cpp"), "-o", exe, "-lz"], check=True)
    return exe


def test_the_header_on_the_host_equals_the_restatement(checker, tmp_path):
    texs = all_textures(); pw = dm(5)
    src = str(tmp_path / "in.bin")
    with open(src, "wb") as f:
        f.write(np.uint32([len(texs)]).tobytes())
        for t in texs:
            f.write(np.uint32([t.w, t.h, t.upload]).tobytes()); f.write(np.ascontiguousarray(t.pixels).tobytes())
    r = subprocess.run([checker, src], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().split("\n"); head = lines[0].split()
    assert len(lines) == 1 + len(texs)
    refs = [ti.chain(ti.level0(t.pixels, t.upload, pw)) for t in texs]
    planes = [ti.alpha_plane(m[0]) for m in refs]
    table, mat_texels, alpha_bytes = ti.layout([(t.w, t.h) for t in texs], [p[0] for p in planes])
    assert head[1] == "1"                                                        # all 256 byte values pass the header's predicate
    assert (int(head[2]), int(head[3])) == (mat_texels, alpha_bytes)
    kinds = set()
    for t, m, (fmt, plane), (base, offs, at), line in zip(texs, refs, planes, table, lines[1:]):
        got = [int(x) for x in line.split()]
        want = [base, len(m), at, fmt, ti.digest([l for l in m]), ti.digest([plane]), ti.digest([np.uint32(offs)])]
        assert got == want, (t.name, got, want)
        assert fmt == (0 if t.fmt in ("srgb8", "unorm8", "f32_alpha_bytes") else 1)
        kinds.add((t.upload, fmt))
    assert len(kinds) == 4                                                       # both 8-bit formats, float sources with byte planes and with float planes
