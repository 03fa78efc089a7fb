"""The "inert when terminal" predicate (rtxpt_amd/csrc/pt_scene.h: inert_bits_of, inert_word, inert_bits_at, inert_when_terminal — what k_inert_bits builds and k_classify reads
before it leaves a terminating hit out of k_shade), CPU only: tests/inert_terminal_check.hip runs the product's own text on the host under AddressSanitizer and
UndefinedBehaviorSanitizer, and its output is held to the numpy restatement of tests/inert_terminal_cases.py, computed from the scene description alone. The device's table is held
to the same restatement in tests/test_gpu_inert_terminal.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

import inert_terminal_cases as itc      # noqa: E402
from rtxpt_amd import scenes            # noqa: E402


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inert") / "inert_terminal_check")
    csrc = os.path.join(ROOT, "rtxpt_amd", "csrc")
    # PT_ALPHA_LUT=0: the header's k / 255 table is a __constant__ object of the device (as in tests/test_texture_sampling.py)
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-DPT_ALPHA_LUT=0", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + csrc, os.path.join(HERE, "inert_terminal_check.hip"), "-o", exe], check=True)
    return exe


def _run(checker, tmp_path, materials, prim_material):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    materials = np.ascontiguousarray(materials); prim_material = np.ascontiguousarray(prim_material, np.uint32)
    with open(src, "wb") as f:
        f.write(np.uint32([len(materials), len(prim_material)]).tobytes()); f.write(materials.tobytes()); f.write(prim_material.tobytes())
    r = subprocess.run([checker, src, dst], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
    assert int(r.stdout.split()[1]) == (len(prim_material) + 15) // 16
    return np.fromfile(dst, np.uint8).reshape(len(prim_material), 4)


def _hold(out, materials, prim_material):
    bits = itc.material_bits(materials)[prim_material]
    assert np.array_equal(out[:, 0], bits)
    for q in (0, 1, 2): assert np.array_equal(out[:, 1 + q].astype(bool), itc.inert(bits, q)), "quality %d" % q


def test_zoo_scene_classes(checker, tmp_path):
    """every kind of surface of the GPU test's scene, by instance: which of them a terminating hit may be dropped on, per nested-dielectric quality"""
    sc, _ = itc.zoo()
    pm = itc.prim_materials(sc); out = _run(checker, tmp_path, sc["materials"], pm)
    _hold(out, sc["materials"], pm)
    assert len(pm) == 12 + 12 + 12 + 2 + 2
    first = {"walls": 0, "light": 10, "glass": 12, "proxy": 24, "card": 36, "tiny": 38}
    want = {"walls": (3, 1, 1, 1), "light": (2, 0, 0, 0), "glass": (1, 1, 0, 0), "proxy": (2, 0, 0, 0), "card": (3, 1, 1, 1), "tiny": (2, 0, 0, 0)}
    for name, p in first.items(): assert tuple(int(v) for v in out[p]) == want[name], (name, out[p])
    # the same materials without the flag / the link: the flag alone decides (the link is re-baked with the lights, the table does not wait for it)
    sc2, _ = itc.zoo(proxy_link=False)
    assert np.array_equal(_run(checker, tmp_path, sc2["materials"], itc.prim_materials(sc2)), out)
    sc3 = itc.all_emissive(sc)
    out3 = _run(checker, tmp_path, sc3["materials"], pm); _hold(out3, sc3["materials"], pm)
    assert not out3[:, 1:].any()


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 33, 1000])
def test_random_materials_and_word_boundaries(checker, tmp_path, n):
    """colours that are zero, minus zero, denormal, below the binary16 range, negative, infinite and NaN in any component; primitive counts around the sixteen of a word"""
    rng = np.random.default_rng(100 + n)
    vals = np.array([0.0, -0.0, 1e-45, 1e-9, 5.9e-8, 6.2e-5, 1.0, -1.0, np.inf, np.nan], np.float32)
    m = np.zeros(64, scenes.MATERIAL_DTYPE)
    e = np.zeros((64, 3), np.float32); pick = rng.random((64, 3)) < 0.25; e[pick] = vals[rng.integers(0, len(vals), int(pick.sum()))]
    m["EmissiveColor"] = e
    m["Flags"] = rng.integers(0, 1 << 32, 64, dtype=np.uint64).astype(np.uint32) & np.uint32(0xF0001FBD | itc.MF_PROXY | itc.MF_THIN)
    m["Flags"][::3] &= ~np.uint32(itc.MF_PROXY)
    pm = rng.integers(0, 64, n).astype(np.uint32)
    out = _run(checker, tmp_path, m, pm); _hold(out, m, pm)
    if n >= 1000: assert 0 < out[:, 1].sum() < n and out[:, 3].sum() < out[:, 1].sum()
