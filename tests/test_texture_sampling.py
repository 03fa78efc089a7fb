"""The texture samplers at non-power-of-two and thin sizes, CPU half: the oracle's sampler (oracle/ptref/scene.h — Texture::texel with a true `%`, build_mips, sample_bilinear,
sample_trilinear, sample_grad_anisotropic, and pathtracer.h's sampleTexture) against the float64 numpy restatement of tests/texture_ref.py on the whole zoo of
tests/texture_cases.py, within the bound derived there; invariants that need no tolerance; and the product's own host-and-device sampler text (rtxpt_amd/csrc/pt_scene.h,
alpha_test_slot with its byte and float alpha planes included) run on the host under the address and undefined-behaviour sanitizers and compared with the oracle row for row."""
import ctypes
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rtxpt_amd import scenes
from oracle import ptref
import texture_cases as tc
import texture_ref as tr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def dm(fn):
    """The project's float32 pow / log2 (pt_dmath.h through the oracle's library): inputs of the filter, not what is under test here."""
    L = ptref.lib()
    def call(x, y=None):
        x = np.ascontiguousarray(x, np.float32); y = np.ascontiguousarray(x if y is None else y, np.float32); out = np.zeros_like(x)
        L.ptref_dmath(fn, x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p), x.size, out.ctypes.data_as(ctypes.c_void_p))
        return out
    return call


@pytest.fixture(scope="module")
def oracle():
    sc, texs, quads = tc.zoo()
    o = ptref.Oracle(); o.set_scene(sc); o.set_settings(scenes.default_settings()); o.resize(8, 8)
    return o


@pytest.fixture(scope="module")
def mips():
    """The float64 mip chains of the zoo, built once."""
    pw = dm(5)
    return [tr.build_mips(tr.level0(t.pixels, t.upload, pow32=pw)) for t in tc.zoo()[1]]


def reference(t, m, rows):
    """texture_ref on probe rows of one texture: (values float64 [n, 4], bound [n, 4])."""
    val = np.zeros((len(rows), 4)); deep = np.zeros(len(rows), np.int64)
    f = lambda c: rows[:, c].copy().view(np.float32)
    k = rows[:, 0] == 0
    if k.any(): val[k], deep[k] = tr.sample_texture(m, t.word, f(4)[k], f(2)[k], f(3)[k])
    k = rows[:, 0] == 1
    if k.any(): val[k] = tr.bilinear(m, rows[k, 4].astype(np.int64), f(2)[k], f(3)[k]); deep[k] = rows[k, 4]
    k = rows[:, 0] == 2
    if k.any(): val[k], deep[k] = tr.anisotropic(m, f(2)[k], f(3)[k], np.stack([f(4), f(5)], 1)[k], np.stack([f(6), f(7)], 1)[k], log2_32=dm(3))[:2]
    return val, tr.bound(m, deep)


def worst_ratio(got, t, m, rows):
    """The largest |got - ref64| / bound over the rows, and the row and channel it is at."""
    ref, bnd = reference(t, m, rows)
    ratio = np.abs(got.astype(np.float64) - ref) / bnd
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    return float(ratio[i]), i


def check_against_reference(probe, mips, who, far=False):
    sc, texs, quads = tc.zoo(); bad = []
    for t in texs:
        rows = tc.far_rows(t) if far else tc.near_rows(t)
        if not len(rows): continue
        assert len(rows) <= 4500                                 # a few thousand rows per texture, every one compared
        got = probe(rows)
        assert np.isfinite(got).all(), t.name
        worst, (i, c) = worst_ratio(got, t, mips[t.index], rows)
        print("%s %-26s %5d rows, largest error / bound %.3f (row %d mode %d channel %d)" % (who, t.name, len(rows), worst, i, rows[i, 0], c))
        if not worst <= 1.0: bad.append((t.name, worst, rows[i].tolist()))
    assert not bad, bad


def test_oracle_sampler_is_within_the_derived_bound_of_the_float64_restatement(oracle, mips):
    check_against_reference(oracle.texture_probe, mips, "oracle")


def test_oracle_sampler_far_range_is_within_the_derived_bound(oracle, mips):
    """2^25 <= |u * dim| <= 2^30 on sides that are no power of two: the wrap is the exact remainder of the integer-valued texel coordinate by the side."""
    check_against_reference(oracle.texture_probe, mips, "oracle far", far=True)


def test_exact_remainder_wrap_keeps_the_plain_forms_floats_below_2_24():
    """The wrap of pt_scene.h wrap_texel_npot / scene.h sample_bilinear, new text against old, in float32 on the texel coordinates of the zoo's near rows (every level, both axes)
    and on random integers of [-2^24 + side, 2^24): r = fmaf(-floor(x / side), side, x); r - floor(r / side) * side returns the floats of x - floor(x / side) * side. (The fused
    step in float64: |q * side| < 2^25 and |x| <= 2^24 make product and sum exact there, so one rounding to float32 is the fused result.) The last `side` integers above -2^24 are
    left out because the OLD text is already wrong there — its product q * side passes 2^24 and rounds: -2^24 on a side of 25 gave 8, the remainder is 9 — and the new one is held
    to the integer remainder on them instead.)"""
    f32 = np.float32; sc, texs, quads = tc.zoo(); rng = np.random.default_rng(5); n = 0
    def old(x, side): return (x - (np.floor(x / side) * side).astype(f32)).astype(f32)
    def new(x, side):
        r = (-np.floor(x / side).astype(np.float64) * np.float64(side) + x.astype(np.float64)).astype(f32)
        return (r - (np.floor(r / side) * side).astype(f32)).astype(f32)
    for t in texs[::len(tc.FORMATS)]:
        rows = tc.near_rows(t); rows = rows[rows[:, 0] == 1]
        for axis, dim in ((2, t.w), (3, t.h)):
            for mip in range(t.levels):
                side = f32(max(1, dim >> mip)); u = rows[rows[:, 4] == mip, axis].copy().view(f32)
                x = np.concatenate([np.floor((u * side).astype(f32) - f32(0.5)), rng.integers(-2 ** 24 + int(side), 2 ** 24, 4000).astype(f32), f32([0.0, -0.0, -1.0, 2.0 ** 24 - 1, -2.0 ** 24 + side])])
                assert (x >= -2.0 ** 24 + side).all() and (x < 2.0 ** 24).all()
                a, b = old(x, side), new(x, side); n += len(x)
                assert np.array_equal(a, b) and (a >= 0).all() and (a < side).all(), (t.name, mip, axis)
                edge = -2.0 ** 24 + np.arange(int(side), dtype=np.float64)
                assert np.array_equal(new(edge.astype(f32), side).astype(np.int64), edge.astype(np.int64) % int(side)), (t.name, mip, axis)
    assert n > 100000


def test_constant_textures_return_their_constant():
    sc, texs = tc.constant_scene()
    o = ptref.Oracle(); o.set_scene(sc); o.set_settings(scenes.default_settings()); o.resize(8, 8)
    want = texs[0].pixels[0, 0]
    for t in texs:
        rows = np.concatenate([tc.near_rows(t), tc.far_rows(t)])
        got = o.texture_probe(rows)
        assert np.array_equal(got.view(np.uint32), np.broadcast_to(want.view(np.uint32), got.shape)), t.name      # (the 1 x 1 texture among them: its texel, everywhere)


def test_integer_shifts_of_uv_are_bit_identical_on_power_of_two_sides(oracle):
    """uv and uv + integer fetch the same texels with the same weights while |u * w| < 2^22, where the shift is still exact in the texel coordinate's float32 bits."""
    sc, texs, quads = tc.zoo(); r = np.random.default_rng(11)
    for t in texs:
        if (t.w & (t.w - 1)) or (t.h & (t.h - 1)): continue
        n = 400
        # multiples of 2^-9 in [-1, 1): uv * dim (dim <= 128) and the shifted uv are exact, whatever the integer
        u, v = (r.integers(-512, 512, n) / 512.0).astype(np.float32), (r.integers(-512, 512, n) / 512.0).astype(np.float32)
        ku, kv = r.integers(-2 ** 12, 2 ** 12, n).astype(np.float32), r.integers(-2 ** 12, 2 ** 12, n).astype(np.float32)
        assert (np.abs((u + ku).astype(np.float64) * t.w) < 2.0 ** 22).all() and (np.abs((v + kv).astype(np.float64) * t.h) < 2.0 ** 22).all()
        for mode, w4 in ((0, np.float32(1.3 - 0.5 * (t.word >> 24))), (1, np.uint32(0)), (1, np.uint32(t.levels - 1))):
            a = oracle.texture_probe(tc._rows(mode, t.word if mode == 0 else t.index, u, v, w4))
            b = oracle.texture_probe(tc._rows(mode, t.word if mode == 0 else t.index, u + ku, v + kv, w4))
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (t.name, mode)


def test_one_texel_texture_returns_its_texel_everywhere(oracle, mips):
    sc, texs, quads = tc.zoo()
    for t in texs:
        if (t.w, t.h) != (1, 1): continue
        rows = tc.near_rows(t); got = oracle.texture_probe(rows); want = mips[t.index][0][0, 0].astype(np.float32)
        bil = rows[:, 0] != 2
        assert np.array_equal(got[bil].view(np.uint32), np.broadcast_to(want.view(np.uint32), got[bil].shape)), t.name
        # the N-tap average of a texel with a full mantissa rounds: its running sum k * c (k <= 16) at most once per addition and the division once — within 16 roundings
        # of 2^-24; tests/texture_cases.py constant_scene has the 1 x 1 texture whose texel survives that to the bit
        assert np.allclose(got[~bil], want, rtol=17 * 2.0 ** -24, atol=0), t.name


def alpha_reference(rows, mips):
    """texture_ref's verdict on alpha-test candidates: (opaque [n] bool, decided [n] bool — the float64 opacity is further from the cutoff than the derived bound)."""
    sc, texs, quads = tc.zoo()
    uv = tc.alpha_texcoords(rows); q = (rows[:, 0] >> 1).astype(np.int64)
    opaque = np.zeros(len(rows), bool); decided = np.zeros(len(rows), bool)
    for qi, (t, _, cutoff) in enumerate(quads):
        k = q == qi
        if not k.any(): continue
        a = tr.bilinear(mips[t.index], 0, uv[k, 0], uv[k, 1])[:, 3]
        bnd = tr.bound(mips[t.index], np.zeros(int(k.sum())))[:, 3]
        opaque[k] = a >= float(cutoff); decided[k] = np.abs(a - float(cutoff)) > bnd
    return opaque, decided


def test_alpha_candidates_are_decided_by_the_reference_alone(mips):
    """What the GPU alpha test leans on: at least 99 % of the 20 000 candidates lie further from their cutoff than the bound, and both answers occur on every plane format."""
    rows = tc.alpha_candidates(); opaque, decided = alpha_reference(rows, mips)
    assert decided.mean() >= 0.99, decided.mean()
    sc, texs, quads = tc.zoo(); fmt = np.array([tc.FORMATS.index(quads[q][0].fmt) for q in rows[:, 0] >> 1])
    for f in range(len(tc.FORMATS)): assert 0.1 < opaque[fmt == f].mean() < 0.9, (tc.FORMATS[f], opaque[fmt == f].mean())


def test_oracle_closest_hits_agree_with_the_reference_opacity(oracle, mips):
    """A ray along +z into one quad's layer range alone: the oracle's AlphaTest (sample_bilinear(...).w >= cutoff at the hit's texture coordinate) lets it through exactly where
    the float64 opacity is below the cutoff."""
    sc, texs, quads = tc.zoo()
    rows = tc.alpha_candidates(6000); opaque, decided = alpha_reference(rows, mips)
    prim = rows[:, 0].astype(np.int64); u, v = rows[:, 1].copy().view(np.float32).astype(np.float64), rows[:, 2].copy().view(np.float32).astype(np.float64)
    P = sc["positions"].reshape(-1, 4, 3).astype(np.float64)[prim >> 1]
    c = np.where((prim & 1)[:, None] == 0, [0, 1, 2], [0, 2, 3])
    p0, p1, p2 = (P[np.arange(len(prim)), c[:, k]] for k in range(3))
    hit = p0 * (1 - u - v)[:, None] + p1 * u[:, None] + p2 * v[:, None]
    inside = (u > 0.02) & (v > 0.02) & (u + v < 0.98)                           # away from the edges: the ray's own barycentrics differ from (u, v) by roundings only
    rays = np.concatenate([hit - [0, 0, 0.2], np.zeros((len(hit), 1)), np.tile([0.0, 0.0, 1.0], (len(hit), 1)), np.full((len(hit), 1), 0.4)], 1).astype(np.float32)
    got = oracle.trace_closest(rays).view(np.uint32)[:, 1] != 0xFFFFFFFF
    # the traced barycentrics move the texture coordinate by ~1e-6 of the quad: only candidates whose opacity is well away from the cutoff are compared
    uv = tc.alpha_texcoords(rows); clear = np.zeros(len(rows), bool)
    for qi, (t, _, cutoff) in enumerate(quads):
        k = (prim >> 1) == qi
        if k.any(): clear[k] = np.abs(tr.bilinear(mips[t.index], 0, uv[k, 0], uv[k, 1])[:, 3] - float(cutoff)) > 1e-3
    k = inside & clear
    assert k.mean() > 0.8 and np.array_equal(got[k], opaque[k]), (k.mean(), int((got[k] != opaque[k]).sum()))


# ---- the product's sampler text on the host, under sanitizers
@pytest.fixture(scope="module")
def host_checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("texhost") / "texture_host_check")
    csrc = os.path.join(ROOT, "rtxpt_amd", "csrc")
    # PT_ALPHA_LUT=0: the k / 255 table is a __constant__ object of the device; the header's other arm forms the same quotients by division
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt", "-DPT_ALPHA_LUT=0",
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-I" + csrc, os.path.join(HERE, "texture_host_check.hip"), "-o", exe], check=True)
    return exe


def test_product_sampler_on_the_host_is_clean_under_sanitizers_and_equals_the_oracle(host_checker, oracle, tmp_path):
    """tests/texture_host_check.hip fills a DeviceScene as upload_textures does (exactly sized host allocations: one past a plane or a texture's texels is a sanitizer report),
    runs pt_scene.h's samplers and alpha_test_slot over the zoo's rows, far range included, and writes what they returned; the oracle's probe returns the same bits."""
    sc, texs, quads = tc.zoo()
    rows = np.concatenate([np.concatenate([tc.near_rows(t), tc.far_rows(t)]) for t in texs])
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(np.uint32([len(texs), len(rows)]).tobytes())
        for t in texs:
            f.write(np.uint32([t.w, t.h]).tobytes()); f.write(tr.level0(t.pixels, t.upload, pow32=dm(5)).tobytes())
        f.write(rows.tobytes())
    r = subprocess.run([host_checker, src, dst], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]
    out = np.fromfile(dst, np.uint32).reshape(len(rows), 5)
    want = oracle.texture_probe(rows)
    assert np.array_equal(out[:, :4], want.view(np.uint32)), "first differing row %s" % rows[np.nonzero((out[:, :4] != want.view(np.uint32)).any(1))[0][0]].tolist()
    # alpha_test_slot at the same uv of the same texture (mode 1 rows of level 0; cutoff 0.5): the oracle's opacity decides the same way
    k = (rows[:, 0] == 1) & (rows[:, 4] == 0)
    assert k.sum() > 10000 and np.array_equal(out[k, 4], (want[k, 3] >= np.float32(0.5)).astype(np.uint32))
    fmts = [int(x) for x in r.stdout.split()[1:1 + len(texs)]]
    assert fmts == [0 if t.fmt in ("srgb8", "unorm8", "f32_alpha_bytes") else 1 for t in texs]      # the plane format upload_textures' rule picks
