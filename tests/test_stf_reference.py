"""Stochastic texture filtering, CPU half (tests/test_gpu_stf.py is the GPU half): the numpy restatement tests/stf_ref.py of rtxpt_amd/csrc/pt_stf.h on the texture zoo of
tests/texture_cases.py — LINEAR's expectation is the trilinear value of tests/texture_ref.py, CUBIC's weights are well formed and its expectation is a float64 B-spline
convolution, POINT ignores its random numbers, numbers on the decision thresholds pick the tap the definition says — and the product's own text (pt_stf.h is host-and-device
text) run on the host as a stand-alone program, plainly and under the address and undefined-behaviour sanitizers, bit for bit equal to the restatement."""
import os
import subprocess
import sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import texture_cases as tc
import texture_ref as tr
import stf_ref as sr
from test_texture_sampling import dm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32


@pytest.fixture(scope="module")
def level0():
    pw = dm(5)
    return [tr.level0(t.pixels, t.upload, pow32=pw) for t in tc.zoo()[1]]


@pytest.fixture(scope="module")
def mips(level0):
    """The float64 mip chains of the zoo (texture_ref's), built once."""
    return [tr.build_mips(l) for l in level0]


def _expectation(filt, t, m, word, u, v, lam):
    mip, x, y, p = sr.candidates(filt, t.w, t.h, t.levels, word, lam, u, v)
    assert (p >= 0).all() and np.abs(p.sum(1) - 1.0).max() < 1e-12
    e = np.zeros((len(u), 4))
    for l in np.unique(mip):
        k = mip == l
        e += np.where(k[..., None], m[l][np.where(k, y, 0), np.where(k, x, 0)] * p[..., None], 0.0).sum(1)
    return e, mip.max(1)


def test_linear_is_unbiased(mips):
    """Sum over the eight candidates of probability x texel (float64 texels of texture_ref's chain) == texture_ref.sample_texture, within texture_ref.bound of the deepest level
    read — on every row, the far range included: there the fraction is 0 and one texel has probability 1."""
    worst = 0.0
    for t in tc.zoo()[1]:
        word, u, v, lam = sr.lookup_rows(t, tc.material_rows); m = mips[t.index]
        e, _ = _expectation(sr.LINEAR, t, m, word, u, v, lam)
        ref, deep = tr.sample_texture(m, t.word, lam, u, v)
        ratio = np.abs(e - ref) / tr.bound(m, deep); worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (t.name, float(ratio.max()))
    print("LINEAR: largest |expectation - trilinear| / bound over the zoo: %.3g" % worst)


def _cubic_reference(t, m, word, u, v, lam):
    """The direct float64 convolution: at each of the two levels sum_{j, i} B_j(ay) B_i(ax) texel(flx - 1 + i, fly - 1 + j) with the cubic B-spline's weights in float64 at the
    float32 fractions, exact integer coordinates wrapped by an exact modulo; the two levels blended by f."""
    m0, m1, f = sr.levels32(sr.lambda32(word, lam), np.full(len(u), t.levels))
    out = []
    for mip in (m0, m1):
        val = np.zeros((len(u), 4))
        for l in np.unique(mip):
            k = mip == l; lv = m[l]; mh, mw = lv.shape[:2]
            (flx, ax), (fly, ay) = sr.frac32(u[k], F32(mw)), sr.frac32(v[k], F32(mh))
            bx, by = sr.bspline_weights64(ax), sr.bspline_weights64(ay); x0, y0 = flx.astype(np.int64), fly.astype(np.int64)
            acc = np.zeros((int(k.sum()), 4))
            for j in range(4):
                for i in range(4): acc += (by[:, j] * bx[:, i])[:, None] * lv[(y0 - 1 + j) % mh, (x0 - 1 + i) % mw]
            val[k] = acc
        out.append(val)
    f = f.astype(np.float64)[:, None]
    return out[0] * (1.0 - f) + out[1] * f


def test_cubic_is_well_formed_and_unbiased(mips):
    """The float32 weights are >= 0 and sum to 1 within 4 ulp (of 1: 4 x 2^-23) at every fraction the rows produce and on a dense sweep of [0, 1). The expectation over the 32
    candidates equals the direct float64 convolution. Tolerance, derived: the tap probabilities are the float32 thresholds' differences (the last tap takes 1 - c2); each weight
    carries at most 4 float32 roundings of values <= 1 (2 x 2^-23), each threshold one more per sum, so a probability is within 6 x 2^-23 of the exact weight and the four of an
    axis within 24 x 2^-23 in total; two axes: |E - ref| <= 48 x 2^-23 x max |texel|. Rows whose coordinate passes 2^23 texels are left to the equality tests: there float32 no
    longer holds flx - 1 and flx + 2 apart, the taps collapse onto representable coordinates, and an exact-integer convolution is no longer what the filter estimates."""
    sweep = np.concatenate([np.linspace(0, 1, 200001)[:-1].astype(np.float32), F32([0.0, sr.ONE_BELOW, 0.5, 2.0 ** -24, 2.0 ** -60])])
    w = sr.bspline_weights32(sweep)
    assert (w >= 0).all() and np.abs(w.astype(np.float64).sum(1) - 1.0).max() <= 4 * 2.0 ** -23
    assert np.abs(w.astype(np.float64) - sr.bspline_weights64(sweep)).max() <= 2 * 2.0 ** -23
    worst = 0.0
    for t in tc.zoo()[1]:
        word, u, v, lam = sr.lookup_rows(t, tc.material_rows); m = mips[t.index]
        near = (np.abs(u.astype(np.float64)) * t.w < 2.0 ** 23) & (np.abs(v.astype(np.float64)) * t.h < 2.0 ** 23)
        word, u, v, lam = word[near], u[near], v[near], lam[near]
        for side in (t.w, max(1, t.w >> 1)):
            ax = sr.frac32(u, F32(side))[1]; ww = sr.bspline_weights32(ax)
            assert (ww >= 0).all() and np.abs(ww.astype(np.float64).sum(1) - 1.0).max() <= 4 * 2.0 ** -23
        e, _ = _expectation(sr.CUBIC, t, m, word, u, v, lam)
        ref = _cubic_reference(t, m, word, u, v, lam)
        tol = 48 * 2.0 ** -23 * np.abs(m[0]).reshape(-1, 4).max(0)
        ratio = np.abs(e - ref) / tol; worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (t.name, float(ratio.max()))
    print("CUBIC: largest |expectation - convolution| / tolerance over the zoo: %.3g" % worst)


def test_point_ignores_u():
    for t in tc.zoo()[1]:
        word, u, v, lam = sr.lookup_rows(t, tc.material_rows); r = np.random.default_rng(t.index)
        a = sr.pick(sr.POINT, t.w, t.h, t.levels, word, lam, u, v, np.zeros((len(u), 4), np.float32))
        for rnd in (sr.random_u(r, len(u)), np.full((len(u), 4), sr.ONE_BELOW, np.float32)):
            b = sr.pick(sr.POINT, t.w, t.h, t.levels, word, lam, u, v, rnd)
            assert all(np.array_equal(p, q) for p, q in zip(a, b)), t.name
        # and it is the texel whose area holds the coordinate, at the nearer level
        m0, m1, f = sr.levels32(sr.lambda32(word, lam), np.full(len(u), t.levels)); mip = np.where(f.astype(np.float64) < 0.5, m0, m1)
        assert np.array_equal(a[0], mip)
        mw = np.maximum(1, t.w >> mip)
        assert np.array_equal(a[1], np.floor((u * mw.astype(np.float32)).astype(np.float32).astype(np.float64)).astype(np.int64) % mw)


def _scalar_pick_axis(filt, coord, side, u):
    """One axis of one lookup in Python floats (float64 holds every float32 exactly, and comparisons of float32 values are exact in it): the definition, written a second time."""
    fx = float(F32(F32(coord) * F32(side)) - F32(0.5)); fl = float(np.floor(fx)); a = float(F32(fx) - F32(fl))
    if filt == sr.LINEAR: return fl + (1.0 if u < a else 0.0)
    w = sr.bspline_weights32(F32([a]))[0]; c0 = float(w[0]); c1 = float(F32(w[0] + w[1])); c2 = float(F32(F32(w[0] + w[1]) + w[2]))
    return fl - 1.0 + (u >= c0) + (u >= c1) + (u >= c2)


@pytest.mark.parametrize("filt", [sr.LINEAR, sr.CUBIC])
def test_threshold_edges_pick_the_tap_the_definition_says(filt):
    """u = 0, the largest float below 1, and the floats just below and exactly at every threshold (ax, ay, f; c0 .. c2 of either axis): the vectorised restatement picks what the
    definition, evaluated lookup by lookup in Python floats, says. u < a takes the upper tap; u == a does not."""
    seen = set()
    for t in tc.zoo()[1][::5] + tc.zoo()[1][3::5]:
        word, u, v, lam = sr.lookup_rows(t, tc.material_rows); r = np.random.default_rng(1000 + t.index)
        near = (np.abs(u.astype(np.float64)) * t.w < 2.0 ** 23) & (np.abs(v.astype(np.float64)) * t.h < 2.0 ** 23)
        k = r.permutation(np.nonzero(near)[0])[:200]; word, u, v, lam = word[k], u[k], v[k], lam[k]
        rnd = sr.threshold_u(filt, t.w, t.h, t.levels, word, lam, u, v, r)
        mip, x, y = sr.pick(filt, t.w, t.h, t.levels, word, lam, u, v, rnd)
        m0, m1, f = sr.levels32(sr.lambda32(word, lam), np.full(len(u), t.levels))
        for i in range(len(u)):
            want_mip = int(m1[i]) if float(rnd[i, 2]) < float(f[i]) else int(m0[i])
            mw, mh = max(1, t.w >> want_mip), max(1, t.h >> want_mip)
            want = (want_mip, int(_scalar_pick_axis(filt, u[i], mw, float(rnd[i, 0]))) % mw, int(_scalar_pick_axis(filt, v[i], mh, float(rnd[i, 1]))) % mh)
            assert (int(mip[i]), int(x[i]), int(y[i])) == want, (t.name, i, rnd[i].tolist())
            if float(rnd[i, 2]) == float(f[i]) and f[i] > 0: seen.add("at f")
            if float(rnd[i, 2]) == float(np.nextafter(f[i], F32(-1))) and f[i] > 0: seen.add("below f")
            if rnd[i, 0] == 0: seen.add("zero")
            if rnd[i, 0] == sr.ONE_BELOW: seen.add("one below")
    assert seen == {"at f", "below f", "zero", "one below"}
    # the two comparisons themselves, on one hand-made lookup: a 4-texel row, coordinate 0.3 -> fx = 0.7, flx = 0, ax = 0.7 (float32)
    a = float(F32(F32(0.3) * F32(4.0)) - F32(0.5))
    pick_x = lambda uu: int(sr.pick(filt, 4, 1, 3, np.uint32(3 << 16), F32(0.0), F32([0.3]), F32([0.0]), F32([[uu, 0, 0, 0]]))[1][0])
    if filt == sr.LINEAR:
        assert pick_x(np.nextafter(F32(a), F32(0))) == 1 and pick_x(F32(a)) == 0 and pick_x(0.0) == 1 and pick_x(sr.ONE_BELOW) == 0
    else:
        c = sr.thresholds32(sr.bspline_weights32(F32([a])))[0]
        assert [pick_x(np.nextafter(c[j], F32(0))) for j in range(3)] == [3, 0, 1] and [pick_x(c[j]) for j in range(3)] == [0, 1, 2] and pick_x(0.0) == 3 and pick_x(sr.ONE_BELOW) == 2


# ---- the product's text on the host
def _build(tmp, name, extra):
    exe = str(tmp / name); csrc = os.path.join(ROOT, "rtxpt_amd", "csrc")
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fhip-fp32-correctly-rounded-divide-sqrt", "-DPT_ALPHA_LUT=0"] + extra +
                   ["-I" + csrc, os.path.join(HERE, "stf_host_check.hip"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("stfhost")
    return _build(tmp, "stf_host_check", []), _build(tmp, "stf_host_check_san", ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"])


def test_product_text_on_the_host_equals_the_restatement_and_is_clean_under_sanitizers(host_programs, level0, tmp_path):
    """tests/stf_host_check.hip over every filter's rows on every texture of the zoo (random u and u on the thresholds, the far range included) plus rows of the random source:
    level, x, y and the texel — the float32 chain as the library builds it — equal tests/stf_ref.py bit for bit; the sanitizer build writes the same file and reports nothing."""
    texs = tc.zoo()[1]
    per = [(t, f, sr.probe_rows(t, f, tc.material_rows)) for t in texs for f in (sr.POINT, sr.LINEAR, sr.CUBIC)]
    r = np.random.default_rng(7); draw = np.zeros((300, 12), np.uint32); draw[:, 0] = 1
    draw[:, 6] = (r.integers(0, 4096, 300) << 16) | r.integers(0, 4096, 300); draw[:, 7] = r.integers(0, 40, 300); draw[:, 8] = r.integers(0, 1 << 20, 300)
    rows = np.concatenate([p[2] for p in per] + [draw])
    src = str(tmp_path / "in.bin")
    with open(src, "wb") as f:
        f.write(np.uint32([len(texs), len(rows)]).tobytes())
        for t in texs: f.write(np.uint32([t.w, t.h]).tobytes()); f.write(level0[t.index].tobytes())
        f.write(rows.tobytes())
    outs = []
    for k, exe in enumerate(host_programs):
        dst = str(tmp_path / ("out%d.bin" % k))
        p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
        assert p.returncode == 0 and p.stdout.startswith("ok") and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stdout[-2000:] + p.stderr[-4000:]
        outs.append(np.fromfile(dst, np.uint32).reshape(len(rows), 8))
    assert np.array_equal(outs[0], outs[1])
    out = outs[0]; at = 0
    for t, filt, rr in per:
        got = out[at:at + len(rr)]; at += len(rr)
        mip, x, y = sr.pick_rows(t, rr)
        bad = (got[:, 4] != mip) | (got[:, 5] != x) | (got[:, 6] != y)
        assert not bad.any(), "%s filter %d: %d of %d rows differ; first: %s host %s restatement %s" % (t.name, filt, int(bad.sum()), len(rr), rr[bad][0].tolist(), got[bad][0, 4:7].tolist(), [int(mip[bad][0]), int(x[bad][0]), int(y[bad][0])])
        m32 = sr.build_mips32(level0[t.index])
        texel = np.zeros((len(rr), 4), np.float32)
        for l in np.unique(mip): k = mip == l; texel[k] = m32[l][y[k], x[k]]
        assert np.array_equal(got[:, :4], texel.view(np.uint32)), (t.name, filt)
    # the random source: SampleGeneratorVertexBase::make(pixel, vertex, sample), the generator with effect seed Base in uniform mode, four numbers — in numpy
    def hash32(x):
        x = x.astype(np.uint64); M = np.uint64(0xFFFFFFFF)
        x ^= x >> np.uint64(16); x = (x * np.uint64(0x21f0aaad)) & M; x ^= x >> np.uint64(15); x = (x * np.uint64(0xf35a2d97)) & M; x ^= x >> np.uint64(15)
        return x
    def combine(seed, value):
        M = np.uint64(0xFFFFFFFF)
        return seed ^ ((hash32(value) + np.uint64(0x9e3779b9) + ((seed << np.uint64(6)) & M) + (seed >> np.uint64(2))) & M)
    d = draw.astype(np.uint64); M = np.uint64(0xFFFFFFFF)
    h = combine(hash32((d[:, 7] + np.uint64(0x035F9F29)) & M), d[:, 6]); h = combine(h, np.zeros_like(h)); h = combine(h, d[:, 8])
    want = []
    for _ in range(4): h = hash32(h); want.append(((h >> np.uint64(8)).astype(np.float32) / F32(16777216.0)).astype(np.float32))
    assert np.array_equal(out[at:, :4], np.stack(want, 1).view(np.uint32)) and not out[at:, 4:].any()
