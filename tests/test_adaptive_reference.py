"""The numpy restatement of adaptive sampling (tests/adaptive_ref.py) held to answers worked by hand: no device. tests/test_gpu_adaptive.py holds the device to the
restatement; this file is what keeps the restatement itself honest."""
import numpy as np
import pytest

import rtxpt_amd as pt
from tests import adaptive_ref as ar

F = np.float32


def frame_list(w, h):
    return pt.shard_layout(w, h, 0, 1)


def test_constant_picture_retires_at_min_samples_unless_threshold_is_zero():
    w, h = 20, 12
    samples = np.broadcast_to(np.array([0.25, 0.5, 0.75, 1.0], F), (16, h, w, 4)).copy()
    px = frame_list(w, h)
    for thr in (1e-30, 0.02, np.inf):
        r = ar.run(samples, px, 4, 16, 2, thr, 0.01)
        assert np.all(r["block_error"] == 0) and r["active"].size == 0 and np.all(r["counts"] == 4)
        assert r["stats"] == dict(rounds=2, evaluations=1, samplesTraced=4 * w * h, unconvergedPixels=0, minCount=4, maxCount=4)
        assert np.array_equal(r["radiance"], samples[0]) and np.array_equal(r["half"], samples[0])
    r = ar.run(samples, px, 4, 16, 2, 0.0, 0.01)      # E < 0 never holds
    assert np.all(r["block_error"] == 0) and np.array_equal(r["active"], px) and np.all(r["counts"] == 16)
    assert r["stats"] == dict(rounds=8, evaluations=7, samplesTraced=16 * w * h, unconvergedPixels=w * h, minCount=16, maxCount=16)
    assert r["active_counts"] == [w * h] * 8


def test_one_pixel_alternating_between_zero_and_two():
    """a 1 x 1 frame: one block of one pixel; even samples are 0, odd samples 2 in every channel"""
    samples = np.zeros((4, 1, 1, 4), F); samples[1::2, ..., :3] = 2.0; samples[..., 3] = 1.0
    px = np.array([0], np.uint32)
    # n = 2: A = 0 + (2 - 0) * (1 / 2) = 1, H = sample 0 = 0; d = 1 + 1 + 1 = 3, b = 3, e = 3 / sqrt(3); E = e / 1
    r = ar.run(samples, px, 2, 2, 2, 0.0, 0.01)
    assert np.array_equal(r["radiance"][0, 0], [1, 1, 1, 1]) and np.array_equal(r["half"][0, 0], [0, 0, 0, 1])
    E2 = F(3.0) / np.sqrt(F(3.0))
    assert r["block_error"][0, 0] == E2 and abs(float(E2) - 3 ** 0.5) < 1e-6
    # n = 4: A = 1 + (0 - 1) * (1 / 3), then A + (2 - A) * (1 / 4); H = 0 + (0 - 0) * (1 / 2) = 0; d = b = A + A + A, e = d / sqrt(b)
    r = ar.run(samples, px, 2, 4, 2, 0.0, 0.01)
    A = F(1.0) + (F(0.0) - F(1.0)) * (F(1.0) / F(3.0)); A = A + (F(2.0) - A) * (F(1.0) / F(4.0))
    assert r["radiance"][0, 0, 0] == A and abs(float(A) - 1.0) < 1e-6 and np.array_equal(r["half"][0, 0], [0, 0, 0, 1])
    d = (A + A) + A
    E4 = (d / np.sqrt(d)) / F(1.0)
    assert r["block_error"][0, 0] == E4 and abs(float(E4) - 3 ** 0.5) < 1e-6
    assert r["stats"]["evaluations"] == 2 and r["counts"][0, 0] == 4
    # the same pixel retires at 2 with a threshold just above E2, and not with E2 itself (strictly below)
    assert ar.run(samples, px, 2, 4, 2, np.nextafter(E2, F(2)), 0.01)["counts"][0, 0] == 2
    assert ar.run(samples, px, 2, 4, 2, E2, 0.01)["counts"][0, 0] == 4


def test_partial_blocks_of_a_13_by_10_frame():
    w, h = 13, 10
    px = frame_list(w, h)
    blocks = ar.blocks_of(px, w)
    assert [c for _, c in blocks] == [64, 40, 16, 10] and [f for f, _ in blocks] == [0, 64, 104, 120]
    for first, count in blocks:      # a block's entries are one 8 x 8 screen block, row by row
        xs, ys = px[first:first + count] >> 16, px[first:first + count] & 0xFFFF
        assert np.all(xs >> 3 == xs[0] >> 3) and np.all(ys >> 3 == ys[0] >> 3)
    # every pixel's error is exactly 1 (A = (1, 1, 1), H = 0, floor 9 -> 3 / 3): a block's sum is its count only if the lanes past the count hold 0
    samples = np.zeros((2, h, w, 4), F); samples[1, ..., :3] = 2.0
    r = ar.run(samples, px, 2, 2, 2, 0.0, 9.0)
    assert np.all(r["block_error"] == 1.0) and r["block_error"].shape == (2, 2)
    assert ar.tree_sum(np.ones(10, F)) == 10 and ar.tree_sum(np.ones(64, F)) == 64 and ar.tree_sum([]) == 0
    assert ar.block_error(np.full(40, 3.0, F)) == 3.0


def test_tree_sum_order_and_accuracy():
    rng = np.random.default_rng(7)
    for count in (1, 2, 10, 33, 63, 64):
        v = (rng.random(count) * 10.0 ** rng.integers(-3, 4, count)).astype(F)
        got = ar.tree_sum(v)
        # the order, written out: pairs 32 apart first
        p = np.zeros(64, F); p[:count] = v
        for off in (32, 16, 8, 4, 2, 1): p = (p[:off] + p[off:2 * off]).astype(F)
        assert got == p[0]
        # positive terms: the roundings of one level add up to at most half an ulp of each partial sum, together below one ulp of the total; six levels
        exact = float(np.sum(v.astype(np.float64)))
        assert abs(float(got) - exact) <= 6 * float(np.spacing(F(exact))) * 1.01
    # block_errors is the same tree for many blocks at once
    e = rng.random(64 + 40 + 1).astype(F); blocks = [(0, 64), (64, 40), (104, 1)]
    assert np.array_equal(ar.block_errors(e, blocks), np.array([ar.block_error(e[f:f + c]) for f, c in blocks], F)) and ar.block_errors(e, []).size == 0
    # and it is this tree, not a running sum: 2^24 + 1 + 1 + ... loses every 1 in sequence, the tree adds the ones to each other first
    v = np.ones(64, F); v[0] = 2.0 ** 24
    seq = F(0)
    for x in v: seq = F(seq + x)
    assert seq == 2.0 ** 24 and ar.tree_sum(v) == 2.0 ** 24 + 64 - 2      # (v[0] + v[32] = 2^24 + 1 rounds to even: 2^24)


def test_nan_and_inf_pixels_count_as_converged():
    A = np.array([[np.nan, 1, 1, 1], [np.inf, 1, 1, 1], [1, 1, 1, 1], [1, -np.inf, 1, 1], [2, 2, 2, 1]], F)
    H = np.array([[1, 1, 1, 1], [1, 1, 1, 1], [np.nan, 1, 1, 1], [1, 1, 1, 1], [1, 1, 1, 1]], F)
    e = ar.pixel_error(A, H, 0.01)
    assert np.array_equal(e[:4], [0, 0, 0, 0]) and e[4] == F(3.0) / np.sqrt(F(6.0))
    # in a frame: a NaN pixel does not keep its block alive
    samples = np.ones((4, 8, 8, 4), F); samples[:, 3, 5, 0] = np.nan
    r = ar.run(samples, frame_list(8, 8), 2, 4, 2, 1e-6, 0.01)
    assert r["active"].size == 0 and np.all(r["counts"] == 2) and r["block_error"][0, 0] == 0


def test_active_set_never_grows_and_keeps_its_order():
    rng = np.random.default_rng(3)
    w, h = 44, 20
    samples = rng.random((16, h, w, 4)).astype(F) * np.linspace(0.01, 4.0, w, dtype=F)[None, None, :, None]
    px = frame_list(w, h)
    first = ar.run(samples, px, 4, 4, 2, 0.0, 0.01)
    thr = np.median(first["block_error"])
    r = ar.run(samples, px, 4, 16, 2, thr, 0.01)
    assert all(a >= b for a, b in zip(r["active_counts"], r["active_counts"][1:])) and r["active_counts"][0] == w * h
    assert 0 < r["retired_at"][4] < len(ar.blocks_of(px, w))
    pos = {int(p): i for i, p in enumerate(px)}
    idx = [pos[int(p)] for p in r["active"]]
    assert idx == sorted(idx) and len(set(idx)) == len(idx)
    assert r["stats"]["samplesTraced"] == int(r["counts"].sum()) == 2 * sum(r["active_counts"])
    # a pixel's count is the n at which its block retired, the same for the whole block
    for f0, c in ar.blocks_of(px, w):
        ys, xs = px[f0:f0 + c] & 0xFFFF, px[f0:f0 + c] >> 16
        assert len(set(r["counts"][ys, xs].tolist())) == 1


def test_dark_floor_takes_effect_on_a_black_block():
    # even samples 0, odd samples 1e-4: A = 5e-5, H = 0: relative to sqrt(b) the error is sqrt(1.5e-4) ~ 0.0122, relative to sqrt(darkFloor = 0.01) it is 1.5e-3
    samples = np.zeros((2, 8, 8, 4), F); samples[1, ..., :3] = 1e-4
    px = frame_list(8, 8)
    lo = ar.run(samples, px, 2, 2, 2, 0.0, 1e-12)["block_error"][0, 0]
    hi = ar.run(samples, px, 2, 2, 2, 0.0, 0.01)["block_error"][0, 0]
    A = F(0.0) + (F(1e-4) - F(0.0)) * F(0.5); d = (A + A) + A
    assert lo == d / np.sqrt(d) and hi == d / np.sqrt(F(0.01)) and abs(float(hi) - 1.5e-3) < 1e-8 and float(lo) > 8 * float(hi)
    # all black: 0 / sqrt(floor) = 0, not 0 / 0
    black = ar.run(np.zeros((2, 8, 8, 4), F), px, 2, 2, 2, 1e-9, 0.01)
    assert black["block_error"][0, 0] == 0 and black["active"].size == 0


def test_parameter_constraints_are_asserted():
    s = np.zeros((4, 8, 8, 4), F); px = frame_list(8, 8)
    for bad in ((4, 4, 3), (3, 4, 2), (4, 6, 4), (2, 4, 4), (8, 4, 2)):
        with pytest.raises(AssertionError):
            ar.run(s, px, *bad, 0.0, 0.01)
