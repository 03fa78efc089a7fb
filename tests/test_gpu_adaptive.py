"""Adaptive sampling on the device (run with -m gpu; include/mi355pt.h pt_render_adaptive, rtxpt_amd/csrc/pt_adaptive.h / .hip / _api.hip, pt_frame.hip render_pixel_list):
the rank's pixels are sampled in rounds, and the 8 x 8 blocks whose error estimate is below the threshold leave the traced list between rounds. Everything is compared bit for
bit: with tests/adaptive_ref.py — the numpy restatement of the two means, the error, the tree sum and the compaction, fed with the per-sample pictures of the existing path
(reset_accumulation(); render(s, 1); radiance()) — and, without the restatement, with what plain render(0, n) leaves in the pixels that received n samples.
The frame: the Cornell box C1 at 44 x 20 — two 32 x 32 tiles (so two ranks), blocks 4 wide at the right edge and 4 high at the bottom — with minSamples 4, step 2,
maxSamples 16. The threshold is the median block error at the first evaluation, taken from the restatement; nothing is pinned to a number. With it the restatement retires
blocks at 4, retires at least one strictly between 4 and 16 and keeps pixels to 16 (asserted: the tests cannot pass on an empty case).
A round has 880 x 2 = 1760 paths or fewer, so in the product default (tail kernel below 4096 live paths) every round goes to the tail kernel; the suite's contexts have it off."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 44, 20
MIN, STEP, MAX = 4, 2, 16
DARK = 0.01
_cache = {}


def _bits(a): return np.ascontiguousarray(a).view(np.uint32)


def _once(key, make):
    if key not in _cache: _cache[key] = make()
    return _cache[key]


def _scene():
    from rtxpt_amd import scenes
    sc, cam = scenes.cornell_box("C1")
    return sc, scenes.bridge_camera(W, H, **cam), scenes.config_settings("C1")


def _tracer(**kw):
    import rtxpt_amd as pt
    sc, camd, S = _scene()
    t = pt.PathTracer(**kw); t.set_scene(sc); t.set_camera(camd); t.set_settings(S); t.resize(W, H)
    return t


def _params(threshold, **kw):
    import rtxpt_amd as pt
    return pt.adaptive_default_params(**dict(dict(minSamples=MIN, step=STEP, maxSamples=MAX, threshold=threshold, darkFloor=DARK), **kw))


def _base():
    """the one context of the module (the suite's configuration: tail kernel off)"""
    return _once("tracer", _tracer)


def _fixed(n):
    """plain render(0, n): radiance and statistics"""
    def make():
        t = _base(); t.reset_accumulation(); st = t.render(0, n)
        return t.radiance(), st
    return _once(("fixed", n), make)


def _samples():
    """one picture per sample index, from the existing path"""
    def make():
        t = _base(); out = []
        for s in range(MAX):
            t.reset_accumulation(); t.render(s, 1); out.append(t.radiance())
        return np.stack(out)
    return _once("samples", make)


def _pixels(rank=0, world=1):
    import rtxpt_amd as pt
    return pt.shard_layout(W, H, rank, world)


def _threshold():
    """the median block error at the first evaluation, from the restatement alone"""
    from tests import adaptive_ref as ar
    return _once("threshold", lambda: np.float32(np.median(ar.run(_samples(), _pixels(), MIN, MIN, STEP, 0.0, DARK)["block_error"])))


def _want():
    from tests import adaptive_ref as ar
    def make():
        r = ar.run(_samples(), _pixels(), MIN, MAX, STEP, _threshold(), DARK)
        between = sum(v for n, v in r["retired_at"].items() if MIN < n < MAX)
        assert r["retired_at"][MIN] >= 1 and between >= 1 and int((r["counts"] == MAX).sum()) >= 1, \
            "the scene does not exercise the loop: retired %s, counts %s" % (r["retired_at"], np.unique(r["counts"]))
        return r
    return _once("want", make)


def _adaptive(t, threshold, **kw):
    stats, frame = t.render_adaptive(_params(threshold, **kw))
    return dict(radiance=t.radiance(), active=t.adaptive_active(), stats=stats, frame=frame, **t.adaptive_state())


def _got():
    return _once("got", lambda: _adaptive(_base(), _threshold()))


def _assert_same(got, want, what):
    for k in ("radiance", "half", "counts", "block_error", "active"):
        a, b = _bits(got[k]), _bits(want[k])
        assert a.shape == b.shape and np.array_equal(a, b), "%s: %s differs in %d words" % (what, k, int((a != b).sum()) if a.shape == b.shape else -1)
    for k in ("rounds", "evaluations", "samplesTraced", "unconvergedPixels", "minCount", "maxCount"):
        assert got["stats"][k] == want["stats"][k], "%s: %s is %s, expected %s" % (what, k, got["stats"][k], want["stats"][k])


# ---- 1. the device against the restatement
def test_matches_the_restatement():
    want, got = _want(), _got()
    print("threshold %.9g, retired at %s, active per round %s" % (_threshold(), want["retired_at"], want["active_counts"]))
    _assert_same(got, want, "device against restatement")
    assert got["stats"]["errorPassMs"] >= 0 and np.isfinite(got["stats"]["errorPassMs"]) and got["frame"]["pathsTraced"] == want["stats"]["samplesTraced"]


# ---- 2. the per-pixel property: no restatement involved
def test_a_pixel_with_n_samples_holds_what_plain_rendering_gives_it():
    got = _got()
    counts = sorted(set(got["counts"].ravel().tolist()))
    assert len(counts) >= 3 and counts[0] == MIN and counts[-1] == MAX
    for n in counts:
        m = got["counts"] == n
        a, b = _bits(got["radiance"])[m], _bits(_fixed(n)[0])[m]
        assert np.array_equal(a, b), "%d pixels with %d samples differ from render(0, %d)" % (int((a != b).any(-1).sum()), n, n)


# ---- 3. threshold 0: nothing retires
def test_threshold_zero_is_the_fixed_frame():
    t = _base()
    got = _adaptive(t, 0.0)
    assert np.array_equal(_bits(got["radiance"]), _bits(_fixed(MAX)[0])) and np.all(got["counts"] == MAX)
    assert got["stats"]["unconvergedPixels"] == W * H == got["active"].size and np.array_equal(got["active"], _pixels())
    assert got["stats"]["rounds"] == MAX // STEP and got["stats"]["evaluations"] == (MAX - MIN) // STEP + 1 and got["stats"]["samplesTraced"] == W * H * MAX
    t.reset_accumulation()
    rays = [t.render(s, STEP) for s in range(0, MAX, STEP)]
    assert np.array_equal(_bits(t.radiance()), _bits(_fixed(MAX)[0]))
    for k in ("extendRays", "shadowRays", "hits", "pathsTraced"):
        assert got["frame"][k] == sum(int(r[k]) for r in rays) and got["frame"][k] > 0, k


# ---- 4. threshold +inf: everything retires at the first evaluation
def test_threshold_infinity_stops_at_min_samples():
    got = _adaptive(_base(), np.inf)
    assert np.array_equal(_bits(got["radiance"]), _bits(_fixed(MIN)[0])) and np.all(got["counts"] == MIN)
    assert got["active"].size == 0 and got["stats"]["unconvergedPixels"] == 0 and got["stats"]["rounds"] == MIN // STEP and got["stats"]["evaluations"] == 1
    assert (got["stats"]["minCount"], got["stats"]["maxCount"]) == (MIN, MIN)


# ---- 5. the routes a round can take
@pytest.mark.parametrize("route", ["tail_default", "tail_above_frame", "packets_0", "packets_1", "packets_2", "fused_off"])
def test_routes_give_the_same_result(route, monkeypatch):
    want, base = _want(), _got()
    if route == "tail_default": monkeypatch.delenv("MI355PT_TAIL_PATHS", raising=False)      # the product default: 4096 live paths, more than a round ever has
    if route.startswith("packets_"): monkeypatch.setenv("MI355PT_FIRST_VERTEX_PACKETS", route[-1])
    t = _tracer()
    if route == "tail_above_frame": t.set_tail_paths(W * H * MAX * 2)
    if route == "fused_off": t.set_fused_traversal(0)
    got = _adaptive(t, _threshold()); t.close()
    if route.startswith("tail_"): assert got["frame"]["tailLaunches"] >= got["stats"]["rounds"]
    else: assert got["frame"]["tailLaunches"] == 0
    _assert_same(got, want, route)
    _assert_same(got, base, route + " against the module's context")
    for k in ("extendRays", "shadowRays", "hits"): assert got["frame"][k] == base["frame"][k], (route, k)


# ---- 6. two ranks decide what the whole frame decides
def test_shards_equal_the_whole_frame():
    from tests import adaptive_ref as ar
    single = _got()
    act = set(single["active"].tolist())
    total = 0
    for rank in range(2):
        own = _pixels(rank, 2); assert 0 < own.size < W * H
        ys, xs = (own & 0xFFFF).astype(np.int64), (own >> 16).astype(np.int64)
        mine = np.zeros((H, W), bool); mine[ys, xs] = True
        t = _tracer(shard_rank=rank, shard_count=2); got = _adaptive(t, _threshold()); t.close()
        for k in ("radiance", "half", "counts"):
            assert np.array_equal(_bits(got[k])[mine], _bits(single[k])[mine]), (rank, k)
            assert not _bits(got[k])[~mine].any(), (rank, k, "pixels of the other rank are not zero")
        blocks = np.zeros_like(mine[::8, ::8]); blocks[ys >> 3, xs >> 3] = True
        assert np.array_equal(_bits(got["block_error"])[blocks], _bits(single["block_error"])[blocks]) and not _bits(got["block_error"])[~blocks].any()
        assert np.array_equal(got["active"], np.array([p for p in own.tolist() if p in act], np.uint32)), rank
        # and against the restatement run on the rank's list
        _assert_same(got, ar.run(_samples(), own, MIN, MAX, STEP, _threshold(), DARK), "rank %d" % rank)
        total += got["stats"]["samplesTraced"]
    assert total == single["stats"]["samplesTraced"]


# ---- 6b. a frame large enough for the other paths of the compaction and the driver
def test_large_frame_scan_chunks_and_pipelined_batches():
    """1280 x 832: 16 640 blocks are 65 chunks of the scan — more than one chunk, and more than the 64 chunk sums one step of the totals' carry loop takes — and 1 064 960 pixels
    x 2 samples are 2.1 M paths a round: four pipelined batches, whose accumulation the evaluation waits for on the main stream. No per-sample pictures at this size: the result
    is held to plain rendering (the per-pixel property) and to itself — the block errors follow from the two buffers the device left (a retired block's are never touched
    again), the active list from the block errors, the counts from both."""
    import rtxpt_amd as pt
    from rtxpt_amd import scenes
    from tests import adaptive_ref as ar
    w, h, mx = 1280, 832, 8
    sc, cam = scenes.cornell_box("C1")
    t = pt.PathTracer(); t.set_scene(sc); t.set_camera(scenes.bridge_camera(w, h, **cam)); t.set_settings(scenes.config_settings("C1")); t.resize(w, h)
    own = pt.shard_layout(w, h, 0, 1); ys, xs = (own & 0xFFFF).astype(np.int64), (own >> 16).astype(np.int64)
    blocks = ar.blocks_of(own, w); assert len(blocks) == 16640 > 64 * 256 and w * h * STEP >= 1 << 21
    t.render_adaptive(_params(0.0, maxSamples=MIN))
    E0 = t.adaptive_state()["block_error"]
    thr = np.float32(np.median(E0[E0 > 0]))
    stats, frame = t.render_adaptive(_params(thr, maxSamples=mx))
    got = dict(radiance=t.radiance(), active=t.adaptive_active(), **t.adaptive_state())
    # block errors from the buffers; the active list from the block errors; the counts block by block
    E = ar.block_errors(ar.pixel_error(got["radiance"][ys, xs], got["half"][ys, xs], DARK), blocks)
    firsts = np.array([f for f, _ in blocks]); by, bx = ys[firsts] >> 3, xs[firsts] >> 3
    assert np.array_equal(_bits(got["block_error"][by, bx]), _bits(E))
    alive = ~(got["block_error"] < thr)
    assert np.array_equal(got["active"], own[alive[ys >> 3, xs >> 3]]) and 0 < got["active"].size < own.size and stats["unconvergedPixels"] == got["active"].size
    per_block = got["counts"][ys[firsts], xs[firsts]]
    assert np.array_equal(got["counts"][ys, xs], np.repeat(per_block, [c for _, c in blocks])) and np.all(per_block[alive[by, bx]] == mx)
    assert set(per_block.tolist()) <= set(range(MIN, mx + 1, STEP)) and len(set(per_block.tolist())) >= 2
    assert stats["samplesTraced"] == int(got["counts"].sum(dtype=np.uint64)) == frame["pathsTraced"] and (stats["minCount"], stats["maxCount"]) == (MIN, mx)
    # the per-pixel property
    for n in sorted(set(per_block.tolist())):
        t.reset_accumulation(); t.render(0, n)
        m = got["counts"] == n
        assert np.array_equal(_bits(got["radiance"])[m], _bits(t.radiance())[m]), "pixels with %d samples differ from render(0, %d)" % (n, n)
    t.close()


# ---- 7. the interface
def test_refusals():
    import rtxpt_amd as pt
    t = pt.PathTracer()
    with pytest.raises(pt.PtError) as e: t.render_adaptive(_params(0.02))
    assert e.value.code == pt.PT_ERROR_NOT_READY
    t.close()
    t = _tracer()
    bad = [dict(step=3, minSamples=3, maxSamples=6), dict(step=0), dict(step=1, minSamples=1, maxSamples=4), dict(minSamples=5), dict(maxSamples=15), dict(minSamples=0),
           dict(minSamples=8, maxSamples=4), dict(step=8, minSamples=4, maxSamples=16), dict(darkFloor=0.0), dict(darkFloor=-1.0), dict(darkFloor=np.nan), dict(threshold=np.nan)]
    for kw in bad:
        with pytest.raises(pt.PtError) as e: t.render_adaptive(_params(kw.pop("threshold", 0.02), **kw))
        assert e.value.code == pt.PT_ERROR_INVALID_ARGUMENT and "adaptive parameters" in str(e.value), kw
    t.set_neeat(True)
    with pytest.raises(pt.PtError) as e: t.render_adaptive(_params(0.02))
    assert e.value.code == pt.PT_ERROR_INVALID_ARGUMENT and "NEE-AT" in str(e.value)
    t.set_neeat(False)
    t.set_local_light_sampling(None, feedback=True)
    with pytest.raises(pt.PtError) as e: t.render_adaptive(_params(0.02))
    assert e.value.code == pt.PT_ERROR_INVALID_ARGUMENT and "NEE-AT" in str(e.value)
    t.set_local_light_sampling(None, feedback=False)
    with pytest.raises(pt.PtError) as e: t.adaptive_state()      # nothing rendered yet
    assert e.value.code == pt.PT_ERROR_NOT_READY
    # none of the refusals touched the accumulation: plain rendering still works and has its bits
    t.reset_accumulation(); t.render(0, MIN)
    assert np.array_equal(_bits(t.radiance()), _bits(_fixed(MIN)[0]))
    t.close()


def test_render_is_refused_until_the_accumulation_is_reset():
    import rtxpt_amd as pt
    t = _base()
    first = _adaptive(t, _threshold())
    with pytest.raises(pt.PtError) as e: t.render(MAX, 1)
    assert e.value.code == pt.PT_ERROR_NOT_READY and "pt_reset_accumulation" in str(e.value)
    assert np.array_equal(_bits(t.radiance()), _bits(first["radiance"]))      # the refusal changed nothing
    again = _adaptive(t, _threshold())      # another adaptive call starts over
    _assert_same(again, first, "second adaptive call"); _assert_same(again, _want(), "second adaptive call against the restatement")
    t.reset_accumulation()
    t.render(0, MIN)
    assert np.array_equal(_bits(t.radiance()), _bits(_fixed(MIN)[0]))
    t.resize(W, H)      # a resize drops the state as well
    with pytest.raises(pt.PtError) as e: t.adaptive_active()
    assert e.value.code == pt.PT_ERROR_NOT_READY
    t.render(0, MIN)
    assert np.array_equal(_bits(t.radiance()), _bits(_fixed(MIN)[0]))


def test_display_tail_reads_the_adaptive_result():
    t = _base()
    t.reset_accumulation(); t.render(0, MIN)
    want = (t.tonemap(), t.average_luminance())
    _adaptive(t, np.inf)
    got = (t.tonemap(), t.average_luminance())
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and want[0].any()
    t.reset_accumulation()
