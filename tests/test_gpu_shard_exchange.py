"""The four per-pixel records a tile-sharded frame moves between ranks (run with -m gpu; rtxpt_amd/csrc/pt_shard.hip) through the public pack / unpack calls, one table with a
row per record: the radiance (16 bytes per pixel), the NEE-AT reservoirs with exported depth (12), the build pass's guides (16) and the whole stable-plane record (284). Frames
of 70 x 45 (partial tiles on both axes; six tiles) on 4 and on 8 ranks — two of the eight own nothing — as contexts of one process. Every row: the packed buffer of a rank is
the record's read-back in pt_shard_layout order; unpacking some ranks changes exactly their pixels; unpacking all gives the unsharded context's read-back; an empty rank packs
and is unpacked; the refusals, with the return codes and texts the exports have always had. Then the RCCL form as far as one device goes: the two gathers as a world-of-one
loop-back, interleaved and across a resize (the staging is shared: grown by the large record, reused by the small one), and their refusals on a sharded context."""
import os, sys
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rtxpt_amd import scenes

pytestmark = pytest.mark.gpu
W, H = 70, 45
WORLDS = (4, 8)
INVALID, NOT_READY = 1, 6
NO_PLANES = "no stable planes of this frame size yet: pt_build_stable_planes"


def _tiles(px): return (px & 0xFFFF).astype(np.int64), (px >> 16).astype(np.int64)


# ---- the read-backs: every pixel's record as (H, W, words) uint32, from the public getters
def _read_radiance(t): return t.radiance().view(np.uint32)


def _read_feedback(t):      # (the exported depth, the record's third word, has no getter: test_the_ranks_records_are_the_unsharded_contexts_record holds it)
    w, c = t.light_feedback(0); return np.stack([w.view(np.uint32), c], -1)


def _read_guides(t):
    p = t.get_stable_planes(); return np.concatenate([p["depth"].view(np.uint32)[..., None], p["spec_hit_t"].view(np.uint32)[..., None], p["motion_vectors"].view(np.uint32)], -1)


_ADDRESS = {}


def _read_planes(t):
    p = t.get_stable_planes(); h, w = p["depth"].shape
    if (w, h) not in _ADDRESS: _ADDRESS[(w, h)] = np.array([[[scenes.stable_planes_address(x, y, pl, w, h) for pl in range(3)] for x in range(w)] for y in range(h)])
    return np.concatenate([np.moveaxis(p["header"], 0, -1), p["planes"][_ADDRESS[(w, h)]].reshape(h, w, 60), p["stable_radiance"].view(np.uint32), p["depth"].view(np.uint32)[..., None],
                           p["spec_hit_t"].view(np.uint32)[..., None], p["motion_vectors"].view(np.uint32), p["throughput"][..., None]], -1)


def _live(rec):      # the plane records of dead planes (header word 0xFFFFFFFF) are nobody's: what the build pass leaves there is not part of the frame
    out = rec.copy()
    for pl in range(3): out[..., 4 + 20 * pl:24 + 20 * pl][rec[..., pl] == 0xFFFFFFFF] = 0
    return out


# the rows. words: of the record; read / held: the read-back and how many of the record's words it covers; setup: which contexts hold it; small / not_ready / bad: the refusals'
# (code, text) — text None: the export sets none
ROWS = {
    "radiance": dict(words=4, pack="pack_shard", unpack="unpack_shard", read=_read_radiance, held=4, setup="planes", small=("destination too small", "source too small"),
                     not_ready=((INVALID, "bad argument"), (INVALID, "bad argument")), bad="bad argument"),
    "feedback": dict(words=3, pack="neeat_pack_feedback", unpack="neeat_unpack_feedback", read=_read_feedback, held=2, setup="neeat",
                     small=("destination too small (12 bytes per owned pixel)", "source too small (12 bytes per pixel of that rank)"),
                     not_ready=((NOT_READY, "no NEE-AT frame yet: pt_set_neeat, then pt_render"),) * 2, bad=None),
    "guides": dict(words=4, pack="pack_stable_plane_guides", unpack="unpack_stable_plane_guides", read=_read_guides, held=4, setup="planes",
                   small=("destination too small (16 bytes per owned pixel)", "source too small (16 bytes per pixel of that rank)"),
                   not_ready=((NOT_READY, NO_PLANES), (NOT_READY, NO_PLANES + " (it allocates the buffers)")), bad=None),
    "planes": dict(words=71, pack="pack_stable_planes", unpack="unpack_stable_planes", read=_read_planes, held=71, setup="planes",
                   small=("destination too small (pt_stable_planes_shard_bytes)", "source too small (pt_stable_planes_shard_bytes)"),
                   not_ready=((NOT_READY, NO_PLANES), (NOT_READY, NO_PLANES + " (it allocates the buffers)")), bad=None),
}


def _fill_planes(t):      # the realtime passes and a reference-mode sample: planes, guides and radiance
    sc, cam = scenes.stable_planes_zoo(); t.set_scene(sc); t.set_settings(scenes.config_settings("C2"))
    def frame(w, h):
        t.set_camera(scenes.bridge_camera(w, h, **cam)); t.resize(w, h)
        prm = scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cam), sub_samples=1)
        t.build_stable_planes(5, prm); t.fill_stable_planes(5, prm); t.render(0, 1)
    t.frame = frame; frame(W, H)


def _fill_neeat(t):      # one reference-mode frame with the baker: the reservoirs and the exported depth
    sc, cam = scenes.bistro_like(scale=0.02, tex_size=128); t.set_scene(sc); t.set_settings(scenes.default_settings(NEEType=2, useFp16Types=1))
    t.set_camera(scenes.bridge_camera(W, H, **cam)); t.resize(W, H); t.set_neeat(True)
    t.set_view_projection(scenes.view_projection(W, H, **cam)); t.render(0, 1)      # (with a view projection the frame exports its depth: the third word is not zero)


FILL = {"planes": _fill_planes, "neeat": _fill_neeat}


def _device_words(n):
    """n zeroed words on the device, for the library to write. The library packs on a stream of its own that does not wait for torch's: torch's fill must have run before
    the pointer is handed over, or it may land on top of what the library wrote."""
    import torch
    b = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda"); torch.cuda.synchronize(); return b      # (an empty rank still hands in a pointer)


@pytest.fixture(scope="module")
def frames():
    """setup -> world -> (the unsharded context, the ranks, every rank's pixel list); filled once, the ranks' records packed once (before anything is unpacked anywhere)"""
    import rtxpt_amd as pt
    out, made = {}, []
    for setup, fill in FILL.items():
        one = pt.PathTracer(); fill(one); made.append(one); out[setup] = {}
        for world in WORLDS:
            ranks = [pt.PathTracer(shard_rank=r, shard_count=world) for r in range(world)]
            for t in ranks: fill(t)
            made += ranks; out[setup][world] = (one, ranks, [pt.shard_layout(W, H, r, world) for r in range(world)])
    packed = {}
    for name, row in ROWS.items():
        for world, (one, ranks, px) in out[row["setup"]].items():
            for r, t in enumerate(ranks):
                b = _device_words(px[r].size * row["words"])
                getattr(t, row["pack"])(b.data_ptr(), px[r].size * row["words"] * 4); packed[(name, world, r)] = b
    out["packed"] = packed
    yield out
    for t in made: t.close()


def _words(buf, n, words): return buf.cpu().numpy().view(np.uint32)[:n * words].reshape(n, words)


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", list(ROWS))
def test_pack_layout_and_unpack(frames, name, world):
    row = ROWS[name]; one, ranks, px = frames[row["setup"]][world]; packed = frames["packed"]; held = row["held"]
    assert sum(p.size for p in px) == W * H and (world != 8 or [p.size for p in px].count(0) == 2)
    # pack layout: rank r's buffer is its read-back at its pixels, in pt_shard_layout order
    for r, t in enumerate(ranks):
        ys, xs = _tiles(px[r]); assert t.shard_info()[0] == px[r].size
        if not px[r].size: continue      # (an empty rank has packed, in `frames`, and is unpacked below; it has traced nothing to read back)
        assert np.array_equal(_words(packed[(name, world, r)], px[r].size, row["words"])[:, :held], row["read"](t)[ys, xs]), "rank %d" % r
    # selective unpack on a rank 0 of this row's own (no other row's unpack has been there): exactly those ranks' pixels change, to what their owners hold
    import rtxpt_amd as pt
    root = pt.PathTracer(shard_rank=0, shard_count=world); FILL[row["setup"]](root); some = [r for r in range(1, world) if r % 2 == 1]
    want = row["read"](root)
    for r in some:
        getattr(root, row["unpack"])(packed[(name, world, r)].data_ptr(), px[r].size * row["words"] * 4, r)
        ys, xs = _tiles(px[r]); want[ys, xs] = _words(packed[(name, world, r)], px[r].size, row["words"])[:, :held]
    assert np.array_equal(row["read"](root), want)
    # full unpack: with every rank in (an empty one too), rank 0 holds the unsharded context's record
    for r in range(1, world): getattr(root, row["unpack"])(packed[(name, world, r)].data_ptr(), px[r].size * row["words"] * 4, r)
    got, whole = row["read"](root), row["read"](one)
    root.close()
    assert np.array_equal(_live(got), _live(whole)) if name == "planes" else np.array_equal(got, whole)


@pytest.mark.parametrize("name", ["radiance", "feedback", "guides"])
def test_the_ranks_records_are_the_unsharded_contexts_record(frames, name):
    """every word of the record, also one without a getter (the reservoirs' exported depth): the ranks' packed buffers, put in the unsharded context's pixel order, are that
    context's own packed buffer; and that context takes a changed record back word for word (its own pack is its read-back)"""
    import torch
    import rtxpt_amd as pt
    row = ROWS[name]; words = row["words"]; n = W * H * words
    def pack_of(t): b = _device_words(n); getattr(t, row["pack"])(b.data_ptr(), n * 4); return b
    for world in WORLDS:
        one, ranks, px = frames[row["setup"]][world]
        whole = pack_of(one)
        order = pt.shard_layout(W, H, 0, 1); at = np.zeros((H, W), np.int64); ys, xs = _tiles(order); at[ys, xs] = np.arange(W * H)
        got = np.zeros((W * H, words), np.uint32)
        for r in range(world):
            ys, xs = _tiles(px[r]); got[at[ys, xs]] = _words(frames["packed"][(name, world, r)], px[r].size, words)
        want = _words(whole, W * H, words)
        assert np.array_equal(got, want), "world %d: differing words per column %s of %d pixels" % (world, (got != want).sum(0).tolist(), W * H)
    if name == "feedback": assert len(np.unique(want[:, 2])) > 16      # (the exported depth is a picture, not a constant)
    changed = whole ^ 0x00010001; torch.cuda.synchronize()
    getattr(one, row["unpack"])(changed.data_ptr(), n * 4, 0); assert torch.equal(pack_of(one), changed)
    getattr(one, row["unpack"])(whole.data_ptr(), n * 4, 0); assert torch.equal(pack_of(one), whole)


def _refused(call, code, text):
    import rtxpt_amd as pt
    with pytest.raises(pt.PtError) as e: call()
    assert e.value.code == code and (text is None or str(e.value).endswith(": " + text)), str(e.value)


@pytest.mark.parametrize("name", list(ROWS))
def test_refusals(frames, name):
    """a null context, a null pointer, a context that is not ready, a buffer one byte too small, rank >= world: the codes and texts of every export"""
    import ctypes
    import rtxpt_amd as pt
    row = ROWS[name]; one, ranks, px = frames[row["setup"]][4]; t = ranks[1]; n = px[1].size * row["words"] * 4; buf = frames["packed"][(name, 4, 1)]; ptr = buf.data_ptr()
    pack, unpack = getattr(t, row["pack"]), getattr(t, row["unpack"])
    L = pt.load_library(); cpack, cunpack = getattr(L, "pt_" + row["pack"]), getattr(L, "pt_" + row["unpack"])
    assert cpack(None, ctypes.c_void_p(ptr), ctypes.c_size_t(n)) == INVALID and cunpack(None, ctypes.c_void_p(ptr), ctypes.c_size_t(n), ctypes.c_uint32(1)) == INVALID
    _refused(lambda: pack(0, n), INVALID, row["bad"]); _refused(lambda: unpack(0, n, 1), INVALID, row["bad"])
    _refused(lambda: pack(ptr, n - 1), INVALID, row["small"][0]); _refused(lambda: unpack(ptr, n - 1, 1), INVALID, row["small"][1])
    _refused(lambda: unpack(ptr, n, 4), INVALID, row["bad"])
    # not ready: the radiance before pt_resize; the reservoirs before a NEE-AT frame, the planes before a build pass of this frame size
    blank = pt.PathTracer(shard_rank=1, shard_count=4)
    if name != "radiance": blank.resize(W, H)
    _refused(lambda: getattr(blank, row["pack"])(ptr, n), *row["not_ready"][0]); _refused(lambda: getattr(blank, row["unpack"])(ptr, n, 1), *row["not_ready"][1])
    blank.close()
    assert np.array_equal(_words(buf, px[1].size, row["words"])[:, :row["held"]], row["read"](t)[_tiles(px[1])])      # and nothing was written


def test_the_two_gathers_interleaved_and_across_a_resize():
    """One context with a world-of-one communicator: pt_gather_stable_planes, then pt_gather, at 70 x 45, at 45 x 70 and at 70 x 45 again — the loop-back poisons the context's
    buffers between pack and unpack, so what is read afterwards has been through the staging and RCCL: the large record grows the staging, the small one reuses it."""
    import rtxpt_amd as pt
    t = pt.PathTracer(); _fill_planes(t)
    t.gather(); t.gather_stable_planes()      # no communicator, a world of one: nothing to do
    t.comm_init(pt.comm_unique_id(), 0, 1)
    for w, h in ((W, H), (H, W), (W, H)):
        t.frame(w, h)
        planes, radiance = _read_planes(t), _read_radiance(t)
        for _ in range(2):
            t.gather_stable_planes(); t.gather()
            assert np.array_equal(_read_planes(t), planes) and np.array_equal(_read_radiance(t), radiance), (w, h)
    t.comm_destroy(); t.close()


def test_a_sharded_context_gathers_only_with_a_communicator(frames):
    one, ranks, px = frames["planes"][4]
    for t in (ranks[0], ranks[3]):
        _refused(t.gather, NOT_READY, "pt_comm_init first"); _refused(t.gather_stable_planes, NOT_READY, "pt_comm_init first")
    before = _read_radiance(one); one.gather(); one.gather_stable_planes(); assert np.array_equal(_read_radiance(one), before)      # unsharded, no communicator: nothing to do
    import rtxpt_amd as pt
    blank = pt.PathTracer(shard_rank=0, shard_count=4)
    _refused(blank.gather, NOT_READY, "pt_resize first"); blank.resize(W, H); _refused(blank.gather_stable_planes, NOT_READY, NO_PLANES)
    blank.close()
