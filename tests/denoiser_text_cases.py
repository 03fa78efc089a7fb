"""The cases the denoiser passes are pinned on, shared by the CPU tests that hold the numpy restatement against the compiled reference text (tests/test_denoiser_inputs_text.py),
the fixture generator (tests/golden/make_denoiser_inputs_golden.py) and the GPU tests (tests/test_gpu_zzz_denoiser_inputs.py, which need no oracle: they read the fixture).

  zoo frames      the oracle's build + fill + DenoiseSpecHitT of stable_planes_cases (the oracle equals the reference text there: tests/test_stable_planes.py)
  thin lens       the fp32 zoo through a camera with ApertureRadius > 0: the NRD pass's viewZ takes Bridge::computeCameraRay's lens sample
  realtime        two frames of realtime_cases' zoo_realtime with a moving camera
  fuzz            seeded synthetic frames built record by record, drawn so that every branch of the three entry points is taken both ways (branch_census counts them)
"""
import numpy as np
from rtxpt_amd import scenes
import denoiser_inputs_ref as ref
import stable_planes_cases as spc
import realtime_cases as rc

f32 = np.float32
ZOO = ("zoo_fp32", "zoo_lp16", "zoo_two_planes_no_psr", "zoo_one_plane_depth4", "zoo_object_motion")
THIN_LENS = dict(aperture_radius=0.05, focal_distance=3.0)      # a lens wide enough to move every ray origin by centimetres


def zoo_setup(name, w=spc.W, h=spc.H, **camera):
    """spc.setup at any size, with bridge-camera overrides (the thin lens)"""
    lp16, over, kw = spc.cases()[name][:3]
    sc, cam = scenes.stable_planes_zoo(*spc.cases()[name][3:]); cam = dict(cam); cam.update(camera)
    S = scenes.config_settings("C2")
    for k, v in over.items(): S[k] = v
    if lp16: S["useFp16Types"] = 1
    camd = scenes.bridge_camera(w, h, **cam)
    prev = dict(cam); prev["pos"] = tuple(np.asarray(cam["pos"]) + np.array([0.03, 0.01, 0.02]))
    prm = scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cam), prev_world_to_clip=scenes.view_projection(w, h, **prev), sub_samples=spc.SUBSAMPLES, **kw)
    return sc, camd, S, prm, lp16


def oracle_zoo_case(name, w=spc.W, h=spc.H, tag=None, **camera):
    """one zoo frame as the oracle renders it: build pass, the fill passes, DenoiseSpecHitT"""
    from oracle import ptref
    motion = name in spc.motion_cases()
    sc, camd, S, prm, lp16 = zoo_setup(spc.motion_cases()[name] if motion else name, w, h, **camera)
    o = ptref.Oracle(lp16=lp16); o.set_scene(sc); o.set_camera(camd); o.set_settings(S); o.resize(w, h)
    if motion: o.set_previous_pose(*scenes.previous_pose(sc))
    fr = o.build_stable_planes(spc.SAMPLE, prm)
    for s in range(spc.SUBSAMPLES): o.fill_stable_planes(spc.SAMPLE + s, prm, fr)
    fr["spec_hit_t"] = ptref.denoise_spec_hit_t(fr["depth"], fr["spec_hit_t"])
    rays = None
    if camera:      # the restatement's camera_rays stops at the pinhole camera: a thin-lens case takes the oracle's rays (ptref_camera_ray), one call a pixel
        rays = {}
        for p in range(3):
            a = np.array([[o.camera_ray(x, y, spc.SAMPLE + p) for x in range(w)] for y in range(h)], f32); rays[p] = (a[..., :3].copy(), a[..., 3:].copy())
    o.close()
    return dict(name=tag or name, frame=fr, sp=prm, dn=ref.case_params(camd), cam=camd, S=S, w=w, h=h, base=spc.SAMPLE, rays=rays)


def oracle_realtime_cases(frames=2):
    """realtime_cases' zoo_realtime with the oracle: the baker around the build pass, the fill passes, DenoiseSpecHitT; the camera moves between the frames"""
    from oracle import ptref
    make, S, w, h, _, subs, step, kw = rc.cases()["zoo_realtime"]
    sc, cam = make()
    o = ptref.Oracle(lp16=bool(int(S["useFp16Types"]))); o.set_scene(sc); o.set_camera(scenes.bridge_camera(w, h, **cam)); o.set_settings(S); o.resize(w, h); o.set_neeat(True)
    out = []
    for f in range(frames):
        cur, prev = rc.camera(cam, step, f), rc.camera(cam, step, max(f - 1, 0))
        prm = scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cur), prev_world_to_clip=scenes.view_projection(w, h, **prev), sub_samples=subs, **kw)
        camd = scenes.bridge_camera(w, h, **cur); o.set_camera(camd)
        o.neeat_update_begin(); fr = o.build_stable_planes(f * subs, prm); o.neeat_update_end(fr["depth"], fr["motion_vectors"])
        for s in range(subs): o.fill_stable_planes(f * subs + s, prm, fr)
        fr = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in fr.items()}
        fr["spec_hit_t"] = ptref.denoise_spec_hit_t(fr["depth"], fr["spec_hit_t"])
        out.append(dict(name="zoo_realtime_frame%d" % f, frame=fr, sp=prm, dn=ref.case_params(camd), cam=camd, S=S, w=w, h=h, base=f * subs, rays=None))
    o.close()
    return out


def hand_text_cases():
    """test_denoiser_inputs.hand_cases with the camera the GPU suite gives them (the zoo's, at the frame's size)"""
    import test_denoiser_inputs as cpu
    _, cam = scenes.stable_planes_zoo(); out = []
    for c in cpu.hand_cases():
        out.append(dict(name="hand_" + c["name"], frame=c["frame"], sp=c["sp"], dn=c["dn"], cam=scenes.bridge_camera(c["w"], c["h"], **cam), S=scenes.config_settings("C2"), w=c["w"], h=c["h"], base=0, rays=None))
    return out


# ---- the seeded fuzz. (width, height, active planes, grey luminance, DLSS-RR clamp K, suppression K): sizes of at least 4 096 pixels, one of them no multiple of 8 either way,
# plane counts 3, 2, 1; K = 0 once; a grey luminance large enough for NRDRadianceClamp's min(255, ...) to be the bound once
FUZZ = ((64, 64, 3, 0.18, 1.5, 0.6), (72, 57, 2, 0.18, 2.0, 0.6), (128, 32, 1, 0.18, 1.0, 0.0), (67, 62, 3, 4.0, 0.0, 0.3))


def _unit(rng):
    v = rng.normal(size=3)
    return (v / np.linalg.norm(v)).astype(f32)


def fuzz_case(index):
    w, h, active, grey, K, suppress = FUZZ[index]
    rng = np.random.default_rng(0xD150 + index)
    fr = ref.make_frame(w, h)
    pick = lambda values, p=None: values[rng.choice(len(values), p=p)]
    for y in range(h):
        for x in range(w):
            sky_pixel = rng.random() < 0.08          # nothing but sky (or nothing at all) on every plane: the guide normal stays at its 1e-6 start, the albedo floor applies
            black = rng.random() < 0.06              # no radiance anywhere: max3(combined) = 0
            n0 = _unit(rng)
            for p in range(3):                       # (planes beyond the active count get records too: the text must not look at them)
                if rng.random() >= (0.9, 0.6, 0.45)[p]: continue
                v = int(pick((1, 1, 2, 3, 5)))
                branch = 0 if rng.random() < 0.03 else (1 << (2 * (v - 1))) | int(rng.integers(0, 1 << (2 * (v - 1)))) | (int(rng.integers(0, 2)) << (2 * (v - 1) + 1))      # firstbithigh / 2 + 1 = v either way; 0: the just-started id
                thp = {0: (0, 0, 0), 1: tuple(rng.uniform(0.02, 0.9, 3)), 2: tuple(rng.uniform(1.1, 3.0, 3)), 3: (0.0, float(rng.uniform(0, 1)), 0.0)}[int(pick((0, 1, 1, 1, 2, 3)))]
                est = lambda: tuple(0.0 if rng.random() < 0.12 else float(rng.uniform(0.01, 1.0)) for _ in range(3))
                big = rng.random() < 0.15
                rad = np.zeros(3) if (black or rng.random() < 0.1) else rng.uniform(0.0, 600.0 if big else 2.0, 3)
                normal = -n0 if (p == 1 and rng.random() < 0.2) else (n0 if p == 0 else _unit(rng))      # some plane-1 normals oppose plane 0's
                rec = ref.make_record(origin=rng.uniform(-2, 2, 3), direction=_unit(rng), scene_length=np.inf if (sky_pixel or rng.random() < 0.12) else float(rng.uniform(0.3, 20.0)),
                                      thp=thp, mv=tuple(rng.uniform(-3, 3, 3)), roughness=float(pick((0.0, 0.05, 0.12, 0.2, 0.3, 0.6, 1.0))), vertex=v, diff_est=est(), spec_est=est(),
                                      normal=normal, noisy=tuple(rad) + (float(rng.uniform(0, 1.5) * rad.mean()),))
                if rng.random() < 0.04: rec[15] = rng.integers(0, 1 << 32, dtype=np.uint64).astype(np.uint32)      # any word is an input to OctToNDirUnorm32
                ref.put(fr, x, y, p, branch, rec, w, h)
            ref.set_dominant(fr, x, y, int(rng.integers(0, 3)), float(rng.uniform(0.1, 30.0)))
            if not black and rng.random() < 0.6:
                fr["stable_radiance"][y, x] = ref.f32_to_half(np.append(rng.uniform(0, 40.0 if rng.random() < 0.2 else 1.0, 3), 0).astype(f32))
            fr["spec_hit_t"][y, x] = pick((0.0, 5e-4, float(rng.uniform(0.01, 15.0))), p=(0.3, 0.1, 0.6))
            fr["motion_vectors"][y, x] = ref.f32_to_half(np.append(rng.uniform(-4, 4, 3), 0).astype(f32))
    _, cam = scenes.stable_planes_zoo()
    cur = dict(cam); prev = dict(cam); prev["pos"] = tuple(np.asarray(cam["pos"]) + np.array([0.05, -0.02, 0.03]))
    camd = scenes.bridge_camera(w, h, **cur)
    sp = scenes.stable_planes_params(w, h, scenes.view_projection(w, h, **cur), prev_world_to_clip=scenes.view_projection(w, h, **prev), active_planes=active)
    dn = ref.case_params(camd, grey=grey, DLSSRRBrightnessClampK=K, stablePlanesSuppressPrimaryIndirectSpecularK=suppress)
    return dict(name="fuzz%d" % index, frame=fr, sp=sp, dn=dn, cam=camd, S=scenes.config_settings("C2"), w=w, h=h, base=3, rays=None)


def crop(case, w, h):
    """the top-left w x h pixels of a case as a frame of its own (records re-addressed for the smaller frame)"""
    fr, W, H = case["frame"], case["w"], case["h"]
    out = ref.make_frame(w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    out["header"] = fr["header"][:, :h, :w].copy()
    for p in range(3): out["planes"][scenes.stable_planes_address(xs, ys, p, w, h)] = fr["planes"][scenes.stable_planes_address(xs, ys, p, W, H)]
    for k in ("stable_radiance", "depth", "spec_hit_t", "motion_vectors", "throughput"): out[k] = fr[k][:h, :w].copy()
    c = dict(case); c["frame"] = out; c["w"], c["h"] = w, h
    _, cam = scenes.stable_planes_zoo(); c["cam"] = scenes.bridge_camera(w, h, **cam)      # the zoo's camera at the window's size (same pose: the case's matWorldToView stays)
    return c


def branch_census(case, rr, per):
    """How many pixels take each side of each branch of the three entry points, from the frame's inputs and the compiled text's outputs alone (rr: its DLSS-RR outputs,
    per: {plane: its state after that plane's prepare}). name -> (pixels on one side, pixels on the other)."""
    fr, w, h = case["frame"], case["w"], case["h"]
    P = ref.Planes(fr, w, h); active = int(min(max(int(case["sp"]["activeStablePlaneCount"]), 1), 3)); dn = case["dn"]
    c = {}
    live_any = np.zeros((h, w), bool)
    for p in range(active):
        rec = P.rec(p); valid = P.branch(p) != ref.INVALID; finite = np.isfinite(Planes_f(rec, 7)); live = valid & finite; live_any |= live
        c["plane %d branch id valid / invalid" % p] = (valid.sum(), (~valid).sum())
        c["plane %d SceneLength finite / inf" % p] = (live.sum(), (valid & ~finite).sum())
        dE, sE = ref.Planes.unpack_two(rec[..., 12:15])
        zero = ((dE == 0) | (sE == 0)).any(-1)
        c["plane %d BSDF estimate with / without an exact zero" % p] = ((live & zero).sum(), (live & ~zero).sum())
        vi = ref.vertex_index_from_branch(P.branch(p))
        c["plane %d vertex index <= 1 / > 1" % p] = ((live & (vi <= 1)).sum(), (live & (vi > 1)).sum())
        c["plane %d dominant / not dominant" % p] = ((live & (P.dominant() == p)).sum(), (live & (P.dominant() != p)).sum())
        border = np.zeros((h, w), bool); border[0] = border[-1] = True; border[:, 0] = border[:, -1] = True
        c["plane %d relaxed pixel at the frame border / inside" % p] = ((live & (vi > 1) & border).sum(), (live & (vi > 1) & ~border).sum())
        # NRDRadianceClamp: a clamped radiance leaves with the clamp's luminance (to rounding), an unclamped one with less
        cmax = min(f32(255), f32(dn["preExposedGrayLuminance"]) * (f32(dn["denoiserRadianceClampK"]) * f32(16)))
        with np.errstate(all="ignore"):
            lum = np.maximum(ref.luminance(per[p]["nrd_diff_radiance_hit_dist"][..., :3]), ref.luminance(per[p]["nrd_spec_radiance_hit_dist"][..., :3]))
        c["plane %d luminance at / below the NRD clamp" % p] = ((live & (lum >= cmax * f32(0.9999))).sum(), (live & (lum < cmax * f32(0.9999))).sum())
        if p >= 1:
            thp, _ = ref.Planes.unpack_two(rec[..., 8:11]); a = ref.average(thp)
            c["plane %d throughput average 0 / in (0, 1)" % p] = ((valid & (a == 0)).sum(), (valid & (a > 0) & (a < 1)).sum())
            c["plane %d throughput average > 1 / <= 1" % p] = ((valid & (a > 1)).sum(), (valid & (a <= 1)).sum())
    # the layer weights of the DLSS-RR pass (PostProcess.hlsl:244-272), recomputed for the census only: every available plane's weight is at least 0.01 / (3 x 0.2 + 3 x 0.01 + 0.05),
    # so `weight > 1e-6` can be false for no input at all; the census shows it (the second count is 0 by construction, and test_fuzz... asserts exactly that)
    tw = np.zeros((h, w, 3), f32); tw[..., 0] = 1; av = np.zeros((h, w, 3), f32); av[..., 0] = 1
    for p in range(1, active):
        ok = P.branch(p) != ref.INVALID; thp, _ = ref.Planes.unpack_two(P.rec(p)[..., 8:11]); a = ref.saturate(ref.average(thp))
        tw[..., p] = np.where(ok, a, tw[..., p]); tw[..., 0] = np.where(ok, ref.saturate(tw[..., 0] - a), tw[..., 0]); av[..., p] = np.where(ok, f32(1), av[..., p])
    sw = tw * f32(0.2) + f32(0.01)
    for d in range(3): sw[..., d] = np.where(P.dominant() == d, sw[..., d] + f32(0.05), sw[..., d])
    sw = sw * av; sw = sw / ((sw[..., 0] + sw[..., 1]) + sw[..., 2])[..., None]
    lw = np.stack([(P.branch(p) != ref.INVALID) & np.isfinite(Planes_f(P.rec(p), 7)) for p in range(active)], -1)
    c["layer weight above / not above 1e-6"] = ((lw & (sw[..., :active] > f32(1e-6))).sum(), (lw & ~(sw[..., :active] > f32(1e-6))).sum())
    nr = ref.half_to_f32(rr["rr_normal_roughness"]); rough = nr[..., 3]
    # the guide normal that fell below 1e-5 is replaced by exactly (0, 0, 1); a normalised sum is that only by accident
    reset = (nr[..., 0] == 0) & (nr[..., 1] == 0) & (nr[..., 2] == 1)
    c["guide-normal length below / above 1e-5"] = (reset.sum(), (~reset).sum())
    # the albedo floor: without a live plane and without stable radiance both albedos are 0 and the text adds 0.05; counted where that is certain from the inputs
    sr = ref.stable_radiance(fr); dark = ~live_any & (sr == 0).all(-1)
    floor = rr["rr_diffuse_albedo"] == ref.pack_r11g11b10(np.array([0.05, 0.05, 0.05], f32))
    c["albedo sum below 0.05 (floor added) / not"] = ((dark & floor).sum(), (~floor).sum())
    K = f32(dn["DLSSRRBrightnessClampK"]); mx = ref.max3(rr["output_color"][..., :3])
    with np.errstate(all="ignore"):
        total = sr.copy()
        for p in range(active):
            rec = P.rec(p); live = (P.branch(p) != ref.INVALID) & np.isfinite(Planes_f(rec, 7)); total = np.where(live[..., None], total + ref.Planes.noisy(rec)[..., :3], total)
        before = ref.max3(total)
    c["maxRadiance above / not above DLSSRRBrightnessClampK"] = ((before > K).sum(), (~(before > K)).sum())
    assert np.all(mx[before > K] <= K * f32(1.0001))
    ht = np.asarray(fr["spec_hit_t"], f32)
    c["specHitT above / not above 1e-3"] = ((ht > f32(1e-3)).sum(), (~(ht > f32(1e-3))).sum())
    c["mixed roughness below / not below kSpecularRoughnessThreshold"] = ((rough < f32(0.25)).sum(), (~(rough < f32(0.25))).sum())
    taken = (ht > f32(1e-3)) & (rough < f32(0.25))
    r0 = P.rec(0); d0 = r0[..., 4:7].view(f32); n0 = ref.Planes.normal(r0)
    with np.errstate(all="ignore"):
        zobj = ref.dot(n0, d0 - (f32(2) * ref.dot(d0, n0))[..., None] * n0) * ht
        axis_z = np.where(zobj < 0, -n0[..., 2], n0[..., 2])
    c["specular MV: zObj < 0 / >= 0"] = ((taken & (zobj < 0)).sum(), (taken & (zobj >= 0)).sum())
    c["specular MV: n.z < 0 / >= 0 in the ONB"] = ((taken & (axis_z < 0)).sum(), (taken & (axis_z >= 0)).sum())
    return {k: (int(a), int(b)) for k, (a, b) in c.items()}


def Planes_f(rec, i): return rec[..., i].view(f32)
