"""An independent numpy restatement of the device denoiser (rtxpt_amd/csrc/pt_relax.h, docs/WIDENING.md N5): the temporal pass, the history clamp and the a-trous passes of one
plane, over the NRD buffers tests/denoiser_inputs_ref.py's nrd_prepare() leaves. A sibling of denoiser_inputs_ref.py with the same arithmetic rules: every step one binary32
operation in the stated order (numpy float32 arrays and constants), dot products as (x + y) + z, min / max / saturate as comparisons, sums over taps in scan-line order
(dy outer, dx inner), the bilinear 2 x 2 in the order (0, 0) (1, 0) (0, 1) (1, 1). The device is held to it bit for bit (tests/test_gpu_zzz_relax_denoiser.py).

A plane's history is a dict of arrays (new_history()); settings are anything indexable by the names of PtDenoiseSettings (a dict from settings(), or a record of
rtxpt_amd.DENOISE_SETTINGS_DTYPE)."""
import numpy as np
import denoiser_inputs_ref as ref

f32 = np.float32
FLT_MAX = ref.FLT_MAX
fmax, fmin, saturate, luminance, dot = ref.fmax, ref.fmin, ref.saturate, ref.luminance, ref.dot

# NrdConfig.cpp:15-47, SampleUI.h:294-296; luminanceSigmaScale is the project's own
DEFAULTS = dict(atrousIterationNum=5, depthThreshold=0.004, lobeAngleFraction=0.7, diffuseMaxAccumulatedFrameNum=25, specularMaxAccumulatedFrameNum=40,
                diffuseMaxFastAccumulatedFrameNum=5, specularMaxFastAccumulatedFrameNum=6, enableAntiFirefly=1, disocclusionThreshold=0.03, disocclusionThresholdAlternate=0.2,
                useDisocclusionThresholdMix=1, luminanceSigmaScale=4.0)
HISTORY_CLAMP_SIGMA, HISTORY_CLAMP_RELAX_MUL, LUM_EPS, SPATIAL_VARIANCE_BELOW, MAX_REPROJECTION = f32(2), f32(3), f32(1e-6), f32(4), f32(32768)
B3 = (f32(0.375), f32(0.25), f32(0.0625))      # (6, 4, 1) / 16 by |offset|


def settings(**kw):
    unknown = set(kw) - set(DEFAULTS); assert not unknown, unknown
    return dict(DEFAULTS, **kw)


def ndir_to_oct_unorm32(n):
    """Utils.hlsli NDirToOctUnorm32 as the device evaluates it (pt_lights.h), over [..., 3]"""
    n = np.asarray(n, f32)
    s = (np.abs(n[..., 0]) + np.abs(n[..., 1])) + np.abs(n[..., 2])
    n = n / s[..., None]
    sx, sy = np.where(n[..., 0] >= 0, f32(1), f32(-1)).astype(f32), np.where(n[..., 1] >= 0, f32(1), f32(-1)).astype(f32)
    fold = ~(n[..., 2] >= 0)
    x = np.where(fold, (f32(1) - np.abs(n[..., 1])) * sx, n[..., 0]).astype(f32)
    y = np.where(fold, (f32(1) - np.abs(n[..., 0])) * sy, n[..., 1]).astype(f32)
    x, y = x * f32(0.5) + f32(0.5), y * f32(0.5) + f32(0.5)
    x, y = saturate(x * f32(0.5) + f32(0.5)), saturate(y * f32(0.5) + f32(0.5))
    return (x * f32(65534)).astype(np.uint32) | ((y * f32(65534)).astype(np.uint32) << np.uint32(16))


def finite0(v): return np.where(np.abs(v) <= FLT_MAX, v, f32(0)).astype(f32)


def shifted(a, dx, dy):
    """(b, inside): b[y, x] = a[y + dy, x + dx] where that is inside the frame (0 elsewhere)"""
    h, w = a.shape[:2]
    out = np.zeros_like(a); inside = np.zeros((h, w), bool)
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    if y1 > y0 and x1 > x0:
        out[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]; inside[y0:y1, x0:x1] = True
    return out, inside


def same_surface(expected_abs_z, n, abs_z, n_t, thr, cone_cos):
    return (np.abs(abs_z - expected_abs_z) <= thr * expected_abs_z) & (dot(n, n_t) >= cone_cos)


def new_history(width, height):
    z = lambda *s: np.zeros((height, width) + s, f32)
    return {"diff_len": z(4), "spec_len": z(4), "fast_diff_m1": z(4), "fast_spec_m1": z(4), "m2": z(2), "view_z": z(), "oct": np.zeros((height, width), np.uint32)}


def _accumulate(valid, c, lum, h, hf, hm2, max_frames, max_fast):
    length = fmin(h[..., 3] + f32(1), f32(max_frames))
    alpha = f32(1) / length; alpha_fast = f32(1) / fmin(length, f32(max_fast))
    acc = h[..., :3] + (c - h[..., :3]) * alpha[..., None]
    fast = hf[..., :3] + (c - hf[..., :3]) * alpha_fast[..., None]
    m1 = hf[..., 3] + (lum - hf[..., 3]) * alpha
    m2 = hm2 + (lum * lum - hm2) * alpha
    v = valid[..., None]
    return (np.where(v, acc, c).astype(f32), np.where(v, fast, c).astype(f32), np.where(valid, length, f32(1)).astype(f32), np.where(valid, m1, lum).astype(f32),
            np.where(valid, m2, lum * lum).astype(f32))


def temporal(nrd, S, prev, width, height):
    """the temporal pass: returns (history of this frame before the clamp, guide); prev: the plane's history of the previous frame, or None (reset / first frame)"""
    h, w = height, width
    z = np.asarray(nrd["nrd_view_z"], f32); sky = z == FLT_MAX
    nr = np.asarray(nrd["nrd_normal_roughness"], f32)
    oct_n = ndir_to_oct_unorm32(np.where(sky[..., None], f32([0, 0, 1]), nr[..., :3]).astype(f32))
    n = ref.oct_to_ndir_unorm32(oct_n)
    abs_z = np.abs(z)
    cd, cs = finite0(np.asarray(nrd["nrd_diff_radiance_hit_dist"], f32)[..., :3]), finite0(np.asarray(nrd["nrd_spec_radiance_hit_dist"], f32)[..., :3])
    ld, ls = luminance(cd), luminance(cs)
    dt, dta = f32(S["disocclusionThreshold"]), f32(S["disocclusionThresholdAlternate"])
    thr = (dt + (dta - dt) * ref.load_unorm8(nrd["nrd_disocclusion_threshold_mix"])).astype(f32) if int(S["useDisocclusionThresholdMix"]) else np.full((h, w), dt, f32)
    cone = f32(1) - f32(S["lobeAngleFraction"])
    if int(S["enableAntiFirefly"]):
        max_d = np.zeros((h, w), f32); max_s = np.zeros((h, w), f32); any_valid = np.zeros((h, w), bool)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if not dx and not dy: continue
                zt, ins = shifted(z, dx, dy); nt, _ = shifted(n, dx, dy); ldt, _ = shifted(ld, dx, dy); lst, _ = shifted(ls, dx, dy)
                valid = ins & (zt != FLT_MAX) & same_surface(abs_z, n, np.abs(zt), nt, thr, cone)
                any_valid |= valid
                max_d = np.where(valid, fmax(max_d, ldt), max_d).astype(f32); max_s = np.where(valid, fmax(max_s, lst), max_s).astype(f32)
        cd = np.where((any_valid & (ld > max_d))[..., None], cd * (max_d / ld)[..., None], cd).astype(f32)
        cs = np.where((any_valid & (ls > max_s))[..., None], cs * (max_s / ls)[..., None], cs).astype(f32)
        ld, ls = luminance(cd), luminance(cs)
    mv = ref.half_to_f32(np.asarray(nrd["nrd_motion_vectors"], np.uint16))
    ys, xs = np.mgrid[0:h, 0:w]
    fx = ((xs.astype(f32) + f32(0.5)) + mv[..., 0]) - f32(0.5); fy = ((ys.astype(f32) + f32(0.5)) + mv[..., 1]) - f32(0.5)
    wsum = np.zeros((h, w), f32); h0, h1, h2, h3 = (np.zeros((h, w, 4), f32) for _ in range(4)); m2d = np.zeros((h, w), f32); m2s = np.zeros((h, w), f32)
    if prev is not None:
        ok = (np.abs(fx) < MAX_REPROJECTION) & (np.abs(fy) < MAX_REPROJECTION)
        fx, fy = np.where(ok, fx, f32(0)).astype(f32), np.where(ok, fy, f32(0)).astype(f32)
        flx, fly = np.floor(fx).astype(f32), np.floor(fy).astype(f32)
        tx, ty = fx - flx, fy - fly
        ix, iy = flx.astype(np.int64), fly.astype(np.int64)
        expected = abs_z + mv[..., 2]
        bw = [(f32(1) - tx) * (f32(1) - ty), tx * (f32(1) - ty), (f32(1) - tx) * ty, tx * ty]
        for k in range(4):
            qx, qy = ix + (k & 1), iy + (k >> 1)
            ins = ok & (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h) & (bw[k] > 0)
            qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            pz = prev["view_z"][qy, qx]
            valid = ins & (pz != FLT_MAX) & same_surface(expected, n, np.abs(pz), ref.oct_to_ndir_unorm32(prev["oct"][qy, qx]), thr, cone)
            b = bw[k]
            wsum = np.where(valid, wsum + b, wsum).astype(f32)
            v4 = valid[..., None]
            h0 = np.where(v4, h0 + prev["diff_len"][qy, qx] * b[..., None], h0).astype(f32); h1 = np.where(v4, h1 + prev["spec_len"][qy, qx] * b[..., None], h1).astype(f32)
            h2 = np.where(v4, h2 + prev["fast_diff_m1"][qy, qx] * b[..., None], h2).astype(f32); h3 = np.where(v4, h3 + prev["fast_spec_m1"][qy, qx] * b[..., None], h3).astype(f32)
            m2d = np.where(valid, m2d + prev["m2"][qy, qx, 0] * b, m2d).astype(f32); m2s = np.where(valid, m2s + prev["m2"][qy, qx, 1] * b, m2s).astype(f32)
    valid = wsum > 0
    h0, h1, h2, h3 = (a / wsum[..., None] for a in (h0, h1, h2, h3)); m2d, m2s = m2d / wsum, m2s / wsum
    acc_d, fast_d, len_d, m1_d, m2_d = _accumulate(valid, cd, ld, h0, h2, m2d, int(S["diffuseMaxAccumulatedFrameNum"]), int(S["diffuseMaxFastAccumulatedFrameNum"]))
    acc_s, fast_s, len_s, m1_s, m2_s = _accumulate(valid, cs, ls, h1, h3, m2s, int(S["specularMaxAccumulatedFrameNum"]), int(S["specularMaxFastAccumulatedFrameNum"]))
    cat = lambda rgb, a: np.where(sky[..., None], f32(0), np.concatenate([rgb, a[..., None]], -1)).astype(f32)
    cur = {"diff_len": cat(acc_d, len_d), "spec_len": cat(acc_s, len_s), "fast_diff_m1": cat(fast_d, m1_d), "fast_spec_m1": cat(fast_s, m1_s),
           "m2": np.where(sky[..., None], f32(0), np.stack([m2_d, m2_s], -1)).astype(f32), "view_z": z.copy(), "oct": np.where(sky, np.uint32(0), oct_n).astype(np.uint32)}
    guide = {"view_z": z.copy(), "oct": cur["oct"].copy(), "normal": n, "roughness": np.where(sky, f32(0), nr[..., 3]).astype(f32),
             "length": np.where(sky, f32(0), fmin(len_d, len_s)).astype(f32)}
    return cur, guide


def history_clamp(nrd, S, cur, guide, width, height):
    """the fast-history clamp: updates cur's accumulated radiance in place and returns the first a-trous input pair (radiance + temporal variance)"""
    h, w = height, width
    sky = guide["view_z"] == FLT_MAX
    relax = ref.load_unorm8(nrd["nrd_combined_history_clamp_relax"])
    cnt = np.zeros((h, w), f32); sums = {k: [np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32)] for k in ("fast_diff_m1", "fast_spec_m1")}
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            skt, ins = shifted(sky, dx, dy); valid = ins & ~skt
            cnt = np.where(valid, cnt + f32(1), cnt).astype(f32)
            for k in sums:
                ft, _ = shifted(cur[k][..., :3], dx, dy)
                sums[k][0] = np.where(valid[..., None], sums[k][0] + ft, sums[k][0]).astype(f32); sums[k][1] = np.where(valid[..., None], sums[k][1] + ft * ft, sums[k][1]).astype(f32)
    out = []
    for key, fast, cap, mi in (("diff_len", "fast_diff_m1", "diffuseMaxFastAccumulatedFrameNum", 0), ("spec_len", "fast_spec_m1", "specularMaxFastAccumulatedFrameNum", 1)):
        hist = cur[key]
        mean = sums[fast][0] / cnt[..., None]; m2 = sums[fast][1] / cnt[..., None]
        sigma = np.sqrt(fmax(m2 - mean * mean, f32(0))).astype(f32)
        k = (HISTORY_CLAMP_SIGMA + relax * (HISTORY_CLAMP_SIGMA * HISTORY_CLAMP_RELAX_MUL)).astype(f32)
        lo, hi = mean - sigma * k[..., None], mean + sigma * k[..., None]
        clamped = fmin(fmax(hist[..., :3], lo), hi)
        do = (~sky) & (hist[..., 3] > f32(int(S[cap])))
        hist[..., :3] = np.where(do[..., None], clamped, hist[..., :3])
        m1 = cur[fast][..., 3]
        var = fmax(cur["m2"][..., mi] - m1 * m1, f32(0))
        out.append(np.where(sky[..., None], f32(0), np.concatenate([hist[..., :3], var[..., None]], -1)).astype(f32))
    return out


def _geometry_weights(C, b, centre, zt, nt):
    if centre: w = np.full(zt.shape, b, f32); return w, w      # the centre tap is its own surface: stops 1
    wz = saturate(f32(1) - np.abs(np.abs(zt) - C["abs_z"]) * C["inv_depth"])
    dn = dot(C["n"], nt)
    g = b * wz
    return g * saturate((dn - C["cone_d"]) * C["inv_cone_d"]), g * saturate((dn - C["cone_s"]) * C["inv_cone_s"])


def atrous(S, guide, in_d, in_s, iteration, last, hit_dist, width, height):
    """one a-trous iteration (step 1 << iteration) over the radiance + variance pairs; last: the result as the denoised radiance (.w: 0 / the hit distance)"""
    h, w = height, width; st = 1 << iteration
    z, n = guide["view_z"], guide["normal"]; sky = z == FLT_MAX
    f = f32(S["lobeAngleFraction"]); lobe_s = f * guide["roughness"]
    C = {"abs_z": np.abs(z), "n": n, "cone_d": f32(1) - f, "inv_cone_d": f32(1) / fmax(f, f32(1e-6)), "cone_s": f32(1) - lobe_s, "inv_cone_s": f32(1) / fmax(lobe_s, f32(1e-6))}      # reciprocals: one division per centre
    C["inv_depth"] = f32(1) / fmax(f32(S["depthThreshold"]) * C["abs_z"], f32(1e-20))
    lum_d, lum_s = luminance(in_d[..., :3]), luminance(in_s[..., :3])
    var_d, var_s = in_d[..., 3].copy(), in_s[..., 3].copy()
    taps = []
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            zt, ins = shifted(z, dx * st, dy * st)
            valid = ins & (zt != FLT_MAX) & ~sky
            if not valid.any(): continue
            taps.append((B3[abs(dx)] * B3[abs(dy)], not dx and not dy, valid, zt, shifted(n, dx * st, dy * st)[0], shifted(in_d, dx * st, dy * st)[0], shifted(in_s, dx * st, dy * st)[0]))
    if iteration == 0:
        E = [np.zeros((h, w), f32) for _ in range(5)]
        for b, centre, valid, zt, nt, dT, sT in taps:
            wd, _ = _geometry_weights(C, b, centre, zt, nt)
            ldt, lst = luminance(dT[..., :3]), luminance(sT[..., :3])
            for i, term in enumerate((wd, wd * ldt, wd * (ldt * ldt), wd * lst, wd * (lst * lst))): E[i] = np.where(valid, E[i] + term, E[i]).astype(f32)
        d1, d2, s1, s2 = E[1] / E[0], E[2] / E[0], E[3] / E[0], E[4] / E[0]
        short = guide["length"] < SPATIAL_VARIANCE_BELOW
        var_d = np.where(short, fmax(d2 - d1 * d1, f32(0)), var_d).astype(f32); var_s = np.where(short, fmax(s2 - s1 * s1, f32(0)), var_s).astype(f32)
    scale = f32(S["luminanceSigmaScale"])
    inv_sigma_d = f32(1) / (scale * np.sqrt(fmax(var_d, f32(0))).astype(f32) + LUM_EPS); inv_sigma_s = f32(1) / (scale * np.sqrt(fmax(var_s, f32(0))).astype(f32) + LUM_EPS)
    sum_d, sum_s = np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32); vd, vs, swd, sws = (np.zeros((h, w), f32) for _ in range(4))
    for b, centre, valid, zt, nt, dT, sT in taps:
        wd, ws = _geometry_weights(C, b, centre, zt, nt)
        if scale > 0:
            wd = wd * saturate(f32(1) - np.abs(luminance(dT[..., :3]) - lum_d) * inv_sigma_d)
            ws = ws * saturate(f32(1) - np.abs(luminance(sT[..., :3]) - lum_s) * inv_sigma_s)
        v3 = valid[..., None]
        sum_d = np.where(v3, sum_d + dT[..., :3] * wd[..., None], sum_d).astype(f32); sum_s = np.where(v3, sum_s + sT[..., :3] * ws[..., None], sum_s).astype(f32)
        vd = np.where(valid, vd + (wd * wd) * (var_d if centre else dT[..., 3]), vd).astype(f32); vs = np.where(valid, vs + (ws * ws) * (var_s if centre else sT[..., 3]), vs).astype(f32)
        swd = np.where(valid, swd + wd, swd).astype(f32); sws = np.where(valid, sws + ws, sws).astype(f32)
    out_d = np.concatenate([sum_d / swd[..., None], (vd / (swd * swd))[..., None]], -1)
    out_s = np.concatenate([sum_s / sws[..., None], (vs / (sws * sws))[..., None]], -1)
    if last: out_d[..., 3] = 0; out_s[..., 3] = hit_dist
    return np.where(sky[..., None], f32(0), out_d).astype(f32), np.where(sky[..., None], f32(0), out_s).astype(f32)


def denoise_plane(nrd, S, prev, width, height, reset=False, stages=None):
    """pt_denoise_plane over the NRD buffers `nrd` (nrd_prepare's state after the plane's call). prev: the plane's history or None. Returns (diffuse [h, w, 4], specular [h, w, 4],
    history lengths [h, w, 2], history for the next frame). stages (a dict): receives the pre-spatial accumulation and every iteration's result."""
    with np.errstate(all="ignore"):
        cur, guide = temporal(nrd, S, None if reset else prev, width, height)
        d, s = history_clamp(nrd, S, cur, guide, width, height)
        if stages is not None: stages["accumulated"] = (d.copy(), s.copy()); stages["iterations"] = []
        n = int(S["atrousIterationNum"]); assert 2 <= n <= 8
        hit = np.asarray(nrd["nrd_spec_radiance_hit_dist"], f32)[..., 3]
        for i in range(n):
            d, s = atrous(S, guide, d, s, i, i + 1 == n, hit, width, height)
            if stages is not None: stages["iterations"].append((d.copy(), s.copy()))
        lengths = np.stack([cur["diff_len"][..., 3], cur["spec_len"][..., 3]], -1).astype(f32)
        return d, s, lengths, cur


def denoise_frame(frame, sp_params, dn_params, S, width, height, rays, histories, state=None, reset=False):
    """pt_denoise_frame: Sample::Denoise's loop with this denoiser. histories: {plane: history} of the previous frame (updated in place). Returns (state, {plane: (diff, spec, lengths)})"""
    active = int(min(max(int(sp_params["activeStablePlaneCount"]), 1), 3))
    st = ref.empty_state(width, height) if state is None else state
    per = {}
    for i, p in enumerate(range(active - 1, -1, -1)):
        st = ref.nrd_prepare(st, frame, sp_params, dn_params, width, height, p, i == 0, *rays[p])
        d, s, lengths, histories[p] = denoise_plane(st, S, histories.get(p), width, height, reset)
        per[p] = (d, s, lengths)
        st["output_color"] = ref.nrd_merge(st, frame, width, height, p, d, s)
    return st, per
