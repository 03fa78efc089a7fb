"""A numpy float32 restatement of adaptive sampling (include/mi355pt.h pt_render_adaptive, rtxpt_amd/csrc/pt_adaptive.h / .hip): the two running means, the per-pixel error,
the per-block tree sum, the compaction of the active lists and the loop over the rounds. Every value is formed by the same binary32 operations in the same order as on the
device, so the tests compare bit for bit. It traces nothing: its input is one picture per sample index, which the tests take from the existing path
(reset_accumulation(); render(s, 1); radiance()) or make up.
"""
import numpy as np

F = np.float32


def fold(mean, col, index):
    """sample `index` (0-based) folded into the running mean of the samples before it: blend = 1 / (index + 1); blend < 1 ? mean + (col - mean) * blend : col (lerpf's order)"""
    blend = F(1.0) / F(index + 1)
    if not blend < F(1.0):
        return col.astype(F).copy()
    return (mean + (col - mean) * blend).astype(F)


def pixel_error(A, H, dark_floor):
    """A, H: [n, 4] float32 -> e [n]: d = |A.x-H.x| + |A.y-H.y| + |A.z-H.z| (left to right), b = A.x + A.y + A.z, e = d / sqrt(max(b, darkFloor)); NaN and inf count as 0"""
    A = np.asarray(A, F); H = np.asarray(H, F)
    with np.errstate(all="ignore"):
        d = (np.abs(A[:, 0] - H[:, 0]) + np.abs(A[:, 1] - H[:, 1])) + np.abs(A[:, 2] - H[:, 2])
        b = (A[:, 0] + A[:, 1]) + A[:, 2]
        e = (d / np.sqrt(np.fmax(b, F(dark_floor)))).astype(F)
        e[~(e < F(np.inf))] = F(0.0)
    return e


def tree_sum(values):
    """up to 64 float32 values in v[0 .. count), zeros behind them; for off in 32, 16, 8, 4, 2, 1: v[i] = v[i] + v[i + off] for i < off; -> v[0]"""
    values = np.asarray(values, F); assert values.size <= 64
    v = np.zeros(64, F); v[:values.size] = values
    with np.errstate(all="ignore"):
        off = 32
        while off:
            v[:off] = v[:off] + v[off:2 * off]
            off >>= 1
    return v[0]


def block_error(e):
    """E of a block whose pixels' errors are e (list order): tree_sum(e) / (float)count"""
    with np.errstate(all="ignore"):
        return F(tree_sum(e) / F(len(e)))


def block_errors(e, blocks):
    """block_error of every (first, count) run of e at once: the same tree, one row of 64 a block"""
    if not blocks:
        return np.zeros(0, F)
    firsts = np.array([f for f, _ in blocks], np.int64); cnt = np.array([c for _, c in blocks], np.int64); assert cnt.min() >= 1 and cnt.max() <= 64
    lanes = np.arange(64)[None, :]; live = lanes < cnt[:, None]
    v = np.zeros((len(blocks), 64), F); v[live] = np.asarray(e, F)[(firsts[:, None] + lanes)[live]]
    with np.errstate(all="ignore"):
        off = 32
        while off:
            v[:, :off] = v[:, :off] + v[:, off:2 * off]
            off >>= 1
        return (v[:, 0] / cnt.astype(F)).astype(F)


def blocks_of(pixels, width):
    """the 8 x 8 screen blocks of a pixel list (x << 16 | y) as runs [(first, count)]: a block's pixels are consecutive entries, and consecutive blocks differ"""
    pixels = np.asarray(pixels, np.uint32)
    if pixels.size == 0:
        return []
    bid = ((pixels & 0xFFFF) >> 3).astype(np.int64) * ((width + 7) // 8) + (pixels >> 19)
    starts = np.concatenate([[0], np.nonzero(bid[1:] != bid[:-1])[0] + 1, [pixels.size]])
    return [(int(a), int(b - a)) for a, b in zip(starts[:-1], starts[1:])]


def run(samples, pixels, min_samples, max_samples, step, threshold, dark_floor):
    """The loop of pt_render_adaptive over one rank's pixel list. samples: [S, h, w, 4] float32, samples[s] the picture of sample index s alone (S >= max_samples unless
    everything retires earlier). Returns a dict: radiance, half [h, w, 4]; counts [h, w] u32; block_error [ceil(h / 8), ceil(w / 8)]; active (u32, list order);
    active_counts (the active pixels of every round traced); retired_at {n: blocks retired at the evaluation at n samples}; stats (PtAdaptiveStats without the time)."""
    samples = np.asarray(samples, F); h, w = samples.shape[1:3]
    assert step >= 2 and step % 2 == 0 and min_samples % step == 0 and max_samples % step == 0 and step <= min_samples <= max_samples
    threshold = F(threshold)
    pixels = np.asarray(pixels, np.uint32)
    A = np.zeros((h, w, 4), F); H = np.zeros((h, w, 4), F); counts = np.zeros((h, w), np.uint32); berr = np.zeros(((h + 7) // 8, (w + 7) // 8), F)
    active = pixels.copy(); blocks = blocks_of(active, w)
    n = 0; rounds = evaluations = 0; traced = 0; active_counts = []; retired_at = {}
    while active.size and n < max_samples:
        ys = (active & 0xFFFF).astype(np.int64); xs = (active >> 16).astype(np.int64)
        active_counts.append(int(active.size))
        a = A[ys, xs]; hf = H[ys, xs]
        for s in range(step):
            index = n + s
            col = samples[index][ys, xs]
            a = fold(a, col, index)
            if index % 2 == 0:
                hf = fold(hf, col, index // 2)
        A[ys, xs] = a; H[ys, xs] = hf; counts[ys, xs] += np.uint32(step)
        n += step; rounds += 1; traced += int(active.size) * step
        if n < min_samples:
            continue
        evaluations += 1
        e = pixel_error(a, hf, dark_floor)
        keep_pix = []; keep_blocks = []; kept = 0
        for (first, count), E in zip(blocks, block_errors(e, blocks)):
            berr[ys[first] >> 3, xs[first] >> 3] = E
            if not E < threshold:
                keep_blocks.append((kept, count)); keep_pix.append(active[first:first + count]); kept += count
        retired_at[n] = len(blocks) - len(keep_blocks)
        active = np.concatenate(keep_pix) if keep_pix else np.zeros(0, np.uint32)
        blocks = keep_blocks
    own = counts[(pixels & 0xFFFF).astype(np.int64), (pixels >> 16).astype(np.int64)]
    stats = dict(rounds=rounds, evaluations=evaluations, samplesTraced=traced, unconvergedPixels=int(active.size),
                 minCount=int(own.min()) if own.size else 0, maxCount=int(own.max()) if own.size else 0)
    return dict(radiance=A, half=H, counts=counts, block_error=berr, active=active, active_counts=active_counts, retired_at=retired_at, stats=stats)
