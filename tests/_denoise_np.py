"""Host restatements of the event-denoising definitions (include/evk.h, "Event denoising").

seq_*  : the literal sequential loop over a per-pixel (per-class) timestamp map -- this IS the definition.
fast_* : the same results vectorised (lexsort + searchsorted) for larger streams; tests/test_cpu_denoise.py pins them to seq_*.

Time differences are formed in float64 from the stored values; "earlier" means a smaller stream index; a polarity class is
p > 0."""
import numpy as np


def _cols(xs, ys, ts, ps, use_polarity):
    x = np.asarray(xs).astype(np.int64).reshape(-1)
    y = np.asarray(ys).astype(np.int64).reshape(-1)
    t = np.asarray(ts).reshape(-1).astype(np.float64)
    c = (np.asarray(ps).reshape(-1) > 0).astype(np.int64) if use_polarity else np.zeros(len(x), dtype=np.int64)
    return x, y, t, c


def seq_support(xs, ys, ts, ps, dt, sensor_size, radius=1, include_self=False, same_polarity=False):
    H, W = sensor_size
    x, y, t, c = _cols(xs, ys, ts, ps, same_polarity)
    last_t = np.zeros((2, H, W), dtype=np.float64)
    seen = np.zeros((2, H, W), dtype=bool)
    out = np.zeros(len(x), dtype=np.uint8)
    r = int(radius)
    for i in range(len(x)):
        xi, yi, ci, ti = x[i], y[i], c[i], t[i]
        y0, y1, x0, x1 = max(0, yi - r), min(H, yi + r + 1), max(0, xi - r), min(W, xi + r + 1)
        hit = seen[ci, y0:y1, x0:x1] & (ti - last_t[ci, y0:y1, x0:x1] <= dt)
        n = int(hit.sum())
        if not include_self and hit[yi - y0, xi - x0]:
            n -= 1
        out[i] = n
        last_t[ci, yi, xi] = ti
        seen[ci, yi, xi] = True
    return out


def seq_refractory(xs, ys, ts, ps, refractory, sensor_size, per_polarity=False):
    H, W = sensor_size
    x, y, t, c = _cols(xs, ys, ts, ps, per_polarity)
    last_t = np.zeros((2, H, W), dtype=np.float64)
    seen = np.zeros((2, H, W), dtype=bool)
    keep = np.zeros(len(x), dtype=bool)
    for i in range(len(x)):
        xi, yi, ci, ti = x[i], y[i], c[i], t[i]
        if not seen[ci, yi, xi] or ti - last_t[ci, yi, xi] >= refractory:
            keep[i] = True
            last_t[ci, yi, xi] = ti
            seen[ci, yi, xi] = True
    return keep


def _grouped(x, y, c, H, W):
    """order (indices grouped by key, ascending inside a key) and the sorted composite key * N + index."""
    n = len(x)
    key = (c * H + y) * W + x
    idx = np.arange(n, dtype=np.int64)
    order = np.lexsort((idx, key))
    return key, order, key[order] * max(n, 1) + order


def fast_support(xs, ys, ts, ps, dt, sensor_size, radius=1, include_self=False, same_polarity=False):
    H, W = sensor_size
    x, y, t, c = _cols(xs, ys, ts, ps, same_polarity)
    n = len(x)
    out = np.zeros(n, dtype=np.int64)
    if n == 0:
        return out.astype(np.uint8)
    _, order, comp = _grouped(x, y, c, H, W)
    idx = np.arange(n, dtype=np.int64)
    r = int(radius)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx == 0 and dy == 0 and not include_self:
                continue
            xx, yy = x + dx, y + dy
            inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            kq = np.where(inside, (c * H + yy) * W + xx, 0)
            pos = np.searchsorted(comp, kq * n + idx, side="left") - 1      # the last (key, index) pair below (kq, i)
            ok = inside & (pos >= 0)
            prev = comp[np.maximum(pos, 0)]
            ok &= prev // n == kq
            j = prev % n
            ok &= t - t[j] <= dt
            out += ok
    return out.astype(np.uint8)


def fast_support_keep(support, k):
    return np.asarray(support) >= k


def fast_refractory(xs, ys, ts, ps, refractory, sensor_size, per_polarity=False):
    H, W = sensor_size
    x, y, t, c = _cols(xs, ys, ts, ps, per_polarity)
    n = len(x)
    keep = np.zeros(n, dtype=bool)
    if n == 0:
        return keep
    key, order, _ = _grouped(x, y, c, H, W)
    sk = key[order]
    starts = np.flatnonzero(np.r_[True, sk[1:] != sk[:-1]])
    lens = np.diff(np.r_[starts, n])
    by = np.argsort(-lens, kind="stable")
    starts, lens = starts[by], lens[by]
    last = np.zeros(len(starts), dtype=np.float64)
    s = 0
    while s < lens[0]:
        m = int(np.searchsorted(-lens, -s, side="left"))        # runs longer than s: the first m
        if m <= 2:
            break
        ev = order[starts[:m] + s]
        tv = t[ev]
        k = tv - last[:m] >= refractory if s else np.ones(m, dtype=bool)
        keep[ev] = k
        last[:m] = np.where(k, tv, last[:m])
        s += 1
    for q in range(len(starts)):                                  # the few longest runs: a scalar walk each
        if lens[q] <= s:
            break
        ev = order[starts[q] + s:starts[q] + lens[q]]
        tv = t[ev].tolist()
        lt, have, flags = float(last[q]), s > 0, []
        for v in tv:
            kp = (not have) or (v - lt >= refractory)
            if kp:
                lt, have = v, True
            flags.append(kp)
        keep[ev] = flags
    return keep


RUN_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 769)        # and one empty pixel


def run_length_scene(seed=7):
    """The smallest scene on which the wave path of a run walk (k_dn_refractory, k_reconstruct) can go wrong: a 3 x 4 sensor, one
    run of each length of RUN_LENGTHS and one empty pixel -- a wave's step is 256 positions and its pipeline is three steps deep,
    so the lengths straddle one, two and three steps -- 3266 events interleaved in stream order by a seeded shuffle, integer tick
    times that are non-decreasing with ties and stay below 32768 (the int16 kind holds them), both polarities.
    -> x, y, t, p as int64 / float64 / int64, and the size (3, 4)"""
    rng = np.random.default_rng(seed)
    H, W = 3, 4
    lengths = rng.permutation(np.array(RUN_LENGTHS + (0,)))
    pix = rng.permutation(np.repeat(np.arange(H * W), lengths))
    n = len(pix)
    t = np.sort(rng.integers(0, 8_000, n)).astype(np.float64)
    p = rng.integers(0, 2, n) * 2 - 1
    assert n == 3266 and (np.diff(t) == 0).any() and t[-1] < 32768 and sorted(np.bincount(pix, minlength=H * W)) == sorted(lengths)
    return (pix % W).astype(np.int64), (pix // W).astype(np.int64), t, p.astype(np.int64), (H, W)
