"""The definition of event stereo (include/evk.h, "Event stereo") restated literally in numpy: float64 ages and
their quantisation with one rounding per operation, integer costs summed term by term, and the winner, the three tests and the
sub-pixel step as integer comparisons.  Nothing here is shared with the product; the tests compare the device with it bit for bit."""
import numpy as np

BIG = np.int64(1) << 40                                    # more than any cost: marks a disparity that is not admissible


# ---- surfaces --------------------------------------------------------------------------------------------------------------------

def ages(xs, ys, ts, ps, sensor_size, t_refs, polarity="ignore"):
    """(K, C, H, W) float64: T_k - t of the last event of class c at (x, y) among the events with t < T_k; +inf without one"""
    H, W = sensor_size
    C = 2 if polarity == "split" else 1
    t_refs = np.asarray(t_refs, dtype=np.float64).reshape(-1)
    ts = np.asarray(ts, dtype=np.float64)
    out = np.full((len(t_refs), C, H, W), np.inf)
    for k, T in enumerate(t_refs):
        for i in range(len(ts)):
            if not ts[i] < T:
                break                                       # (the stamps are non-decreasing)
            c = int(ps[i] > 0) if C == 2 else 0
            out[k, c, int(ys[i]), int(xs[i])] = T - ts[i]
    return out


def quantise(a, tau):
    """uint8: v = 1.0 - a / tau; 0 unless v > 0, else min(255, floor(256.0 v))"""
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        v = 1.0 - a / np.float64(tau)
        f = np.floor(256.0 * v)
    q = np.zeros(a.shape, dtype=np.uint8)
    pos = v > 0                                             # (a NaN fails)
    q[pos] = np.minimum(255.0, f[pos]).astype(np.uint8)
    return q


# ---- costs -----------------------------------------------------------------------------------------------------------------------

def cost_volume(QL, QR, d_min, D, r):
    """(K, D, H, W) int64 costs, every window term added on its own; -1 where d is not admissible"""
    QL, QR = np.asarray(QL, dtype=np.int64), np.asarray(QR, dtype=np.int64)
    K, C, H, W = QL.shape
    far = d_min + D - 1
    PL = np.zeros((K, C, H + 2 * r, W + 2 * r), dtype=np.int64)
    PL[:, :, r:r + H, r:r + W] = QL
    PR = np.zeros((K, C, H + 2 * r, W + 2 * r + far), dtype=np.int64)       # column j holds the right pixel j - r - far
    PR[:, :, r:r + H, r + far:r + far + W] = QR
    out = np.empty((K, D, H, W), dtype=np.int64)
    for i in range(D):
        d = d_min + i
        diff = np.abs(PL - PR[:, :, :, far - d:far - d + W + 2 * r]).sum(axis=1)       # |QL[.., y', x'] - QR[.., y', x' - d]|, over c
        s = np.zeros((K, H, W), dtype=np.int64)
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                s += diff[:, dy:dy + H, dx:dx + W]
        s[:, :, :min(d, W)] = -1                            # x - d < 0
        out[:, i] = s
    return out


def match(QL, QR, d_min, D, r, min_activity=128, uniqueness=10, max_mean_cost=None, lr_tolerance=1, subpixel=True, volume=None):
    """-> disparity float32 (NaN), index int32 (-1), cost int32 (-1), mask bool, each (K, H, W); and the candidates"""
    K, C, H, W = np.asarray(QL).shape
    vol = cost_volume(QL, QR, d_min, D, r) if volume is None else np.asarray(volume, dtype=np.int64)
    adm = vol >= 0
    key = np.where(adm, vol, BIG)
    cand = (np.asarray(QL).max(axis=1) >= min_activity) & adm.any(axis=1)
    istar = key.argmin(axis=1)                              # the first least: the smallest d on ties
    c1 = np.take_along_axis(key, istar[:, None], axis=1)[:, 0]
    steps = np.arange(D)[None, :, None, None]
    rest = np.where(np.abs(steps - istar[:, None]) > 1, key, BIG)
    c2 = rest.min(axis=1)
    has_c2 = c2 < BIG
    valid = cand.copy()
    valid &= ~has_c2 | (c2 * (100 - uniqueness) >= 100 * c1)
    if max_mean_cost is not None:
        valid &= c1 <= int(np.floor(float(max_mean_cost) * C * (2 * r + 1) ** 2))
    dstar = d_min + istar
    if lr_tolerance is not None:
        # the right image's own winner: at x', the d with x' + d <= W - 1 of least cost[d - d_min, y, x' + d]
        right = np.full((K, D, H, W), BIG, dtype=np.int64)
        for i in range(D):
            d = d_min + i
            if d < W:
                right[:, i, :, :W - d] = key[:, i, :, d:]
        dR = d_min + right.argmin(axis=1)
        kk, yy, xx = np.nonzero(valid)
        xr = xx - dstar[kk, yy, xx]
        ok = np.abs(dR[kk, yy, xr] - dstar[kk, yy, xx]) <= lr_tolerance
        valid[kk, yy, xx] = ok
    disp = dstar.astype(np.float32)
    if subpixel:
        inside = (istar >= 1) & (istar <= D - 2)
        cm = np.take_along_axis(key, np.clip(istar - 1, 0, D - 1)[:, None], axis=1)[:, 0]
        cp = np.take_along_axis(key, np.clip(istar + 1, 0, D - 1)[:, None], axis=1)[:, 0]
        both = inside & (cm < BIG) & (cp < BIG)
        den = cm - 2 * c1 + cp
        fit = both & (den > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            sub = dstar.astype(np.float64) + (cm - cp).astype(np.float64) / (2 * den).astype(np.float64)
        disp = np.where(fit, sub.astype(np.float32), disp)
    disparity = np.where(valid, disp, np.float32(np.nan)).astype(np.float32)
    index = np.where(valid, dstar, -1).astype(np.int32)
    cost = np.where(cand, c1, -1).astype(np.int32)
    return disparity, index, cost, valid, cand


def disparity_to_depth(d, fx, baseline):
    d = np.asarray(d, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d > 0, (fx * baseline) / d, np.nan)


# ---- random surfaces -----------------------------------------------------------------------------------------------------------

def random_pair(rng, K, C, H, W, density=0.5, shift=None, noise=0.2):
    """QL random bytes at `density`; QR the same scene `shift` pixels to the left (its own random shift per row band when None),
    a share `noise` of its pixels redrawn"""
    QL = (rng.integers(0, 256, (K, C, H, W)) * (rng.random((K, C, H, W)) < density)).astype(np.uint8)
    QR = np.zeros_like(QL)
    for y0 in range(0, H, 8):
        s = int(rng.integers(0, max(W // 2, 1))) if shift is None else shift
        if s < W:
            QR[:, :, y0:y0 + 8, :W - s] = QL[:, :, y0:y0 + 8, s:]
    redraw = rng.random(QR.shape) < noise
    QR[redraw] = (rng.integers(0, 256, QR.shape) * (rng.random(QR.shape) < density)).astype(np.uint8)[redraw]
    return QL, QR


# ---- the seeded scene ------------------------------------------------------------------------------------------------------------

SCENE_SIZE = (48, 96)                                      # (H, W)
SCENE_TAU = 0.010
SCENE_END = 0.020
SCENE_DISPARITIES = (4, 9)
SCENE_D, SCENE_R, SCENE_ACTIVITY = 16, 3, 128


def scene(seed=3, dots=56):
    """Dots on two fronto-parallel planes (disparities 4 and 9) that move across a 48 x 96 rectified pair for 20 ms: a dot fires
    an event at every pixel it enters, on the left at (x, y) and on the right at (x - d, y) up to 0.1 ms later.  -> dict with the
    two streams (stamps non-decreasing), the dots' last left pixels and their true disparities."""
    rng = np.random.default_rng(seed)
    H, W = SCENE_SIZE
    d = np.asarray(SCENE_DISPARITIES)[rng.integers(0, 2, dots)]
    x0, y0 = rng.uniform(12, W - 4, dots), rng.uniform(3, H - 3, dots)
    speed, angle = rng.uniform(600.0, 1400.0, dots), rng.uniform(0, 2 * np.pi, dots)      # pixels per second
    vx, vy = speed * np.cos(angle), speed * np.sin(angle)
    pol = rng.integers(0, 2, dots) * 2 - 1
    left, right, last = [], [], np.full((dots, 2), -1, dtype=np.int64)
    for t in np.linspace(0.0, SCENE_END, 801)[:-1]:
        px, py = np.rint(x0 + vx * t).astype(np.int64), np.rint(y0 + vy * t).astype(np.int64)
        for j in range(dots):
            if (px[j], py[j]) == tuple(last[j]):
                continue
            last[j] = (px[j], py[j])
            if 0 <= px[j] < W and 0 <= py[j] < H:
                left.append((t, px[j], py[j], pol[j]))
                if px[j] - d[j] >= 0:
                    right.append((t + rng.uniform(0.0, 1e-4), px[j] - d[j], py[j], pol[j]))

    def columns(rows):
        rows = sorted(rows, key=lambda e: e[0])
        return {"ts": np.array([e[0] for e in rows], dtype=np.float64), "xs": np.array([e[1] for e in rows], dtype=np.int64),
                "ys": np.array([e[2] for e in rows], dtype=np.int64), "ps": np.array([e[3] for e in rows], dtype=np.int64)}
    return {"left": columns(left), "right": columns(right), "pixels": last, "true_disparity": d}


def stream(cols):
    return cols["xs"], cols["ys"], cols["ts"], cols["ps"]
