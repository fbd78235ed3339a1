"""Host restatements of the plane-fit flow definitions (include/evk.h, "Plane-fit flow").

seq_*   the definition, literally: one sequential loop over the stream with a per-class map of the last time stamp at every pixel;
        the sums, the cofactors, the rejection rounds and the result in Python's own integers and float64, one operation at a time
        (no fused multiply-add, the double sums in row-major order from 0.0).
fast_*  vectorised over the events on _time_surface_np.fast_local_time_surfaces(decay=None, include_self=True); the double sums
        are an explicit loop over the <= 81 window elements (np.sum over that axis would sum pairwise).  Pinned to seq_* in
        tests/test_cpu_plane_flow.py; what the GPU tests use on larger streams.  Finite times only (a missing sample is age +inf).

Both return (flow (M, 2) float32, valid (M,) bool, lifetime (M,) float32); *_field return (field (2, H, W) float32, count (H, W)
int32)."""
import math

import numpy as np

import _time_surface_np as TS

NAN32 = np.float32(np.nan)


def _columns(x, y, t, p, polarity):
    if polarity not in ("same", "ignore"):
        raise ValueError(polarity)
    x, y = np.asarray(x).astype(np.int64).reshape(-1), np.asarray(y).astype(np.int64).reshape(-1)
    t = np.asarray(t).reshape(-1).astype(np.float64)   # (exact for every column kind but int64 beyond 2^53)
    c = (np.asarray(p).reshape(-1) > 0).astype(np.int64) if polarity == "same" else np.zeros(len(x), dtype=np.int64)
    return x, y, t, c, 2 if polarity == "same" else 1


def _rows(n, select):
    if select is None:
        return np.arange(n)
    select = np.asarray(select, dtype=np.int64).reshape(-1)
    if len(select) and (select.min() < 0 or select.max() >= n):
        raise IndexError(select)
    return select


def fit_plane(samples, min_samples):
    """samples: (dx, dy, tau) in row-major order of the window -> (a, b, c) or None when the fit fails"""
    n = sx = sy = sxx = sxy = syy = 0
    st = sxt = syt = 0.0
    for dx, dy, tau in samples:
        n, sx, sy, sxx, sxy, syy = n + 1, sx + dx, sy + dy, sxx + dx * dx, sxy + dx * dy, syy + dy * dy
        st = st + tau
        sxt = sxt + float(dx) * tau
        syt = syt + float(dy) * tau
    c11, c12, c13 = syy * n - sy * sy, sx * sy - sxy * n, sxy * sy - syy * sx
    c22, c23, c33 = sxx * n - sx * sx, sxy * sx - sxx * sy, sxx * syy - sxy * sxy
    D = sxx * c11 + sxy * c12 + sx * c13
    if n < min_samples or D == 0:
        return None
    a = ((float(c11) * sxt + float(c12) * syt) + float(c13) * st) / float(D)
    b = ((float(c12) * sxt + float(c22) * syt) + float(c23) * st) / float(D)
    c = ((float(c13) * sxt + float(c23) * syt) + float(c33) * st) / float(D)
    return a, b, c


def flow_of_samples(samples, min_samples=5, outlier_threshold=None, iterations=2, max_speed=None):
    """the definition on the samples in use of one event -> (vx, vy, lifetime) as float32, or None when the event is invalid"""
    samples = list(samples)
    plane = fit_plane(samples, min_samples)
    if outlier_threshold is not None:
        for _ in range(iterations):
            if plane is None:
                break
            a, b, c = plane
            kept = [(dx, dy, tau) for dx, dy, tau in samples
                    if (dx == 0 and dy == 0) or not abs(((a * float(dx) + b * float(dy)) + c) - tau) > outlier_threshold]
            if len(kept) == len(samples):
                break
            samples = kept
            plane = fit_plane(samples, min_samples)
    if plane is None:
        return None
    a, b, _ = plane
    g = a * a + b * b
    if not g > 0.0 or (max_speed is not None and not 1.0 / g <= max_speed * max_speed):
        return None
    return np.float32(a / g), np.float32(b / g), np.float32(math.sqrt(g))


def seq_local_plane_flow(x, y, t, p, dt, sensor_size, radius=2, polarity="same", min_samples=5, outlier_threshold=None, iterations=2,
                         max_speed=None, select=None):
    H, W = sensor_size
    x, y, t, c, classes = _columns(x, y, t, p, polarity)
    n, r, dt = len(x), int(radius), float(dt)
    last = np.zeros((classes, H, W), dtype=np.float64)
    seen = np.zeros((classes, H, W), dtype=bool)
    flow = np.full((n, 2), NAN32, dtype=np.float32)
    life = np.full(n, NAN32, dtype=np.float32)
    valid = np.zeros(n, dtype=bool)
    for i in range(n):
        ti = float(t[i])
        samples = []
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                xx, yy = x[i] + dx, y[i] + dy
                if dx == 0 and dy == 0:
                    samples.append((0, 0, 0.0))
                elif 0 <= xx < W and 0 <= yy < H and seen[c[i], yy, xx]:
                    tj = float(last[c[i], yy, xx])
                    if ti - tj <= dt:
                        samples.append((dx, dy, tj - ti))
        got = flow_of_samples(samples, min_samples, outlier_threshold, iterations, max_speed)
        if got is not None:
            flow[i, 0], flow[i, 1], life[i] = got
            valid[i] = True
        last[c[i], y[i], x[i]] = t[i]
        seen[c[i], y[i], x[i]] = True
    rows = _rows(n, select)
    return flow[rows], valid[rows], life[rows]


def field_of_flow(x, y, p, flow, valid, sensor_size, polarity="same"):
    """the field of the definition from per-event flows: per pixel class p <= 0 first, then p > 0, each in ascending index"""
    H, W = sensor_size
    x, y, _, c, classes = _columns(x, y, np.zeros(len(np.asarray(x).reshape(-1))), p, polarity)
    total = np.zeros((2, H, W), dtype=np.float64)
    count = np.zeros((H, W), dtype=np.int64)
    for cls in range(classes):
        for i in range(len(x)):
            if c[i] == cls and valid[i]:
                total[0, y[i], x[i]] = total[0, y[i], x[i]] + float(flow[i, 0])
                total[1, y[i], x[i]] = total[1, y[i], x[i]] + float(flow[i, 1])
                count[y[i], x[i]] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        field = np.where(count > 0, total / count, 0.0).astype(np.float32)
    return field, count.astype(np.int32)


def seq_plane_flow_field(x, y, t, p, dt, sensor_size, polarity="same", **fit):
    flow, valid, _ = seq_local_plane_flow(x, y, t, p, dt, sensor_size, polarity=polarity, **fit)
    return field_of_flow(x, y, p, flow, valid, sensor_size, polarity)


# ---- vectorised over the events ---------------------------------------------------------------------------------------------------

def _fit_all(use, tau, dxs, dys, min_samples):
    """use, tau: (M, PP) -> a, b, c (float64, meaningless where not ok), ok"""
    u = use.astype(np.int64)
    n, sx, sy = u.sum(1), (u * dxs).sum(1), (u * dys).sum(1)
    sxx, sxy, syy = (u * dxs * dxs).sum(1), (u * dxs * dys).sum(1), (u * dys * dys).sum(1)
    st, sxt, syt = np.zeros(len(u)), np.zeros(len(u)), np.zeros(len(u))
    with np.errstate(all="ignore"):
        for k in range(use.shape[1]):                  # row-major, one addition at a time
            st = np.where(use[:, k], st + tau[:, k], st)
            sxt = np.where(use[:, k], sxt + float(dxs[k]) * tau[:, k], sxt)
            syt = np.where(use[:, k], syt + float(dys[k]) * tau[:, k], syt)
        c11, c12, c13 = syy * n - sy * sy, sx * sy - sxy * n, sxy * sy - syy * sx
        c22, c23, c33 = sxx * n - sx * sx, sxy * sx - sxx * sy, sxx * syy - sxy * sxy
        D = sxx * c11 + sxy * c12 + sx * c13
        ok = (n >= min_samples) & (D != 0)
        Dd = np.where(ok, D, 1).astype(np.float64)
        f = lambda v: v.astype(np.float64)  # noqa: E731
        a = ((f(c11) * sxt + f(c12) * syt) + f(c13) * st) / Dd
        b = ((f(c12) * sxt + f(c22) * syt) + f(c23) * st) / Dd
        c = ((f(c13) * sxt + f(c23) * syt) + f(c33) * st) / Dd
    return a, b, c, ok


def fast_local_plane_flow(x, y, t, p, dt, sensor_size, radius=2, polarity="same", min_samples=5, outlier_threshold=None, iterations=2,
                          max_speed=None, select=None):
    r, dt = int(radius), float(dt)
    P = 2 * r + 1
    n = len(np.asarray(x).reshape(-1))
    rows = _rows(n, select)
    age = TS.fast_local_time_surfaces(x, y, t, p, None, sensor_size, radius=r, decay=None, polarity=polarity, include_self=True,
                                      select=rows).reshape(len(rows), P * P)
    dys, dxs = (v.reshape(-1) for v in np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij"))
    centre = (dxs == 0) & (dys == 0)
    with np.errstate(invalid="ignore"):
        use = np.isfinite(age) & (age <= dt)
        tau = np.where(np.isfinite(age), 0.0 - age, 0.0)
    use[:, centre] = True
    a, b, c, ok = _fit_all(use, tau, dxs, dys, min_samples)
    if outlier_threshold is not None:
        for _ in range(iterations):
            with np.errstate(all="ignore"):
                e = np.abs(((a[:, None] * dxs.astype(np.float64) + b[:, None] * dys.astype(np.float64)) + c[:, None]) - tau)
            drop = use & ~centre & (e > outlier_threshold) & ok[:, None]
            if not drop.any():
                break
            use = use & ~drop                          # (an event that dropped nothing, or failed, refits to the same result)
            a, b, c, ok = _fit_all(use, tau, dxs, dys, min_samples)
    with np.errstate(all="ignore"):
        g = a * a + b * b
        valid = ok & (g > 0.0)
        if max_speed is not None:
            valid &= 1.0 / g <= float(max_speed) * float(max_speed)
        flow = np.stack([a / g, b / g], axis=1).astype(np.float32)
        life = np.sqrt(g).astype(np.float32)
    flow[~valid], life[~valid] = NAN32, NAN32
    return flow, valid, life


def fast_field_of_flow(x, y, p, flow, valid, sensor_size, polarity="same"):
    H, W = sensor_size
    x, y, _, c, classes = _columns(x, y, np.zeros(len(np.asarray(x).reshape(-1))), p, polarity)
    idx = np.concatenate([np.flatnonzero((c == cls) & valid) for cls in range(classes)]) if len(x) else np.zeros(0, dtype=np.int64)
    total = np.zeros((2, H, W), dtype=np.float64)
    count = np.zeros((H, W), dtype=np.int64)
    for ch in range(2):                                # np.add.at adds one element at a time, in the order of idx
        np.add.at(total[ch], (y[idx], x[idx]), flow[idx, ch].astype(np.float64))
    np.add.at(count, (y[idx], x[idx]), 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        field = np.where(count > 0, total / count, 0.0).astype(np.float32)
    return field, count.astype(np.int32)


def fast_plane_flow_field(x, y, t, p, dt, sensor_size, polarity="same", **fit):
    flow, valid, _ = fast_local_plane_flow(x, y, t, p, dt, sensor_size, polarity=polarity, **fit)
    return fast_field_of_flow(x, y, p, flow, valid, sensor_size, polarity)


# ---- streams the CPU and the GPU tests share --------------------------------------------------------------------------------------

EDGE_DT, EDGE_TH = 400.0, 40.0


def edge_scene(seed=2014, n=3000, H=24, W=32, noise=0.2):
    """A slanted edge that moves at (0.020, 0.010) pixels per tick over the sensor, on integer ticks (ties occur): the edge events
    (+1) fall on the line x + y / 2 = 0.025 t - 6 with a position jitter of up to one pixel, and `noise` of the events are uniform
    over the sensor with either polarity.  Sorted by tick.  -> int64 x, y, float64 t, int64 p."""
    rng = np.random.default_rng(seed)
    ticks = int((W + H / 2 + 6) / 0.025)
    t = np.sort(rng.integers(0, ticks, n))
    is_noise = rng.random(n) < noise
    y = rng.integers(0, H, n)
    x = np.floor(0.025 * t - 6.0 - y / 2.0 + rng.uniform(-0.5, 0.5, n)).astype(np.int64)
    off = (x < 0) | (x >= W)
    x = np.where(is_noise | off, rng.integers(0, W, n), x)
    p = np.where(is_noise | off, rng.integers(0, 2, n) * 2 - 1, 1)
    return x.astype(np.int64), y.astype(np.int64), t.astype(np.float64), p.astype(np.int64)


HAND_SIZE, HAND_CENTRE = (9, 11), (5, 4)


def window_stream(taus, r=2, p=1):
    """One event per window pixel around HAND_CENTRE with a time (taus[dy + r][dx + r], None: the pixel does not fire; the centre
    entry is ignored), in row-major order, then the event under test at HAND_CENTRE with t = 0: it is the last event of the stream
    and its samples are tau = the given times (all <= 0 relative to it is not required: the stream may be unsorted)."""
    cx, cy = HAND_CENTRE
    ev = [(cx + dx, cy + dy, taus[dy + r][dx + r]) for dy in range(-r, r + 1) for dx in range(-r, r + 1)
          if (dx or dy) and taus[dy + r][dx + r] is not None]
    ev.append((cx, cy, 0.0))
    a = np.array(ev, dtype=np.float64)
    return a[:, 0].astype(np.int64), a[:, 1].astype(np.int64), a[:, 2], np.full(len(a), p, dtype=np.int64)


def plane_taus(a, b, r=2, c=0.0):
    return [[a * dx + b * dy + c for dx in range(-r, r + 1)] for dy in range(-r, r + 1)]
