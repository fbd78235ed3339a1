"""Host restatements of the time-surface definitions (include/evk.h, "Time surfaces").

seq_*  : the literal sequential loop over a per-pixel, per-class timestamp map (for HATS a per-pixel list of past times) -- this
         IS the definition.
fast_* : the same results vectorised (lexsort + searchsorted) for larger streams; tests/test_cpu_time_surface.py pins them to seq_*.

Ages are formed in float64 from the stored values; "earlier" means a smaller stream index; a polarity class is p > 0; an age is
+inf where no earlier event exists or the pixel lies off the sensor.  Values: decay "exp" float32(exp(-a / tau)), "linear"
float32(max(0, 1 - a / tau)), None the float64 age."""
import numpy as np

INF = np.inf


def _cols(xs, ys, ts, ps, two):
    x = np.asarray(xs).astype(np.int64).reshape(-1)
    y = np.asarray(ys).astype(np.int64).reshape(-1)
    t = np.asarray(ts).reshape(-1).astype(np.float64)
    c = (np.asarray(ps).reshape(-1) > 0).astype(np.int64) if two else np.zeros(len(x), dtype=np.int64)
    return x, y, t, c


def value(age, decay, tau):
    age = np.asarray(age, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if decay is None:
            return age
        if decay == "exp":
            return np.exp(-age / tau).astype(np.float32)
        assert decay == "linear"
        return np.maximum(0.0, 1.0 - age / tau).astype(np.float32)


def _cuts(t, t_refs, indices):
    """(m_k, T_k) of the queries; T_k is None for a cut at 0 (an empty surface)."""
    assert (t_refs is None) != (indices is None)
    if t_refs is not None:
        refs = np.asarray(t_refs, dtype=np.float64).reshape(-1)
        return [(int(np.searchsorted(t, T, side="left")), float(T)) for T in refs]
    return [(int(m), float(t[int(m) - 1]) if int(m) > 0 else None) for m in np.asarray(indices).reshape(-1)]


# ---- the surface of active events ---------------------------------------------------------------------------------------------

def seq_time_surfaces(xs, ys, ts, ps, tau, sensor_size, t_refs=None, indices=None, decay="exp", polarity="split"):
    H, W = sensor_size
    assert polarity in ("split", "ignore")
    x, y, t, c = _cols(xs, ys, ts, ps, polarity == "split")
    C = 2 if polarity == "split" else 1
    out = []
    for m, T in _cuts(t, t_refs, indices):
        last_t = np.zeros((C, H, W), dtype=np.float64)
        seen = np.zeros((C, H, W), dtype=bool)
        for j in range(m):
            last_t[c[j], y[j], x[j]] = t[j]
            seen[c[j], y[j], x[j]] = True
        age = np.full((C, H, W), INF)
        if m > 0:
            age[seen] = T - last_t[seen]
        out.append(value(age, decay, tau))
    return np.stack(out)


def _grouped(x, y, c, H, W):
    """the sorted composite key * N + index of the events: grouped by key = (class, pixel), ascending index inside a key"""
    n = len(x)
    key = (c * H + y) * W + x
    order = np.lexsort((np.arange(n, dtype=np.int64), key))
    return key[order] * max(n, 1) + order


def _last_before(comp, n, kq, m, t, T):
    """age T - t[last event of key kq with an index below m]; +inf where there is none (kq, m, T broadcast together)"""
    pos = np.searchsorted(comp, kq * n + m, side="left") - 1
    prev = comp[np.maximum(pos, 0)]
    ok = (pos >= 0) & (prev // n == kq)
    with np.errstate(invalid="ignore"):
        return np.where(ok, T - t[prev % n], INF)


def fast_time_surfaces(xs, ys, ts, ps, tau, sensor_size, t_refs=None, indices=None, decay="exp", polarity="split"):
    H, W = sensor_size
    assert polarity in ("split", "ignore")
    x, y, t, c = _cols(xs, ys, ts, ps, polarity == "split")
    C = 2 if polarity == "split" else 1
    n = len(x)
    out = []
    comp = _grouped(x, y, c, H, W) if n else None
    keys = np.arange(C * H * W, dtype=np.int64)
    for m, T in _cuts(t, t_refs, indices):
        age = np.full(C * H * W, INF) if m == 0 else _last_before(comp, n, keys, m, t, T)
        out.append(value(age.reshape(C, H, W), decay, tau))
    return np.stack(out)


# ---- per-event local surfaces -------------------------------------------------------------------------------------------------

def _channels(polarity):
    assert polarity in ("ignore", "same", "split")
    return polarity != "ignore", 2 if polarity == "split" else 1


def seq_local_time_surfaces(xs, ys, ts, ps, tau, sensor_size, radius=3, decay="exp", polarity="same", include_self=True,
                            select=None):
    H, W = sensor_size
    two, C = _channels(polarity)
    x, y, t, c = _cols(xs, ys, ts, ps, two)
    n, r = len(x), int(radius)
    P = 2 * r + 1
    last_t = np.zeros((2, H, W), dtype=np.float64)
    seen = np.zeros((2, H, W), dtype=bool)
    age = np.full((n, C, P, P), INF)
    for i in range(n):
        for ch in range(C):
            cls = ch if C == 2 else c[i]
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    yy, xx = y[i] + dy, x[i] + dx
                    if not (0 <= yy < H and 0 <= xx < W):
                        continue
                    if include_self and dx == 0 and dy == 0 and cls == c[i]:
                        age[i, ch, dy + r, dx + r] = 0.0
                    elif seen[cls, yy, xx]:
                        age[i, ch, dy + r, dx + r] = t[i] - last_t[cls, yy, xx]
        last_t[c[i], y[i], x[i]] = t[i]
        seen[c[i], y[i], x[i]] = True
    if select is not None:
        age = age[np.asarray(select, dtype=np.int64).reshape(-1)]
    return value(age, decay, tau)


def fast_local_time_surfaces(xs, ys, ts, ps, tau, sensor_size, radius=3, decay="exp", polarity="same", include_self=True,
                             select=None):
    H, W = sensor_size
    two, C = _channels(polarity)
    x, y, t, c = _cols(xs, ys, ts, ps, two)
    n, r = len(x), int(radius)
    P = 2 * r + 1
    idx = np.arange(n, dtype=np.int64) if select is None else np.asarray(select, dtype=np.int64).reshape(-1)
    age = np.full((len(idx), C, P, P), INF)
    if n == 0 or len(idx) == 0:
        return value(age, decay, tau)
    comp = _grouped(x, y, c, H, W)
    xi, yi, ci, ti = x[idx], y[idx], c[idx], t[idx]
    for ch in range(C):
        cls = np.full(len(idx), ch) if C == 2 else ci
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                xx, yy = xi + dx, yi + dy
                inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                kq = np.where(inside, (cls * H + yy) * W + xx, 0)
                a = np.where(inside, _last_before(comp, n, kq, idx, t, ti), INF)
                if include_self and dx == 0 and dy == 0:
                    a = np.where(cls == ci, 0.0, a)
                age[:, ch, dy + r, dx + r] = a
    return value(age, decay, tau)


# ---- HATS ---------------------------------------------------------------------------------------------------------------------

def _hats_result(h, counts, normalise, return_counts):
    if normalise:
        h = h / np.maximum(counts, 1)[..., None, None]
    h = h.astype(np.float32)
    return (h, counts.astype(np.int32)) if return_counts else h


def seq_averaged_time_surfaces(xs, ys, ts, ps, tau, dt, sensor_size, cell_size=10, radius=3, normalise=True, return_counts=False):
    H, W = sensor_size
    x, y, t, c = _cols(xs, ys, ts, ps, True)
    r, cell = int(radius), int(cell_size)
    P = 2 * r + 1
    Cy, Cx = -(-H // cell), -(-W // cell)
    h = np.zeros((Cy, Cx, 2, P, P), dtype=np.float64)
    counts = np.zeros((Cy, Cx, 2), dtype=np.int64)
    past = {}
    for i in range(len(x)):
        gy, gx = y[i] // cell, x[i] // cell
        counts[gy, gx, c[i]] += 1
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                yy, xx = y[i] + dy, x[i] + dx
                if not (0 <= yy < H and 0 <= xx < W) or yy // cell != gy or xx // cell != gx:
                    continue
                s = 0.0
                for tj in past.get((c[i], yy, xx), ()):
                    if t[i] - tj <= dt:
                        s += np.exp(-(t[i] - tj) / tau)
                h[gy, gx, c[i], dy + r, dx + r] += s
        past.setdefault((c[i], y[i], x[i]), []).append(t[i])
    return _hats_result(h, counts, normalise, return_counts)


def fast_averaged_time_surfaces(xs, ys, ts, ps, tau, dt, sensor_size, cell_size=10, radius=3, normalise=True, return_counts=False):
    """needs non-decreasing ts: then "within dt" is "an index from J_i on", J_i the first index with t_i - t[J_i] <= dt"""
    H, W = sensor_size
    x, y, t, c = _cols(xs, ys, ts, ps, True)
    assert (np.diff(t) >= 0).all()
    n, r, cell = len(x), int(radius), int(cell_size)
    P = 2 * r + 1
    Cy, Cx = -(-H // cell), -(-W // cell)
    h = np.zeros((Cy, Cx, 2, P, P), dtype=np.float64)
    counts = np.zeros((Cy, Cx, 2), dtype=np.int64)
    if n == 0:
        return _hats_result(h, counts, normalise, return_counts)
    gy, gx = y // cell, x // cell
    np.add.at(counts, (gy, gx, c), 1)
    idx = np.arange(n, dtype=np.int64)
    first = np.searchsorted(t, t - dt, side="left")
    while True:                                  # the window test is t_i - t_j <= dt itself, not t_j >= t_i - dt
        down = (first > 0) & (t - t[np.maximum(first - 1, 0)] <= dt)
        up = (first < idx) & (t - t[np.minimum(first, n - 1)] > dt)
        if not (down | up).any():
            break
        first = first - down + (up & ~down)
    comp = _grouped(x, y, c, H, W)
    t_run = t[comp % n]
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            xx, yy = x + dx, y + dy
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H) & (yy // cell == gy) & (xx // cell == gx)
            kq = np.where(ok, (c * H + yy) * W + xx, 0)
            lo = np.searchsorted(comp, kq * n + first, side="left")
            hi = np.where(ok, np.searchsorted(comp, kq * n + idx, side="left"), lo)
            s = np.zeros(n)
            d = 0
            while True:
                live = lo + d < hi
                if not live.any():
                    break
                s[live] += np.exp(-(t[live] - t_run[lo[live] + d]) / tau)
                d += 1
            np.add.at(h, (gy, gx, c, dy + r, dx + r), s)
    return _hats_result(h, counts, normalise, return_counts)
