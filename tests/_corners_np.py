"""Host restatements of the corner definitions (include/evk.h, "Corner detection").

seq_*   the definition, literally: one sequential loop over the stream with a per-class map of the last time stamp / the last
        index at every pixel; eFAST tries every start and every length of an arc, Harris evaluates the formulas in float64.
fast_*  the same maps, but the circle values / patches of all events are collected first and the tests run vectorised over the
        events (the arc test as "the L newest values of the circle are contiguous and strictly newer than the rest").  Pinned
        to seq_* in tests/test_cpu_corners.py; what the GPU tests use on larger streams."""
import numpy as np

BORDER = 4
C3 = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
      (-2, 2), (-1, 3)]
C4 = [(0, 4), (1, 4), (2, 3), (3, 2), (4, 1), (4, 0), (4, -1), (3, -2), (2, -3), (1, -4), (0, -4), (-1, -4), (-2, -3), (-3, -2),
      (-4, -1), (-4, 0), (-4, 1), (-3, 2), (-2, 3), (-1, 4)]
S = np.array([1, 4, 6, 4, 1])
D = np.array([-1, -2, 0, 2, 1])
_AC = np.arange(5) - 2
G = np.exp(-(_AC[:, None] ** 2 + _AC[None, :] ** 2) / 2.0)
G = G / G.sum()


def _columns(x, y, t, p, polarity):
    if polarity not in ("same", "ignore"):
        raise ValueError(polarity)
    x, y = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    t = np.asarray(t).astype(np.float64)               # (exact for every column kind but int64 beyond 2^53)
    c = (np.asarray(p) > 0).astype(np.int64) if polarity == "same" else np.zeros(len(x), dtype=np.int64)
    return x, y, t, c, 2 if polarity == "same" else 1


def _eligible(x, y, H, W):
    return (x >= BORDER) & (x < W - BORDER) & (y >= BORDER) & (y < H - BORDER)


def _rows(n, select):
    if select is None:
        return np.arange(n)
    select = np.asarray(select, dtype=np.int64).reshape(-1)
    if len(select) and (select.min() < 0 or select.max() >= n):
        raise IndexError(select)
    return select


def has_arc(v, lmin, lmax):
    """the definition: some start s and length L with min(arc) > max(rest)"""
    m = len(v)
    for L in range(lmin, lmax + 1):
        for s in range(m):
            arc = [v[(s + j) % m] for j in range(L)]
            rest = [v[(s + j) % m] for j in range(L, m)]
            if min(arc) > max(rest):
                return True
    return False


def seq_fast_corners(x, y, t, p, sensor_size, polarity="same", select=None):
    H, W = sensor_size
    x, y, t, c, classes = _columns(x, y, t, p, polarity)
    n = len(x)
    last = np.full((classes, H, W), -np.inf)
    out = np.zeros(n, dtype=bool)
    for i in range(n):
        if BORDER <= x[i] < W - BORDER and BORDER <= y[i] < H - BORDER:
            v3 = [last[c[i], y[i] + dy, x[i] + dx] for dx, dy in C3]
            v4 = [last[c[i], y[i] + dy, x[i] + dx] for dx, dy in C4]
            out[i] = has_arc(v3, 3, 6) and has_arc(v4, 4, 8)
        last[c[i], y[i], x[i]] = t[i]
    return out[_rows(n, select)]


def harris_score_of_patch(b, k=0.04):
    """the formulas of the definition on one 9 x 9 patch of 0 / 1, in float64"""
    b = np.asarray(b).astype(np.int64)
    assert b.shape == (9, 9)
    Ix, Iy = np.zeros((5, 5), dtype=np.int64), np.zeros((5, 5), dtype=np.int64)
    for a in range(5):
        for c in range(5):
            for u in range(5):
                for v in range(5):
                    Ix[a, c] += S[u] * D[v] * b[a + u, c + v]
                    Iy[a, c] += D[u] * S[v] * b[a + u, c + v]
    A = float((G * Ix * Ix).sum()) / 144.0
    B = float((G * Iy * Iy).sum()) / 144.0
    C = float((G * Ix * Iy).sum()) / 144.0
    return A * B - C * C - k * (A + B) ** 2


def _check_window(n_last, dt):
    if (n_last is None) == (dt is None):
        raise TypeError("exactly one of n_last and dt")


def seq_harris_scores(x, y, t, p, sensor_size, n_last=None, dt=None, polarity="same", k=0.04, select=None):
    _check_window(n_last, dt)
    H, W = sensor_size
    x, y, t, c, classes = _columns(x, y, t, p, polarity)
    n = len(x)
    last = np.full((classes, H, W), -1, dtype=np.int64)       # the index of the last event
    out = np.full(n, np.nan, dtype=np.float32)
    for i in range(n):
        if BORDER <= x[i] < W - BORDER and BORDER <= y[i] < H - BORDER:
            b = np.zeros((9, 9), dtype=np.int64)
            for dy in range(-4, 5):
                for dx in range(-4, 5):
                    j = last[c[i], y[i] + dy, x[i] + dx]
                    if dx == 0 and dy == 0:
                        b[4, 4] = 1
                    elif j >= 0:
                        b[dy + 4, dx + 4] = (j >= i - n_last) if dt is None else (t[i] - t[j] <= dt)
            out[i] = np.float32(harris_score_of_patch(b, k))
        last[c[i], y[i], x[i]] = i
    return out[_rows(n, select)]


# ---- vectorised over the events ---------------------------------------------------------------------------------------------------

def _arcs(v, lmin, lmax):
    """(n, m) circle values -> (n,) bool.  A valid arc of length L is the set of the L newest values: the L-th newest value must be
    finite and strictly newer than the (L + 1)-th, and the set {v >= L-th newest} must be one cyclic run."""
    n, m = v.shape
    srt = -np.sort(-v, axis=1)                         # descending
    ok = np.zeros(n, dtype=bool)
    for L in range(lmin, lmax + 1):
        low = srt[:, L - 1]
        strict = np.isfinite(low) & (low > srt[:, L])
        mask = v >= low[:, None]
        steps = (mask != np.roll(mask, 1, axis=1)).sum(axis=1)
        ok |= strict & (mask.sum(axis=1) == L) & (steps == 2)
    return ok


def fast_fast_corners(x, y, t, p, sensor_size, polarity="same", select=None):
    H, W = sensor_size
    x, y, t, c, classes = _columns(x, y, t, p, polarity)
    n = len(x)
    el = _eligible(x, y, H, W)
    dxs = np.array([q[0] for q in C3 + C4])
    dys = np.array([q[1] for q in C3 + C4])
    last = np.full((classes, H, W), -np.inf)
    v = np.full((n, 36), -np.inf)
    for i in range(n):
        if el[i]:
            v[i] = last[c[i], y[i] + dys, x[i] + dxs]
        last[c[i], y[i], x[i]] = t[i]
    out = el & _arcs(v[:, :16], 3, 6) & _arcs(v[:, 16:], 4, 8)
    return out[_rows(n, select)]


def fast_harris_scores(x, y, t, p, sensor_size, n_last=None, dt=None, polarity="same", k=0.04, select=None):
    _check_window(n_last, dt)
    H, W = sensor_size
    x, y, t, c, classes = _columns(x, y, t, p, polarity)
    n = len(x)
    el = _eligible(x, y, H, W)
    last = np.full((classes, H, W), -1, dtype=np.int64)
    idx = np.flatnonzero(el)
    pj = np.full((len(idx), 9, 9), -1, dtype=np.int64)
    pos = 0
    for i in range(n):
        if el[i]:
            pj[pos] = last[c[i], y[i] - 4:y[i] + 5, x[i] - 4:x[i] + 5]
            pos += 1
        last[c[i], y[i], x[i]] = i
    have = pj >= 0
    if dt is None:
        b = have & (pj >= (idx - n_last)[:, None, None])
    else:
        b = have & (t[idx][:, None, None] - t[np.maximum(pj, 0)] <= dt)
    b[:, 4, 4] = True
    b = b.astype(np.int64)
    win = np.lib.stride_tricks.sliding_window_view(b, (5, 5), axis=(1, 2))      # (m, a, c, u, v)
    Ix = np.einsum("macuv,u,v->mac", win, S, D)
    Iy = np.einsum("macuv,u,v->mac", win, D, S)
    A = (G * Ix * Ix).sum(axis=(1, 2)) / 144.0
    B = (G * Iy * Iy).sum(axis=(1, 2)) / 144.0
    C = (G * Ix * Iy).sum(axis=(1, 2)) / 144.0
    out = np.full(n, np.nan, dtype=np.float32)
    out[idx] = (A * B - C * C - k * (A + B) ** 2).astype(np.float32)
    return out[_rows(n, select)]


# ---- streams the CPU and the GPU tests share --------------------------------------------------------------------------------------

def mixed_scene():
    """24 x 28; the outline of a 9-pixel square moves along the diagonal over 300 integer ticks (ties occur): 3000 edge events, +1 on
    its top and left sides and -1 on the others, and 300 uniform noise events; stable-sorted by tick."""
    H, W, side, ticks = 24, 28, 9, 300
    rng = np.random.default_rng(2017)
    ring = [(a, 0) for a in range(side)] + [(0, b) for b in range(1, side)]                       # top and left: +1
    ring += [(a, side - 1) for a in range(1, side)] + [(side - 1, b) for b in range(1, side - 1)]     # bottom and right: -1
    ring = np.array(ring)
    pol = np.where(np.arange(len(ring)) < 2 * side - 1, 1, -1)
    tick = np.repeat(np.arange(ticks), 10)
    shift = (tick * (H - side)) // (ticks - 1)
    pick = rng.integers(0, len(ring), len(tick))
    x = np.concatenate([ring[pick, 0] + shift, rng.integers(0, W, 300)])
    y = np.concatenate([ring[pick, 1] + shift, rng.integers(0, H, 300)])
    p = np.concatenate([pol[pick], rng.integers(0, 2, 300) * 2 - 1])
    t = np.concatenate([tick, rng.integers(0, ticks, 300)])
    o = np.argsort(t, kind="stable")
    return x[o].astype(np.int64), y[o].astype(np.int64), t[o].astype(np.float64), p[o].astype(np.int64), (H, W)


HAND_SIZE, HAND_CENTRE = (13, 20), (6, 6)             # the patch of the centre covers x, y in 2 .. 10; x >= 11 lies outside it


def circle_stream(v3, v4, p3=1, p4=1):
    """One event per circle pixel with a time (None: the pixel does not fire), C3 then C4, then the event under test at HAND_CENTRE
    (+1, t = 1000): it is the last event of the stream.  p3 / p4: the polarity of the circle events."""
    cx, cy = HAND_CENTRE
    ev = [(cx + dx, cy + dy, v, p3) for (dx, dy), v in zip(C3, v3) if v is not None]
    ev += [(cx + dx, cy + dy, v, p4) for (dx, dy), v in zip(C4, v4) if v is not None]
    ev.append((cx, cy, 1000.0, 1))
    a = np.array(ev, dtype=np.float64)
    return a[:, 0].astype(np.int64), a[:, 1].astype(np.int64), a[:, 2], a[:, 3].astype(np.int64)


def arc(m, start, length, new=10.0, old=1.0):
    """a circle of m times: `length` elements from `start` (cyclic) at `new`, the others at `old`"""
    v = [old] * m
    for j in range(length):
        v[(start + j) % m] = new                       # (ties inside an arc are harmless)
    return v


def patch_stream(b):
    """One event (+1, t = its position) per set pixel of the 9 x 9 patch b around HAND_CENTRE, row by row, then the event under test"""
    cx, cy = HAND_CENTRE
    ev = [(cx + dx, cy + dy) for dy in range(-4, 5) for dx in range(-4, 5) if b[dy + 4][dx + 4] and (dx or dy)]
    ev.append((cx, cy))
    a = np.array(ev, dtype=np.int64)
    return a[:, 0], a[:, 1], np.arange(len(a), dtype=np.float64), np.ones(len(a), dtype=np.int64)


def lone_patch():
    b = np.zeros((9, 9), dtype=np.int64)
    b[4, 4] = 1
    return b


def edge_patch():
    b = lone_patch()
    b[:, 4] = 1                                        # a vertical line through the centre
    return b


def l_patch():
    b = lone_patch()
    b[4, 4:] = 1                                       # from the centre to the right ...
    b[4:, 4] = 1                                       # ... and downwards
    return b
