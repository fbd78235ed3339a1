"""float64 numpy restatement of the average-timestamp loss of a dense flow field (include/evk.h, "Average-timestamp objective",
steps 1', 2-7 and 8'): the four planes [T+, C+, T-, C-], the pair of images, the loss and its adjoint
gradient with respect to the field, for one sample or a batch given by offsets.  Steps 5-7 are those of tests/_zhu_np.py.

f32_coords: the kernels sample the field and warp in float32 (k_warp_flow_field_f32's expressions, the normalise / denormalise
round trip included), form the normalised timestamp in float32 and take floor / fraction of float32 coordinates; True restates
that (what the GPU tests compare with), False keeps float64 throughout and samples the field at (x, y) itself (the definition:
what the finite-difference tests differentiate).
warped=(xw, yw): the warped coordinates are taken as given instead of computed (the GPU tests pass warp_events_flow_torch's
output: the per-pixel slope is discontinuous at pixel edges, so both sides must put every event in the same cell); for
direction 'both' a pair of such pairs, forward then backward.  The field weights b_j and dt are still the restatement's own."""
import numpy as np

import _zhu_np as Z

DIRECTIONS = ("forward", "backward")


def sample(flow, x, y, f32_coords=False):
    """Bilinear sample of flow (2, H, W) at (x, y), zero padding -> u, v, corners: four (yy, xx, weight, inside) tuples."""
    H, W = flow.shape[-2:]
    if f32_coords:
        f = np.float32
        fl = np.asarray(flow, dtype=f)
        xv, yv = np.asarray(x, dtype=f), np.asarray(y, dtype=f)
        wm1, hm1 = f(W - 1), f(H - 1)
        gx, gy = xv / wm1 * f(2) - f(1), yv / hm1 * f(2) - f(1)
        ix, iy = (gx + f(1)) / f(2) * wm1, (gy + f(1)) / f(2) * hm1
    else:
        f = np.float64
        fl = np.asarray(flow, dtype=f)
        ix, iy = np.asarray(x, dtype=f), np.asarray(y, dtype=f)
    xf, yf = np.floor(ix), np.floor(iy)
    w, nn = ix - xf, iy - yf
    e, ss = f(1) - w, f(1) - nn
    x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
    corners = []
    for yy, xx, wt in ((y0, x0, e * ss), (y0, x0 + 1, w * ss), (y0 + 1, x0, e * nn), (y0 + 1, x0 + 1, w * nn)):
        corners.append((yy, xx, wt, (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)))
    uv = []
    for c in range(2):
        acc = None
        for yy, xx, wt, inside in corners:
            val = np.where(inside, fl[c][np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], f(0)) * wt
            acc = val if acc is None else acc + val
        uv.append(acc)
    return uv[0], uv[1], corners


def time_constants(t, direction, f32_coords=False):
    """-> dt = t - t_ref and tau, per event: forward t_ref = t_last, tau = (t - t_first) / tdiv; backward t_ref = t_first,
    tau = (t_last - t) / tdiv; tdiv = t_last - t_first + 1e-6 (float32 arithmetic with f32_coords)."""
    f = np.float32 if f32_coords else np.float64
    tf = np.asarray(t, dtype=f)
    tdiv = f(f(tf[-1] - tf[0]) + f(1e-6))
    if direction == "forward":
        return tf - tf[-1], (tf - tf[0]) / tdiv
    if direction == "backward":
        return tf - tf[0], (tf[-1] - tf) / tdiv
    raise ValueError(direction)


def warp(flow, x, y, t, direction="forward", f32_coords=False):
    """(x', y') = (x + u dt, y + v dt) (step 1')."""
    u, v, _ = sample(flow, x, y, f32_coords)
    dt, _ = time_constants(t, direction, f32_coords)
    f = np.float32 if f32_coords else np.float64
    return np.asarray(x, dtype=f) + u * dt, np.asarray(y, dtype=f) + v * dt


def _events(flow, x, y, t, p, direction, f32_coords, warped, p_scale):
    """Per counted event: (cell index on the canvas, dx, dy, tau, positive, dt, field corners) and the mask over all events."""
    H, W = flow.shape[-2:]
    u, v, corners = sample(flow, x, y, f32_coords)
    dt, tau = time_constants(t, direction, f32_coords)
    if warped is None:
        f = np.float32 if f32_coords else np.float64
        xw, yw = np.asarray(x, dtype=f) + u * dt, np.asarray(y, dtype=f) + v * dt
    else:
        xw, yw = warped
    xw, yw = np.asarray(xw, dtype=np.float64), np.asarray(yw, dtype=np.float64)
    pv = np.asarray(p, dtype=np.float64) * float(p_scale)
    with np.errstate(invalid="ignore"):
        keep = (xw > 0) & (xw <= W) & (yw > 0) & (yw <= H) & (xw < W) & (yw < H) & ~np.isnan(pv)
    xc, yc = xw[keep], yw[keep]
    px, py = np.floor(xc), np.floor(yc)
    idx = py.astype(np.int64) * (W + 1) + px.astype(np.int64)
    corners = [(yy[keep], xx[keep], wt[keep].astype(np.float64), inside[keep]) for yy, xx, wt, inside in corners]
    return (idx, xc - px, yc - py, tau[keep].astype(np.float64), pv[keep] > 0, dt[keep].astype(np.float64), corners), keep


def _splat(shape, ev):
    idx, dx, dy, tau, pos = ev[:5]
    cw, size = shape[1], shape[0] * shape[1]
    out = np.zeros((4, size))
    ax, ay = 1.0 - dx, 1.0 - dy
    for sel, base in ((pos, 0), (~pos, 2)):
        for off, wt in ((0, ax * ay), (1, dx * ay), (cw, ax * dy), (cw + 1, dx * dy)):
            out[base] += np.bincount(idx[sel] + off, weights=(tau * wt)[sel], minlength=size)
            out[base + 1] += np.bincount(idx[sel] + off, weights=wt[sel], minlength=size)
    return out.reshape((4,) + shape)


def _one(flow, x, y, t, p, sigma, direction, f32_coords, warped, p_scale, want_grad):
    """(planes, loss, gradient | None) of one sample in one direction."""
    flow = np.asarray(flow)
    H, W = flow.shape[-2:]
    shape = (H + 1, W + 1)
    g = np.zeros((2, H, W))
    if len(t) == 0:
        return np.zeros((4,) + shape), 0.0, g
    ev, _ = _events(flow, x, y, t, p, direction, f32_coords, warped, p_scale)
    pl = _splat(shape, ev)
    loss = Z.loss_of_planes(pl, sigma)
    if not want_grad:
        return pl, loss, None
    idx, dx, dy, tau, pos, dt, corners = ev
    cw = W + 1
    for sel, base in ((pos, 0), (~pos, 2)):
        T, C = pl[base], pl[base + 1]
        S = Z._blur(Z._blur(T / (1.0 + C), sigma), sigma)
        gT, gC = (2.0 * S / (1.0 + C)).reshape(-1), (-2.0 * S * T / (1.0 + C) ** 2).reshape(-1)
        q, fx, fy = idx[sel], dx[sel], dy[sel]

        def slopes(img):
            a, b, c, d = img[q], img[q + 1], img[q + cw], img[q + cw + 1]
            return (b - a) * (1.0 - fy) + (d - c) * fy, (c - a) * (1.0 - fx) + (d - b) * fx
        tx, ty = slopes(gT)
        cx, cy = slopes(gC)
        ex, ey = dt[sel] * (tau[sel] * tx + cx), dt[sel] * (tau[sel] * ty + cy)
        for yy, xx, wt, inside in corners:
            m = inside[sel]
            j = (yy[sel] * W + xx[sel])[m]
            g[0] += np.bincount(j, weights=(wt[sel] * ex)[m], minlength=H * W).reshape(H, W)
            g[1] += np.bincount(j, weights=(wt[sel] * ey)[m], minlength=H * W).reshape(H, W)
    return pl, loss, g


def _directions(direction, warped):
    if direction == "both":
        return list(zip(DIRECTIONS, warped if warped is not None else (None, None)))
    return [(direction, warped)]


def planes(flow, x, y, t, p, direction="forward", f32_coords=False, warped=None, p_scale=1.0):
    """(4, H+1, W+1) float64 [T+, C+, T-, C-] (steps 1'-4), one direction."""
    return _one(flow, x, y, t, p, 0.0, direction, f32_coords, warped, p_scale, False)[0]


def images(flow, x, y, t, p, **kw):
    return Z.averages(planes(flow, x, y, t, p, **kw))


def loss(flow, x, y, t, p, sigma=2.0, direction="forward", f32_coords=False, warped=None, p_scale=1.0):
    return sum(_one(flow, x, y, t, p, sigma, d, f32_coords, w, p_scale, False)[1] for d, w in _directions(direction, warped))


def loss_and_grad(flow, x, y, t, p, sigma=2.0, direction="forward", f32_coords=False, warped=None, p_scale=1.0):
    """loss and dloss/dflow (2, H, W) float64 (step 8')."""
    total, g = 0.0, 0.0
    for d, w in _directions(direction, warped):
        _, one, gd = _one(flow, x, y, t, p, sigma, d, f32_coords, w, p_scale, True)
        total, g = total + one, g + gd
    return total, g


def batch_loss_and_grad(flow, x, y, t, p, offsets, sigma=2.0, direction="forward", f32_coords=False, p_scale=1.0):
    """flow (B, 2, H, W), concatenated events, offsets (B + 1,) -> losses (B,), gradients (B, 2, H, W)."""
    res = [loss_and_grad(flow[b], x[a:e], y[a:e], t[a:e], p[a:e], sigma, direction, f32_coords, None, p_scale)
           for b, (a, e) in enumerate(zip(offsets[:-1], offsets[1:]))]
    return np.array([r[0] for r in res]), np.stack([r[1] for r in res])


def scene(h=24, w=32, n=3000, integer=False, seed=0, duration=0.05, speed=60.0):
    """Random events on an (h, w) sensor and a smooth random field of up to `speed` px/s -> flow (2, h, w), x, y, t, p float64.
    float32-exact values, so that the GPU and the restatement start from the same numbers."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    flow = np.stack([speed * np.sin(0.31 * xx + 0.17 * yy + 0.3), speed * np.cos(0.23 * xx - 0.29 * yy)])
    flow = (flow + rng.normal(0.0, 0.1 * speed, flow.shape)).astype(np.float32).astype(np.float64)
    if integer:
        x, y = rng.integers(0, w, n).astype(np.float64), rng.integers(0, h, n).astype(np.float64)
    else:
        x, y = rng.uniform(0.0, w - 1.0, n), rng.uniform(0.0, h - 1.0, n)
    t = np.sort(rng.uniform(0.0, duration, n))
    p = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    x, y, t = (a.astype(np.float32).astype(np.float64) for a in (x, y, t))
    return flow, x, y, t, p
