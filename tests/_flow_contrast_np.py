"""float64 numpy restatement of the contrast (focus) loss of a dense flow field (include/evk.h, "Contrast loss of a flow
field", steps 1-7): the image of warped events, the variance / mean-square loss of its blur and the adjoint
gradient with respect to the field, for one sample or a batch given by offsets.  The field sample, the time constants and the
warp are those of tests/_flow_loss_np.py; the blur is scipy.ndimage.gaussian_filter (mode 'reflect') in float64.

f32_coords / warped=: as in tests/_flow_loss_np.py (the GPU tests pass warp_events_flow_torch's output, so that both sides put
every event in the same cell; for direction 'both' a pair of such pairs, forward then backward).
f32_images=True: the image, its blur B, S = blur(B) and the adjoint image are stored as float32, as the kernels store them (each
axis pass of the blur is evaluated in float64 and rounded once, which is what scipy does on a float32 array); the sums stay
float64.  The difference to the float64 result is the rounding a float32 post pass cannot avoid: where B is almost constant -- a
blur wider than the canvas -- var(B) and the slopes of the adjoint image cancel, and that rounding is all that is left of them.
f32_images=<numpy Generator>: every stored value is moved by -1, 0 or +1 units in the last place besides, drawn from it: another
realisation of the same rounding (a value one unit off is what a float32 sum in another order stores)."""
import numpy as np
from scipy.ndimage import gaussian_filter

from _flow_loss_np import DIRECTIONS, sample, scene, time_constants, warp  # noqa: F401  (scene, warp: for the tests)

OBJECTIVES = ("variance", "mean_square")


def blur(a, sigma):
    return gaussian_filter(a, sigma) if sigma > 0 else a


def _events(flow, x, y, t, p, direction, f32_coords, warped, p_scale, use_polarity):
    """Per counted event: (cell index on the canvas, dx, dy, q, dt, field corners), and the mask over all events (steps 1, 2)."""
    H, W = flow.shape[-2:]
    u, v, corners = sample(flow, x, y, f32_coords)
    dt, _ = time_constants(t, direction, f32_coords)
    if warped is None:
        f = np.float32 if f32_coords else np.float64
        xw, yw = np.asarray(x, dtype=f) + u * dt, np.asarray(y, dtype=f) + v * dt
    else:
        xw, yw = warped
    xw, yw = np.asarray(xw, dtype=np.float64), np.asarray(yw, dtype=np.float64)
    q = np.asarray(p, dtype=np.float64) * float(p_scale)
    if f32_coords:
        q = q.astype(np.float32).astype(np.float64)          # the kernels cast the weight to float32 once
    if not use_polarity:
        q = np.abs(q)
    with np.errstate(invalid="ignore"):
        keep = (xw > 0) & (xw < W) & (yw > 0) & (yw < H) & ~np.isnan(q)
    xc, yc = xw[keep], yw[keep]
    px, py = np.floor(xc), np.floor(yc)
    idx = py.astype(np.int64) * (W + 1) + px.astype(np.int64)
    corners = [(yy[keep], xx[keep], wt[keep].astype(np.float64), inside[keep]) for yy, xx, wt, inside in corners]
    return (idx, xc - px, yc - py, q[keep], dt[keep].astype(np.float64), corners), keep


def _splat(shape, ev):
    idx, dx, dy, q = ev[:4]
    cw, size = shape[1], shape[0] * shape[1]
    out = np.zeros(size)
    ax, ay = 1.0 - dx, 1.0 - dy
    for off, wt in ((0, ax * ay), (1, dx * ay), (cw, ax * dy), (cw + 1, dx * dy)):
        out += np.bincount(idx + off, weights=q * wt, minlength=size)
    return out.reshape(shape)


def _stored(a, f32_images):
    if f32_images is False:
        return a
    a = np.asarray(a, dtype=np.float32)
    if isinstance(f32_images, np.random.Generator):
        step = f32_images.integers(-1, 2, a.shape)
        up, down = np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))
        a = np.where(step > 0, up, np.where(step < 0, down, a)).astype(np.float32)
    return a


def loss_of_image(img, sigma, objective="variance", f32_images=False):
    """Steps 4-5 -> (loss, B)."""
    b = np.asarray(blur(_stored(img, f32_images), sigma), dtype=np.float64)
    if objective == "variance":
        return -np.mean((b - b.mean()) ** 2), b
    if objective == "mean_square":
        return -np.mean(b ** 2), b
    raise ValueError(objective)


def adjoint_of_image(b, sigma, objective="variance", f32_images=False):
    """Step 6: G = dL/dI from the blurred image B."""
    s = np.asarray(blur(_stored(b, f32_images), sigma), dtype=np.float64)
    g = -2.0 / b.size * (s - b.mean() if objective == "variance" else s)
    return np.asarray(_stored(g, f32_images), dtype=np.float64)


def _one(flow, x, y, t, p, sigma, objective, direction, f32_coords, warped, p_scale, use_polarity, want_grad, f32_images=False):
    """(iwe, loss, gradient | None) of one sample in one direction."""
    flow = np.asarray(flow)
    H, W = flow.shape[-2:]
    shape = (H + 1, W + 1)
    g = np.zeros((2, H, W))
    if objective not in OBJECTIVES:
        raise ValueError(objective)
    if len(t) == 0:
        return np.zeros(shape), 0.0, g
    ev, _ = _events(flow, x, y, t, p, direction, f32_coords, warped, p_scale, use_polarity)
    img = _splat(shape, ev)
    loss, b = loss_of_image(img, sigma, objective, f32_images)
    if not want_grad:
        return img, loss, None
    idx, dx, dy, q, dt, corners = ev
    cw = W + 1
    G = adjoint_of_image(b, sigma, objective, f32_images).reshape(-1)
    a_, b_, c_, d_ = G[idx], G[idx + 1], G[idx + cw], G[idx + cw + 1]
    ex = dt * q * ((b_ - a_) * (1.0 - dy) + (d_ - c_) * dy)
    ey = dt * q * ((c_ - a_) * (1.0 - dx) + (d_ - b_) * dx)
    for yy, xx, wt, inside in corners:
        m = inside & (wt != 0)
        j = (yy * W + xx)[m]
        g[0] += np.bincount(j, weights=(wt * ex)[m], minlength=H * W).reshape(H, W)
        g[1] += np.bincount(j, weights=(wt * ey)[m], minlength=H * W).reshape(H, W)
    return img, loss, g


def _directions(direction, warped):
    if direction == "both":
        return list(zip(DIRECTIONS, warped if warped is not None else (None, None)))
    return [(direction, warped)]


def iwe(flow, x, y, t, p, direction="forward", f32_coords=False, warped=None, p_scale=1.0, use_polarity=True):
    """(H+1, W+1) float64 (steps 1-3), one direction."""
    return _one(flow, x, y, t, p, 0.0, "variance", direction, f32_coords, warped, p_scale, use_polarity, False)[0]


def kept(flow, x, y, t, p, direction="forward", f32_coords=False, warped=None, p_scale=1.0):
    """The mask of the events that count."""
    return _events(np.asarray(flow), x, y, t, p, direction, f32_coords, warped, p_scale, True)[1]


def loss(flow, x, y, t, p, sigma=1.0, objective="variance", direction="forward", f32_coords=False, warped=None, p_scale=1.0,
         use_polarity=True):
    return sum(_one(flow, x, y, t, p, sigma, objective, d, f32_coords, w, p_scale, use_polarity, False)[1]
               for d, w in _directions(direction, warped))


def loss_and_grad(flow, x, y, t, p, sigma=1.0, objective="variance", direction="forward", f32_coords=False, warped=None,
                  p_scale=1.0, use_polarity=True, f32_images=False):
    """loss and dloss/dflow (2, H, W) float64 (step 7)."""
    total, g = 0.0, 0.0
    for d, w in _directions(direction, warped):
        _, one, gd = _one(flow, x, y, t, p, sigma, objective, d, f32_coords, w, p_scale, use_polarity, True, f32_images)
        total, g = total + one, g + gd
    return total, g


def batch_loss_and_grad(flow, x, y, t, p, offsets, sigma=1.0, objective="variance", direction="forward", f32_coords=False,
                        p_scale=1.0, use_polarity=True):
    """flow (B, 2, H, W), concatenated events, offsets (B + 1,) -> losses (B,), gradients (B, 2, H, W)."""
    res = [loss_and_grad(flow[b], x[a:e], y[a:e], t[a:e], p[a:e], sigma, objective, direction, f32_coords, None, p_scale,
                         use_polarity) for b, (a, e) in enumerate(zip(offsets[:-1], offsets[1:]))]
    return np.array([r[0] for r in res]), np.stack([r[1] for r in res])
