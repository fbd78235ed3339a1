"""numpy restatement of the rotation and xyztheta motion models (DESIGN.md "Rotation and xyztheta warps"): warps and
Jacobians in float64, IWE / dIWE splats in float64 with np.add.at, blur with scipy.ndimage.gaussian_filter, the variance
objective and the gradient sums of the other objectives, and the two synthetic scenes the tests optimise on."""
import numpy as np
from scipy.ndimage import gaussian_filter

ROTATION, XYZTHETA = "rotation", "xyztheta"
DIMS = {ROTATION: 3, XYZTHETA: 4}


def warp(model, x, y, t, t0, params, center=(0.0, 0.0)):
    """-> x', y', jx (dims, n), jy (dims, n), float64."""
    x, y, t = (np.asarray(a, dtype=np.float64) for a in (x, y, t))
    dt = t - t0
    if model == ROTATION:
        cx, cy, om = (float(v) for v in params)
        u, v = x - cx, y - cy
        th = -om * dt
        c, s = np.cos(th), np.sin(th)
        xo = cx + c * u - s * v
        yo = cy + s * u + c * v
        jx = np.stack([1.0 - c, s, dt * (s * u + c * v)])
        jy = np.stack([-s, 1.0 - c, -dt * (c * u - s * v)])
    else:
        vx, vy, vz, om = (float(v) for v in params)
        u, v = x - center[0], y - center[1]
        xo = x - dt * (vx + vz * u - om * v)
        yo = y - dt * (vy + vz * v + om * u)
        z = np.zeros_like(dt)
        jx = np.stack([-dt, z, -dt * u, dt * v])
        jy = np.stack([z, -dt, -dt * v, -dt * u])
    return xo, yo, jx, jy


def iwe(model, params, x, y, t, p, img_size=(180, 240), sensor_size=(180, 240), use_polarity=True, compute_gradient=True,
        center=(0.0, 0.0), p_scale=1.0):
    """get_iwe: warp at t0 = t[-1], events_bounds_mask(0, W, 0, H), inner clip at the padded canvas, bilinear splat."""
    H, W = int(sensor_size[0]) + 1, int(sensor_size[1]) + 1
    dims = DIMS[model]
    img = np.zeros((H, W))
    d_img = np.zeros((dims, H, W))
    if len(t) == 0:
        return img, (d_img if compute_gradient else None)
    xw, yw, jx, jy = warp(model, x, y, t, float(np.asarray(t, dtype=np.float64)[-1]), params, center)
    pd = np.asarray(p, dtype=np.float64) * p_scale
    if not use_polarity:
        pd = np.abs(pd)
    keep = (xw > 0) & (xw <= img_size[1]) & (yw > 0) & (yw <= img_size[0])
    xf, yf = xw.astype(np.float32), yw.astype(np.float32)
    keep &= (xf < W - 1) & (yf < H - 1)
    xf, yf, mp = xf[keep].astype(np.float64), yf[keep].astype(np.float64), pd[keep]
    jx, jy = jx[:, keep], jy[:, keep]
    px, py = np.floor(xf), np.floor(yf)
    dx, dy = xf - px, yf - py
    px, py = px.astype(np.int64), py.astype(np.int64)
    ax, ay = 1.0 - dx, 1.0 - dy
    np.add.at(img, (py, px), mp * ax * ay)
    np.add.at(img, (py, px + 1), mp * dx * ay)
    np.add.at(img, (py + 1, px), mp * ax * dy)
    np.add.at(img, (py + 1, px + 1), mp * dx * dy)
    if not compute_gradient:
        return img, None
    for i in range(dims):
        w1, w2 = jx[i] * mp, jy[i] * mp
        np.add.at(d_img[i], (py, px), -w1 * ay - w2 * ax)
        np.add.at(d_img[i], (py, px + 1), w1 * ay - w2 * dx)
        np.add.at(d_img[i], (py + 1, px), -w1 * dy + w2 * ax)
        np.add.at(d_img[i], (py + 1, px + 1), w1 * dy + w2 * dx)
    return img, d_img


def _blur(a, sigma):
    return gaussian_filter(a, sigma) if sigma > 0 else a


def blurred(img, d_img, sigma, mix, blur_iwe):
    """(a, d): d = one 3-D filter of d_img with `mix` (Q4), else plane by plane; a = img, blurred with blur_iwe."""
    if sigma > 0:
        d = gaussian_filter(d_img, sigma) if mix else np.stack([gaussian_filter(c, sigma) for c in d_img])
    else:
        d = d_img
    return (_blur(img, sigma) if blur_iwe else img), d


def variance_f(img, sigma):
    return -np.var(_blur(img, sigma))


def variance_grad(img, d_img, sigma, reference_exact=True):
    a, d = blurred(img, d_img, sigma, reference_exact, not reference_exact)
    return -np.array([np.mean(2.0 * (a - a.mean()) * d[i]) for i in range(d.shape[0])])


def gradsums(img, d_img, sigma, g, blur_iwe):
    """sum g(a) d_i over the planes with d = 3-D blurred d_img (Q4)."""
    a, d = blurred(img, d_img, sigma, True, blur_iwe)
    ga = g(a)
    return np.array([np.sum(ga * d[i]) for i in range(d.shape[0])]), a.size


def objective(model, x, y, t, p, sigma=1.0, reference_exact=False, center=(0.0, 0.0), img_size=(180, 240)):
    """(f, grad) callables of the variance objective for scipy (numpy arrays of the events bound)."""
    def f(q):
        return variance_f(iwe(model, q, x, y, t, p, img_size, compute_gradient=False, center=center)[0], sigma)

    def g(q):
        img, d_img = iwe(model, q, x, y, t, p, img_size, center=center)
        return variance_grad(img, d_img, sigma, reference_exact)
    return f, g


# ---- synthetic scenes ---------------------------------------------------------------------------------------------------
ROT_TRUTH = np.array([110.0, 95.0, 1.5])            # centre (110, 95), 1.5 rad/s
ROT_START = np.array([104.0, 100.0, 1.2])
XYZ_TRUTH = np.array([40.0, -25.0, 2.0, 1.0])       # px/s, px/s, 1/s, rad/s about XYZ_CENTER
XYZ_START = np.array([34.0, -20.0, 1.7, 0.8])
XYZ_CENTER = (120.0, 90.0)
TOL = {ROTATION: np.array([2.0, 2.0, 0.05]), XYZTHETA: np.array([3.0, 3.0, 0.05, 0.05])}


def scene(model, n=20000, points=250, duration=0.1, seed=0):
    """Events of `points` scene points seen at random times over `duration` s, moving so that the model at the truth
    maps every event back onto its point at t0 = t[-1]; unit polarities.  -> x, y, t, p (float64)."""
    rng = np.random.default_rng(seed)
    sx = rng.uniform(30, 210, points)
    sy = rng.uniform(25, 155, points)
    k = rng.integers(0, points, n)
    t = np.sort(rng.uniform(0.0, duration, n))
    t[-1] = duration
    dt = t - t[-1]
    if model == ROTATION:
        cx, cy, om = ROT_TRUTH
        th = om * dt                    # the inverse of theta = -omega dt
        c, s = np.cos(th), np.sin(th)
        u, v = sx[k] - cx, sy[k] - cy
        x, y = cx + c * u - s * v, cy + s * u + c * v
    else:
        vx, vy, vz, om = XYZ_TRUTH
        up, vp = sx[k] - XYZ_CENTER[0], sy[k] - XYZ_CENTER[1]
        # [u'; v'] = M [u; v] - dt [vx; vy], M = [[1 - dt vz, dt om], [-dt om, 1 - dt vz]]
        a, b = 1.0 - dt * vz, dt * om
        ru, rv = up + dt * vx, vp + dt * vy
        det = a * a + b * b
        u = (a * ru - b * rv) / det
        v = (b * ru + a * rv) / det
        x, y = XYZ_CENTER[0] + u, XYZ_CENTER[1] + v
    p = np.ones(n)
    return x, y, t, p
