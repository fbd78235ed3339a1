"""float64 numpy restatement of the average-timestamp objective (include/evk.h, "Average-timestamp objective"; DESIGN.md
section 6) for the linear flow and the four parametric models: the four planes [T+, C+, T-, C-], the pair of average-timestamp
images, the loss and its adjoint gradient.  Warps and Jacobians are those of tests/_motion_models_np.py and
tests/_motion_models8_np.py, plus the linear flow.

f32_coords: the kernels cast the warped coordinates to float32 before floor / fraction (as get_iwe does, Q7) and form the
normalised timestamp in float32 on float32 columns; True restates that (what the GPU tests compare with), False keeps float64
throughout (the definition itself: what the finite-difference tests differentiate)."""
import numpy as np
from scipy.ndimage import gaussian_filter

import _motion_models8_np as M8
import _motion_models_np as M4

LINVEL, ROTATION, XYZTHETA, ANGVEL, PLANAR = "linvel", M4.ROTATION, M4.XYZTHETA, M8.ANGVEL, M8.PLANAR
MODELS = (LINVEL, ROTATION, XYZTHETA, ANGVEL, PLANAR)
DIMS = {LINVEL: 2, ROTATION: 3, XYZTHETA: 4, ANGVEL: 3, PLANAR: 8}


def warp(model, x, y, t, t0, params, center=(0.0, 0.0), camera_matrix=M8.K_DEFAULT):
    """-> x', y', jx (dims, n), jy (dims, n), float64."""
    if model == LINVEL:
        x, y, t = (np.asarray(a, dtype=np.float64) for a in (x, y, t))
        dt = t - t0
        z = np.zeros_like(dt)
        return x - dt * float(params[0]), y - dt * float(params[1]), np.stack([-dt, z]), np.stack([z, -dt])
    if model in (ROTATION, XYZTHETA):
        return M4.warp(model, x, y, t, t0, params, center)
    return M8.warp(model, x, y, t, t0, params, center, camera_matrix)


def _events(model, params, x, y, t, p, img_size, sensor_size, center, camera_matrix, f32_coords, t_ref=None):
    """Per counted event: (px, py, dx, dy, tau, positive, jx, jy) and the boolean mask over all events."""
    H, W = int(sensor_size[0]) + 1, int(sensor_size[1]) + 1
    t64 = np.asarray(t, dtype=np.float64)
    t0 = float(t64[-1]) if t_ref is None else float(t_ref)
    xw, yw, jx, jy = warp(model, x, y, t64, t0, params, center, camera_matrix)
    if f32_coords and np.asarray(t).dtype == np.float32:
        tf = np.asarray(t, dtype=np.float32)
        tdiv = np.float32(np.float32(tf[-1] - tf[0]) + np.float32(1e-6))
        tau = ((tf - tf[0]) / tdiv).astype(np.float64)
    else:
        tau = (t64 - t64[0]) / (t64[-1] - t64[0] + 1e-6)
        if f32_coords:
            tau = tau.astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        keep = (xw > 0) & (xw <= img_size[1]) & (yw > 0) & (yw <= img_size[0])
        if f32_coords:
            xc, yc = xw.astype(np.float32), yw.astype(np.float32)
        else:
            xc, yc = xw, yw
        keep &= (xc < W - 1) & (yc < H - 1)
    pv = np.asarray(p, dtype=np.float64)
    keep &= ~np.isnan(pv)
    xc, yc = xc[keep].astype(np.float64), yc[keep].astype(np.float64)
    px, py = np.floor(xc), np.floor(yc)
    dx, dy = xc - px, yc - py
    return (px.astype(np.int64), py.astype(np.int64), dx, dy, tau[keep], pv[keep] > 0, jx[:, keep], jy[:, keep]), keep


def mask(model, params, x, y, t, p, img_size=(180, 240), sensor_size=None, center=(0.0, 0.0), camera_matrix=M8.K_DEFAULT,
         f32_coords=False, t_ref=None):
    """Which events count (step 2 of the definition)."""
    sensor_size = img_size if sensor_size is None else sensor_size
    if len(t) == 0:
        return np.zeros(0, dtype=bool)
    return _events(model, params, x, y, t, p, img_size, sensor_size, center, camera_matrix, f32_coords, t_ref)[1]


def _splat(shape, ev):
    px, py, dx, dy, tau, pos, _, _ = ev
    out = np.zeros((4,) + shape)
    ax, ay = 1.0 - dx, 1.0 - dy
    for sel, base in ((pos, 0), (~pos, 2)):
        for ox, oy, wt in ((0, 0, ax * ay), (1, 0, dx * ay), (0, 1, ax * dy), (1, 1, dx * dy)):
            np.add.at(out[base], (py[sel] + oy, px[sel] + ox), (tau * wt)[sel])
            np.add.at(out[base + 1], (py[sel] + oy, px[sel] + ox), wt[sel])
    return out


def planes(model, params, x, y, t, p, img_size=(180, 240), sensor_size=None, center=(0.0, 0.0), camera_matrix=M8.K_DEFAULT,
           f32_coords=False, t_ref=None):
    """(4, H+1, W+1) float64 [T+, C+, T-, C-] (steps 1-4)."""
    sensor_size = img_size if sensor_size is None else sensor_size
    shape = (int(sensor_size[0]) + 1, int(sensor_size[1]) + 1)
    if len(t) == 0:
        return np.zeros((4,) + shape)
    ev, _ = _events(model, params, x, y, t, p, img_size, sensor_size, center, camera_matrix, f32_coords, t_ref)
    return _splat(shape, ev)


def averages(pl):
    """(2, H+1, W+1) [A+, A-] = T_c / (1 + C_c) (step 5)."""
    return np.stack([pl[0] / (1.0 + pl[1]), pl[2] / (1.0 + pl[3])])


def images(model, params, x, y, t, p, **kw):
    return averages(planes(model, params, x, y, t, p, **kw))


def _blur(a, sigma):
    return gaussian_filter(a, sigma) if sigma > 0 else a


def loss_of_planes(pl, sigma=2.0):
    return float(sum(np.sum(_blur(a, sigma) ** 2) for a in averages(pl)))


def loss(model, params, x, y, t, p, sigma=2.0, **kw):
    """sum B_+^2 + sum B_-^2 (steps 6-7), to be minimised."""
    return loss_of_planes(planes(model, params, x, y, t, p, **kw), sigma)


def grad(model, params, x, y, t, p, sigma=2.0, img_size=(180, 240), sensor_size=None, center=(0.0, 0.0),
         camera_matrix=M8.K_DEFAULT, f32_coords=False, t_ref=None):
    """The adjoint gradient (step 8), (dims,) float64."""
    sensor_size = img_size if sensor_size is None else sensor_size
    shape = (int(sensor_size[0]) + 1, int(sensor_size[1]) + 1)
    g = np.zeros(DIMS[model])
    if len(t) == 0:
        return g
    ev, _ = _events(model, params, x, y, t, p, img_size, sensor_size, center, camera_matrix, f32_coords, t_ref)
    px, py, dx, dy, tau, pos, jx, jy = ev
    pl = _splat(shape, ev)
    for sel, base in ((pos, 0), (~pos, 2)):
        T, C = pl[base], pl[base + 1]
        S = _blur(_blur(T / (1.0 + C), sigma), sigma)
        gT, gC = 2.0 * S / (1.0 + C), -2.0 * S * T / (1.0 + C) ** 2
        qx, qy, fx, fy = px[sel], py[sel], dx[sel], dy[sel]

        def slopes(img):
            a, b, c, d = img[qy, qx], img[qy, qx + 1], img[qy + 1, qx], img[qy + 1, qx + 1]
            return (b - a) * (1.0 - fy) + (d - c) * fy, (c - a) * (1.0 - fx) + (d - b) * fx
        tx, ty = slopes(gT)
        cx, cy = slopes(gC)
        ex, ey = tau[sel] * tx + cx, tau[sel] * ty + cy
        g += jx[:, sel] @ ex + jy[:, sel] @ ey
    return g


# ---- synthetic scenes ---------------------------------------------------------------------------------------------------
LV_TRUTH = np.array([40.0, -25.0])
LV_START = np.array([34.0, -20.0])
TRUTH = {LINVEL: LV_TRUTH, ROTATION: M4.ROT_TRUTH, XYZTHETA: M4.XYZ_TRUTH, ANGVEL: M8.AV_TRUTH, PLANAR: M8.PF_TRUTH}
START = {LINVEL: LV_START, ROTATION: M4.ROT_START, XYZTHETA: M4.XYZ_START, ANGVEL: M8.AV_START, PLANAR: M8.PF_START}
TOL = {LINVEL: np.array([3.0, 3.0]), ROTATION: M4.TOL[ROTATION], XYZTHETA: M4.TOL[XYZTHETA], ANGVEL: M8.TOL[ANGVEL],
       PLANAR: M8.TOL[PLANAR]}
CENTER = {LINVEL: (0.0, 0.0), ROTATION: (0.0, 0.0), XYZTHETA: M4.XYZ_CENTER, ANGVEL: (0.0, 0.0), PLANAR: M8.PF_CENTER}


def scene(model, n=20000, points=250, duration=0.1, seed=0):
    """The scene of the motion-model tests for `model` (events of scene points that the model at TRUTH[model] maps back onto
    their point at t[-1]; the linear flow: the same construction), with a polarity per scene point instead of all ones, so
    that both classes of the objective are exercised.  -> x, y, t, p float64."""
    if model == LINVEL:
        rng = np.random.default_rng(seed)
        sx, sy = rng.uniform(30, 210, points), rng.uniform(25, 155, points)
        k = rng.integers(0, points, n)
        t = np.sort(rng.uniform(0.0, duration, n))
        t[-1] = duration
        dt = t - t[-1]
        x, y = sx[k] + dt * LV_TRUTH[0], sy[k] + dt * LV_TRUTH[1]
    elif model in (ROTATION, XYZTHETA):
        x, y, t, _ = M4.scene(model, n, points, duration, seed)
    else:
        x, y, t, _ = M8.scene(model, n, points, duration, seed)
    # the scenes draw the point of every event as their third random array: the same draw gives the polarity of its point
    rng = np.random.default_rng(seed)
    rng.uniform(30, 210, points)
    rng.uniform(25, 155, points)
    k = rng.integers(0, points, n)
    p = np.where(np.arange(points) % 2 == 0, 1.0, -1.0)[k]
    return x, y, t, p
