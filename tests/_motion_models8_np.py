"""numpy restatement of the angular-velocity and planar-flow motion models (DESIGN.md "Angular-velocity and planar-flow
warps"): warps and Jacobians in float64 (the formulas of include/evk.h, term by term), IWE / dIWE splats over `dims` planes
in float64 with np.add.at, and the two synthetic scenes the tests optimise on.  Blur, variance and gradient sums are those
of tests/_motion_models_np.py."""
import numpy as np

from _motion_models_np import blurred, gradsums, variance_f, variance_grad  # noqa: F401

ANGVEL, PLANAR = "angular_velocity", "planar_flow"
DIMS = {ANGVEL: 3, PLANAR: 8}
K_DEFAULT = np.array([[200.0, 0.0, 120.0], [0.0, 200.0, 90.0], [0.0, 0.0, 1.0]])


def hat(v):
    """[v]x, (..., 3) -> (..., 3, 3)."""
    v = np.asarray(v, dtype=np.float64)
    z = np.zeros(v.shape[:-1])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def so3(theta):
    """(R = exp([theta]x), Jr(theta)) per row of theta (n, 3); a series below |theta| = 1e-2, exactly I at 0."""
    a2 = np.sum(theta * theta, axis=-1)
    small = a2 < 1e-4
    a = np.sqrt(np.where(small, 1.0, a2))
    s, c = np.sin(a), np.cos(a)
    A = np.where(small, 1.0 - a2 / 6.0 + a2 * a2 / 120.0, s / a)
    B = np.where(small, 0.5 - a2 / 24.0 + a2 * a2 / 720.0, (1.0 - c) / np.where(small, 1.0, a2))
    C = np.where(small, 1.0 / 6.0 - a2 / 120.0 + a2 * a2 / 5040.0, (a - s) / (np.where(small, 1.0, a2) * a))
    T = hat(theta)
    T2 = T @ T
    eye = np.eye(3)
    R = eye + A[:, None, None] * T + B[:, None, None] * T2
    Jr = eye - B[:, None, None] * T + C[:, None, None] * T2
    return R, Jr


def warp(model, x, y, t, t0, params, center=(0.0, 0.0), camera_matrix=K_DEFAULT):
    """-> x', y', jx (dims, n), jy (dims, n), float64.  Angular velocity: NaN x', y' (and Jacobians) behind the camera."""
    x, y, t = (np.asarray(a, dtype=np.float64) for a in (x, y, t))
    dt = t - t0
    if model == ANGVEL:
        K = np.asarray(camera_matrix, dtype=np.float64)
        fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
        w = np.asarray(params, dtype=np.float64)
        b = np.stack([(x - cx) / fx, (y - cy) / fy, np.ones_like(x)], -1)
        R, Jr = so3(w[None, :] * dt[:, None])
        P = np.einsum("nij,nj->ni", R, b)
        dP = -(R @ hat(b) @ Jr) * dt[:, None, None]                     # (n, 3, 3): dP_i / dw_k
        P0, P1, P2 = P[:, 0], P[:, 1], P[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            xo, yo = fx * P0 / P2 + cx, fy * P1 / P2 + cy
            jx = (fx / P2)[:, None] * dP[:, 0, :] - (fx * P0 / P2 ** 2)[:, None] * dP[:, 2, :]
            jy = (fy / P2)[:, None] * dP[:, 1, :] - (fy * P1 / P2 ** 2)[:, None] * dP[:, 2, :]
        bad = ~((P2 > 0) & np.all(np.isfinite(P), axis=1))
        xo[bad] = yo[bad] = np.nan
        jx[bad] = jy[bad] = np.nan
        return xo, yo, jx.T.copy(), jy.T.copy()
    a = [float(v) for v in params]
    u, v = x - center[0], y - center[1]
    xo = x - dt * (a[0] + a[1] * u + a[2] * v + a[6] * u * u + a[7] * u * v)
    yo = y - dt * (a[3] + a[4] * u + a[5] * v + a[6] * u * v + a[7] * v * v)
    z = np.zeros_like(dt)
    jx = np.stack([-dt, -dt * u, -dt * v, z, z, z, -dt * u * u, -dt * u * v])
    jy = np.stack([z, z, z, -dt, -dt * u, -dt * v, -dt * u * v, -dt * v * v])
    return xo, yo, jx, jy


def splat(xw, yw, jx, jy, p, img_size=(180, 240), sensor_size=(180, 240), use_polarity=True, compute_gradient=True,
          p_scale=1.0):
    """events_bounds_mask(0, W, 0, H) (NaN rejected), inner clip at the padded canvas, bilinear splat of the IWE and of
    the dims dIWE planes (w1 = jx_i mp, w2 = jy_i mp)."""
    H, W = int(sensor_size[0]) + 1, int(sensor_size[1]) + 1
    dims = jx.shape[0]
    img = np.zeros((H, W))
    d_img = np.zeros((dims, H, W))
    pd = np.asarray(p, dtype=np.float64) * p_scale
    if not use_polarity:
        pd = np.abs(pd)
    with np.errstate(invalid="ignore"):
        keep = (xw > 0) & (xw <= img_size[1]) & (yw > 0) & (yw <= img_size[0])
    xf, yf = xw[keep].astype(np.float32), yw[keep].astype(np.float32)
    k2 = (xf < W - 1) & (yf < H - 1)
    xf, yf, mp = xf[k2].astype(np.float64), yf[k2].astype(np.float64), pd[keep][k2]
    jx, jy = jx[:, keep][:, k2], jy[:, keep][:, k2]
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


def iwe(model, params, x, y, t, p, img_size=(180, 240), sensor_size=(180, 240), use_polarity=True, compute_gradient=True,
        center=(0.0, 0.0), camera_matrix=K_DEFAULT, p_scale=1.0):
    """get_iwe: warp at t0 = t[-1], then splat(); in slices of a million events (the sums are the same)."""
    H, W = int(sensor_size[0]) + 1, int(sensor_size[1]) + 1
    img, d_img = np.zeros((H, W)), (np.zeros((DIMS[model], H, W)) if compute_gradient else None)
    if len(t) == 0:
        return img, d_img
    t0 = float(np.asarray(t, dtype=np.float64)[-1])
    for s in range(0, len(t), 1 << 20):
        sl = slice(s, s + (1 << 20))
        xw, yw, jx, jy = warp(model, x[sl], y[sl], t[sl], t0, params, center, camera_matrix)
        i, d = splat(xw, yw, jx, jy, p[sl], img_size, sensor_size, use_polarity, compute_gradient, p_scale)
        img += i
        if compute_gradient:
            d_img += d
    return img, d_img


def objective(model, x, y, t, p, sigma=1.0, reference_exact=False, center=(0.0, 0.0), camera_matrix=K_DEFAULT,
              img_size=(180, 240)):
    """(f, grad) callables of the variance objective for scipy (numpy arrays of the events bound)."""
    def f(q):
        return variance_f(iwe(model, q, x, y, t, p, img_size, compute_gradient=False, center=center,
                              camera_matrix=camera_matrix)[0], sigma)

    def g(q):
        img, d_img = iwe(model, q, x, y, t, p, img_size, center=center, camera_matrix=camera_matrix)
        return variance_grad(img, d_img, sigma, reference_exact)
    return f, g


def xyztheta_as_planar(q):
    """xyztheta_warp(center) at (vx, vy, vz, w) = planar_flow_warp(center) at these parameters."""
    vx, vy, vz, w = q
    return np.array([vx, vz, -w, vy, w, vz, 0.0, 0.0])


def linvel_as_planar(q):
    return np.array([q[0], 0.0, 0.0, q[1], 0.0, 0.0, 0.0, 0.0])


# ---- synthetic scenes ---------------------------------------------------------------------------------------------------
AV_TRUTH = np.array([0.8, -0.6, 1.2])                # rad/s, with K_DEFAULT
AV_START = np.array([0.6, -0.4, 1.0])
PF_CENTER = (120.0, 90.0)
PF_TRUTH = np.array([40.0, 0.5, -0.3, -25.0, 0.2, 0.6, 2e-3, -1.5e-3])
PF_START = np.array([35.0, 0.4, -0.2, -20.0, 0.15, 0.5, 0.0, 0.0])
TOL = {ANGVEL: np.array([0.05, 0.05, 0.05]),
       PLANAR: np.array([3.0, 0.1, 0.1, 3.0, 0.1, 0.1, 1e-3, 1e-3])}


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
    if model == ANGVEL:
        # x = pi(K exp([-w dt]x) K^-1 x0)
        K = K_DEFAULT
        b = np.stack([(sx[k] - K[0, 2]) / K[0, 0], (sy[k] - K[1, 2]) / K[1, 1], np.ones(n)], -1)
        R, _ = so3(-AV_TRUTH[None, :] * dt[:, None])
        P = np.einsum("nij,nj->ni", R, b)
        x, y = K[0, 0] * P[:, 0] / P[:, 2] + K[0, 2], K[1, 1] * P[:, 1] / P[:, 2] + K[1, 2]
    else:
        # x - dt f(x) = x0: fixed point x = x0 + dt f(x) (a contraction: |dt grad f| << 1)
        a = PF_TRUTH
        x0, y0 = sx[k], sy[k]
        x, y = x0.copy(), y0.copy()
        for _ in range(60):
            u, v = x - PF_CENTER[0], y - PF_CENTER[1]
            x = x0 + dt * (a[0] + a[1] * u + a[2] * v + a[6] * u * u + a[7] * u * v)
            y = y0 + dt * (a[3] + a[4] * u + a[5] * v + a[6] * u * v + a[7] * v * v)
    p = np.ones(n)
    return x, y, t, p
