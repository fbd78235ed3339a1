"""The definition of camera tracking (include/evk.h, "Camera tracking") restated literally in float64 numpy: the
per-point residual and Jacobian with one rounding per operation in the order the header states, the robust weights, the sums by
math.fsum, the exponential of se(3), and the Levenberg-Marquardt loop.  Nothing here is shared with the product; the tests compare
the device's per-point values with it bit for bit, and its sums within the bound of the summation."""
import math

import numpy as np

LAMBDA0, LAMBDA_MIN, LAMBDA_MAX = 1e-3, 1e-9, 1e6
STATUS = ("converged", "stalled", "max_evals", "lost")


# ---- per point -------------------------------------------------------------------------------------------------------------------

def residuals(P, S, intrinsics, R, t):
    """-> r (M,), J (M, 6), valid (M,) bool; r and J are NaN where the point is not valid"""
    fx, fy, cx, cy = (np.float64(v) for v in intrinsics)
    P, R, t = np.asarray(P, dtype=np.float64), np.asarray(R, dtype=np.float64), np.asarray(t, dtype=np.float64)
    S = np.asarray(S)
    assert S.dtype == np.float32 and S.ndim == 2
    H, W = S.shape
    with np.errstate(all="ignore"):
        X = ((R[0, 0] * P[:, 0] + R[0, 1] * P[:, 1]) + R[0, 2] * P[:, 2]) + t[0]
        Y = ((R[1, 0] * P[:, 0] + R[1, 1] * P[:, 1]) + R[1, 2] * P[:, 2]) + t[1]
        Z = ((R[2, 0] * P[:, 0] + R[2, 1] * P[:, 1]) + R[2, 2] * P[:, 2]) + t[2]
        valid = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (Z > 0.0)
        u = fx * (X / Z) + cx
        v = fy * (Y / Z) + cy
        valid &= (u >= 0.0) & (u < np.float64(W - 1)) & (v >= 0.0) & (v < np.float64(H - 1))
        fu, fv = np.floor(u), np.floor(v)
        x0, y0 = np.where(valid, fu, 0.0).astype(np.int64), np.where(valid, fv, 0.0).astype(np.int64)
        S00, S01 = S[y0, x0].astype(np.float64), S[y0, x0 + 1].astype(np.float64)
        S10, S11 = S[y0 + 1, x0].astype(np.float64), S[y0 + 1, x0 + 1].astype(np.float64)
        valid &= np.isfinite(S00) & np.isfinite(S01) & np.isfinite(S10) & np.isfinite(S11)
        a, b = u - fu, v - fv
        a1, b1 = 1.0 - a, 1.0 - b
        r = b1 * (a1 * S00 + a * S01) + b * (a1 * S10 + a * S11)
        gx = b1 * (S01 - S00) + b * (S11 - S10)
        gy = a1 * (S10 - S00) + a * (S11 - S01)
        qx, qy = gx * fx, gy * fy
        j0, j1 = qx / Z, qy / Z
        j2 = -((qx * X + qy * Y) / (Z * Z))
        J = np.stack((j0, j1, j2, Y * j2 - Z * j1, Z * j0 - X * j2, X * j1 - Y * j0), axis=1)
    r = np.where(valid, r, np.nan)
    J = np.where(valid[:, None], J, np.nan)
    return r, J, valid


def weights(r, loss="l2", delta=None):
    """-> (w, rho) of the residuals r"""
    r = np.asarray(r, dtype=np.float64)
    if loss == "l2":
        return np.ones_like(r), r * r
    assert loss == "huber" and delta > 0
    delta, ar = np.float64(delta), np.abs(r)
    tail = ar > delta
    with np.errstate(all="ignore"):
        return np.where(tail, delta / ar, 1.0), np.where(tail, delta * (2.0 * ar - delta), r * r)


def products(P, S, intrinsics, R, t, loss="l2", delta=None):
    """the 29 terms of every valid point, (n, 29): (w J_i) J_j for i <= j row-major, (w J_i) r, rho, 1"""
    r, J, valid = residuals(P, S, intrinsics, R, t)
    r, J = r[valid], J[valid]
    w, rho = weights(r, loss, delta)
    wJ = w[:, None] * J
    cols = [wJ[:, i] * J[:, j] for i in range(6) for j in range(i, 6)] + [wJ[:, i] * r for i in range(6)] + [rho, np.ones_like(r)]
    return np.stack(cols, axis=1) if len(r) else np.zeros((0, 29))


def unpack(sums):
    """29 sums -> A (6, 6), g (6,), c, n"""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = sums[:21]
    A = A + np.triu(A, 1).T
    return A, np.array(sums[21:27], dtype=np.float64), float(sums[27]), int(sums[28])


def terms(P, S, intrinsics, R, t, loss="l2", delta=None):
    """-> A, g, c, n with every sum correctly rounded (math.fsum)"""
    T = products(P, S, intrinsics, R, t, loss, delta)
    return unpack([math.fsum(T[:, k]) for k in range(29)])


# ---- poses -----------------------------------------------------------------------------------------------------------------------

def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_exp(xi):
    """xi = (upsilon, omega) -> (R, t) of exp(xi^)"""
    xi = np.asarray(xi, dtype=np.float64)
    W = hat(xi[3:])
    th2 = float(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5])
    th = math.sqrt(th2)
    if th2 < 1e-8:                                          # (the closed forms cancel: 1 - cos th is 0 below 1e-8)
        A, B, C = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0, 1.0 / 6.0 - th2 / 120.0
    else:
        sh = math.sin(0.5 * th)
        A, B, C = math.sin(th) / th, (2.0 * sh * sh) / th2, (th - math.sin(th)) / (th2 * th)
    W2 = W @ W
    return (np.eye(3) + A * W) + B * W2, ((np.eye(3) + B * W) + C * W2) @ xi[:3]


def left(xi, R, t):
    """exp(xi^) (R, t)"""
    dR, dt = se3_exp(xi)
    return dR @ R, dR @ t + dt


def matrix(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def project(P, intrinsics, R, t):
    """(M, 2) pixel coordinates of the points under (R, t)"""
    fx, fy, cx, cy = intrinsics
    X = np.asarray(P, dtype=np.float64) @ np.asarray(R).T + np.asarray(t)
    return np.stack((fx * X[:, 0] / X[:, 2] + cx, fy * X[:, 1] / X[:, 2] + cy), axis=1)


def reprojection_error(P, intrinsics, pose_a, pose_b):
    """the distances in pixels between the projections of the points under two (R, t)"""
    return np.sqrt(((project(P, intrinsics, *pose_a) - project(P, intrinsics, *pose_b)) ** 2).sum(axis=1))


# ---- the loop --------------------------------------------------------------------------------------------------------------------

def solve(A, g, lam):
    """(A + lam diag A) d = -g by Cholesky -> d, or None when the matrix is not positive definite"""
    M = A + lam * np.diag(np.diag(A))
    try:
        L = np.linalg.cholesky(M)
    except np.linalg.LinAlgError:
        return None
    d = np.linalg.solve(L.T, np.linalg.solve(L, -g))
    return d if np.all(np.isfinite(d)) else None


def register(P, S, intrinsics, R, t, loss="huber", delta=64.0, max_evals=50, min_points=12, step_tol=1e-10, evaluate=terms):
    """-> (R, t, c, n, evaluations, status)"""
    R, t = np.array(R, dtype=np.float64), np.array(t, dtype=np.float64)
    A, g, c, n = evaluate(P, S, intrinsics, R, t, loss, delta)
    evals = 1
    if n < min_points:
        return R, t, c, n, evals, "lost"
    lam, status = LAMBDA0, "max_evals"
    while evals < max_evals:
        if lam > LAMBDA_MAX:
            status = "stalled"
            break
        d = solve(A, g, lam)
        if d is None:
            lam = 10.0 * lam
            continue
        Rc, tc = left(d, R, t)
        Ac, gc, cc, nc = evaluate(P, S, intrinsics, Rc, tc, loss, delta)
        evals += 1
        if nc >= min_points and cc / nc < c / n:
            R, t, A, g, c, n = Rc, tc, Ac, gc, cc, nc
            lam = max(lam / 10.0, LAMBDA_MIN)
            if math.sqrt(float((d * d).sum())) < step_tol:
                status = "converged"
                break
        else:
            lam = 10.0 * lam
    return R, t, c, n, evals, status


# ---- the seeded scene ------------------------------------------------------------------------------------------------------------

SCENE_SIZE = (60, 80)
SCENE_INTRINSICS = (70.0, 70.0, 39.5, 29.5)
SCENE_SIGMA = 3.0
SCENE_SEED = 7
SCENE_STARTS = 6
SCENE_END_ERROR = 0.1701                                    # px: the largest end of the six starts, measured (tests/test_cpu_track.py)


def basin(uv, size=SCENE_SIZE, sigma=SCENE_SIGMA):
    """(H, W) float32: 255 (1 - exp(-d^2 / (2 sigma^2))), d the distance of the pixel to the nearest of the projections uv"""
    H, W = size
    yy, xx = np.mgrid[0:H, 0:W]
    d2 = ((xx[..., None] - uv[:, 0]) ** 2 + (yy[..., None] - uv[:, 1]) ** 2).min(axis=-1)
    return (255.0 * (1.0 - np.exp(-d2 / (2.0 * sigma * sigma)))).astype(np.float32)


def scene_points(rng):
    """about 400 points: the edges of a slanted plane's texture (lines on it) and a nearer box in front"""
    pts = []
    for k in range(6):                                      # six lines across the plane Z = 3 + 0.4 X
        x = rng.uniform(-1.4, 1.4, 40)
        y = np.full(40, -0.9 + 0.36 * k) + 0.05 * np.sin(3.0 * x + k)
        pts.append(np.stack((x, y, 3.0 + 0.4 * x), axis=1))
    for k in range(4):                                      # the outline of a box at Z = 1.6
        s = rng.uniform(-0.3, 0.3, 40)
        e = np.full(40, 0.3)
        x, y = ((s, -e), (s, e), (-e, s), (e, s))[k]
        pts.append(np.stack((x + 0.1, y - 0.05, np.full(40, 1.6)), axis=1))
    return np.concatenate(pts)


def scene_pose(k=1):
    """the true current-from-reference pose of slice k: k steps of a small motion"""
    return se3_exp(k * np.array([0.020, -0.012, 0.015, 0.004, -0.006, 0.008]))


def scene(seed=SCENE_SEED):
    """points, the surface whose basin lies under their true projections, the true pose, and SCENE_STARTS starts whose mean
    reprojection error against the truth is uniform in 1 .. 2.5 px"""
    rng = np.random.default_rng(seed)
    P = scene_points(rng)
    R, t = scene_pose()
    S = basin(project(P, SCENE_INTRINSICS, R, t))
    starts = []
    for _ in range(SCENE_STARTS):
        xi = rng.normal(size=6) * np.array([0.02, 0.02, 0.02, 0.01, 0.01, 0.01])
        target = rng.uniform(1.0, 2.5)
        for _ in range(4):                                  # the error is close to linear in the size of xi
            xi = xi * (target / reprojection_error(P, SCENE_INTRINSICS, left(xi, R, t), (R, t)).mean())
        starts.append(left(xi, R, t))
    return {"points": P, "surface": S, "pose": (R, t), "starts": starts}
