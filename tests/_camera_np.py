"""The definition of camera calibration (include/evk.h, "Camera calibration") restated literally in numpy:
lens distortion and its inverse, the forward (event) and inverse (image) rectification maps, the event look-up, the image remap and
Bouguet's stereo rectification, every step float64 with one rounding per operation in the order evk.h states.  Nothing here is
shared with the product; the tests compare the device with it bit for bit (radtan, none) or within the stated bound (equidistant,
whose atan / tan are the platform's)."""
import numpy as np

MODELS = ("none", "radtan", "equidistant")
SMALL_R = 1e-8
HALF_PI = np.pi / 2
F = np.float64                                              # the arithmetic's type (precision() swaps it for a check of the reference)


class precision:
    """with precision(np.longdouble): the same restatement in another floating type"""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        global F
        self.old, F = F, self.dtype

    def __exit__(self, *exc):
        global F
        F = self.old


def coefficients(model, distortion):
    """the five doubles the kernels take: radtan (k1, k2, p1, p2, k3), equidistant (k1, k2, k3, k4, 0), none zeros"""
    d = np.zeros(5)
    src = [] if distortion is None else list(np.asarray(distortion, dtype=F).reshape(-1))
    assert len(src) in {"none": (0,), "radtan": (4, 5), "equidistant": (4,)}[model], (model, src)
    d[:len(src)] = src
    return d


def intrinsics(K):
    K = np.asarray(K, dtype=F)
    return F(K[0, 0]), F(K[1, 1]), F(K[0, 2]), F(K[1, 2])


# ---- the lens ----------------------------------------------------------------------------------------------------------------------

def _radtan_terms(a, b, d):
    k1, k2, p1, p2, k3 = d
    aa, bb, ab = a * a, b * b, a * b
    r2 = aa + bb
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    dx = (2.0 * p1) * ab + p2 * (r2 + 2.0 * aa)
    dy = p1 * (r2 + 2.0 * bb) + (2.0 * p2) * ab
    return rad, dx, dy


def _theta_d(th, d):
    th2 = th * th
    return th * (1.0 + th2 * (d[0] + th2 * (d[1] + th2 * (d[2] + th2 * d[3]))))


def distort(a, b, model, d):
    """normalised (a, b) -> distorted normalised (a', b')"""
    a, b = np.asarray(a, dtype=F), np.asarray(b, dtype=F)
    with np.errstate(all="ignore"):
        if model == "none":
            return a.copy(), b.copy()
        if model == "radtan":
            rad, dx, dy = _radtan_terms(a, b, d)
            return a * rad + dx, b * rad + dy
        r = np.sqrt(a * a + b * b)
        thd = _theta_d(np.arctan(r), d)
        s = np.where(r < SMALL_R, 1.0, thd / r)
        return a * s, b * s


def undistort(ad, bd, model, d, fx, fy, iterations=20, tolerance=1e-6):
    """distorted normalised (a', b') -> (a, b, valid); NaN where not valid"""
    ad, bd = np.asarray(ad, dtype=F), np.asarray(bd, dtype=F)
    with np.errstate(all="ignore"):
        ok = np.ones(ad.shape, dtype=bool)
        if model == "none":
            a, b = ad.copy(), bd.copy()
        elif model == "radtan":
            a, b = ad.copy(), bd.copy()
            for _ in range(iterations):
                rad, dx, dy = _radtan_terms(a, b, d)
                icd = 1.0 / rad
                a, b = (ad - dx) * icd, (bd - dy) * icd
        else:
            rd = np.sqrt(ad * ad + bd * bd)
            th = rd.copy()
            c3, c5, c7, c9 = 3.0 * d[0], 5.0 * d[1], 7.0 * d[2], 9.0 * d[3]
            for _ in range(iterations):
                th2 = th * th
                f = _theta_d(th, d) - rd
                fp = 1.0 + th2 * (c3 + th2 * (c5 + th2 * (c7 + th2 * c9)))
                th = th - f / fp
            ok &= (th >= 0.0) & (th < HALF_PI)
            s = np.where(rd < SMALL_R, 1.0, np.tan(th) / rd)
            a, b = ad * s, bd * s
        ok &= np.isfinite(a) & np.isfinite(b)
        ar, br = distort(a, b, model, d)
        ok &= (np.abs(fx * (ar - ad)) <= tolerance) & (np.abs(fy * (br - bd)) <= tolerance)
        return np.where(ok, a, np.nan), np.where(ok, b, np.nan), ok


# a strong barrel lens: r' = r (1 - 0.45 r^2) has its maximum 0.574 at r = 0.861, and the corners of this sensor lie at r' = 0.89 --
# no undistorted point maps there, the fixed point cannot converge, and the corners must come out invalid
DIVERGENT = {"K": np.array([[60.0, 0.0, 47.5], [0.0, 60.0, 23.5], [0.0, 0.0, 1.0]]), "model": "radtan", "distortion": (-0.45, 0.0, 0.0, 0.0),
             "sensor_size": (48, 96)}


# ---- points and maps -----------------------------------------------------------------------------------------------------------------

def _rotate(M, a, b):
    """M (a, b, 1): each row ((m0 a + m1 b) + m2)"""
    M = np.asarray(M, dtype=F)
    return tuple((M[i, 0] * a + M[i, 1] * b) + M[i, 2] for i in range(3))


def forward_points(x, y, K, model, d, R=None, new_K=None, iterations=20, tolerance=1e-6):
    """raw pixels -> rectified coordinates (u, v, valid): undistort, rotate by R, project with new_K"""
    fx, fy, cx, cy = intrinsics(K)
    gx, gy, ox, oy = intrinsics(K if new_K is None else new_K)
    x, y = np.asarray(x, dtype=F), np.asarray(y, dtype=F)
    with np.errstate(all="ignore"):
        a, b, ok = undistort((x - cx) / fx, (y - cy) / fy, model, d, fx, fy, iterations, tolerance)
        X, Y, Z = _rotate(np.eye(3) if R is None else R, a, b)
        ok = ok & (Z > 0.0)
        u, v = gx * (X / Z) + ox, gy * (Y / Z) + oy
        return np.where(ok, u, np.nan), np.where(ok, v, np.nan), ok


def inverse_points(u, v, K, model, d, R=None, new_K=None):
    """rectified pixels -> raw coordinates (x, y, valid): back through new_K, rotate by R^T, distort, project with K"""
    fx, fy, cx, cy = intrinsics(K)
    gx, gy, ox, oy = intrinsics(K if new_K is None else new_K)
    u, v = np.asarray(u, dtype=F), np.asarray(v, dtype=F)
    with np.errstate(all="ignore"):
        X, Y, Z = _rotate(np.eye(3) if R is None else np.asarray(R, dtype=F).T, (u - ox) / gx, (v - oy) / gy)
        ok = Z > 0.0
        a, b = distort(X / Z, Y / Z, model, d)
        x, y = fx * a + cx, fy * b + cy
        ok = ok & np.isfinite(x) & np.isfinite(y)
        return np.where(ok, x, np.nan), np.where(ok, y, np.nan), ok


def grid(size):
    h, w = size
    i = np.arange(h * w, dtype=np.int64)
    return (i % max(w, 1)).astype(F), (i // max(w, 1)).astype(F)


def maps(K, model, d, sensor_size, R=None, new_K=None, out_size=None, iterations=20, tolerance=1e-6):
    """-> forward (2, H, W), forward_valid (H, W), inverse (2, H', W'), inverse_valid (H', W')"""
    out_size = tuple(sensor_size) if out_size is None else tuple(out_size)
    u, v, fv = forward_points(*grid(sensor_size), K, model, d, R, new_K, iterations, tolerance)
    x, y, iv = inverse_points(*grid(out_size), K, model, d, R, new_K)
    return (np.stack((u, v)).reshape((2,) + tuple(sensor_size)), fv.reshape(sensor_size),
            np.stack((x, y)).reshape((2,) + out_size), iv.reshape(out_size))


# ---- events through the forward map ----------------------------------------------------------------------------------------------------

def rectify_events(xs, ys, ts, ps, forward, forward_valid, out_size, mode="nearest"):
    """-> (xs', ys', ts', ps', kept indices).  A coordinate that is no integer or off the raw sensor raises ValueError.  nearest: the
    coordinates keep the dtype of xs; subpixel: float64."""
    xs, ys = np.asarray(xs), np.asarray(ys)
    _, H, W = forward.shape
    Ho, Wo = out_size
    xd, yd = xs.astype(F), ys.astype(F)
    on = (xd == np.trunc(xd)) & (yd == np.trunc(yd)) & (xd >= 0) & (xd < W) & (yd >= 0) & (yd < H)
    if not on.all():
        raise ValueError("event coordinates must be integers on the raw sensor")
    xi, yi = xd.astype(np.int64), yd.astype(np.int64)
    u, v, ok = forward[0, yi, xi], forward[1, yi, xi], forward_valid[yi, xi].astype(bool)
    with np.errstate(all="ignore"):
        if mode == "nearest":
            u, v = np.rint(u) + 0.0, np.rint(v) + 0.0           # (+ 0.0: a rounded -0.3 is the pixel 0, not -0)
            keep = ok & (u >= 0) & (u < Wo) & (v >= 0) & (v < Ho)
        else:
            keep = ok & (u >= 0) & (u <= Wo - 1) & (v >= 0) & (v <= Ho - 1)
    idx = np.nonzero(keep)[0]
    dt = xs.dtype if mode == "nearest" else F
    return (u[idx].astype(dt), v[idx].astype(dt), None if ts is None else np.asarray(ts)[idx], None if ps is None else np.asarray(ps)[idx],
            idx.astype(np.int64))


# ---- images through the inverse map --------------------------------------------------------------------------------------------------

def _to_dtype(v, dtype):
    """one rounding of float64 values to the plane's dtype (uint8: half to even, then clamped to 0 .. 255)"""
    dtype = np.dtype(dtype)
    with np.errstate(all="ignore"):
        if dtype == np.uint8:
            r = np.rint(v)
            return np.where(r > 0.0, np.minimum(r, 255.0), 0.0).astype(np.uint8)
        return np.asarray(v).astype(dtype)


def remap(planes, inverse, inverse_valid, interpolation="nearest", fill=0):
    """(P, H, W) planes -> (P, H', W').  bilinear: out = b1 (a1 v00 + a v01) + b (a1 v10 + a v11) in float64, taps off the sensor = fill"""
    planes = np.asarray(planes)
    P, H, W = planes.shape
    mx, my = inverse[0], inverse[1]
    fill_t = _to_dtype(np.asarray(fill, dtype=F), planes.dtype)
    out = np.empty((P,) + mx.shape, dtype=planes.dtype)
    with np.errstate(all="ignore"):
        sx, sy = np.rint(mx), np.rint(my)
        ok = inverse_valid.astype(bool) & (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
        if interpolation == "nearest":
            sxi, syi = np.where(ok, sx, 0).astype(np.int64), np.where(ok, sy, 0).astype(np.int64)
            for p in range(P):
                out[p] = np.where(ok, planes[p, syi, sxi], fill_t)
            return out
        x0, y0 = np.floor(mx), np.floor(my)
        a, b = mx - x0, my - y0
        a1, b1 = 1.0 - a, 1.0 - b
        x0i, y0i = np.where(ok, x0, 0).astype(np.int64), np.where(ok, y0, 0).astype(np.int64)

        def tap(p, yy, xx):
            on = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            return np.where(on, planes[p, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(F), F(fill_t))
        for p in range(P):
            v = b1 * (a1 * tap(p, y0i, x0i) + a * tap(p, y0i, x0i + 1)) + b * (a1 * tap(p, y0i + 1, x0i) + a * tap(p, y0i + 1, x0i + 1))
            out[p] = np.where(ok, _to_dtype(v, planes.dtype), fill_t)
    return out


# ---- stereo rectification (Bouguet) ----------------------------------------------------------------------------------------------------

def rodrigues(om):
    om = np.asarray(om, dtype=F)
    th = np.sqrt((om * om).sum())
    if th < 1e-12:
        return np.eye(3)
    k = om / th
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)


def rotation_vector(R):
    R = np.asarray(R, dtype=F)
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * np.sqrt((w * w).sum()), 0.5 * (np.trace(R) - 1.0)
    th = np.arctan2(s, c)
    return np.zeros(3) if s < 1e-12 else w * (th / (2.0 * s))


def stereo_rectify(K_left, K_right, sensor_size, R, T, out_size=None):
    """X_right = R X_left + T.  -> (R_left, R_right, new_K, baseline): half of R to each camera, the baseline onto -x, one new_K"""
    r_r = rodrigues(-0.5 * rotation_vector(R))
    t = r_r @ np.asarray(T, dtype=F).reshape(3)
    b = np.sqrt((t * t).sum())
    e = np.array([-1.0, 0.0, 0.0])
    w = np.cross(t / b, e)
    s = np.sqrt((w * w).sum())
    wR = np.eye(3) if s < 1e-12 else rodrigues(w * (np.arctan2(s, (t / b) @ e) / s))
    KL, KR = np.asarray(K_left, dtype=F), np.asarray(K_right, dtype=F)
    H, W = sensor_size
    Ho, Wo = (H, W) if out_size is None else out_size
    f = (KL[0, 0] + KL[1, 1] + KR[0, 0] + KR[1, 1]) / 4.0
    new_K = np.array([[f, 0.0, (KL[0, 2] + KR[0, 2]) / 2.0 + (Wo - W) / 2.0], [0.0, f, (KL[1, 2] + KR[1, 2]) / 2.0 + (Ho - H) / 2.0],
                      [0.0, 0.0, 1.0]])
    return wR @ r_r.T, wR @ r_r, new_K, b


# ---- the seeded raw stereo scene -------------------------------------------------------------------------------------------------------

import _stereo_np as S                                      # noqa: E402  (sizes, tau and the matcher: imported, not restated)

SCENE_K = np.array([[130.0, 0.0, 47.5], [0.0, 130.0, 23.5], [0.0, 0.0, 1.0]])
SCENE_T = np.array([-0.1, 0.002, -0.001])
SCENE_OM = np.array([0.006, -0.016, 0.009])                 # the relative rotation: 1.1 degrees
SCENE_CALIBRATION = {                                       # (left, right) coefficients
    "radtan": ((-0.25, 0.08, 0.0012, -0.0008), (-0.23, 0.07, -0.001, 0.0011)),
    "equidistant": ((-0.06, 0.015, -0.006, 0.0015), (-0.045, 0.012, -0.0045, 0.0015)),
}


def scene_cameras(model):
    """the two cameras of a raw scene: (K, model, d, R_rect) each, and the shared new_K and baseline"""
    R_l, R_r, new_K, base = stereo_rectify(SCENE_K, SCENE_K, S.SCENE_SIZE, rodrigues(SCENE_OM), SCENE_T)
    if model == "none":
        return (SCENE_K, "none", coefficients("none", None), np.eye(3)), (SCENE_K, "none", coefficients("none", None), np.eye(3)), SCENE_K, base
    dl, dr = (coefficients(model, c) for c in SCENE_CALIBRATION[model])
    return (SCENE_K, model, dl, R_l), (SCENE_K, model, dr, R_r), new_K, base


def raw_scene(model, seed=3, dots=56):
    """The dots of _stereo_np.scene (the same draws in the same order) kept as sub-pixel rectified tracks on the planes d = 4 and
    d = 9; every track is carried into each camera's raw pixels through that camera's rotation and lens (inverse_points), and a dot
    fires an event when it enters a new raw pixel.  model 'none': no lens, no rotation -- the yardstick.  -> dict as scene()'s, with
    `pixels` the dots' last rectified left pixels."""
    rng = np.random.default_rng(seed)
    H, W = S.SCENE_SIZE
    d = np.asarray(S.SCENE_DISPARITIES)[rng.integers(0, 2, dots)]
    x0, y0 = rng.uniform(12, W - 4, dots), rng.uniform(3, H - 3, dots)
    speed, angle = rng.uniform(600.0, 1400.0, dots), rng.uniform(0, 2 * np.pi, dots)
    vx, vy = speed * np.cos(angle), speed * np.sin(angle)
    pol = rng.integers(0, 2, dots) * 2 - 1
    camL, camR, new_K, _ = scene_cameras(model)
    rows = {"left": [], "right": []}
    last = {"left": np.full((dots, 2), -1, dtype=np.int64), "right": np.full((dots, 2), -1, dtype=np.int64)}
    pixels = np.full((dots, 2), -1, dtype=np.int64)
    for t in np.linspace(0.0, S.SCENE_END, 801)[:-1]:
        u, v = x0 + vx * t, y0 + vy * t
        pixels = np.stack((np.rint(u), np.rint(v)), axis=1).astype(np.int64)
        for side, cam, uu in (("left", camL, u), ("right", camR, u - d)):
            K, m, dd, R = cam
            x, y, ok = inverse_points(uu, v, K, m, dd, R, new_K)
            px, py = np.rint(np.where(ok, x, -1.0)).astype(np.int64), np.rint(np.where(ok, y, -1.0)).astype(np.int64)
            for j in range(dots):
                if (px[j], py[j]) == tuple(last[side][j]):
                    continue
                last[side][j] = (px[j], py[j])
                if ok[j] and 0 <= px[j] < W and 0 <= py[j] < H and uu[j] >= 0:
                    rows[side].append((t + (rng.uniform(0.0, 1e-4) if side == "right" else 0.0), px[j], py[j], pol[j]))

    def columns(rs):
        rs = sorted(rs, key=lambda e: e[0])
        return {"ts": np.array([e[0] for e in rs], dtype=F), "xs": np.array([e[1] for e in rs], dtype=np.int64),
                "ys": np.array([e[2] for e in rs], dtype=np.int64), "ps": np.array([e[3] for e in rs], dtype=np.int64)}
    return {"left": columns(rows["left"]), "right": columns(rows["right"]), "pixels": pixels, "true_disparity": d,
            "cameras": (camL, camR), "new_K": new_K}


def scene_maps(sc, side):
    K, m, dd, R = sc["cameras"][0 if side == "left" else 1]
    return maps(K, m, dd, S.SCENE_SIZE, R, sc["new_K"])


def scene_surfaces(sc, how):
    """the quantised surfaces (QL, QR) of a raw scene: 'raw' as the events are, 'events' after rectify_events(nearest), 'images' after
    remap (nearest) of the raw surfaces"""
    out = []
    for side in ("left", "right"):
        xs, ys, ts, ps = S.stream(sc[side])
        if how == "events":
            fwd, fv, _, _ = scene_maps(sc, side)
            xs, ys, ts, ps, _ = rectify_events(xs, ys, ts, ps, fwd, fv, S.SCENE_SIZE)
        q = S.quantise(S.ages(xs, ys, ts, ps, S.SCENE_SIZE, [S.SCENE_END]), S.SCENE_TAU)
        if how == "images":
            _, _, inv, iv = scene_maps(sc, side)
            q = remap(q.reshape((-1,) + S.SCENE_SIZE), inv, iv).reshape(q.shape)
        out.append(q)
    return out


def scene_share(sc, QL, QR):
    """(candidate dots, the share of them whose winner lies within one disparity of the truth): no uniqueness or left-right test"""
    H, W = S.SCENE_SIZE
    px, d = sc["pixels"], sc["true_disparity"]
    disp, idx, cost, valid, cand = S.match(QL, QR, 0, S.SCENE_D, S.SCENE_R, S.SCENE_ACTIVITY, uniqueness=0, lr_tolerance=None)
    inside = (px[:, 0] >= 0) & (px[:, 0] < W) & (px[:, 1] >= 0) & (px[:, 1] < H)
    j = np.nonzero(inside)[0]
    j = j[cand[0, px[j, 1], px[j, 0]]]
    good = np.abs(idx[0, px[j, 1], px[j, 0]].astype(np.int64) - d[j]) <= 1
    return len(j), float(good.mean()) if len(j) else 0.0
