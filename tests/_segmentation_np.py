"""float64 numpy restatement of motion segmentation by motion compensation (include/evk.h, "Motion segmentation", steps 1-6;
DESIGN.md section 6): the L cluster images of warped events weighted by the associations P (L, N), the loss -sum_l Var(B_l) with
its adjoint gradient, the assignment step and the alternating loop of segment_events.  Warps, Jacobians and the mask are those
of tests/_zhu_np.py; the blur is scipy.ndimage.gaussian_filter (mode 'reflect') in float64.

f32_coords: as in tests/_zhu_np.py -- True casts the warped coordinates to float32 before floor / fraction, as the kernels do
(what the GPU tests compare with); False keeps float64 throughout (what the finite-difference tests differentiate).
f32_images (loss_and_grad): as in tests/_flow_contrast_np.py -- the cluster images, their blurs and the adjoint images stored as
float32, optionally moved by a unit in the last place: the rounding of a float32 post pass, measured on the CPU."""
from collections import namedtuple

import numpy as np
import scipy.optimize as opt
from scipy.ndimage import gaussian_filter

import _motion_models8_np as M8
import _zhu_np as Z
from _flow_contrast_np import _stored


def blur(a, sigma):
    return gaussian_filter(a, sigma) if sigma > 0 else a


def _cluster_events(model, params, x, y, t, p, img_size, center, camera_matrix, f32_coords):
    """Per cluster: (index into the events, px, py, dx, dy, jx, jy) of the events that count under theta_l (steps 1)."""
    out = []
    for q in np.asarray(params, dtype=np.float64):
        (px, py, dx, dy, _, _, jx, jy), keep = Z._events(model, q, x, y, t, p, img_size, img_size, center, camera_matrix, f32_coords)
        out.append((np.flatnonzero(keep), px, py, dx, dy, jx, jy))
    return out


def weights(probs, p, use_polarity):
    """q (L, N) of step 2: P, times the sign of the polarity with use_polarity; P == 0 or NaN adds nothing."""
    q = np.nan_to_num(np.asarray(probs, dtype=np.float64), nan=0.0)
    if use_polarity:
        q = q * np.where(np.asarray(p, dtype=np.float64) > 0, 1.0, -1.0)[None, :]
    return q


def _splat(shape, ce, q):
    idx, px, py, dx, dy = ce[:5]
    cw, size = shape[1], shape[0] * shape[1]
    cell, w = py * cw + px, q[idx]
    ax, ay = 1.0 - dx, 1.0 - dy
    out = np.zeros(size)
    for off, wt in ((0, ax * ay), (1, dx * ay), (cw, ax * dy), (cw + 1, dx * dy)):
        out += np.bincount(cell + off, weights=w * wt, minlength=size)
    return out.reshape(shape)


def _shape(img_size):
    return int(img_size[0]) + 1, int(img_size[1]) + 1


def iwes(model, params, probs, x, y, t, p, img_size=(180, 240), use_polarity=False, center=(0.0, 0.0),
         camera_matrix=M8.K_DEFAULT, f32_coords=False):
    """(L, H+1, W+1) float64 (steps 1-3)."""
    params = np.asarray(params, dtype=np.float64)
    shape = _shape(img_size)
    if len(t) == 0:
        return np.zeros((len(params),) + shape)
    q = weights(probs, p, use_polarity)
    ces = _cluster_events(model, params, x, y, t, p, img_size, center, camera_matrix, f32_coords)
    return np.stack([_splat(shape, ce, q[l]) for l, ce in enumerate(ces)])


def loss_of_iwes(imgs, sigma):
    """Step 4: -sum_l Var(B_l), the clusters summed in order."""
    total = 0.0
    for img in imgs:
        total += -np.var(blur(img, sigma))
    return total


def loss(model, params, probs, x, y, t, p, sigma=1.0, **kw):
    return loss_of_iwes(iwes(model, params, probs, x, y, t, p, **kw), sigma)


def _bilinear(img, px, py, dx, dy):
    return img[py, px] * ((1.0 - dx) * (1.0 - dy)) + img[py, px + 1] * (dx * (1.0 - dy)) + \
        img[py + 1, px] * ((1.0 - dx) * dy) + img[py + 1, px + 1] * (dx * dy)


def loss_and_grad(model, params, probs, x, y, t, p, sigma=1.0, img_size=(180, 240), use_polarity=False, center=(0.0, 0.0),
                  camera_matrix=M8.K_DEFAULT, f32_coords=False, f32_images=False):
    """(loss, dloss/dparams (L, dims)) by the adjoint (steps 4-5)."""
    params = np.asarray(params, dtype=np.float64)
    shape = _shape(img_size)
    g = np.zeros((len(params), Z.DIMS[model]))
    if len(t) == 0:
        return 0.0, g
    q = weights(probs, p, use_polarity)
    ces = _cluster_events(model, params, x, y, t, p, img_size, center, camera_matrix, f32_coords)
    total = 0.0
    for l, ce in enumerate(ces):
        idx, px, py, dx, dy, jx, jy = ce
        b = np.asarray(blur(_stored(_splat(shape, ce, q[l]), f32_images), sigma), dtype=np.float64)
        total += -np.var(b)
        G = -2.0 / b.size * (np.asarray(blur(_stored(b, f32_images), sigma), dtype=np.float64) - b.mean())
        G = np.asarray(_stored(G, f32_images), dtype=np.float64)
        a_, b_, c_, d_ = G[py, px], G[py, px + 1], G[py + 1, px], G[py + 1, px + 1]
        ex = q[l][idx] * ((b_ - a_) * (1.0 - dy) + (d_ - c_) * dy)
        ey = q[l][idx] * ((c_ - a_) * (1.0 - dx) + (d_ - b_) * dx)
        g[l] = jx @ ex + jy @ ey
    return total, g


def assign(model, params, probs, x, y, t, p, sigma=1.0, img_size=(180, 240), use_polarity=False, center=(0.0, 0.0),
           camera_matrix=M8.K_DEFAULT, f32_coords=False, blurred=None):
    """Step 6 -> (P' (L, N) float32, labels (N,), S (N,), c (L, N), B (L, H+1, W+1)).  blurred: the B_l to gather from (default:
    those of `probs`)."""
    params = np.asarray(params, dtype=np.float64)
    probs = np.asarray(probs)
    L, n = len(params), len(t)
    shape = _shape(img_size)
    c = np.zeros((L, n))
    if n == 0:
        return np.zeros((L, 0), dtype=np.float32), np.zeros(0, dtype=np.int64), np.zeros(0), c, np.zeros((L,) + shape)
    q = weights(probs, p, use_polarity)
    ces = _cluster_events(model, params, x, y, t, p, img_size, center, camera_matrix, f32_coords)
    if blurred is None:
        blurred = np.stack([blur(_splat(shape, ce, q[l]), sigma) for l, ce in enumerate(ces)])
    sgn = np.where(np.asarray(p, dtype=np.float64) > 0, 1.0, -1.0) if use_polarity else np.ones(n)
    for l, (idx, px, py, dx, dy, _, _) in enumerate(ces):
        c[l, idx] = np.maximum(0.0, sgn[idx] * _bilinear(blurred[l], px, py, dx, dy))
    S = np.zeros(n)
    for l in range(L):
        S += c[l]
    new = np.asarray(probs, dtype=np.float32).copy()
    on = S > 0
    new[:, on] = (c[:, on] / S[on]).astype(np.float32)
    return new, np.argmax(new, axis=0), S, c, blurred


Result = namedtuple("Result", ["params", "probs", "labels", "loss", "history"])


def segment(model, x, y, t, p, x0, img_size, n_outer=6, inner_maxiter=10, sigma=1.0, use_polarity=False, probs0=None, **kw):
    """segment_events restated: BFGS on the stacked parameters with P fixed, then one assignment step; history holds the loss
    after every outer iteration (new motions, new associations)."""
    x0 = np.asarray(x0, dtype=np.float64)
    L, n = x0.shape[0], len(t)
    probs = np.full((L, n), 1.0 / L, dtype=np.float32) if probs0 is None else np.asarray(probs0, dtype=np.float32)
    params, labels, history = x0.copy(), None, []
    kw = dict(kw, img_size=img_size, use_polarity=use_polarity)

    def fun(v):
        f, g = loss_and_grad(model, v.reshape(x0.shape), probs, x, y, t, p, sigma, **kw)
        return f, g.reshape(-1)
    for _ in range(n_outer):
        res = opt.minimize(fun, params.reshape(-1), jac=True, method="BFGS", options={"maxiter": int(inner_maxiter)})
        params = res.x.reshape(x0.shape)
        probs, labels = assign(model, params, probs, x, y, t, p, sigma, **kw)[:2]
        history.append(loss(model, params, probs, x, y, t, p, sigma, **kw))
    return Result(params, probs, labels, history[-1], history)


# ---- synthetic scenes ---------------------------------------------------------------------------------------------------
FLOWS2 = np.array([[40.0, 0.0], [-25.0, 30.0]])
FLOWS3 = np.array([[40.0, 0.0], [-25.0, 30.0], [0.0, -45.0]])
CANVAS = (48, 64)


def scene(flows, sources, per, T=0.5, canvas=CANVAS, seed=0, noise=0.15, push_every=0):
    """len(flows) clusters of `sources` point sources; every source emits `per` events at sorted uniform times in [0, T] along
    source + flow (t - T) plus N(0, noise) px, with one polarity per source; merged by time.  push_every > 0 moves every
    push_every-th event off the canvas.  -> x, y, t, p, cluster of every event (float64 / int)."""
    rng = np.random.default_rng(seed)
    H, W = canvas
    xs, ys, ts, ps, ks = [], [], [], [], []
    for k, (vx, vy) in enumerate(np.asarray(flows, dtype=np.float64)):
        for s in range(sources):
            sx, sy = rng.uniform(4.0, W - 4.0), rng.uniform(4.0, H - 4.0)
            t = np.sort(rng.uniform(0.0, T, per))
            xs.append(sx + vx * (t - T) + rng.normal(0.0, noise, per))
            ys.append(sy + vy * (t - T) + rng.normal(0.0, noise, per))
            ts.append(t)
            ps.append(np.full(per, 1.0 if s % 2 == 0 else -1.0))
            ks.append(np.full(per, k))
    x, y, t, p, k = (np.concatenate(a) for a in (xs, ys, ts, ps, ks))
    order = np.argsort(t, kind="stable")
    x, y, t, p, k = x[order], y[order], t[order], p[order], k[order]
    if push_every:
        x = x.copy()
        x[::push_every] += 3.0 * W
    return x, y, t, p, k.astype(np.int64)


def start(flows, seed):
    """truth + U(-8, 8) per component."""
    return np.asarray(flows, dtype=np.float64) + np.random.default_rng(1000 + seed).uniform(-8.0, 8.0, np.shape(flows))
