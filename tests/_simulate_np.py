"""The definition of the event simulator (include/evk.h, "Event simulation") as literal Python float loops:
per pixel one walk over the frame intervals, one threshold crossing at a time.  Python floats are IEEE float64 and every operation
below is one rounding, which is what the definition fixes.  seq_simulate is what tests/test_cpu_simulate.py pins on hand-worked
cases and what tests/test_gpu_simulate.py compares the device with, bit for bit.  Nothing here is vectorised: the test shapes are
small."""
import math

import numpy as np

MAX_STEPS = 65536                                      # EVK_SIMULATE_MAX_STEPS


def _map(c, H, W, what):
    c = np.asarray(c, dtype=np.float64)
    c = np.full((H, W), float(c)) if c.ndim == 0 else c
    assert c.shape == (H, W) and np.isfinite(c).all() and (c > 0).all(), what
    return c


def seq_simulate(frames, frame_ts, c_on=0.2, c_off=0.2, refractory=0.0, reference=None, last_event_ts=None):
    """-> (xs, ys, ts, ps, R, tl, overflow): the events in the defined order (int64, int64, float64, int64 +1 / -1), the state after
    the last interval as (H, W) float64 arrays, and the number of pixel-intervals in which the step limit ended the loop while a
    further crossing was still due.  c_on, c_off: scalars or (H, W) maps."""
    frames = np.asarray(frames).astype(np.float64)
    F, H, W = frames.shape
    T = [float(v) for v in np.asarray(frame_ts).astype(np.float64).reshape(-1)]
    assert F >= 2 and len(T) == F and all(math.isfinite(v) for v in T) and all(b > a for a, b in zip(T, T[1:]))
    con, coff = _map(c_on, H, W, "c_on"), _map(c_off, H, W, "c_off")
    refractory = float(refractory)
    assert refractory >= 0.0
    R_out = (frames[0] if reference is None else np.asarray(reference).astype(np.float64)).copy()
    tl_out = (np.full((H, W), -np.inf) if last_event_ts is None else np.asarray(last_event_ts).astype(np.float64)).copy()
    assert R_out.shape == (H, W) and tl_out.shape == (H, W)
    events = []                                        # (t, pixel, emission number in the pixel, p)
    overflow = 0
    for q in range(H * W):
        y, x = divmod(q, W)
        R, tl = float(R_out[y, x]), float(tl_out[y, x])
        cp, cm = float(con[y, x]), float(coff[y, x])
        k = 0
        for f in range(F - 1):
            L0, L1, T0, T1 = float(frames[f, y, x]), float(frames[f + 1, y, x]), T[f], T[f + 1]
            d = L1 - L0
            dT = T1 - T0
            if not math.isfinite(d) or d == 0.0:
                continue
            steps = 0
            while steps < MAX_STEPS:
                if d > 0.0 and R + cp <= L1:
                    R = R + cp
                    p = 1
                elif d < 0.0 and R - cm >= L1:
                    R = R - cm
                    p = -1
                else:
                    break
                steps += 1
                frac = (R - L0) / d
                if frac < 0.0:
                    frac = 0.0
                elif frac > 1.0:
                    frac = 1.0
                t = T0 + frac * dT
                if t - tl >= refractory:
                    events.append((t, q, k, p))
                    k += 1
                tl = t
            else:
                if (d > 0.0 and R + cp <= L1) or (d < 0.0 and R - cm >= L1):
                    overflow += 1
        R_out[y, x], tl_out[y, x] = R, tl
    events.sort(key=lambda e: e[:3])                   # ascending t; equal t by pixel index; then in emission order
    xs = np.array([e[1] % W for e in events], dtype=np.int64)
    ys = np.array([e[1] // W for e in events], dtype=np.int64)
    ts = np.array([e[0] for e in events], dtype=np.float64)
    ps = np.array([e[3] for e in events], dtype=np.int64)
    return xs, ys, ts, ps, R_out, tl_out, overflow


# ---- the scenes the CPU and GPU tests share (seeded: the same arrays in every process) ------------------------------------------

def scene(F, H, W, seed, edge=3.0, texture=0.6, noise=0.05, t0=1.0e6, dt=1000.0):
    """-> (frames float64 (F, H, W) in the log domain, frame_ts float64 (F,)): a sigmoid edge that sweeps the width once over a
    texture scrolling the other way, plus per-frame noise; frame times near t0, about dt apart, jittered."""
    rng = np.random.default_rng(seed)
    x = np.arange(W, dtype=np.float64)[None, :]
    y = np.arange(H, dtype=np.float64)[:, None]
    phase = rng.uniform(0.0, 2.0 * np.pi, size=3)
    frames = np.empty((F, H, W))
    for f in range(F):
        pos = -2.0 + (W + 4.0) * f / (F - 1)
        sig = edge / (1.0 + np.exp(-(x - pos + 0.15 * (y - H / 2)) / 1.5))
        tex = texture * (np.sin(0.55 * (x + 1.7 * f) + phase[0]) * np.cos(0.35 * y + phase[1]) + 0.5 * np.sin(0.9 * (y - 0.8 * f) + phase[2]))
        frames[f] = sig + tex + noise * rng.standard_normal((H, W))
    frame_ts = t0 + dt * np.arange(F) + rng.uniform(-0.2 * dt, 0.2 * dt, size=F)
    return frames, frame_ts


def scene_a():
    return scene(9, 48, 64, seed=1)


def scene_b():
    return scene(6, 12, 70, seed=2)


def tie_scene():
    """every value dyadic: crossing times collide exactly, across pixels and with the frame times"""
    rng = np.random.default_rng(3)
    return rng.integers(-8, 9, size=(5, 8, 70)).astype(np.float64) * 0.25, 4096.0 + 1024.0 * np.arange(5)
