"""The definition of the intensity reconstruction (include/evk.h, "Intensity reconstruction") as literal
loops in float64: per pixel one merged walk over the pixel's events, the frame times and the queries.  seq_reconstruct is what
tests/test_cpu_reconstruct.py pins on hand-worked cases and what tests/test_gpu_reconstruct.py compares the device with, together
with the per-element bound A that scales the tolerance.  Nothing here is vectorised: the test shapes are small."""
import math

import numpy as np

TOL_REASSOC = 2.0 ** -36                               # the factor of A in the tolerance (derivation: test_gpu_reconstruct.py)


def seq_reconstruct(xs, ys, ts, ps, alpha, sensor_size, t_refs=None, indices=None, c_on=0.1, c_off=0.1, initial=None, t_start=None,
                    frames=None, frame_ts=None):
    """-> (want float32 (K, H, W), A float64 (K, H, W)).  The arguments are those of leaky_integrator / complementary_filter; the
    times are the values the device holds (no offset).  A = |initial| + max_f |frames[f]| + the sum of |c_j| exp(-alpha (T_k -
    t_j)) over the counted events."""
    H, W = sensor_size
    xs, ys, ps = np.asarray(xs), np.asarray(ys), np.asarray(ps)
    ts = np.asarray(ts).astype(np.float64)
    n = len(ts)
    assert (np.diff(ts) >= 0).all() and (t_refs is None) != (indices is None)
    alpha, c_on, c_off = float(alpha), float(c_on), float(c_off)
    nf = 0 if frames is None else len(frame_ts)
    if nf:
        frames = np.asarray(frames).astype(np.float64)
        frame_ts = [float(v) for v in np.asarray(frame_ts).astype(np.float64)]
        assert frames.shape == (nf, H, W) and all(b > a for a, b in zip(frame_ts, frame_ts[1:]))
    if t_start is None:
        t_start = frame_ts[0] if nf else (float(ts[0]) if n else (float(np.asarray(t_refs).reshape(-1)[0]) if t_refs is not None else 0.0))
    t_start = float(t_start)
    if initial is None:
        initial = frames[0] if nf else np.zeros((H, W))
    initial = np.asarray(initial).astype(np.float64)
    if t_refs is not None:
        T = [float(v) for v in np.asarray(t_refs).astype(np.float64).reshape(-1)]
        cuts = [int(np.searchsorted(ts, v, side="left")) for v in T]          # the events with ts < T_k
    else:
        cuts = [int(m) for m in np.asarray(indices).reshape(-1)]
        T = [float(ts[m - 1]) if m > 0 else t_start for m in cuts]
    assert len(T) >= 1 and all(b >= a for a, b in zip(T, T[1:])) and T[0] >= t_start
    assert all(b >= a for a, b in zip(cuts, cuts[1:])) and 0 <= cuts[0] and cuts[-1] <= n
    pixel_events = [[] for _ in range(H * W)]
    for j in range(n):
        assert 0 <= xs[j] < W and 0 <= ys[j] < H
        pixel_events[int(ys[j]) * W + int(xs[j])].append(j)
    want = np.empty((len(T), H, W), dtype=np.float32)
    bound = np.empty((len(T), H, W), dtype=np.float64)
    for key in range(H * W):
        y, x = divmod(key, W)
        L, now = float(initial[y, x]), t_start
        fmax = max(abs(float(frames[f, y, x])) for f in range(nf)) if nf else 0.0
        counted = []                                   # (t_j, |c_j|) of the events counted so far

        def advance(to):
            """L from `now` to `to` under the frame target, split at every frame time inside (now, to)"""
            nonlocal L, now
            while to > now:
                g = 0
                while g < nf and frame_ts[g] <= now:   # the first frame time after `now`
                    g += 1
                target = float(frames[max(g - 1, 0), y, x]) if nf else 0.0
                b = frame_ts[g] if g < nf and frame_ts[g] < to else to
                if alpha != 0.0:                       # (alpha == 0: an advance leaves L as it is)
                    L = target + (L - target) * math.exp(-alpha * (b - now))
                now = b
                if b == to:
                    return

        run, r = pixel_events[key], 0
        for k in range(len(T)):
            while r < len(run) and run[r] < cuts[k]:
                j = run[r]
                r += 1
                if ts[j] < t_start:
                    continue
                advance(float(ts[j]))
                c = c_on if ps[j] > 0 else -c_off
                L += c
                counted.append((float(ts[j]), abs(c)))
            advance(T[k])
            want[k, y, x] = L
            bound[k, y, x] = abs(float(initial[y, x])) + fmax + sum(c * math.exp(-alpha * (T[k] - tj)) for tj, c in counted)
    return want, bound


def tolerance(want, bound, factor=TOL_REASSOC):
    """|got - want| <= spacing(float32(want)) + factor * A + 2^-126, per element"""
    return np.spacing(np.abs(want.astype(np.float32))).astype(np.float64) + factor * bound + 2.0 ** -126
