"""Timings of camera tracking (event_utils_amd.depth.tracking; evk_track.hip) on a 640x480 surface: one registration_terms call at
M = 2 000 points and at M = 300 000 (a dense mask), with one pose and with eight, and a whole register_points.  The points lie on a
slanted plane in front of the camera; the surface is the Gaussian-of-distance basin (sigma 3 px) under their projections at a pose
a few pixels from the start.  Per case: the public call, the bare library entry on resident buffers (what the loop inside the
library pays per evaluation, less its read-back), and two yardsticks: the same evaluation written in torch on the device in
float64 (what a user would write without the kernel; its sums are compared with the kernel's) and the numpy restatement of the
tests on the host.  Every timed repetition runs CALLS calls between two synchronisations; the median per call is reported.  No time
here is a pass / fail criterion.
usage: timeout 900 python tools/track_time.py [--quick] [--trace] [--out profiles/track_time.txt]
--trace runs only a few evaluations of each size and writes nothing: the command for a kernel trace."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZE = (480, 640)
INTRINSICS = (520.0, 520.0, 319.5, 239.5)
COUNTS = (2_000, 300_000)
SIGMA, DELTA, CALLS = 3.0, 64.0, 20


def camera():
    fx, fy, cx, cy = INTRINSICS
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def scene(m, seed=0):
    """points on the plane Z = 3 + 0.4 X whose projections cover the sensor, the basin under their projections at `truth`, and a
    start about two pixels away"""
    import _track_np as N
    from scipy.ndimage import distance_transform_edt
    rng = np.random.default_rng(seed)
    h, w = SIZE
    if m >= h * w // 2:                                     # dense: every pixel of a mask
        v, u = np.divmod(rng.permutation(h * w)[:m].astype(np.float64), w)
    else:                                                   # semi-dense: points along forty curves
        s = rng.uniform(0.0, 1.0, m)
        k = rng.integers(0, 40, m)
        u, v = 20.0 + 600.0 * s, 12.0 * k + 6.0 + 5.0 * np.sin(9.0 * s + k)
    fx, fy, cx, cy = INTRINSICS
    a, b = (u - cx) / fx, (v - cy) / fy
    Z = 3.0 / (1.0 - 0.4 * a)
    P = np.stack((a * Z, b * Z, Z), axis=1)
    truth = N.se3_exp([0.010, -0.006, 0.008, 0.002, -0.003, 0.003])
    uv = N.project(P, INTRINSICS, *truth)
    hit = np.ones(SIZE, dtype=bool)
    inside = (uv[:, 0] > -0.5) & (uv[:, 0] < w - 0.5) & (uv[:, 1] > -0.5) & (uv[:, 1] < h - 0.5)
    hit[np.rint(uv[inside, 1]).astype(int), np.rint(uv[inside, 0]).astype(int)] = False
    d = distance_transform_edt(hit)
    S = (255.0 * (1.0 - np.exp(-d * d / (2.0 * SIGMA * SIGMA)))).astype(np.float32)
    return P, S, truth


def torch_terms(P, S, T, delta):
    """the evaluation in torch, float64 on the device -> (29,) sums in the library's order"""
    import torch
    fx, fy, cx, cy = INTRINSICS
    h, w = S.shape
    X = P @ T[:3, :3].T + T[:3, 3]
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    u, v = fx * (x / z) + cx, fy * (y / z) + cy
    ok = torch.isfinite(X).all(dim=1) & (z > 0) & (u >= 0) & (u < w - 1) & (v >= 0) & (v < h - 1)
    fu, fv = torch.floor(u), torch.floor(v)
    x0, y0 = torch.where(ok, fu, 0.0).long(), torch.where(ok, fv, 0.0).long()
    flat = S.reshape(-1).double()
    s00, s01, s10, s11 = (flat[(y0 + dy) * w + x0 + dx] for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)))
    a, b = u - fu, v - fv
    r = (1 - b) * ((1 - a) * s00 + a * s01) + b * ((1 - a) * s10 + a * s11)
    gx, gy = (1 - b) * (s01 - s00) + b * (s11 - s10), (1 - a) * (s10 - s00) + a * (s11 - s01)
    j3 = torch.stack((gx * fx / z, gy * fy / z, -(gx * fx * x + gy * fy * y) / (z * z)), dim=1)
    J = torch.cat((j3, torch.linalg.cross(X, j3)), dim=1)
    ar = r.abs()
    tail = ar > delta
    wgt = torch.where(tail, delta / ar, 1.0) * ok
    rho = torch.where(tail, delta * (2 * ar - delta), r * r)
    J, r, rho = (torch.where(ok[:, None] if q.dim() == 2 else ok, q, 0.0) for q in (J, r, rho))
    A = (J * wgt[:, None]).T @ J
    g = (J * wgt[:, None]).T @ r
    iu = torch.triu_indices(6, 6, device=P.device)
    return torch.cat((A[iu[0], iu[1]], g, rho.sum()[None], ok.sum()[None].double()))


def main():
    import torch
    import _track_np as N
    import event_utils_amd as E
    from event_utils_amd import _device as D
    from event_utils_amd import _lib
    quick, trace = "--quick" in sys.argv, "--trace" in sys.argv
    reps = 3 if quick else 9
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "track_time.txt")
    K = camera()

    def median_ms(fn, calls=CALLS):
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / calls)
        return float(np.median(ts))

    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def row(name, ms, extra=""):
        say("%-78s %9.4f ms%s" % (name, ms, extra))
        return ms

    def bare(P, S, poses):
        """the library entry on resident buffers: -> a function of no arguments, and the sums it fills"""
        nb = len(poses)
        scratch = torch.empty(int(_lib.lib().evk_track_scratch_bytes(len(P), nb)), dtype=torch.uint8, device="cuda")
        sums = torch.empty((nb, 29), dtype=torch.float64, device="cuda")
        p12 = np.ascontiguousarray(np.stack([np.concatenate((T[:3, :3].reshape(9), T[:3, 3])) for T in poses]))
        args = (D.ptr(P), len(P), D.ptr(S), SIZE[0], SIZE[1], *INTRINSICS, D.host_ptr(p12), nb, _lib.EVK_TRACK_HUBER, DELTA, D.ptr(scratch),
                D.ptr(sums), D.stream())
        return (lambda: _lib.call("evk_track_terms", *args)), sums, (scratch, p12)

    say("camera tracking timings: %d x %d surface, loss huber, delta %g; median of %d repetitions of %d calls; %s"
        % (SIZE[1], SIZE[0], DELTA, reps, CALLS, torch.cuda.get_device_name(0)))
    for m in COUNTS:
        Pn, Sn, truth = scene(m)
        start = N.left(np.array([0.004, 0.003, -0.004, -0.0015, 0.002, 0.002]), *truth)
        T0 = N.matrix(*start)
        P, S = torch.from_numpy(Pn).cuda(), torch.from_numpy(Sn).cuda()
        one = [T0]
        eight = [N.matrix(*N.left(0.001 * np.array([b, -b, 1.0, 0.1 * b, 0.2, -0.1 * b]), *start)) for b in range(8)]
        if trace:
            for poses in (one, eight):
                fn, _, keep = bare(P, S, poses)
                for _ in range(5):
                    fn()
            E.register_points(P, S, K, T0, delta=DELTA)
            torch.cuda.synchronize()
            continue
        say("")
        off = N.reprojection_error(Pn, INTRINSICS, start, truth).mean()
        say("M = %d points (%.0f bytes each way: 24 of the point, 16 of the surface), the start %.2f px from the truth" % (m, 40.0, off))
        for poses, what in ((one, "B = 1"), (eight, "B = 8")):
            stack = np.stack(poses)
            row("  registration_terms, %s, the public call" % what, median_ms(lambda: E.registration_terms(P, S, K, stack, "huber", DELTA)))
            fn, sums, keep = bare(P, S, poses)
            row("  evk_track_terms, %s, the library entry on resident buffers" % what, median_ms(fn))
        fn, sums, keep = bare(P, S, one)
        fn()
        T0d = torch.from_numpy(T0).cuda()
        ref = torch_terms(P, S, T0d, DELTA)
        worst = float(((sums[0] - ref).abs() / ref.abs().clamp_min(1e-300)).max())
        say("  the torch form gives the kernel's sums: count %d = %d, largest relative difference %.1e" % (int(sums[0, 28]), int(ref[28]), worst))
        row("  yardstick: the same evaluation in torch on the device, float64, B = 1", median_ms(lambda: torch_terms(P, S, T0d, DELTA)))
        t0 = time.perf_counter()
        for _ in range(3):
            N.products(Pn, Sn, INTRINSICS, *start, "huber", DELTA).sum(axis=0)
        row("  yardstick: the numpy restatement on the host (products and their sums)", (time.perf_counter() - t0) * 1e3 / 3)
        reg = E.register_points(P, S, K, T0, delta=DELTA)
        end = N.reprojection_error(Pn, INTRINSICS, (reg.pose[:3, :3], reg.pose[:3, 3]), truth).mean()
        ms = row("  register_points, the whole call: %d evaluations, %s, %.2f -> %.3f px" % (reg.evaluations, reg.status, off, end),
                 median_ms(lambda: E.register_points(P, S, K, T0, delta=DELTA), calls=2))
        say("    %.4f ms an evaluation (two launches, a read-back of 29 doubles, the 6 x 6 solve on the host)" % (ms / reg.evaluations))
        if m >= SIZE[0] * SIZE[1] // 2:
            say("    (a dense mask leaves the surface almost no basin, max %.0f of 255: a case for the time, not for the pose)" % float(Sn.max()))
    if trace:
        return
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
