"""Timings of zhu_timestamp_objective at 640x480 with 100 k, 1 M and 10 M events, for the linear flow and each parametric
model, on the same seeded device events (float32 columns resident in HBM):
  value         evaluate_function: the fused splat (LDS bands) + the post pass,
  value direct  the same with the direct global-atomic splat (impl 'direct'),
  composed      what exists without the fused path: warp() materialised -> bounds mask -> masked events removed ->
                events_to_timestamp_image_torch -> blur and sum in torch (value only),
  value+grad    evaluate_function_and_gradient: splat + post pass with the adjoint images + the gather pass,
  variance f+g  variance_objective.evaluate_function_and_gradient on the same events (reference_exact=False, sigma 1).
There is no earlier implementation of the gradient: its cost is reported as a multiple of the value-only evaluation and of
the variance objective's value + gradient.  Every shape is warmed up, every repetition synchronises before and after; the
median is reported.  Kernel times: run this under `rocprofv3 --kernel-trace --stats` (--quick: fewer repetitions).
usage: python tools/zhu_time.py [--quick] [--out profiles/zhu_time.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import event_utils_amd as E  # noqa: E402
from event_utils_amd import _lib  # noqa: E402
from event_utils_amd.contrast_max import objectives as O  # noqa: E402

SIZES = (100_000, 1_000_000, 10_000_000)
SENSOR = (480, 640)
SIGMA = 2.0


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def composed(ev, w, q, ss):
    """The loss from the pieces that exist without the fused path (value only)."""
    xd, yd, td, pd = (c.double() for c in (ev.x, ev.y, ev.t, ev.p))
    xw, yw, _, _ = w.warp(xd, yd, td, None, float(ev.t_at(-1)), q)
    keep = (E.events_bounds_mask(xw, yw, 0, ss[1], 0, ss[0]) > 0) & torch.isfinite(xw) & torch.isfinite(yw)
    xf, yf = xw.float(), yw.float()
    keep &= (xf < ss[1]) & (yf < ss[0])
    # (the time stamps are normalised by the ends of the KEPT events here: a timing comparison, not a parity one)
    pos, neg = E.events_to_timestamp_image_torch(xf[keep], yf[keep], ev.t[keep], pd[keep].float(), sensor_size=ss)
    loss = 0.0
    for a in (pos, neg):
        b = O.gaussian_filter_device(a.contiguous(), SIGMA)
        loss += float((b.double() ** 2).sum().item())
    return loss


def main():
    quick = "--quick" in sys.argv
    reps = 5 if quick else 15
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "zhu_time.txt")
    assert torch.cuda.is_available(), "needs the GPU"
    H, W = SENSOR
    rows = _lib.lib().evk_tsimg_band_rows(0, H + 1, W + 1)
    lines = ["# zhu_timestamp_objective at %dx%d, sigma %g, device float32 events; median of %d synchronised repetitions after a" % (
                 W, H, SIGMA, reps),
             "# warm-up; ms.  band rows %d (%d bands).  composed: warp() -> mask -> events_to_timestamp_image_torch -> blur, sum" % (
                 rows, -(-(H + 1) // rows) if rows else 0),
             "# (value only; its average divides by the count where this objective divides by 1 + count, so the two values differ).",
             "%-16s %9s %9s %9s %9s %10s %9s %10s %10s %10s" % ("model", "events", "value", "v.direct", "composed", "comp/value",
                                                              "val+grad", "vg/value", "var f+g", "vg/var")]
    print("\n".join(lines), flush=True)
    K = np.array([[W * 0.8, 0.0, W / 2.0], [0.0, W * 0.8, H / 2.0], [0.0, 0.0, 1.0]])
    zhu, zhu_direct, var = E.zhu_timestamp_objective(), E.zhu_timestamp_objective(), E.variance_objective()
    zhu.sensor_size = zhu_direct.sensor_size = var.sensor_size = SENSOR
    zhu_direct.impl = "direct"
    var.reference_exact = False
    for n in SIZES:
        rng = np.random.default_rng(n + W)
        x = rng.uniform(0, W, n).astype(np.float32)
        y = rng.uniform(0, H, n).astype(np.float32)
        t = np.sort(rng.uniform(0, 0.1, n)).astype(np.float32)
        p = (rng.integers(0, 2, n) * 2 - 1).astype(np.float32)
        ev = E.DeviceEvents.from_arrays(x, y, t, p, precision="f32")
        for w, q in ((E.linvel_warp(), (40.0, -25.0)),
                     (E.pure_rotation_warp(), (W / 2 - 10, H / 2 + 5, 1.5)),
                     (E.xyztheta_warp(center=(W / 2, H / 2)), (40.0, -25.0, 2.0, 1.0)),
                     (E.angular_velocity_warp(K), (0.8, -0.6, 1.2)),
                     (E.planar_flow_warp(center=(W / 2, H / 2)), (40.0, 0.5, -0.3, -25.0, 0.2, 0.6, 2e-6, -1.5e-6))):
            q = np.array(q, dtype=np.float64)
            a = (q, ev, None, None, None, w, SENSOR, SIGMA)
            tv = median_ms(lambda: zhu.evaluate_function(*a), reps)
            td = median_ms(lambda: zhu_direct.evaluate_function(*a), reps)
            tc = median_ms(lambda: composed(ev, w, q, SENSOR), max(3, reps // 3))
            tg = median_ms(lambda: zhu.evaluate_function_and_gradient(*a), reps)
            tvar = median_ms(lambda: var.evaluate_function_and_gradient(q, ev, None, None, None, w, SENSOR, 1.0), reps)
            fb, fd = zhu.evaluate_function(*a), zhu_direct.evaluate_function(*a)
            assert abs(fb - fd) <= 1e-5 * abs(fd), (fb, fd)
            lines.append("%-16s %9d %9.3f %9.3f %9.3f %10.1f %9.3f %10.2f %10.3f %10.2f" % (
                w.name.split("_warp")[0], n, tv, td, tc, tc / tv, tg, tg / tv, tvar, tg / tvar))
            print(lines[-1], flush=True)
        del ev
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
