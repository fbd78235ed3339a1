"""Timings of one value-and-gradient evaluation of the variance objective for pure_rotation_warp, xyztheta_warp,
angular_velocity_warp and planar_flow_warp at 100 k, 1 M and 10 M events, on 240x180 and 640x480 sensors, through three
paths on the same seeded device events:
  band          the fused evk_iwe_param_f32 with its LDS-band kernel (the default),
  direct        the same entry with EVK_IWE_DIRECT (global float atomics per contribution; EVK_IMPL=direct),
  materialised  warp() -> events_bounds_mask -> events_to_image_drv (x', y' and the (dims, N) Jacobians in memory),
each followed by the same blur and plane-sum post-pass.  Events are device-resident float32 columns, every shape is warmed
up, every repetition synchronises before and after; the median is reported.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats` (--quick: fewer repetitions).
usage: python tools/motion_models_time.py [--quick] [--out profiles/motion_models_time.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import event_utils_amd as E  # noqa: E402
from event_utils_amd import _device as D  # noqa: E402
from event_utils_amd import _lib  # noqa: E402
from event_utils_amd.contrast_max import objectives as O  # noqa: E402
from event_utils_amd.representations.image import _events_to_image_drv_device  # noqa: E402

SIZES = (100_000, 1_000_000, 10_000_000)
SENSORS = ((180, 240), (480, 640))


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


def post(iwe, d_iwe):
    """The objective's post-pass of evaluate_function_and_gradient (reference_exact=False, sigma 1)."""
    f = O.variance_objective.evaluate_function(obj, blur_sigma=1.0, iwe=iwe)
    return f, O._variance_gradient_planes(iwe, d_iwe, 1.0, False)


obj = E.variance_objective()
obj.reference_exact = False


def fused(ev, w, q, ss, impl):
    iwe, d_iwe = O.iwe_param_device(q, ev, w, ss, True, True, ss, impl)
    return post(iwe, d_iwe)


def materialised(ev, w, q, ss):
    xd, yd, td, pd = (c.double() for c in (ev.x, ev.y, ev.t, ev.p))
    xw, yw, jx, jy = w.warp(xd, yd, td, None, float(ev.t_at(-1)), q, compute_grad=True)
    mask = E.events_bounds_mask(xw, yw, 0, ss[1], 0, ss[0])
    xw, yw, pm, jx, jy = xw * mask, yw * mask, pd * mask, jx * mask, jy * mask
    # events_to_image_drv splats two derivative planes per call (the reference hard-codes 2): planes in pairs
    iwe, d01 = _events_to_image_drv_device(xw, yw, pm, jx[:2], jy[:2], ss, True, 'bilinear', True, True)
    planes = [d01]
    for k in range(2, w.dims, 2):
        jxk, jyk = jx[k:k + 2], jy[k:k + 2]
        if jxk.shape[0] == 1:
            jxk, jyk = torch.cat([jxk, jxk]), torch.cat([jyk, jyk])
        planes.append(_events_to_image_drv_device(xw, yw, pm, jxk, jyk, ss, True, 'bilinear', True, True)[1])
    d_iwe = torch.cat(planes)[:w.dims].to(torch.float32).contiguous()
    return post(iwe.to(torch.float32).contiguous(), d_iwe)


def main():
    quick = "--quick" in sys.argv
    reps = 5 if quick else 15
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles",
                                                                                                "motion_models_time.txt")
    assert torch.cuda.is_available(), "needs the GPU"
    lines = ["# one value + gradient evaluation of variance_objective (reference_exact=False, sigma 1), device float32 events,",
             "# median of %d synchronised repetitions after a warm-up; ms.  rows = evk_iwe_param_band_rows (0: direct)" % reps,
             "%-16s %-8s %9s %5s %6s %10s %10s %13s %9s %9s" % ("model", "sensor", "events", "rows", "bands", "band", "direct",
                                                                "materialised", "mat/band", "dir/band")]
    print(lines[-1], flush=True)
    for ss in SENSORS:
        H, W = ss
        K = np.array([[W * 0.8, 0.0, W / 2.0], [0.0, W * 0.8, H / 2.0], [0.0, 0.0, 1.0]])
        for n in SIZES:
            rng = np.random.default_rng(n + W)
            x = rng.uniform(0, W, n).astype(np.float32)
            y = rng.uniform(0, H, n).astype(np.float32)
            t = np.sort(rng.uniform(0, 0.1, n)).astype(np.float32)
            p = (rng.integers(0, 2, n) * 2 - 1).astype(np.float32)
            ev = E.DeviceEvents.from_arrays(x, y, t, p, precision="f32")
            for w, q in ((E.pure_rotation_warp(), (W / 2 - 10, H / 2 + 5, 1.5)),
                         (E.xyztheta_warp(center=(W / 2, H / 2)), (40.0, -25.0, 2.0, 1.0)),
                         (E.angular_velocity_warp(K), (0.8, -0.6, 1.2)),
                         (E.planar_flow_warp(center=(W / 2, H / 2)), (40.0, 0.5, -0.3, -25.0, 0.2, 0.6, 2e-3, -1.5e-3))):
                rows = _lib.lib().evk_iwe_param_band_rows(w.fused_model, _lib.EVK_IWE_GRADIENT, H + 1, W + 1)
                tb = median_ms(lambda: fused(ev, w, q, ss, "auto"), reps)
                td = median_ms(lambda: fused(ev, w, q, ss, "direct"), reps)
                tm = median_ms(lambda: materialised(ev, w, q, ss), max(3, reps // 3))
                fb, gb = fused(ev, w, q, ss, "auto")
                fm, gm = materialised(ev, w, q, ss)
                assert abs(fb - fm) <= 1e-4 * abs(fm), (fb, fm)
                assert np.abs(gb - gm).max() <= 1e-3 * np.abs(gm).max(), (gb, gm)
                bands = -(-(H + 1) // rows) if rows else 0
                lines.append("%-16s %-8s %9d %5d %6d %10.3f %10.3f %13.3f %9.1f %9.1f" % (
                    w.name.split("_warp")[0], "%dx%d" % (W, H), n, rows, bands, tb, td, tm, tm / tb, td / tb))
                print(lines[-1], flush=True)
            del ev
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
