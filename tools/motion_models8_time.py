"""Timings of one value-and-gradient evaluation of the variance objective for angular_velocity_warp and planar_flow_warp at
100 k, 1 M and 10 M events, on 240x180 and 640x480 sensors, through the three paths of tools/motion_models_time.py:
  band          the fused evk_iwe_param8_f32 with its LDS-band kernel (the default),
  direct        the same entry with EVK_IWE_DIRECT (global float atomics per contribution; EVK_IMPL=direct),
  materialised  warp() -> events_bounds_mask -> events_to_image_drv (x', y' and the (dims, N) Jacobians in memory),
each followed by the same blur and plane-sum post-pass.  Median of 15 synchronised repetitions after a warm-up (--quick: 5).
usage: python tools/motion_models8_time.py [--quick] [--out profiles/motion_models8_time.txt]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_models_time as T  # noqa: E402  (median_ms, fused, materialised; puts the repository on sys.path)
import event_utils_amd as E  # noqa: E402
from event_utils_amd import _lib  # noqa: E402


def main():
    quick = "--quick" in sys.argv
    reps = 5 if quick else 15
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(T.ROOT, "profiles",
                                                                                                "motion_models8_time.txt")
    assert torch.cuda.is_available(), "needs the GPU"
    lines = ["# one value + gradient evaluation of variance_objective (reference_exact=False, sigma 1), device float32 events,",
             "# median of %d synchronised repetitions after a warm-up; ms.  rows = evk_iwe_param8_band_rows (0: direct)" % reps,
             "%-16s %-8s %9s %5s %6s %10s %10s %13s %9s %9s" % ("model", "sensor", "events", "rows", "bands", "band", "direct",
                                                                "materialised", "mat/band", "dir/band")]
    print(lines[-1], flush=True)
    for ss in T.SENSORS:
        H, W = ss
        K = np.array([[W * 0.8, 0.0, W / 2.0], [0.0, W * 0.8, H / 2.0], [0.0, 0.0, 1.0]])
        for n in T.SIZES:
            rng = np.random.default_rng(n + W)
            x = rng.uniform(0, W, n).astype(np.float32)
            y = rng.uniform(0, H, n).astype(np.float32)
            t = np.sort(rng.uniform(0, 0.1, n)).astype(np.float32)
            p = (rng.integers(0, 2, n) * 2 - 1).astype(np.float32)
            ev = E.DeviceEvents.from_arrays(x, y, t, p, precision="f32")
            for w, q in ((E.angular_velocity_warp(K), (0.8, -0.6, 1.2)),
                         (E.planar_flow_warp(center=(W / 2, H / 2)), (40.0, 0.5, -0.3, -25.0, 0.2, 0.6, 2e-3, -1.5e-3))):
                rows = _lib.lib().evk_iwe_param8_band_rows(w.fused_model, _lib.EVK_IWE_GRADIENT, H + 1, W + 1)
                tb = T.median_ms(lambda: T.fused(ev, w, q, ss, "auto"), reps)
                td = T.median_ms(lambda: T.fused(ev, w, q, ss, "direct"), reps)
                tm = T.median_ms(lambda: T.materialised(ev, w, q, ss), max(3, reps // 3))
                fb, gb = T.fused(ev, w, q, ss, "auto")
                fm, gm = T.materialised(ev, w, q, ss)
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
