"""Timings of motion segmentation (event_utils_amd.contrast_max.segmentation) with L = 2, 4, 8 linear-flow clusters and 100 k and
1 M events at 180x240, on seeded float32 events and random associations resident in HBM:
  images        cluster_iwes: one fused splat pass for all L planes,
  composed img  what exists without it: L x (linvel_warp().warp -> bounds mask -> events_to_image_torch(bilinear) with the
                weights P_l) -- 2 L warped columns, float atomics (not repeatable),
  value         segmentation_loss: the splat pass + the post pass per plane,
  composed val  the composition above -> gaussian_filter_device -> var per cluster, summed,
  value+grad    segmentation_loss(compute_gradient=True): one more pass over the events per cluster,
  assign        update_assignments: the splat pass, L blurs and the assignment pass.
The composition cannot produce the gradient or the assignment step, so those two columns have no baseline.  Every shape is
warmed up, every repetition synchronises before and after (host clock); the median is reported.  The images and the value of
the two forms are compared before anything is timed.
usage: python tools/segmentation_time.py [--quick] [--out profiles/segmentation_time.txt]"""
import datetime
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import event_utils_amd as E  # noqa: E402
from event_utils_amd.contrast_max.objectives import gaussian_filter_device  # noqa: E402

SIZES = (100_000, 1_000_000)
CLUSTERS = (2, 4, 8)
SENSOR = (180, 240)
SIGMA = 1.0


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


def composed_images(params, probs, x, y, t, p):
    """The L weighted images from the public calls that exist without the fused path (weights P_l: use_polarity=False)."""
    H, W = SENSOR
    warp, t0 = E.linvel_warp(), float(t[-1].item())
    out = []
    for q, w in zip(params, probs):
        xw, yw, _, _ = warp.warp(x, y, t, p, t0, q)
        keep = (xw > 0) & (xw < W) & (yw > 0) & (yw < H)
        out.append(E.events_to_image_torch(xw[keep].float(), yw[keep].float(), w[keep], sensor_size=SENSOR,
                                           interpolation="bilinear", padding=True))
    return torch.stack(out)


def composed_value(params, probs, x, y, t, p):
    imgs = composed_images(params, probs, x, y, t, p)
    return -sum(torch.var(gaussian_filter_device(img, SIGMA).double(), unbiased=False) for img in imgs)


def main():
    quick = "--quick" in sys.argv
    reps = 5 if quick else 11
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles",
                                                                                             "segmentation_time.txt")
    assert torch.cuda.is_available(), "needs the GPU"
    H, W = SENSOR
    lines = ["# motion segmentation, linear-flow clusters, %dx%d, sigma %g, use_polarity=False, device float32 events and" % (H, W, SIGMA),
             "# associations; median of %d synchronised repetitions after a warm-up, host clock, ms per call, %s on %s."
             % (reps, datetime.date.today().isoformat(), torch.cuda.get_device_name(0)),
             "# composed: L x (linvel_warp().warp -> bounds mask -> events_to_image_torch(bilinear, weights P_l)) [-> gaussian_filter_device",
             "# -> var]: images and value only; it cannot give the gradient or the assignment step.  x = composed / fused.",
             "%2s %9s %9s %10s %6s %9s %10s %6s %11s %9s" % ("L", "events", "images", "composed", "x", "value", "composed", "x",
                                                          "value+grad", "assign")]
    print("\n".join(lines), flush=True)
    warp = E.linvel_warp()
    for L in CLUSTERS:
        for n in SIZES:
            rng = np.random.default_rng(n + L)
            cols = (rng.uniform(1, W - 1, n).astype(np.float32), rng.uniform(1, H - 1, n).astype(np.float32),
                    np.sort(rng.uniform(0, 0.05, n)).astype(np.float32), (rng.integers(0, 2, n) * 2 - 1).astype(np.float32))
            params = rng.uniform(-200.0, 200.0, (L, 2))
            probs = torch.from_numpy(np.ascontiguousarray(rng.dirichlet(np.ones(L), n).T, dtype=np.float32)).cuda()
            ev = E.DeviceEvents.from_arrays(*cols)
            tens = (ev.x, ev.y, ev.t, ev.p)
            args = (params, probs, ev, None, None, None, warp, SENSOR)
            imgs, comp = E.cluster_iwes(*args), composed_images(params, probs, *tens)
            assert float((imgs - comp).abs().max()) <= 1e-4 * float(imgs.abs().max())
            lf, lc = E.segmentation_loss(*args, blur_sigma=SIGMA), float(composed_value(params, probs, *tens))
            assert abs(lf - lc) <= 1e-4 * abs(lf), (lf, lc)
            ti = median_ms(lambda: E.cluster_iwes(*args), reps)
            tci = median_ms(lambda: composed_images(params, probs, *tens), reps)
            tv = median_ms(lambda: E.segmentation_loss(*args, blur_sigma=SIGMA), reps)
            tcv = median_ms(lambda: float(composed_value(params, probs, *tens)), reps)
            tg = median_ms(lambda: E.segmentation_loss(*args, blur_sigma=SIGMA, compute_gradient=True), reps)
            ta = median_ms(lambda: E.update_assignments(*args, blur_sigma=SIGMA), reps)
            lines.append("%2d %9d %9.3f %10.3f %6.2f %9.3f %10.3f %6.2f %11.3f %9.3f" % (L, n, ti, tci, tci / ti, tv, tcv, tcv / tv, tg, ta))
            print(lines[-1], flush=True)
            del ev, tens, probs, imgs, comp
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
