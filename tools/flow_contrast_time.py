"""Timings of the contrast (focus) loss of a dense flow field (flow_field_contrast_loss) with 10 k, 100 k and 1 M events at
180x240 and 480x640, one sample, variance objective, sigma 1, direction 'forward', on seeded float32 events and a smooth seeded
field resident in HBM:
  fused value       flow_field_contrast_loss: time constants + max |q| + one splat pass + the post pass,
  composed value    what exists without it: warp_events_flow_torch -> the bounds mask on the warped columns ->
                    events_to_image_torch(bilinear) -> gaussian_filter_device -> var (float atomics: not repeatable, no gradient),
  fused value+grad  the same call with compute_gradient=True (one more pass over the events),
  torch value+grad  the same graph written in plain torch operations under autograd (grid_sample, index_put with accumulate,
                    conv2d on a reflect-padded image, backward()): how a user gets dloss/dflow without it.
Every shape is warmed up, every repetition synchronises before and after (host clock); the median is reported, with the ratio
baseline / fused.  The losses of the four forms are compared before anything is timed.  Kernel times: run under
`rocprofv3 --kernel-trace --stats` in a run of its own (--quick: fewer repetitions).
usage: python tools/flow_contrast_time.py [--quick] [--out profiles/flow_contrast_time.txt]"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import event_utils_amd as E  # noqa: E402
from event_utils_amd.contrast_max.objectives import gaussian_filter_device, gaussian_kernel1d  # noqa: E402

SIZES = (10_000, 100_000, 1_000_000)
SENSORS = ((180, 240), (480, 640))
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


def composed_value(flow, x, y, t, p):
    """The value from the public calls that exist without the fused path."""
    H, W = flow.shape[-2:]
    xw, yw = E.transforms.warp_events_flow_torch(x, y, t, p, flow)
    keep = (xw > 0) & (xw < W) & (yw > 0) & (yw < H)
    img = E.events_to_image_torch(xw[keep], yw[keep], p[keep], sensor_size=(H, W), interpolation="bilinear", padding=True)
    return -torch.var(gaussian_filter_device(img, SIGMA).double(), unbiased=False)


def torch_loss(flow, x, y, t, p, taps):
    """The definition in torch operations, differentiable in `flow` (float32 throughout, as a training loop would run it)."""
    H, W = flow.shape[-2:]
    grid = torch.stack((x / (W - 1) * 2 - 1, y / (H - 1) * 2 - 1), dim=-1).reshape(1, 1, -1, 2)
    uv = TF.grid_sample(flow[None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, 0]
    dt = t - t[-1]
    xw, yw = x + uv[0] * dt, y + uv[1] * dt
    keep = (xw > 0) & (xw < W) & (yw > 0) & (yw < H)
    xw, yw, pk = xw[keep], yw[keep], p[keep]
    px, py = xw.floor(), yw.floor()
    dx, dy = xw - px, yw - py
    idx = py.long() * (W + 1) + px.long()
    img = torch.zeros((H + 1) * (W + 1), dtype=flow.dtype, device=flow.device)
    for off, wt in ((0, (1 - dx) * (1 - dy)), (1, dx * (1 - dy)), (W + 1, (1 - dx) * dy), (W + 2, dx * dy)):
        img = img.index_put((idx + off,), pk * wt, accumulate=True)
    img = img.reshape(1, 1, H + 1, W + 1)
    r = taps.numel() // 2
    # scipy's 'reflect' (the edge sample repeated) is torch's 'symmetric', which F.pad lacks: flip the borders by hand
    rows = torch.cat((img[:, :, :r].flip(2), img, img[:, :, -r:].flip(2)), dim=2)
    blur = TF.conv2d(rows, taps.reshape(1, 1, -1, 1))
    cols = torch.cat((blur[:, :, :, :r].flip(3), blur, blur[:, :, :, -r:].flip(3)), dim=3)
    blur = TF.conv2d(cols, taps.reshape(1, 1, 1, -1))
    return -torch.var(blur.double(), unbiased=False)


def torch_value_and_grad(flow, cols, taps):
    leaf = flow.detach().clone().requires_grad_(True)
    loss = torch_loss(leaf, *cols, taps)
    loss.backward()
    return loss.detach(), leaf.grad


def main():
    quick = "--quick" in sys.argv
    reps = 7 if quick else 11
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles",
                                                                                             "flow_contrast_time.txt")
    assert torch.cuda.is_available(), "needs the GPU"
    taps = torch.from_numpy(gaussian_kernel1d(SIGMA)[0]).float().cuda()
    lines = ["# flow_field_contrast_loss, variance, sigma %g, direction forward, one sample, device float32 events and field; median" % SIGMA,
             "# of %d synchronised repetitions after a warm-up, host clock, ms per call.  composed: warp_events_flow_torch -> bounds" % reps,
             "# mask -> events_to_image_torch(bilinear) -> gaussian_filter_device -> var (value only).  torch: the same graph in torch",
             "# operations under autograd (value + gradient).  x = baseline / fused.",
             "%-8s %9s %10s %10s %7s %11s %11s %7s" % ("sensor", "events", "fused val", "composed", "x", "fused v+g", "torch v+g", "x")]
    print("\n".join(lines), flush=True)
    for H, W in SENSORS:
        yy, xx = np.mgrid[0:H, 0:W]
        for n in SIZES:
            rng = np.random.default_rng(n + W)
            flow_np = np.stack([60 * np.sin(0.02 * xx + 0.013 * yy), 60 * np.cos(0.017 * xx - 0.021 * yy)]).astype(np.float32)
            cols_np = (rng.uniform(0, W - 1, n).astype(np.float32), rng.uniform(0, H - 1, n).astype(np.float32),
                       np.sort(rng.uniform(0, 0.05, n)).astype(np.float32), (rng.integers(0, 2, n) * 2 - 1).astype(np.float32))
            flow = torch.from_numpy(flow_np).cuda()
            cols = tuple(torch.from_numpy(c).cuda() for c in cols_np)
            fused = lambda g: E.flow_field_contrast_loss(flow, *cols, blur_sigma=SIGMA, compute_gradient=g)  # noqa: E731
            # the four forms compute the same thing (the composition with float atomics, torch in float32 operations of its own)
            lf, gf = fused(True)
            lf = float(lf)
            lc = float(composed_value(flow, *cols))
            lt, gt = torch_value_and_grad(flow, cols, taps)
            assert abs(lf - lc) <= 1e-5 * abs(lf), (lf, lc)
            assert abs(float(lt) - lf) <= 1e-3 * abs(lf), (float(lt), lf)
            # (single pixels differ where float32 torch puts an event in the neighbouring cell: compare in the L2 norm)
            assert float((gt - gf).norm()) <= 5e-2 * float(gf.norm())
            tv = median_ms(lambda: fused(False), reps)
            tc = median_ms(lambda: composed_value(flow, *cols), reps)
            tg = median_ms(lambda: fused(True), reps)
            tt = median_ms(lambda: torch_value_and_grad(flow, cols, taps), reps)
            lines.append("%-8s %9d %10.3f %10.3f %7.2f %11.3f %11.3f %7.2f" % ("%dx%d" % (H, W), n, tv, tc, tc / tv, tg, tt, tt / tg))
            print(lines[-1], flush=True)
            del flow, cols
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
