"""Timings of the average-timestamp loss of a dense flow field (flow_field_timestamp_loss) with 10 k, 100 k and 1 M events per
sample at 180x240 and 480x640, for one sample and for a batch of 8, sigma 2, direction 'forward', on seeded float32 events and a
smooth seeded field resident in HBM:
  fused value       flow_field_timestamp_loss: time constants + one splat pass + the post pass per sample,
  composed value    what exists without it: warp_events_flow_torch -> zhu_timestamp_objective().evaluate_function([0, 0], xw, yw,
                    ts, ps, linvel_warp(), ...) on the materialised warped columns, sample by sample,
  fused value+grad  the same call with compute_gradient=True (one more pass over the events),
  torch value+grad  the same loss written in plain torch operations under autograd (grid_sample, index_put_ with accumulate,
                    conv2d on a reflect-padded image, backward()), sample by sample: how a user gets dloss/dflow without it.
Every shape is warmed up, every repetition synchronises before and after (host clock); the median is reported, with the ratio
baseline / fused.  The losses of the four forms are compared before anything is timed.  Kernel times: run under
`rocprofv3 --kernel-trace --stats` in a run of its own (--quick: fewer repetitions).
usage: python tools/flow_loss_time.py [--quick] [--out profiles/flow_loss_time.txt]"""
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import event_utils_amd as E  # noqa: E402
from event_utils_amd.contrast_max.objectives import gaussian_kernel1d  # noqa: E402

SIZES = (10_000, 100_000, 1_000_000)
SENSORS = ((180, 240), (480, 640))
BATCHES = (1, 8)
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


def composed_value(flows, samples, sensor):
    """The value from the two public calls that exist without the fused path, sample by sample."""
    obj = E.zhu_timestamp_objective()
    obj.sensor_size = sensor
    out = []
    for flow, (x, y, t, p) in zip(flows, samples):
        xw, yw = E.transforms.warp_events_flow_torch(x, y, t, p, flow)
        out.append(obj.evaluate_function(np.zeros(2), xw, yw, t, p, E.linvel_warp(), sensor, SIGMA))
    return out


def torch_loss(flow, x, y, t, p, taps):
    """The definition in torch operations, differentiable in `flow` (float32 throughout, as a training loop would run it)."""
    H, W = flow.shape[-2:]
    grid = torch.stack((x / (W - 1) * 2 - 1, y / (H - 1) * 2 - 1), dim=-1).reshape(1, 1, -1, 2)
    uv = TF.grid_sample(flow[None], grid, mode="bilinear", padding_mode="zeros", align_corners=True)[0, :, 0]
    dt = t - t[-1]
    xw, yw = x + uv[0] * dt, y + uv[1] * dt
    keep = (xw > 0) & (xw < W) & (yw > 0) & (yw < H)
    xw, yw, tk, pk = xw[keep], yw[keep], t[keep], p[keep]
    tau = (tk - t[0]) / (t[-1] - t[0] + 1e-6)
    px, py = xw.floor(), yw.floor()
    dx, dy = xw - px, yw - py
    idx = py.long() * (W + 1) + px.long() + torch.where(pk > 0, 0, 2 * (H + 1) * (W + 1))
    planes = torch.zeros(4 * (H + 1) * (W + 1), dtype=flow.dtype, device=flow.device)
    for off, wt in ((0, (1 - dx) * (1 - dy)), (1, dx * (1 - dy)), (W + 1, (1 - dx) * dy), (W + 2, dx * dy)):
        planes = planes.index_put((idx + off,), tau * wt, accumulate=True)
        planes = planes.index_put((idx + off + (H + 1) * (W + 1),), wt, accumulate=True)
    planes = planes.reshape(2, 2, H + 1, W + 1)
    avg = (planes[:, 0] / (1 + planes[:, 1]))[:, None]
    r = taps.numel() // 2
    # scipy's 'reflect' (the edge sample repeated) is torch's 'symmetric', which F.pad lacks: flip the borders by hand
    rows = torch.cat((avg[:, :, :r].flip(2), avg, avg[:, :, -r:].flip(2)), dim=2)
    blur = TF.conv2d(rows, taps.reshape(1, 1, -1, 1))
    cols = torch.cat((blur[:, :, :, :r].flip(3), blur, blur[:, :, :, -r:].flip(3)), dim=3)
    blur = TF.conv2d(cols, taps.reshape(1, 1, 1, -1))
    return (blur.double() ** 2).sum()


def torch_value_and_grad(flows, samples, taps):
    out = []
    for flow, cols in zip(flows, samples):
        leaf = flow.detach().clone().requires_grad_(True)
        loss = torch_loss(leaf, *cols, taps)
        loss.backward()
        out.append((loss.detach(), leaf.grad))
    return out


def main():
    quick = "--quick" in sys.argv
    reps = 5 if quick else 11
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles",
                                                                                             "flow_loss_time.txt")
    assert torch.cuda.is_available(), "needs the GPU"
    taps = torch.from_numpy(gaussian_kernel1d(SIGMA)[0]).float().cuda()
    lines = ["# flow_field_timestamp_loss, sigma %g, direction forward, device float32 events and field; median of %d synchronised" % (
                 SIGMA, reps),
             "# repetitions after a warm-up, host clock, ms per call (a call evaluates the whole batch).  composed:",
             "# warp_events_flow_torch -> zhu_timestamp_objective.evaluate_function at zero velocity, sample by sample (value only).",
             "# torch: the same loss in torch operations under autograd, sample by sample (value + gradient).  x = baseline / fused.",
             "%-8s %3s %9s %10s %10s %7s %11s %11s %7s" % ("sensor", "B", "events/B", "fused val", "composed", "x", "fused v+g",
                                                         "torch v+g", "x")]
    print("\n".join(lines), flush=True)
    for H, W in SENSORS:
        yy, xx = np.mgrid[0:H, 0:W]
        for B in BATCHES:
            for n in SIZES:
                rng = np.random.default_rng(n + W + B)
                flows_np = np.stack([np.stack([60 * np.sin(0.02 * xx + 0.013 * yy + b), 60 * np.cos(0.017 * xx - 0.021 * yy + b)])
                                     for b in range(B)]).astype(np.float32)
                samples_np = [(rng.uniform(0, W - 1, n).astype(np.float32), rng.uniform(0, H - 1, n).astype(np.float32),
                               np.sort(rng.uniform(0, 0.05, n)).astype(np.float32),
                               (rng.integers(0, 2, n) * 2 - 1).astype(np.float32)) for _ in range(B)]
                flows = torch.from_numpy(flows_np).cuda()
                samples = [tuple(torch.from_numpy(c).cuda() for c in s) for s in samples_np]
                cat = tuple(torch.cat([s[k] for s in samples]) for k in range(4))
                offsets = torch.arange(B + 1, dtype=torch.int64) * n
                if B == 1:
                    fused = lambda g: E.flow_field_timestamp_loss(flows[0], *cat, blur_sigma=SIGMA, compute_gradient=g)  # noqa: E731
                else:
                    fused = lambda g: E.flow_field_timestamp_loss(flows, *cat, blur_sigma=SIGMA, offsets=offsets,  # noqa: E731
                                                                  compute_gradient=g)
                # the four forms compute the same thing (torch in float32 operations of its own)
                lf, gf = fused(True)
                lf, gf = lf.reshape(-1).tolist(), gf.reshape(B, 2, H, W)
                lc = composed_value(flows, samples, (H, W))
                lt = torch_value_and_grad(flows, samples, taps)
                for b in range(B):
                    assert abs(lf[b] - float(lc[b])) <= 1e-6 * lf[b], (lf[b], lc[b])
                    assert abs(float(lt[b][0]) - lf[b]) <= 1e-3 * lf[b], (float(lt[b][0]), lf[b])
                    # (single pixels differ where float32 torch puts an event in the neighbouring cell: compare in the L2 norm)
                    assert float((lt[b][1] - gf[b]).norm()) <= 5e-2 * float(gf[b].norm())
                tv = median_ms(lambda: fused(False), reps)
                tc = median_ms(lambda: composed_value(flows, samples, (H, W)), reps)
                tg = median_ms(lambda: fused(True), reps)
                tt = median_ms(lambda: torch_value_and_grad(flows, samples, taps), max(3, reps // 2))
                lines.append("%-8s %3d %9d %10.3f %10.3f %7.2f %11.3f %11.3f %7.2f" % ("%dx%d" % (H, W), B, n, tv, tc, tc / tv, tg, tt,
                                                                                     tt / tg))
                print(lines[-1], flush=True)
                del flows, samples, cat
                torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
