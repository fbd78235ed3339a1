"""Timings of event stereo (event_utils_amd.depth.stereo; evk_stereo.hip) at 640x480 with 64 disparities and at 346x260 with 32,
radius 3, one and sixteen queries.  The two streams are about 10 M events each: points that move about one pixel per millisecond for
0.1 s, seen on the left at (x, y) and on the right at (x - d, y) with a disparity of their own, as float32 resident columns (a
DeviceEvents per camera); tau = 10 ms and the queries are spread over the last 15 ms.  Per case: the match entry on the surfaces of
the scene (only candidates are matched) and on dense random surfaces (every pixel a candidate: the worst case), the cost-volume
entry, and the whole stereo_disparity call.  Beside them two yardsticks: the two time_surfaces(decay=None) calls on the same events,
which is what the matcher sits on top of, and the same cost volume written in torch on the device (pad, unfold, abs, sum, one
disparity at a time to bound the memory), which is what a user would write without the kernel; its result is compared with the
kernel's.  Every timed repetition synchronises before and after; the median is reported.  No time here is a pass / fail criterion.
usage: timeout 900 python tools/stereo_time.py [--quick] [--out profiles/stereo_time.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("640x480, D = 64, r = 3", (480, 640), 64), ("346x260, D = 32, r = 3", (260, 346), 32))
N_EVENTS = 10_000_000
RADIUS, TAU, DURATION, ACTIVITY = 3, 0.010, 0.100, 128
QUERIES = (1, 16)


def scene(n, size, nd, seed=0):
    """two streams of about n events: (xs, ys, ts, ps) each, stamps non-decreasing"""
    rng = np.random.default_rng(seed)
    h, w = size
    steps = 500
    points = -(-n // steps)
    d = rng.integers(2, nd - 2, points)
    x0, y0 = rng.uniform(0, w, points), rng.uniform(0, h, points)
    speed, angle = rng.uniform(600.0, 1400.0, points), rng.uniform(0, 2 * np.pi, points)
    vx, vy = speed * np.cos(angle), speed * np.sin(angle)
    pol = (rng.integers(0, 2, points) * 2 - 1).astype(np.float32)
    left, right = [], []
    for t in np.linspace(0.0, DURATION, steps, endpoint=False):
        # a point that leaves the sensor comes back in on the other side
        px, py = np.rint(x0 + vx * t).astype(np.int64) % w, np.rint(y0 + vy * t).astype(np.int64) % h
        ts = np.full(points, t, dtype=np.float32)
        left.append((px, py, ts, pol))
        seen = px - d >= 0
        right.append(((px - d)[seen], py[seen], ts[seen], pol[seen]))
    return tuple(tuple(np.concatenate([s[i] for s in side]) for i in range(4)) for side in (left, right))


def main():
    import torch
    import torch.nn.functional as F
    import event_utils_amd as E
    quick = "--quick" in sys.argv
    reps = 3 if quick else 9
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "stereo_time.txt")

    def median_ms(fn, reps=reps):
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    class Lines(list):
        def append(self, line):
            print(line, flush=True)
            list.append(self, line)

    lines = Lines()

    def row(name, ms, extra=""):
        lines.append("%-74s %9.3f ms%s" % (name, ms, extra))
        return ms

    def torch_volume(QL, QR, nd, r):
        """the cost volume of one query in torch: (D, H, W) float32, admissible or not"""
        c, h, w = QL.shape
        win = 2 * r + 1
        UL = F.unfold(F.pad(QL.float()[None], (r, r, r, r)), win).view(c * win * win, h, w)
        UR = F.unfold(F.pad(QR.float()[None], (r + nd - 1, r, r, r)), win).view(c * win * win, h, w + nd - 1)
        return torch.stack([(UL - UR[:, :, nd - 1 - d:nd - 1 - d + w]).abs().sum(dim=0) for d in range(nd)])

    lines.append("event stereo timings: radius %d, tau %g s, min_activity %d, uniqueness 10, lr_tolerance 1, sub-pixel; median of %d; %s"
                 % (RADIUS, TAU, ACTIVITY, reps, torch.cuda.get_device_name(0)))
    for title, size, nd in CASES:
        h, w = size
        left, right = scene(N_EVENTS // (20 if quick else 1), size, nd)
        evl, evr = (E.DeviceEvents.from_arrays(*s, precision="f32") for s in (left, right))
        lines.append("")
        lines.append("%s: %d left and %d right events" % (title, len(left[0]), len(right[0])))
        for nq in QUERIES:
            t_refs = list(np.linspace(DURATION - 0.015, DURATION, nq)) if nq > 1 else [DURATION]
            QL = E.quantised_time_surfaces(evl, None, None, None, TAU, size, t_refs)
            QR = E.quantised_time_surfaces(evr, None, None, None, TAU, size, t_refs)
            res = E.stereo_match(QL, QR, nd - 1, radius=RADIUS, min_activity=ACTIVITY)
            cells = nq * nd * h * w
            lines.append("  K = %d: %.3f of the left pixels are candidates, %.3f valid" % (
                nq, float((res.cost >= 0).float().mean()), float(res.mask.float().mean())))
            ms = row("    stereo_match, the scene's surfaces", median_ms(lambda: E.stereo_match(QL, QR, nd - 1, radius=RADIUS, min_activity=ACTIVITY)))
            rng = torch.Generator(device="cuda").manual_seed(1)
            DL = torch.randint(128, 256, QL.shape, dtype=torch.uint8, device="cuda", generator=rng)
            DR = torch.randint(128, 256, QL.shape, dtype=torch.uint8, device="cuda", generator=rng)
            ms = row("    stereo_match, dense random surfaces (every pixel a candidate)",
                     median_ms(lambda: E.stereo_match(DL, DR, nd - 1, radius=RADIUS, min_activity=ACTIVITY)))
            lines.append("      %.1f G pixel-disparities / s with the left-right pass counted once" % (cells / ms / 1e6))
            ms = row("    stereo_match, dense, no left-right test",
                     median_ms(lambda: E.stereo_match(DL, DR, nd - 1, radius=RADIUS, min_activity=ACTIVITY, lr_tolerance=None)))
            ms = row("    stereo_cost_volume (%.0f MB written)" % (4 * cells / 1e6), median_ms(lambda: E.stereo_cost_volume(QL, QR, nd - 1, radius=RADIUS)))
            lines.append("      %.1f G pixel-disparities / s, %.0f GB/s written" % (cells / ms / 1e6, 4 * cells / ms / 1e6))
            row("    stereo_disparity, the whole call on the two streams",
                median_ms(lambda: E.stereo_disparity(evl, evr, TAU, size, t_refs, nd - 1, radius=RADIUS, min_activity=ACTIVITY)))
            row("    yardstick: two time_surfaces(decay=None) calls on the same events",
                median_ms(lambda: (E.time_surfaces(evl, None, None, None, TAU, size, t_refs=t_refs, decay=None, polarity="ignore"),
                                   E.time_surfaces(evr, None, None, None, TAU, size, t_refs=t_refs, decay=None, polarity="ignore"))))
            row("    quantised_time_surfaces, both cameras",
                median_ms(lambda: (E.quantised_time_surfaces(evl, None, None, None, TAU, size, t_refs),
                                   E.quantised_time_surfaces(evr, None, None, None, TAU, size, t_refs))))
            if nq == 1:
                vol = E.stereo_cost_volume(QL, QR, nd - 1, radius=RADIUS)
                ref = torch_volume(QL[0], QR[0], nd, RADIUS)
                same = bool(((vol[0] < 0) | (vol[0] == ref.to(torch.int32))).all())
                lines.append("    the torch form gives the kernel's costs at every admissible disparity: %s" % same)
                row("    yardstick: the cost volume in torch (pad, unfold, abs, sum), K = 1", median_ms(lambda: torch_volume(QL[0], QR[0], nd, RADIUS)))
                del vol, ref
            del QL, QR, DL, DR, res
        del evl, evr
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
