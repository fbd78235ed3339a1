"""Timings of semi-global matching (event_utils_amd.depth.sgm; evk_sgm.hip) at 640x480 with 64 disparities and at 346x260 with 32,
radius 3, one and sixteen queries, on the scene of tools/stereo_time.py (two streams of about 10 M events, tau = 10 ms, the queries
spread over the last 15 ms).  Per case: sgm_aggregate with eight and with four paths on the scene's cost volume, match_cost_volume on
the aggregated volume with and without the left-right test, and the whole sgm_disparity call on the two streams.  Beside them three
yardsticks: stereo_cost_volume at the same shape (the aggregation reads that volume at least once per direction), stereo_match at
the same shape, and the same aggregation written in torch on the device (vectorised over all the lines of a direction, one step per
pixel along the path: what a user would write without the kernel); its result is compared with the kernel's, bit for bit.  Every
timed repetition synchronises before and after; the median is reported.  No time here is a pass / fail criterion.
usage: timeout 900 python tools/sgm_time.py [--quick] [--out profiles/sgm_time.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from stereo_time import ACTIVITY, CASES, DURATION, N_EVENTS, QUERIES, RADIUS, TAU, scene  # noqa: E402

P1, P2 = 784, 6272                                         # 16 and 128 a pixel of the 7 x 7 window
INF = 1 << 30


def torch_aggregate(vol, p1, p2, directions):
    """sgm_aggregate in torch: (K, D, H, W) int32 in, the same out.  A direction with dy = 0 steps along x with the state
    (K, D, H); any other steps along y with the state (K, D, W), the row before shifted by dx."""
    import torch
    import torch.nn.functional as F
    pres = vol >= 0
    C = vol.clamp(max=1 << 22)
    S = torch.zeros_like(vol)
    for dx, dy in directions:
        axis = 3 if dy == 0 else 2
        n = vol.shape[axis]
        order = range(n) if (dx if dy == 0 else dy) > 0 else range(n - 1, -1, -1)
        prev = None
        for t in order:
            c, p = C.select(axis, t), pres.select(axis, t)
            L = c
            if prev is not None:
                lq = prev
                if dy != 0 and dx != 0:                     # q = (x - dx, y - dy): the row before, moved by dx
                    lq = F.pad(prev, (1, 0), value=INF)[..., :-1] if dx > 0 else F.pad(prev, (0, 1), value=INF)[..., 1:]
                m = lq.min(dim=1, keepdim=True).values
                lo = F.pad(lq, (0, 0, 1, 0), value=INF)[:, :-1]
                hi = F.pad(lq, (0, 0, 0, 1), value=INF)[:, 1:]
                step = torch.minimum(torch.minimum(lq, m + p2), torch.minimum(lo, hi) + p1)
                L = torch.where(m < INF, c + step - m, c)
            prev = torch.where(p, L, torch.full_like(L, INF))
            S.select(axis, t).add_(torch.where(p, L, torch.zeros_like(L)))
    return torch.where(pres, S, torch.full_like(S, -1))


def main():
    import torch
    import event_utils_amd as E
    from event_utils_amd.depth.sgm import DIRECTIONS
    quick = "--quick" in sys.argv
    reps = 3 if quick else 9
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "sgm_time.txt")

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

    lines.append("semi-global matching timings: radius %d, P1 %d, P2 %d, tau %g s, min_activity %d, uniqueness 10, lr_tolerance 1, sub-pixel; "
                 "median of %d; %s" % (RADIUS, P1, P2, TAU, ACTIVITY, reps, torch.cuda.get_device_name(0)))
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
            vol = E.stereo_cost_volume(QL, QR, nd - 1, radius=RADIUS)
            agg = E.sgm_aggregate(vol, P1, P2)
            res = E.match_cost_volume(agg, QL, min_activity=ACTIVITY)
            cells = nq * nd * h * w
            lines.append("  K = %d: a volume of %.0f MB; %.3f of the left pixels are candidates, %.3f valid" % (
                nq, 4 * cells / 1e6, float((res.cost >= 0).float().mean()), float(res.mask.float().mean())))
            ms = row("    sgm_aggregate, eight paths", median_ms(lambda: E.sgm_aggregate(vol, P1, P2, 8)))
            lines.append("      %.1f G cell-directions / s; %.0f GB/s over the 29 volume passes of the design" % (8 * cells / ms / 1e6, 29 * 4 * cells / ms / 1e6))
            row("    sgm_aggregate, four paths", median_ms(lambda: E.sgm_aggregate(vol, P1, P2, 4)))
            for r in ((1, 0), (0, 1), (1, 1)):
                row("    sgm_aggregate, the direction %r alone (with both transposes)" % (r,), median_ms(lambda: E.sgm_aggregate(vol, P1, P2, (r,))))
            ms = row("    match_cost_volume on the aggregated volume", median_ms(lambda: E.match_cost_volume(agg, QL, min_activity=ACTIVITY)))
            row("    match_cost_volume, no left-right test", median_ms(lambda: E.match_cost_volume(agg, QL, min_activity=ACTIVITY, lr_tolerance=None)))
            row("    match_cost_volume, every pixel a candidate (min_activity = 1 on a surface of ones)",
                median_ms(lambda: E.match_cost_volume(agg, torch.ones_like(QL), min_activity=1)))
            row("    sgm_disparity, the whole call on the two streams",
                median_ms(lambda: E.sgm_disparity(evl, evr, TAU, size, t_refs, nd - 1, P1, P2, radius=RADIUS, min_activity=ACTIVITY)))
            row("    yardstick: stereo_cost_volume", median_ms(lambda: E.stereo_cost_volume(QL, QR, nd - 1, radius=RADIUS)))
            row("    yardstick: stereo_match", median_ms(lambda: E.stereo_match(QL, QR, nd - 1, radius=RADIUS, min_activity=ACTIVITY)))
            row("    yardstick: stereo_disparity, the whole call on the two streams",
                median_ms(lambda: E.stereo_disparity(evl, evr, TAU, size, t_refs, nd - 1, radius=RADIUS, min_activity=ACTIVITY)))
            if nq == 1:
                ref = torch_aggregate(vol, P1, P2, DIRECTIONS)
                lines.append("    the torch form gives the kernel's sums bit for bit: %s" % torch.equal(ref, agg))
                row("    yardstick: the same aggregation in torch, eight paths, K = 1", median_ms(lambda: torch_aggregate(vol, P1, P2, DIRECTIONS)))
                del ref
            del QL, QR, vol, agg, res
        del evl, evr
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
