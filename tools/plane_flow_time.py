"""Timings of the plane-fit flow passes (event_utils_amd.features.plane_flow; evk_planeflow.hip) at 10 M float32 events, 640x480,
on resident DeviceEvents rotated over more memory than the 256 MB Infinity Cache (the scene and the method of
tools/time_surface_time.py and tools/corner_time.py): the fit pass for r = 1 .. 4 with and without rejection, the fit over a
selection of 1 M, the field pass, and the public calls end to end.  The yardstick stands beside them, measured in the same process
on the same groupings (two classes): evk_corner_harris with the time window, 80 look-ups per event with the two dependent gathers
(order[], then the time) that the fit at r = 4 makes as well.  Every timed repetition synchronises before and after; the median is
reported.  No time here is a pass / fail criterion.
usage: python tools/plane_flow_time.py [--quick] [--out profiles/plane_flow_time.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_surface_time import COPIES, DT, H, N, SELECT, W, scene  # noqa: E402

TH = 5e-4                                    # seconds: the outlier threshold of the rows "with rejection" (two rounds)
ROUNDS = 2


def main():
    import torch
    import event_utils_amd as E
    from event_utils_amd import _device as D
    from event_utils_amd import _lib
    from event_utils_amd import _grouping as G
    from event_utils_amd.util.event_util import _In
    quick = "--quick" in sys.argv
    n = N // 10 if quick else N
    reps = 5 if quick else 15
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "plane_flow_time.txt")

    def median_ms(fn):
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
    lines.append("plane-fit flow timings: %d float32 events, %dx%d, %d resident copies rotated (%.0f MB), median of %d, dt %g s, "
                 "threshold %g s, %d rounds; %s" % (n, W, H, COPIES, COPIES * 16 * n / 1e6, reps, DT, TH, ROUNDS,
                                                    torch.cuda.get_device_name(0)))
    cols = scene(n)
    evs = [E.DeviceEvents.from_arrays(*cols, precision="f32") for _ in range(COPIES)]
    ins = [_In(e, None, None, None) for e in evs]
    size = (H, W)
    j = [0]

    def nxt():
        j[0] += 1
        return j[0] % COPIES

    def row(name, ms, note=""):
        lines.append("%-52s %9.3f ms%s" % (name, ms, ("   " + note) if note else ""))
        return ms

    row("grouping, two classes (evk_denoise_group)", median_ms(lambda: G.Grouped(ins[nxt()], size, True, "plane_flow_time")))
    groups = [G.Grouped(a, size, True, "plane_flow_time") for a in ins]
    dev = groups[0].dev
    stream = D.stream()
    select = torch.from_numpy(np.sort(np.random.default_rng(1).choice(n, min(SELECT, n), replace=False))).to(dev)
    m = int(select.shape[0])
    scores = torch.empty(n, dtype=torch.float32, device=dev)
    flow = torch.empty((n, 2), dtype=torch.float32, device=dev)
    life = torch.empty(n, dtype=torch.float32, device=dev)
    valid = torch.empty(n, dtype=torch.uint8, device=dev)
    field = torch.empty((2, H, W), dtype=torch.float32, device=dev)
    count = torch.empty((H, W), dtype=torch.int32, device=dev)

    def harris():
        g = groups[nxt()]
        _lib.call("evk_corner_harris", g.t_kind, D.ptr(g.t), n, H, W, 2, _lib.EVK_CORNER_WINDOW_TIME, 1, DT, 0.04, None, n,
                  D.ptr(g.scratch), D.ptr(scores), stream)

    def fit(r, reject, sel=None, rows=n):
        g = groups[nxt()]
        _lib.call("evk_planeflow_fit", g.t_kind, D.ptr(g.t), n, H, W, 2, r, DT, 5, 1 if reject else 0, TH if reject else 0.0, ROUNDS,
                  0, 0.0, D.ptr(sel), rows, D.ptr(g.scratch), D.ptr(flow), D.ptr(life), D.ptr(valid), stream)

    def to_field():
        g = groups[nxt()]
        _lib.call("evk_planeflow_field", n, H, W, 2, D.ptr(g.scratch), D.ptr(flow), D.ptr(valid), D.ptr(field), D.ptr(count), stream)

    yard = row("Harris dt, all events (pass), 80 look-ups", median_ms(harris))
    plain = {}
    for r in (1, 2, 3, 4):
        looks = (2 * r + 1) ** 2 - 1
        plain[r] = row("fit r=%d, no rejection (pass), %d look-ups" % (r, looks), median_ms(lambda: fit(r, False)))
        fit(r, False)
        ok = int(valid.sum().item())
        row("fit r=%d, with rejection (pass)" % r, median_ms(lambda: fit(r, True)))
        fit(r, True)
        lines.append("  valid fits at r=%d: %d without, %d with rejection, of %d" % (r, ok, int(valid.sum().item()), n))
    lines.append("%-52s %9.3f      (target: at most 1.25)" % ("  fit r=4 no rejection / Harris dt", plain[4] / yard))
    row("fit r=2, no rejection, %d selected (pass)" % m, median_ms(lambda: fit(2, False, select, m)))
    row("fit r=4, no rejection, %d selected (pass)" % m, median_ms(lambda: fit(4, False, select, m)))
    fit(2, True)
    row("field pass (evk_planeflow_field), flows of r=2", median_ms(to_field))

    ev = lambda: evs[nxt()]  # noqa: E731
    for r in (1, 2, 3, 4):
        row("local_plane_flow r=%d (end to end)" % r,
            median_ms(lambda: E.local_plane_flow(ev(), None, None, None, DT, sensor_size=size, radius=r)))
        row("local_plane_flow r=%d, with rejection (end to end)" % r,
            median_ms(lambda: E.local_plane_flow(ev(), None, None, None, DT, sensor_size=size, radius=r, outlier_threshold=TH,
                                                 iterations=ROUNDS)))
    row("local_plane_flow r=2, %d selected (end to end)" % m,
        median_ms(lambda: E.local_plane_flow(ev(), None, None, None, DT, sensor_size=size, select=select)))
    row("plane_flow_field r=2, with rejection (end to end)",
        median_ms(lambda: E.plane_flow_field(ev(), None, None, None, DT, sensor_size=size, outlier_threshold=TH, iterations=ROUNDS)))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
