"""Timings of the corner passes (event_utils_amd.features.corners; evk_corner.hip) at 10 M float32 events, 640x480, on resident
DeviceEvents rotated over more memory than the 256 MB Infinity Cache (the scene and the method of tools/time_surface_time.py): the
eFAST pass and the Harris pass for both windows, over all events and over a selection of 1 M, and the public calls end to end.
The yardstick stands beside them, measured in the same process on the same groupings (two classes): evk_denoise_support at r = 3
in pixel order, 49 look-ups per event from one thread.  Every timed repetition synchronises before and after; the median is
reported.  No time here is a pass / fail criterion.
usage: python tools/corner_time.py [--quick] [--out profiles/corner_time.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_surface_time import COPIES, DT, H, N, SELECT, W, scene  # noqa: E402

N_LAST = 2000                                # events: with 10 M events in 0.1 s about 20 us of the stream


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
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "corner_time.txt")

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
    lines.append("corner timings: %d float32 events, %dx%d, %d resident copies rotated (%.0f MB), median of %d, n_last %d, dt %g s; %s"
                 % (n, W, H, COPIES, COPIES * 16 * n / 1e6, reps, N_LAST, DT, torch.cuda.get_device_name(0)))
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

    row("grouping, two classes (evk_denoise_group)", median_ms(lambda: G.Grouped(ins[nxt()], size, True, "corner_time")))
    groups = [G.Grouped(a, size, True, "corner_time") for a in ins]
    dev = groups[0].dev
    stream = D.stream()
    select = torch.from_numpy(np.sort(np.random.default_rng(1).choice(n, min(SELECT, n), replace=False))).to(dev)
    m = int(select.shape[0])

    support = row("support pass r=3, pixel order (evk_denoise), 49 look-ups",
                  median_ms(lambda: groups[nxt()].support(DT, 3, True, 1, True, _lib.EVK_DENOISE_WALK_PIXEL)))
    flags = torch.empty(n, dtype=torch.uint8, device=dev)
    scores = torch.empty(n, dtype=torch.float32, device=dev)

    def fast(sel, rows):
        g = groups[nxt()]
        _lib.call("evk_corner_fast", g.t_kind, D.ptr(g.t), n, H, W, 2, D.ptr(sel), rows, D.ptr(g.scratch), D.ptr(flags), stream)

    def harris(window, sel, rows):
        g = groups[nxt()]
        _lib.call("evk_corner_harris", g.t_kind, D.ptr(g.t), n, H, W, 2, window, N_LAST, DT, 0.04, D.ptr(sel), rows,
                  D.ptr(g.scratch), D.ptr(scores), stream)

    fast_all = row("eFAST, all events (pass), 36 look-ups", median_ms(lambda: fast(None, n)))
    lines.append("%-52s %9.3f      (target: at most 1.25)" % ("  eFAST / support pass", fast_all / support))
    row("eFAST, %d selected (pass)" % m, median_ms(lambda: fast(select, m)))
    for window, label in ((_lib.EVK_CORNER_WINDOW_COUNT, "n_last"), (_lib.EVK_CORNER_WINDOW_TIME, "dt")):
        ms = row("Harris %s, all events (pass), 80 look-ups" % label, median_ms(lambda: harris(window, None, n)))
        lines.append("%-52s %9.3f" % ("  Harris %s / support pass" % label, ms / support))
        row("Harris %s, %d selected (pass)" % (label, m), median_ms(lambda: harris(window, select, m)))
    fast(None, n)
    lines.append("eFAST corners in the scene: %d of %d" % (int(flags.sum().item()), n))

    ev = lambda: evs[nxt()]  # noqa: E731
    row("fast_corners (end to end)", median_ms(lambda: E.fast_corners(ev(), None, None, None, sensor_size=size)))
    row("fast_corners, %d selected (end to end)" % m, median_ms(lambda: E.fast_corners(ev(), None, None, None, sensor_size=size, select=select)))
    row("harris_scores n_last (end to end)", median_ms(lambda: E.harris_scores(ev(), None, None, None, sensor_size=size, n_last=N_LAST)))
    row("harris_scores dt (end to end)", median_ms(lambda: E.harris_scores(ev(), None, None, None, sensor_size=size, dt=DT)))
    row("harris_corners dt, %d selected (end to end)" % m,
        median_ms(lambda: E.harris_corners(ev(), None, None, None, sensor_size=size, dt=DT, select=select)))
    row("corner_events fast, with indices (end to end)",
        median_ms(lambda: E.corner_events(ev(), None, None, None, detector="fast", sensor_size=size, return_index=True)))
    row("corner_events harris dt, with indices (end to end)",
        median_ms(lambda: E.corner_events(ev(), None, None, None, detector="harris", dt=DT, sensor_size=size, return_index=True)))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
