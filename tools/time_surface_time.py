"""Timings of the time-surface passes (event_utils_amd.representations.time_surface; evk_tsurf.hip) at 10 M float32 events, 640x480,
on resident DeviceEvents rotated over more memory than the 256 MB Infinity Cache (as tools/denoise_time.py does): the grouping, the
surface of active events for K = 1 and 8 queries, the local surfaces at r = 1 and 3 over all events and over a selection of 1 M,
and the HATS histograms at cell 10, r = 3.  Every pass stands beside the bytes it writes and the store rate that makes, the local
pass also beside evk_denoise_support at the same radius in pixel order (the same searches without the stores), measured in the
same process.  Every timed repetition synchronises before and after; the median is reported.  No time here is a pass / fail
criterion.
usage: python tools/time_surface_time.py [--quick] [--out profiles/time_surface_time.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W = 10_000_000, 480, 640
COPIES = 6
TAU, DT = 5e-3, 2e-3                         # seconds, on a 0.1 s window
SELECT = 1_000_000


def scene(n):
    """Uniform noise plus a vertical edge sweeping the sensor; microsecond time stamps on a 0.1 s window (tools/denoise_time.py)."""
    rng = np.random.default_rng(0)
    t = np.sort(rng.integers(0, 100_000, n)).astype(np.float64) * 1e-6
    noise = rng.random(n) < 0.5
    x = np.where(noise, rng.integers(0, W, n), np.minimum(W - 1, (t / 0.1 * W).astype(np.int64)))
    y = rng.integers(0, H, n)
    p = rng.integers(0, 2, n) * 2 - 1
    return [a.astype(np.float32) for a in (x, y, t, p)]


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
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "time_surface_time.txt")

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
    lines.append("time-surface timings: %d float32 events, %dx%d, %d resident copies rotated (%.0f MB), median of %d, tau %g s, dt %g s; %s"
                 % (n, W, H, COPIES, COPIES * 16 * n / 1e6, reps, TAU, DT, torch.cuda.get_device_name(0)))
    cols = scene(n)
    evs = [E.DeviceEvents.from_arrays(*cols, precision="f32") for _ in range(COPIES)]
    ins = [_In(e, None, None, None) for e in evs]
    size = (H, W)
    j = [0]

    def nxt():
        j[0] += 1
        return j[0] % COPIES

    def row(name, ms, nbytes=None, note=""):
        rate = "" if nbytes is None else "  %9.1f MB written  %7.1f GB/s" % (nbytes / 1e6, nbytes / ms / 1e6)
        lines.append("%-44s %9.3f ms%s%s" % (name, ms, rate, ("   " + note) if note else ""))

    row("grouping, two classes (evk_denoise_group)", median_ms(lambda: G.Grouped(ins[nxt()], size, True, "time_surface_time")),
        note="(coordinates to int32, classes, keys, radix sort, run table, error read-back)")
    groups = [G.Grouped(a, size, True, "time_surface_time") for a in ins]
    dev = groups[0].dev
    stream = D.stream()

    # the surface of active events
    for nq in (1, 8):
        cuts = torch.from_numpy(np.linspace(n // 8, n, nq).astype(np.int64)).to(dev)
        out = torch.empty((nq, 2, H, W), dtype=torch.float32, device=dev)

        def run(cuts=cuts, out=out, nq=nq):
            g = groups[nxt()]
            _lib.call("evk_tsurf_global", g.t_kind, D.ptr(g.t), n, H, W, 2, nq, D.ptr(cuts), None, _lib.EVK_TSURF_EXP, TAU,
                      D.ptr(g.scratch), D.ptr(out), stream)
        row("global surface, K = %d (pass)" % nq, median_ms(run), out.numel() * 4)
        row("time_surfaces, K = %d (end to end)" % nq,
            median_ms(lambda: E.time_surfaces(evs[nxt()], None, None, None, TAU, sensor_size=size, indices=cuts)))
        del out

    # the local surfaces, beside the support pass at the same radius (pixel order, own class: the same searches, no stores)
    select = torch.from_numpy(np.sort(np.random.default_rng(1).choice(n, min(SELECT, n), replace=False))).to(dev)
    for radius in (1, 3):
        pp = (2 * radius + 1) ** 2
        row("support pass r=%d, pixel order (evk_denoise)" % radius,
            median_ms(lambda: groups[nxt()].support(DT, radius, True, 1, True, _lib.EVK_DENOISE_WALK_PIXEL)), 2 * n)
        for sel, rows, label in ((None, n, "all events"), (select, int(select.shape[0]), "%d selected" % int(select.shape[0]))):
            out = torch.empty((rows, 1, 2 * radius + 1, 2 * radius + 1), dtype=torch.float32, device=dev)

            def run(sel=sel, rows=rows, out=out):
                g = groups[nxt()]
                _lib.call("evk_tsurf_local", g.t_kind, D.ptr(g.t), n, H, W, 2, radius, _lib.EVK_TSURF_EXP, TAU, 0, 1, D.ptr(sel),
                          rows, D.ptr(g.scratch), D.ptr(out), stream)
            row("local surfaces r=%d, %s (pass)" % (radius, label), median_ms(run), rows * pp * 4)
            del out
            torch.cuda.empty_cache()
        row("local_time_surfaces r=%d, %d selected (end to end)" % (radius, int(select.shape[0])),
            median_ms(lambda: E.local_time_surfaces(evs[nxt()], None, None, None, TAU, sensor_size=size, radius=radius, select=select)))

    # HATS
    cy, cx = -(-H // 10), -(-W // 10)
    out = torch.empty((cy, cx, 2, 7, 7), dtype=torch.float32, device=dev)
    counts = torch.empty((cy, cx, 2), dtype=torch.int32, device=dev)
    nbytes = int(_lib.lib().evk_tsurf_scratch_bytes(n))
    t_run = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def hats():
        g = groups[nxt()]
        _lib.call("evk_tsurf_hats", g.t_kind, D.ptr(g.t), n, H, W, 10, 3, TAU, DT, 1, D.ptr(g.scratch), D.ptr(t_run), nbytes,
                  D.ptr(out), D.ptr(counts), stream)
    row("HATS cell 10, r=3 (gather + pass)", median_ms(hats), out.numel() * 4 + counts.numel() * 4 + 8 * n,
        "(of the bytes, %.0f MB are the times gathered into run order)" % (8 * n / 1e6))
    row("averaged_time_surfaces cell 10, r=3 (end to end)",
        median_ms(lambda: E.averaged_time_surfaces(evs[nxt()], None, None, None, TAU, DT, sensor_size=size, cell_size=10, radius=3)))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
