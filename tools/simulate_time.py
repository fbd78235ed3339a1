"""Timings of the event simulator (event_utils_amd.simulation.event_simulator; evk_simulate.hip) at 640x480, F = 32 log-intensity
frames of a moving textured scene sized to give on the order of 10 M events (the actual count is printed): the count pass, the emit
pass, the sort plus gather, and the public call end to end on device frames.  The frames are resident copies rotated over more
memory than the 256 MB Infinity Cache.  Beside each time stand the bytes the pass must move -- 8 F H W read per walk, 12 B of (key,
value) written per event by the emit pass, 24 B per event and 8-bit digit moved by the radix sort plus 8 B per event for its
histograms, 12 B read and 32 B written per event by the gather -- and the rate that makes of the time; last, the share of the call
that is the sort.  Every timed repetition synchronises before and after; the median is reported.  No time here is a pass / fail
criterion.
usage: timeout 600 python tools/simulate_time.py [--quick] [--out profiles/simulate_time.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, F = 480, 640, 32
COPIES = 4                                   # 4 x 78.6 MB of frames
C_ON = C_OFF = 0.2
TARGET = 10_000_000
DT = 1.0e3                                   # microseconds between frames, starting at 1e6


def scene(f, h, w, amplitude):
    """(f, h, w) float64 log frames: three sinusoidal gratings drifting in different directions (a moving textured scene)"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    frames = np.empty((f, h, w))
    for k in range(f):
        frames[k] = amplitude * (np.sin(0.11 * (x - 2.3 * k) + 0.05 * y) + np.sin(0.07 * (y + 1.9 * k) - 0.03 * x + 1.0) +
                                 0.5 * np.sin(0.23 * (x + y - 3.1 * k) + 2.0))
    return frames


def main():
    import torch
    import event_utils_amd as E
    from event_utils_amd import _device as D
    from event_utils_amd import _lib
    quick = "--quick" in sys.argv
    h, w = (H // 4, W // 4) if quick else (H, W)
    reps = 5 if quick else 15
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "simulate_time.txt")
    target = TARGET // 16 if quick else TARGET

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

    # the amplitude that gives about `target` crossings: a pixel-interval has about |d| / c of them, less the part of a contrast
    # that each change of direction leaves over (a factor of 0.83 on this scene)
    unit = scene(F, h, w, 1.0)
    amplitude = target / 0.83 * C_ON / float(np.abs(np.diff(unit, axis=0)).sum())
    host_frames = unit * amplitude
    fts = 1.0e6 + DT * np.arange(F)
    dev = D.require_gpu()
    frames = [torch.from_numpy(host_frames).to(dev) for _ in range(COPIES)]
    dfts = torch.from_numpy(fts).to(dev)
    j = [0]

    def nxt():
        j[0] += 1
        return frames[j[0] % COPIES]

    xs, ys, ts, ps, state = E.simulate_events(frames[0], fts, C_ON, C_OFF, return_state=True)
    total = int(ts.shape[0])
    per_pixel = torch.bincount(ys * w + xs, minlength=h * w)
    assert bool((ts[1:] >= ts[:-1]).all()) and float(ts[0]) >= fts[0] and float(ts[-1]) <= fts[-1]
    lines = Lines()
    lines.append("simulator timings: %dx%d, F = %d float64 log frames (%.1f MB, %d resident copies rotated), c_on = c_off = %g, "
                 "refractory 0: %d events, %.1f per pixel on average, at most %d; median of %d; %s"
                 % (w, h, F, 8 * F * h * w / 1e6, COPIES, C_ON, total, total / (h * w), int(per_pixel.max()), reps,
                    torch.cuda.get_device_name(0)))
    del xs, ys, ts, ps, per_pixel
    stream = D.stream()
    t_first, t_max = float(fts[0]), float(np.max(fts[:-1] + (fts[1:] - fts[:-1])))
    counts = torch.empty(h * w, dtype=torch.int32, device=dev)
    report = torch.empty(2, dtype=torch.int64, device=dev)

    def head(fr):
        return (D.ptr(fr), D.ptr(dfts), F, h, w, C_ON, C_OFF, None, None, 0.0, None, None)

    def count():
        _lib.call("evk_simulate_count", *head(nxt()), D.ptr(counts), D.ptr(report), stream)
    count()
    c64 = counts.to(torch.int64)
    offsets = torch.cumsum(c64, 0) - c64
    assert int(c64.sum()) == total and not report.any()
    keys = torch.empty(total, dtype=torch.int64, device=dev)
    vals = torch.empty(total, dtype=torch.int32, device=dev)
    r_out, tl_out = (torch.empty((h, w), dtype=torch.float64, device=dev) for _ in range(2))

    def emit():
        _lib.call("evk_simulate_emit", *head(nxt()), D.ptr(offsets), total, t_first, 0, D.ptr(keys), D.ptr(vals), D.ptr(r_out),
                  D.ptr(tl_out), stream)
    nbytes = int(_lib.lib().evk_simulate_sort_scratch_bytes(total, h, w, 0, t_first, t_max))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cols = [torch.empty(total, dtype=torch.int64 if k != 2 else torch.float64, device=dev) for k in range(4)]

    def sort():
        _lib.call("evk_simulate_sort", D.ptr(keys), D.ptr(vals), total, h, w, 0, t_first, t_max, D.ptr(scratch), nbytes,
                  *(D.ptr(c) for c in cols), stream)
    key_bits = max(8, int(np.float64(t_max).view(np.uint64) - np.float64(t_first).view(np.uint64)).bit_length())      # (positive times)
    digits = -(-key_bits // 8)
    walk_mb = 8 * F * h * w / 1e6

    def row(name, ms, mb=None):
        lines.append("%-46s %9.3f ms%s" % (name, ms, "" if mb is None else "   %8.1f MB to move, %6.0f GB/s" % (mb, mb / ms)))
        return ms
    t_count = row("count pass (evk_simulate_count)", median_ms(count), walk_mb + 4 * h * w / 1e6)
    t_emit = row("emit pass (evk_simulate_emit)", median_ms(emit), walk_mb + (8 * h * w + 12 * total + 16 * h * w) / 1e6)
    t_sort = row("sort plus gather (evk_simulate_sort)", median_ms(sort), ((24 * digits + 8) * total + 44 * total) / 1e6)
    lines.append("  the sort key spans %d bits: %d digits of 8 bits" % (key_bits, digits))
    row("scan and read-back (torch.cumsum, one .tolist())",
               median_ms(lambda: torch.cat((torch.cumsum(counts.to(torch.int64) & 0xFFFFFFFF, 0)[-1:], report)).tolist()))
    call = row("simulate_events (end to end, device frames)", median_ms(lambda: E.simulate_events(nxt(), fts, C_ON, C_OFF, return_state=True)))
    lines.append("%-46s %9.2f" % ("  sort plus gather over the whole call", t_sort / call))
    lines.append("  (each pass above is timed with a synchronise of its own, the call with one: %.3f ms for the three passes)"
                 % (t_count + t_emit + t_sort))
    lines.append("%-46s %9.1f M events / s" % ("  events per second of the whole call", total / call / 1e3))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
