"""Timings of the event-denoising filters (event_utils_amd.util.event_denoise; evk_denoise.hip) at 10 M float32 events, 640x480,
on resident DeviceEvents rotated over more memory than the 256 MB Infinity Cache (as tools/filter_time.py does): both filters
end to end, the passes one by one (every timed repetition synchronises before and after; the median is reported),
remove_hot_pixels at the same size as the neighbouring row, and the A/B of the run length from which a wave walks a run of the
refractory pass (on the uniform scene and on one with 30 % of the events on one pixel).  Kernel times: run this under
`rocprofv3 --kernel-trace --stats` with --quick.  --host times the vectorised host restatement (tests/_denoise_np.py) instead
and needs no GPU.
usage: python tools/denoise_time.py [--quick] [--host] [--out profiles/denoise_time.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _denoise_np as NP  # noqa: E402

N, H, W = 10_000_000, 480, 640
COPIES = 6
DT, REFRACTORY = 2e-3, 1e-3                  # seconds, on a 0.1 s window
WAVE_RUNS = (64, 256, 1024, 4096, 16384, 1 << 30)


def scene(hot_share=0.0):
    """Uniform noise plus a vertical edge sweeping the sensor; microsecond time stamps on a 0.1 s window."""
    rng = np.random.default_rng(0)
    t = np.sort(rng.integers(0, 100_000, N)).astype(np.float64) * 1e-6
    noise = rng.random(N) < 0.5
    x = np.where(noise, rng.integers(0, W, N), np.minimum(W - 1, (t / 0.1 * W).astype(np.int64)))
    y = rng.integers(0, H, N)
    p = rng.integers(0, 2, N) * 2 - 1
    if hot_share:
        k = rng.random(N) < hot_share
        x[k], y[k], p[k] = 321, 123, 1
    return [a.astype(np.float32) for a in (x, y, t, p)]


def host_main():
    cols = scene()
    t0 = time.perf_counter()
    s = NP.fast_support(*cols, DT, (H, W))
    t1 = time.perf_counter()
    k = NP.fast_refractory(*cols, REFRACTORY, (H, W))
    t2 = time.perf_counter()
    print("host restatement (numpy, one thread), %d events %dx%d: fast_support r=1 %.1f s (kept %d at support 1), "
          "fast_refractory %.1f s (kept %d)" % (N, W, H, t1 - t0, int((s >= 1).sum()), t2 - t1, int(k.sum())))


def main():
    if "--host" in sys.argv:
        return host_main()
    import torch
    import event_utils_amd as E
    from event_utils_amd import _lib
    from event_utils_amd import _grouping as G
    from event_utils_amd.util.event_util import _In
    quick = "--quick" in sys.argv
    reps = 5 if quick else 15
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "denoise_time.txt")

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
    lines.append("denoise timings: %d float32 events, %dx%d, %d resident copies rotated (%.0f MB), median of %d, dt %g s, refractory %g s; %s"
             % (N, W, H, COPIES, COPIES * 16 * N / 1e6, reps, DT, REFRACTORY, torch.cuda.get_device_name(0)))
    cols = scene()
    evs = [E.DeviceEvents.from_arrays(*cols, precision="f32") for _ in range(COPIES)]
    it = [0]

    def ev():
        it[0] += 1
        return evs[it[0] % COPIES]

    size = (H, W)
    r = E.background_activity_filter(ev(), None, None, None, DT, sensor_size=size)
    lines.append("kept: background activity (r=1, support 1) %d, refractory %d of %d"
                 % (len(r), len(E.refractory_filter(ev(), None, None, None, REFRACTORY, sensor_size=size)), N))
    end_to_end = {
        "background_activity_filter r=1": lambda: E.background_activity_filter(ev(), None, None, None, DT, sensor_size=size),
        "background_activity_filter r=3": lambda: E.background_activity_filter(ev(), None, None, None, DT, sensor_size=size, radius=3),
        "refractory_filter": lambda: E.refractory_filter(ev(), None, None, None, REFRACTORY, sensor_size=size),
        "remove_hot_pixels(num_hot=50)": lambda: E.remove_hot_pixels(ev(), None, None, None, size, 50),
    }
    for name, fn in end_to_end.items():
        lines.append("%-34s end to end %8.3f ms" % (name, median_ms(fn)))

    # the passes: one grouping per resident copy, then each pass on its scratch
    groups = [G.Grouped(_In(e, None, None, None), size, False, "denoise_time") for e in evs]
    ins = [_In(e, None, None, None) for e in evs]
    j = [0]

    def nxt():
        j[0] += 1
        return j[0] % COPIES
    lines.append("%-34s %8.3f ms   (coordinates to int32 twice, keys, radix sort over %d key bits, run table, error read-back)"
                 % ("grouping (evk_denoise_group)", median_ms(lambda: G.Grouped(ins[nxt()], size, False, "denoise_time")),
                    max(8, (H * W - 1).bit_length())))
    for radius in (1, 2, 3):             # the A/B of the walk order, alternating
        for walk, wname in ((_lib.EVK_DENOISE_WALK_STREAM, "stream order"), (_lib.EVK_DENOISE_WALK_PIXEL, "pixel order")) * 2:
            lines.append("%-34s %8.3f ms" % ("support pass r=%d, %s" % (radius, wname),
                                             median_ms(lambda: groups[nxt()].support(DT, radius, False, 1, True, walk))))
    lines.append("%-34s %8.3f ms" % ("refractory pass", median_ms(lambda: groups[nxt()].refractory(REFRACTORY))))
    keeps = [g.refractory(REFRACTORY) for g in groups]

    def compaction():
        k = nxt()
        return G.kept(ins[k], keeps[k])
    lines.append("%-34s %8.3f ms   (evk_select_compact with EVK_SELECT_FLAGS, four float32 columns, result read-back)"
                 % ("compaction", median_ms(compaction)))

    lines.append("refractory pass by the run length from which a wave walks a run (A/B in one process, alternating):")
    del groups, keeps, ins, evs
    for fold, share in ((1, 0.0), (4, 0.0), (8, 0.0), (16, 0.0), (32, 0.0), (1, 0.3)):
        torch.cuda.empty_cache()
        h2, w2 = H // fold, W // fold
        c2 = scene(share)
        c2[0], c2[1] = c2[0] % w2, c2[1] % h2        # the same events folded onto a smaller sensor: longer runs
        evs = [E.DeviceEvents.from_arrays(*c2, precision="f32") for _ in range(2)]
        groups = [G.Grouped(_In(e, None, None, None), (h2, w2), False, "denoise_time") for e in evs]
        label = "%dx%d, mean run %.0f events%s" % (w2, h2, N / (h2 * w2), ", 30 % on one pixel" if share else "")
        row = []
        for rounds in range(2):                  # two interleaved rounds: the spread shows next to the difference
            for wr in WAVE_RUNS:
                g = groups[nxt() % len(groups)]
                few = 1 if (share and wr == 1 << 30) else reps      # (one thread walking 3 M events: once is enough)
                row.append((wr, rounds, median_ms(lambda: g.refractory(REFRACTORY, wr), few)))
        for wr in WAVE_RUNS:
            a, b = [ms for w, _, ms in row if w == wr]
            lines.append("  %-44s wave_run %-10s %8.3f / %8.3f ms" % (label, "never" if wr == 1 << 30 else wr, a, b))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
