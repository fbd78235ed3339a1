"""Timings of the intensity reconstruction (event_utils_amd.representations.reconstruction; evk_reconstruct.hip) at 10 M float32
events, 640x480, on resident DeviceEvents rotated over more memory than the 256 MB Infinity Cache (the scene and the method of
tools/time_surface_time.py): the event pass alone for K = 1 and K = 4 queries, the complementary filter with F = 8 frames, and the
public calls end to end.  The yardstick stands beside them, measured in the same process on the same groupings (one class,
grouping excluded from both sides): the refractory pass (evk_denoise_refractory), which walks the same runs with the same two
dependent gathers per event (order[], then the time) and stores one byte per event.  Against it the event pass adds per event one
gathered byte, one float64 exp and a multiply-add, plus the (K, H, W) store.  Last, a stream on which one pixel holds 10 % of the
events, for the default wave_run and for 2^30 (every run walked by one lane).  Every timed repetition synchronises before and after;
the median is reported.  No time here is a pass / fail criterion.
usage: python tools/reconstruct_time.py [--quick] [--out profiles/reconstruct_time.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_surface_time import COPIES, H, N, TAU, W, scene  # noqa: E402

ALPHA = 1.0 / TAU                            # 1 / s: the time constant of the time-surface rows
REFRACTORY = 1e-3                            # seconds (tools/denoise_time.py)
HOT_SHARE = 0.10
SPAN = 0.1                                   # seconds: the window of the scene


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
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "reconstruct_time.txt")

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
    lines.append("reconstruction timings: %d float32 events, %dx%d, %d resident copies rotated (%.0f MB), median of %d, alpha %g / s, "
                 "default wave_run %d; %s" % (n, W, H, COPIES, COPIES * 16 * n / 1e6, reps, ALPHA, _lib.EVK_RECONSTRUCT_WAVE_RUN,
                                              torch.cuda.get_device_name(0)))
    size = (H, W)
    stream = D.stream()
    j = [0]

    def nxt():
        j[0] += 1
        return j[0] % COPIES

    def row(name, ms, note=""):
        lines.append("%-58s %9.3f ms%s" % (name, ms, ("   " + note) if note else ""))
        return ms

    def resident(cols):
        evs = [E.DeviceEvents.from_arrays(*cols, precision="f32") for _ in range(COPIES)]
        ins = [_In(e, None, None, None) for e in evs]
        groups = [G.Grouped(a, size, False, "reconstruct_time") for a in ins]
        flags = [(e.p > 0).to(torch.uint8) for e in evs]
        return evs, ins, groups, flags

    def event_pass(groups, flags, refs, frames=None, fts=None, wave_run=0):
        """-> a closure that runs evk_reconstruct on the next resident copy (the cuts found once, outside the timing)"""
        dev = groups[0].dev
        g = groups[0]
        keys = torch.tensor(refs, dtype=torch.float64, device=dev)
        cuts = torch.zeros(len(refs), dtype=torch.int64, device=dev)
        _lib.call("evk_searchsorted_left", D.ptr(g.t), g.t.element_size(), n, D.ptr(keys), len(refs), D.ptr(cuts), stream)
        out = torch.empty((len(refs), H, W), dtype=torch.float32, device=dev)
        nf = 0 if frames is None else int(frames.shape[0])

        def run():
            c = nxt()
            g = groups[c]
            _lib.call("evk_reconstruct", g.t_kind, D.ptr(g.t), D.ptr(flags[c]), n, H, W, ALPHA, 0.1, 0.1, 0.0, D.ptr(frames[0]) if nf else None,
                      nf, D.ptr(frames), D.ptr(fts), len(refs), D.ptr(cuts), D.ptr(keys), 0, wave_run, D.ptr(g.scratch), D.ptr(out), stream)
        return run

    cols = scene(n)
    evs, ins, groups, flags = resident(cols)
    dev = groups[0].dev
    row("grouping, one class (evk_denoise_group)", median_ms(lambda: G.Grouped(ins[nxt()], size, False, "reconstruct_time")))
    yard = row("refractory pass (evk_denoise_refractory), the yardstick", median_ms(lambda: groups[nxt()].refractory(REFRACTORY)),
               "(n bytes written)")
    refs1, refs4 = [SPAN], [0.25 * SPAN, 0.5 * SPAN, 0.75 * SPAN, SPAN]
    k1 = row("event pass, K = 1 (evk_reconstruct)", median_ms(event_pass(groups, flags, refs1)), "(%.1f MB written)" % (H * W * 4 / 1e6))
    k4 = row("event pass, K = 4 (evk_reconstruct)", median_ms(event_pass(groups, flags, refs4)), "(%.1f MB written)" % (4 * H * W * 4 / 1e6))
    lines.append("%-58s %9.2f / %.2f" % ("  event pass K = 1 / K = 4 over the refractory pass", k1 / yard, k4 / yard))
    rng = np.random.default_rng(2)
    frames = torch.from_numpy(rng.normal(size=(8, H, W))).to(dev)
    fts_host = np.linspace(0.0, SPAN, 8, endpoint=False)
    fts = torch.from_numpy(fts_host).to(dev)
    row("complementary filter, F = 8, K = 1 (evk_reconstruct)", median_ms(event_pass(groups, flags, refs1, frames, fts)))
    c4 = row("complementary filter, F = 8, K = 4 (evk_reconstruct)", median_ms(event_pass(groups, flags, refs4, frames, fts)))
    lines.append("%-58s %9.2f" % ("  complementary filter F = 8, K = 4 over the refractory pass", c4 / yard))

    ev = lambda: evs[nxt()]  # noqa: E731
    row("refractory_filter (end to end)", median_ms(lambda: E.refractory_filter(ev(), None, None, None, REFRACTORY, sensor_size=size)))
    row("leaky_integrator, K = 1 (end to end)",
        median_ms(lambda: E.leaky_integrator(ev(), None, None, None, ALPHA, sensor_size=size, t_refs=refs1)))
    row("leaky_integrator, K = 4 (end to end)",
        median_ms(lambda: E.leaky_integrator(ev(), None, None, None, ALPHA, sensor_size=size, t_refs=refs4)))
    row("complementary_filter, F = 8, K = 4 (end to end)",
        median_ms(lambda: E.complementary_filter(ev(), None, None, None, ALPHA, frames, fts_host, sensor_size=size, t_refs=refs4)))

    # one pixel holds 10 % of the events: what the wave path buys
    del evs, ins, groups, flags
    torch.cuda.empty_cache()
    hot = np.random.default_rng(3).random(n) < HOT_SHARE
    for c, v in zip(cols, (321, 123, None, 1)):
        if v is not None:
            c[hot] = v
    evs, ins, groups, flags = resident(cols)
    lines.append("a stream with %d of %d events on one pixel:" % (int(hot.sum()), n))
    few = max(3, reps // 3)
    row("  refractory pass, default wave_run", median_ms(lambda: groups[nxt()].refractory(REFRACTORY), few))
    row("  event pass, K = 4, default wave_run", median_ms(event_pass(groups, flags, refs4), few))
    row("  event pass, K = 4, wave_run 2^30 (lanes only)", median_ms(event_pass(groups, flags, refs4, wave_run=1 << 30), few))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
