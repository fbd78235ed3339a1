"""Timings of the event filters (event_utils_amd.util.event_util; evk_select.hip) at 10 M float32 events, 640x480, on resident
streams rotated over more memory than the 256 MB Infinity Cache (as bench.py does), against the same filters written with torch
boolean indexing on the same device tensors and the numpy restatement of tests/test_cpu_filters.py on the host.
Every timed repetition synchronises before and after; the median is reported.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats` (--quick: fewer repetitions, no host baseline).
usage: python tools/filter_time.py [--quick] [--out profiles/filter_time.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import event_utils_amd as E  # noqa: E402
from event_utils_amd import _lib  # noqa: E402
from event_utils_amd import _device as D  # noqa: E402
from test_cpu_filters import np_clip_events_to_bounds, np_get_events_from_mask, np_remove_hot_pixels  # noqa: E402

N, H, W = 10_000_000, 480, 640
COPIES = 6                                  # 6 x 160 MB of columns: every call reads its events from HBM
HBM = 8.0e12                                # bytes / s


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    quick = "--quick" in sys.argv
    reps = 5 if quick else 21
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "filter_time.txt")
    rng = np.random.default_rng(0)
    hot = [(int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(50)]
    x = rng.integers(0, W, N)
    y = rng.integers(0, H, N)
    k = rng.random(N) < 0.02
    pick = rng.integers(0, len(hot), N)
    x = np.where(k, np.array([h[0] for h in hot])[pick], x).astype(np.float32)
    y = np.where(k, np.array([h[1] for h in hot])[pick], y).astype(np.float32)
    t = np.sort(rng.uniform(0, 0.1, N)).astype(np.float32)
    p = (rng.integers(0, 2, N) * 2 - 1).astype(np.float32)
    evs = [E.DeviceEvents.from_arrays(x, y, t, p, precision="f32") for _ in range(COPIES)]
    mask = np.zeros((H, W), np.float32)
    mask[:, : W // 2] = 1.0                                   # keeps about 50 %
    mask_d = torch.from_numpy(mask).cuda()
    it = [0]

    def ev():
        it[0] += 1
        return evs[it[0] % COPIES]

    calls = {
        "remove_hot_pixels(num_hot=50)": lambda: E.remove_hot_pixels(ev(), None, None, None, (H, W), 50),
        "clip box ~50 %": lambda: E.clip_events_to_bounds(ev(), None, None, None, (0, H, 0, W // 2)),
        "clip box ~100 %": lambda: E.clip_events_to_bounds(ev(), None, None, None, (H, W)),
        "mask ~50 %": lambda: E.get_events_from_mask(mask_d, ev(), None),
    }

    def torch_hot():
        e = ev()
        xi, yi = e.x.long(), e.y.long()
        flat = yi * W + xi
        img = torch.zeros(H * W, dtype=torch.float64, device="cuda")
        img.index_put_((flat,), e.p.double(), accumulate=True)
        hm = torch.zeros(H * W, dtype=torch.bool, device="cuda")
        hm[torch.topk(img, 50).indices] = True
        keep = ~hm[flat]
        return e.x[keep], e.y[keep], e.t[keep], e.p[keep]

    def torch_box(y0, y1, x0, x1):
        e = ev()
        m = (e.x >= x0) & (e.x < x1) & (e.y >= y0) & (e.y < y1)
        return e.x[m], e.y[m], e.t[m], e.p[m]

    def torch_mask():
        e = ev()
        return torch.nonzero(mask_d[e.y.long(), e.x.long()] >= np.float32(0.01)).squeeze()

    baselines = {
        "remove_hot_pixels(num_hot=50)": torch_hot,
        "clip box ~50 %": lambda: torch_box(0, H, 0, W // 2),
        "clip box ~100 %": lambda: torch_box(0, H, 0, W),
        "mask ~50 %": torch_mask,
    }
    host = {
        "remove_hot_pixels(num_hot=50)": lambda: np_remove_hot_pixels(x.astype(np.int64), y.astype(np.int64), t, p, (H, W), 50),
        "clip box ~50 %": lambda: np_clip_events_to_bounds(x, y, t, p, (0, H, 0, W // 2)),
        "clip box ~100 %": lambda: np_clip_events_to_bounds(x, y, t, p, (H, W)),
        "mask ~50 %": lambda: np_get_events_from_mask(mask, x, y),
    }

    # the compaction alone (evk_select_compact, preallocated buffers, no read-back): box predicate, four float32 columns
    def compaction(y1, x1):
        bufs = [[torch.empty(N, dtype=torch.float32, device="cuda") for _ in range(4)] for _ in range(COPIES)]
        nbytes = int(_lib.lib().evk_select_scratch_bytes(N))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        result = torch.empty(3, dtype=torch.int64, device="cuda")
        params = np.array([0.0, float(x1), 0.0, float(y1)])
        eb = np.full(4, 4, np.int32)
        packs = []
        for e, b in zip(evs, bufs):
            src = np.array([c.data_ptr() for c in (e.x, e.y, e.t, e.p)], np.uint64)
            dst = np.array([c.data_ptr() for c in b], np.uint64)
            packs.append((e, src, dst))
        j = [0]

        def run():
            j[0] += 1
            e, src, dst = packs[j[0] % COPIES]
            _lib.call("evk_select_compact", _lib.EVK_SELECT_BOX, _lib.EVK_SELECT_F32, D.ptr(e.x), D.ptr(e.y), N, D.host_ptr(params),
                      None, 0, 0, 4, D.host_ptr(src), D.host_ptr(dst), D.host_ptr(eb), 2, None, D.ptr(result), D.ptr(scratch),
                      nbytes, None, D.stream())
        run()
        torch.cuda.synchronize()
        kept = int(result[0].item())
        return run, kept

    lines = ["filter timings: %d float32 events, %dx%d, %d resident copies rotated (%.0f MB), median of %d; %s"
             % (N, W, H, COPIES, COPIES * 16 * N / 1e6, reps, torch.cuda.get_device_name(0))]
    for name, fn in calls.items():
        fn()
        baselines[name]()
        ms = median_ms(fn, reps)
        tb = median_ms(baselines[name], reps)
        hs = "not run" if quick else "%.1f ms" % median_ms(host[name], 1)
        lines.append("%-32s event_utils_amd %8.3f ms | torch boolean indexing %8.3f ms (%.2fx) | numpy host %s"
                     % (name, ms, tb, tb / ms, hs))
    for label, (y1, x1) in (("compaction only, box ~50 %", (H, W // 2)), ("compaction only, box ~100 %", (H, W))):
        run, kept = compaction(y1, x1)
        ms = median_ms(run, reps)
        algo = 16 * N + 16 * kept                       # the four columns read (the predicate columns among them) + kept written
        lines.append("%-32s %8.3f ms (3 launches + sync), K = %d: %.0f GB/s algorithmic = %.3f of 8 TB/s"
                     % (label, ms, kept, algo / ms / 1e6, algo / ms / 1e-3 / HBM))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
