"""Crossover of the dataset's voxel paths for ONE long window (event_utils_amd.data_loaders._kernels.ResidentStream): the
window kernel (evk_voxel_windows_f32, every tile streams the whole window) against the one-pass path the dataset takes from
LONG_WINDOW_EVENTS events on (pack the window's rows, then the partition + LDS-tile voxelisation), B = 5, split and combined,
at 240x180 and 346x260: for ONE window (a __getitem__) and for a batch of NB windows in one call (a __getitems__; the
window kernel fills the GPU with all of them, the one-pass path takes them one by one).  Median of REPS synchronised runs.
usage: python tools/window_crossover.py [--out profiles/window_crossover.txt]"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from event_utils_amd.data_loaders import _kernels as K  # noqa: E402

REPS, B, NB = 9, 5, 16
SIZES = (10_000, 30_000, 100_000, 200_000, 350_000, 700_000, 1_500_000)


def median_ms(fn):
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    rng = np.random.default_rng(0)
    n = max(SIZES)
    t = 1.5e9 + np.sort(rng.uniform(0, 1.0, n))
    p = rng.integers(0, 2, n).astype(np.uint8)
    lines = []
    for H, W in ((180, 240), (260, 346)):
        xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.int16)
        s = K.ResidentStream(xy=xy, ts=t, ps=p)
        for split in (True, False):
            for k in SIZES:
                res = {}
                starts = np.linspace(0, n - k, NB).astype(np.int64)
                for tag, wins in (("", [(0, k)]), ("batch%d_" % NB, [(int(a), int(a) + k) for a in starts])):
                    for name, thr in (("window_kernel_ms", 1 << 62), ("one_pass_ms", 0)):
                        K.LONG_WINDOW_EVENTS = thr
                        f = lambda: s.voxel_windows(wins, B, (H, W), split)
                        f()
                        res[tag + name] = round(median_ms(f), 4)
                rec = {"sensor": "%dx%d" % (W, H), "channels": "split" if split else "combined", "events": k, **res}
                print(json.dumps(rec), flush=True)
                lines.append(json.dumps(rec))
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
