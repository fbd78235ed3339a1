"""Timings of the event augmentation (event_utils_amd.augmentation; evk_augment.hip, the subset select of evk_select.hip) at 10 M
events (int64 x, y, p, float64 t; 640x480), on device columns rotated over more memory than the 256 MB Infinity Cache, against
the same calls written with torch (randint / randperm / stable sorts) on the same device tensors and against the reference's
algorithm restated in numpy on the host (np.random draws, np.random.choice without replacement, the structured sort of the
float64 block).  Every timed repetition synchronises before and after; the median is
reported.  Kernel times: run this under `rocprofv3 --kernel-trace --stats` (--quick: fewer repetitions, no host baseline).
usage: python tools/augment_time.py [--quick] [--out profiles/augment_time.txt]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from event_utils_amd.augmentation import event_augmentation as A  # noqa: E402

N, H, W = 10_000_000, 480, 640
COPIES = 3                                  # 3 x 320 MB of columns: every call reads its events from HBM
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


def torch_sort(x, y, t, p):
    """numpy's order of the merged block with torch: stable sorts on the int64 bit patterns, least significant field first."""
    perm = torch.arange(x.shape[0], device=x.device)
    for c in (p, y, x, t):
        perm = perm[torch.sort(c.view(torch.int64)[perm], stable=True).indices]
    return x[perm], y[perm], t[perm], p[perm]


def main():
    quick = "--quick" in sys.argv
    reps = 5 if quick else 15
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "augment_time.txt")
    rng = np.random.default_rng(0)
    x = rng.integers(0, W, N)
    y = rng.integers(0, H, N)
    t = np.sort(rng.uniform(0, 10.0, N))
    p = rng.integers(0, 2, N) * 2 - 1
    copies = [[torch.from_numpy(c).cuda() for c in (x, y, t, p)] for _ in range(COPIES)]
    it = [0]

    def cols():
        it[0] += 1
        return copies[it[0] % COPIES]

    M, R = 1_000_000, N // 2

    def torch_random(m, merged=True):
        c = cols()
        mx, my, lo, hi = c[0].max(), c[1].max(), c[2].min(), c[2].max()
        nx = (torch.rand(m, dtype=torch.float64, device="cuda") * (mx + 1)).long()
        ny = (torch.rand(m, dtype=torch.float64, device="cuda") * (my + 1)).long()
        nt = lo + (hi - lo) * torch.rand(m, dtype=torch.float64, device="cuda")
        np_ = torch.randint(0, 2, (m,), device="cuda") * 2 - 1
        parts = [nx, ny, nt, np_]
        if merged:
            parts = [torch.cat((a.double(), b.double())) for a, b in zip(parts, c)]
        return torch_sort(*[q.double() for q in parts])

    def torch_remove(k, noise=0):
        c = cols()
        idx = torch.randperm(N, device="cuda")[:N - k].sort().values
        kept = [q[idx] for q in c]
        if not noise:
            return kept
        mx, my, lo, hi = c[0].max(), c[1].max(), c[2].min(), c[2].max()
        nz = [(torch.rand(noise, dtype=torch.float64, device="cuda") * (mx + 1)).long().double(),
              (torch.rand(noise, dtype=torch.float64, device="cuda") * (my + 1)).long().double(),
              lo + (hi - lo) * torch.rand(noise, dtype=torch.float64, device="cuda"),
              (torch.randint(0, 2, (noise,), device="cuda") * 2 - 1).double()]
        return torch_sort(*[torch.cat((a.double(), b)) for a, b in zip(kept, nz)])

    def torch_correlated(m):
        c = cols()
        iters = int(m / N) + 1
        idx = torch.randperm(iters * N, device="cuda")[:m]
        e = idx % N
        xj = (torch.randn(m, dtype=torch.float64, device="cuda") * 1.5).trunc()
        yj = (torch.randn(m, dtype=torch.float64, device="cuda") * 1.5).trunc()
        nx = (c[0][e].double() + xj).clamp(0, float(c[0].max()))
        ny = (c[1][e].double() + yj).clamp(0, float(c[1].max()))
        nt = c[2][e] + 0.001 * torch.randn(m, dtype=torch.float64, device="cuda")
        return torch_sort(nx, ny, nt, c[3][e].double())

    def host_block_sort(cols):
        blk = np.stack([np.asarray(c, dtype=np.float64) for c in cols], 1)
        blk.view("i8,i8,i8,i8").sort(order=["f2"], axis=0)
        return blk

    def host_new(m):
        return (np.random.randint(x.max() + 1, size=m), np.random.randint(y.max() + 1, size=m),
                np.random.uniform(t.min(), t.max(), size=m), np.random.randint(2, size=m) * 2 - 1)

    def host_random(m, merged=True):
        new = host_new(m)
        return host_block_sort([np.concatenate((a, b)) for a, b in zip(new, (x, y, t, p))] if merged else new)

    def host_remove(k, noise=0):
        idx = np.random.choice(np.arange(N), size=N - k, replace=False)
        if not noise:
            idx.sort()
            return x[idx], y[idx], t[idx], p[idx]
        return host_block_sort([np.concatenate((c[idx], nz)) for c, nz in zip((x, y, t, p), host_new(noise))])

    def host_correlated(m):
        iters = int(m / N) + 1
        xs = np.concatenate([x + np.trunc(np.random.normal(scale=1.5, size=N)).astype(np.int64) for _ in range(iters)])
        ys = np.concatenate([y + np.trunc(np.random.normal(scale=1.5, size=N)).astype(np.int64) for _ in range(iters)])
        ts = np.concatenate([t + np.random.normal(scale=0.001, size=N) for _ in range(iters)])
        idx = np.random.choice(iters * N, size=m, replace=False)
        blk = np.stack((np.clip(xs[idx], 0, x.max()), np.clip(ys[idx], 0, y.max()), ts[idx], np.tile(p, iters)[idx]), 1)
        blk = blk.astype(np.float64)
        blk.view("i8,i8,i8,i8").sort(order=["f2"], axis=0)
        return blk

    # (name, call, torch baseline, host baseline, algorithmic bytes).  Bytes: 24 B per input event for the bounds reduction
    # (x, y, t) where the call draws random events, the 32-B events read into the result, the 32-B events written
    B = 24 * N
    calls = [
        ("add_random_events(1 M)", lambda: A.add_random_events(*cols(), M, seed=1), lambda: torch_random(M),
         lambda: host_random(M), B + 32 * N + 32 * (N + M)),
        ("add_random_events(1 M, merged=False)", lambda: A.add_random_events(*cols(), M, return_merged=False, seed=1),
         lambda: torch_random(M, merged=False), lambda: host_random(M, merged=False), B + 32 * M),
        ("add_correlated_events(1 M)", lambda: A.add_correlated_events(*cols(), M, seed=1), lambda: torch_correlated(M),
         lambda: host_correlated(M), B + 32 * M + 32 * M),
        ("remove_events(n/2, add_noise=n/10)", lambda: A.remove_events(*cols(), R, add_noise=N // 10, seed=1),
         lambda: torch_remove(R, N // 10), lambda: host_remove(R, N // 10), B + 32 * N + 32 * (N - R + N // 10)),
        ("remove_events(n/2)", lambda: A.remove_events(*cols(), R, seed=1), lambda: torch_remove(R),
         lambda: host_remove(R), 32 * N + 32 * (N - R)),
    ]
    lines = ["augmentation timings: %d events (int64 x, y, p; float64 t), %dx%d, %d resident copies rotated (%.0f MB), median "
             "of %d; %s" % (N, W, H, COPIES, COPIES * 32 * N / 1e6, reps, torch.cuda.get_device_name(0))]
    for name, fn, tb_fn, host_fn, algo in calls:
        fn()
        tb_fn()
        ms = median_ms(fn, reps)
        tb = median_ms(tb_fn, reps)
        if quick:
            hs = "host not run"
        else:
            h = median_ms(host_fn, 1)
            hs = "host numpy (reference algorithm) %.0f ms (%.0fx)" % (h, h / ms)
        lines.append("%-38s %8.3f ms | %5.2f GB algorithmic, %.3f of 8 TB/s | torch %8.3f ms (%.2fx) | %s"
                     % (name, ms, algo / 1e9, algo / ms / 1e-3 / HBM, tb, tb / ms, hs))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
