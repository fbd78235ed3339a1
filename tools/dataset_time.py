"""Items per second of the event-window datasets (event_utils_amd.data_loaders.MemMapDataset, k_events windows of k = 10 000
events, B = 5): a __getitem__ loop against __getitems__ batches of 32 (what torch's DataLoader calls with num_workers=0), at
240x180 and 346x260, split (the reference's default) and combined channels, with and without RobustNorm.  The memmap scene is
synthetic (int16 xy, float64 t, uint8 p; uniform pixels).  Every timed run ends in a device synchronise; the median of REPS
runs is reported, and the bytes of the grid stores per batch (the design's floor) beside it.  RobustNorm alone on a batch
of 32 grids is also timed against the reference's own code (torch.kthvalue, clamp, min / max) on the same device tensors.
Kernel times: run this under `rocprofv3 --kernel-trace --stats`.
usage: python tools/dataset_time.py [--quick] [--out profiles/dataset_time.txt]"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from event_utils_amd.data_loaders import MemMapDataset  # noqa: E402
from event_utils_amd.data_loaders import _kernels as K  # noqa: E402

K_EVENTS, BATCH, B = 10_000, 32, 5


def scene(root, n, H, W, seed=0):
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    np.save(os.path.join(root, "t.npy"), 1.5e9 + np.sort(rng.uniform(0, 10.0, n)))
    np.save(os.path.join(root, "xy.npy"), np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.int16))
    np.save(os.path.join(root, "p.npy"), rng.integers(0, 2, n).astype(np.uint8))
    return root


def torch_robust_norm(x, low_perc=0, top_perc=95):
    """RobustNorm.__call__ of the reference (data_augmentation.py:113-146) on a device tensor: torch's own kernels."""
    def percentile(t, q):
        k = 1 + round(.01 * float(q) * (t.numel() - 1))
        return t.reshape(-1).kthvalue(k).values.item()
    t_max, t_min = percentile(x, top_perc), percentile(x, low_perc)
    if t_max == 0 and t_min == 0:
        return x
    normed = torch.clamp(x, min=t_min, max=t_max)
    return (normed - torch.min(normed)) / (torch.max(normed) + 1e-6)


def median_s(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    quick = "--quick" in sys.argv
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    reps, nbatches = (3, 2) if quick else (7, 4)
    n_items = BATCH * nbatches
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for H, W in ((180, 240), (260, 346)):
            root = scene(os.path.join(tmp, "%dx%d" % (W, H)), K_EVENTS * (n_items + 1), H, W)
            for split in (True, False):
                for norm in (False, True):
                    ds = MemMapDataset(root, transforms={'RobustNorm': {}} if norm else {},
                                       voxel_method={'method': 'k_events', 'k': K_EVENTS, 'sliding_window_w': 0},
                                       combined_voxel_channels=not split, return_frame=False, return_flow=False)
                    one = lambda: [ds[i] for i in range(n_items)]
                    many = lambda: [ds.__getitems__(range(b * BATCH, (b + 1) * BATCH)) for b in range(nbatches)]
                    one(), many()                                   # warm-up: code objects, allocator
                    s1, sb = median_s(one, reps), median_s(many, reps)
                    C = 2 * B if split else B
                    extra = {}
                    if not norm:
                        # RobustNorm alone on one batch of 32 grids: this library's two launches against the reference's code
                        # (torch.kthvalue twice, clamp, min / max) run per item by torch on the same device tensors
                        vox = torch.stack([it['voxel'] for it in ds.__getitems__(range(BATCH))])
                        ours = lambda: K.robust_norm(vox, 0, 95, batch_dims=1)
                        theirs = lambda: [torch_robust_norm(vox[k]) for k in range(BATCH)]
                        ours(), theirs()
                        extra = {"robust_norm_batch32_ms": round(median_s(ours, reps) * 1e3, 3),
                                 "torch_kthvalue_robust_norm_batch32_ms": round(median_s(theirs, reps) * 1e3, 3)}
                    rec = {"sensor": "%dx%d" % (W, H), "channels": "split" if split else "combined", "robust_norm": norm,
                           "k": K_EVENTS, "B": B, "getitem_items_per_s": round(n_items / s1, 1),
                           "getitems32_items_per_s": round(n_items / sb, 1), "speedup": round(s1 / sb, 2),
                           "batch_ms": round(sb / nbatches * 1e3, 3),
                           "grid_store_MB_per_batch": round(BATCH * C * H * W * 4 / 1e6, 1), **extra}
                    print(json.dumps(rec), flush=True)
                    lines.append(json.dumps(rec))
                    del ds
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
