"""Timings of camera calibration (event_utils_amd.calibration.camera; evk_camera.hip) at 640x480 and on the 10 M-event resident
stream the other tools use (float32 DeviceEvents, rotated over more memory than the 256 MB Infinity Cache): both map builds for each
lens model, rectify_events in both modes, remap_images on 1 and 16 uint8 surfaces and on one float32 frame; beside them two
yardsticks: clip_events_to_bounds on the same stream (the same compaction without the gather) and the torch form of rectify_events
(index the map with ys, xs, round, mask, boolean-index four columns).  Every timed repetition synchronises before and after; the
median of 9 is reported.  Kernel times: run this under `rocprofv3 --kernel-trace --stats`.
usage: python tools/camera_time.py [--out profiles/camera_time.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W = 10_000_000, 480, 640
COPIES = 6
REPS = 9
K = np.array([[420.0, 0.0, 318.5], [0.0, 421.0, 241.3], [0.0, 0.0, 1.0]])
LENSES = (("none", None), ("radtan", (-0.31, 0.11, 0.0008, -0.0005, -0.02)), ("equidistant", (-0.048, 0.0113, -0.0489, 0.0339)))
OM = np.radians([0.4, -0.7, 0.3])


def scene():
    """Uniform noise plus a vertical edge sweeping the sensor; microsecond time stamps on a 0.1 s window (tools/denoise_time.py)."""
    rng = np.random.default_rng(0)
    t = np.sort(rng.integers(0, 100_000, N)).astype(np.float64) * 1e-6
    noise = rng.random(N) < 0.5
    x = np.where(noise, rng.integers(0, W, N), np.minimum(W - 1, (t / 0.1 * W).astype(np.int64)))
    y = rng.integers(0, H, N)
    p = rng.integers(0, 2, N) * 2 - 1
    return [a.astype(np.float32) for a in (x, y, t, p)]


def rotation(om):
    th = float(np.sqrt(om @ om))
    k = om / th
    kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * kx + (1.0 - np.cos(th)) * (kx @ kx)


def main():
    import torch
    import event_utils_amd as E
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "camera_time.txt")

    def median_ms(fn):
        fn()
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say("camera timings: %dx%d, %d float32 events, %d resident copies rotated (%.0f MB), median of %d synchronised repetitions; %s"
        % (W, H, N, COPIES, COPIES * 16 * N / 1e6, REPS, torch.cuda.get_device_name(0)))
    R = rotation(OM)
    maps = {}
    for model, dist in LENSES:
        cam = E.CameraModel(K, dist, model, (H, W))
        maps[model] = E.rectification_maps(cam, R)
        say("%-44s %8.3f ms   (forward valid %.4f, inverse valid %.4f)" % (
            "rectification_maps %s (both maps)" % model, median_ms(lambda: E.rectification_maps(cam, R)),
            float(maps[model].forward_valid.double().mean()), float(maps[model].inverse_valid.double().mean())))
    m = maps["radtan"]
    cols = scene()
    evs = [E.DeviceEvents.from_arrays(*cols, precision="f32") for _ in range(COPIES)]
    it = [0]

    def ev():
        it[0] += 1
        return evs[it[0] % COPIES]
    for mode in ("nearest", "subpixel"):
        kept = len(E.rectify_events(ev(), None, None, None, m, mode=mode))
        say("%-44s %8.3f ms   (kept %d of %d)" % ("rectify_events %s" % mode, median_ms(lambda: E.rectify_events(ev(), None, None, None, m, mode=mode)),
                                                  kept, N))
    say("%-44s %8.3f ms   (yardstick: the same compaction, no gather; kept %d)" % (
        "clip_events_to_bounds", median_ms(lambda: E.clip_events_to_bounds(ev(), None, None, None, (H - 8, W - 8))),
        len(E.clip_events_to_bounds(ev(), None, None, None, (H - 8, W - 8)))))

    def torch_form():
        e = ev()
        xi, yi = e.x.long(), e.y.long()
        u, v = torch.round(m.forward[0][yi, xi]), torch.round(m.forward[1][yi, xi])
        keep = m.forward_valid[yi, xi] & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        return u[keep].float(), v[keep].float(), e.t[keep], e.p[keep]
    say("%-44s %8.3f ms   (yardstick: index, round, mask, boolean-index four columns; kept %d)" % ("torch form of rectify_events nearest",
                                                                                                  median_ms(torch_form), len(torch_form()[0])))
    del evs
    torch.cuda.empty_cache()
    rng = np.random.default_rng(1)
    for name, img in (("1 uint8 surface", torch.from_numpy(rng.integers(0, 256, (1, H, W)).astype(np.uint8)).cuda()),
                      ("16 uint8 surfaces", torch.from_numpy(rng.integers(0, 256, (16, H, W)).astype(np.uint8)).cuda()),
                      ("1 float32 frame", torch.from_numpy(rng.random((H, W)).astype(np.float32)).cuda())):
        for interpolation in ("nearest", "bilinear"):
            say("%-44s %8.3f ms" % ("remap_images %s, %s" % (name, interpolation), median_ms(lambda: E.remap_images(img, m, interpolation))))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
