"""GPU: 40 seeded random calibrations against the restatement (tests/_camera_np.py), compared as tests/test_gpu_camera.py compares:
model, coefficients, a rotation of up to five degrees, sensor and output size, event count, mode and input kind are drawn per case.
`none` and `radtan`: the device-built maps are the restatement's bits, and events and images go through them.  `equidistant`: the
flags are equal and the coordinates within 1e-9 px, and events and images go through the restatement's maps, so that they are exact
too."""
import numpy as np
import pytest
import torch

import _camera_np as N
from test_gpu_camera import BOUND, check_events, events_for, same_bits, same_flags

pytestmark = pytest.mark.gpu

KINDS = (("numpy", np.int16), ("numpy", np.int64), ("numpy", np.float32), ("tensors", np.int32), ("tensors", np.float64), ("events_f64", np.float64),
         ("events_f32", np.float32))


def draw(seed):
    rng = np.random.default_rng(1000 + seed)
    model = ("none", "radtan", "equidistant")[seed % 3]
    size = (int(rng.integers(1, 90)), int(rng.integers(1, 300)))
    out = (max(1, size[0] + int(rng.integers(-8, 9))), max(1, size[1] + int(rng.integers(-8, 9))))
    f = rng.uniform(0.7, 1.6) * max(size[0], size[1], 16)
    K = np.array([[f, 0.0, (size[1] - 1) / 2 + rng.uniform(-2, 2)], [0.0, f * rng.uniform(0.95, 1.05), (size[0] - 1) / 2 + rng.uniform(-2, 2)],
                  [0.0, 0.0, 1.0]])
    # small enough that the fixed point converges on most of the sensor: |k1| r^2 stays below 0.2 at the corner (r < 0.8)
    dist = {"none": None,
            "radtan": tuple(rng.uniform(-1, 1, 5) * (0.3, 0.1, 0.003, 0.003, 0.03))[:int(rng.integers(4, 6))],
            "equidistant": tuple(rng.uniform(-1, 1, 4) * (0.1, 0.03, 0.01, 0.003))}[model]
    om = rng.normal(size=3)
    om *= np.radians(rng.uniform(0.0, 5.0)) / np.linalg.norm(om)
    new_K = np.array([[f * rng.uniform(0.8, 1.1), 0.0, (out[1] - 1) / 2], [0.0, f * rng.uniform(0.8, 1.1), (out[0] - 1) / 2], [0.0, 0.0, 1.0]])
    n = int(rng.choice((0, 1, 100, 4096, 4097, 9000, int(rng.integers(2, 20000)))))
    return dict(rng=rng, model=model, size=size, out=out, K=K, dist=dist, R=N.rodrigues(om), new_K=new_K, n=n,
                mode=("nearest", "subpixel")[int(rng.integers(0, 2))], kind=KINDS[int(rng.integers(0, len(KINDS)))],
                interpolation=("nearest", "bilinear")[int(rng.integers(0, 2))], dtype=(np.uint8, np.float32, np.float64)[int(rng.integers(0, 3))],
                iterations=int(rng.integers(8, 30)))


@pytest.mark.parametrize("seed", range(40))
def test_fuzz(seed):
    import event_utils_amd as E
    c = draw(seed)
    rng, model, size, out = c["rng"], c["model"], c["size"], c["out"]
    d = N.coefficients(model, c["dist"])
    want = N.maps(c["K"], model, d, size, c["R"], c["new_K"], out, c["iterations"])
    assert want[1].mean() >= 0.5, "the restatement converges on less than half of the sensor"
    cam = E.CameraModel(c["K"], c["dist"], model, size)
    maps = E.rectification_maps(cam, c["R"], c["new_K"], out, iterations=c["iterations"])
    same_flags(maps.forward_valid, want[1], "forward flags")
    same_flags(maps.inverse_valid, want[3], "inverse flags")
    if model == "equidistant":
        for got, ref, rv in ((maps.forward, want[0], want[1]), (maps.inverse, want[2], want[3])):
            g = got.cpu().numpy()
            assert np.isnan(g[:, ~rv]).all() and (not rv.any() or np.abs(g[:, rv] - ref[:, rv]).max() <= BOUND)
        maps = E.RectificationMaps.from_tensors(cam, want[0], want[2], want[1], want[3], c["new_K"])
    else:
        same_bits(maps.forward, want[0], "forward")
        same_bits(maps.inverse, want[2], "inverse")
    kind, dtype = c["kind"]
    cols = events_for(rng, size, c["n"], dtype)
    check_events(E, cols, kind, maps, want, out, c["mode"], "seed %d %s" % (seed, {k: v for k, v in c.items() if k != "rng"}))
    shape = (int(rng.integers(0, 4)),) + size
    img = rng.integers(0, 256, shape).astype(c["dtype"]) if c["dtype"] == np.uint8 else rng.normal(0.0, 50.0, shape).astype(c["dtype"])
    fill = float(rng.choice((0.0, 2.5, -1.0, 255.5)))
    got = E.remap_images(torch.from_numpy(img).cuda(), maps, c["interpolation"], fill)
    ref = N.remap(img, want[2], want[3], c["interpolation"], fill)
    assert got.is_cuda and tuple(got.shape) == ref.shape and np.array_equal(got.cpu().numpy().view(np.uint8), ref.view(np.uint8))
