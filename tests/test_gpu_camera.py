"""GPU: camera calibration (event_utils_amd/calibration/camera.py, evk_camera.hip) against its restatement (tests/_camera_np.py).
`none` and `radtan`: distort_points, undistort_points and both maps are the restatement's bits, valid flags included.  `equidistant`:
the flags are equal and the coordinates lie within 1e-9 px (the device's atan and tan are not numpy's; the bound is the one
tests/test_cpu_camera.py derives and checks the reference against).  rectify_events and remap_images on maps supplied from the
restatement are exact for every model; on device-built maps the seeded raw stereo scene goes through both rectifications into the
matcher and gives the restatement pipeline's Disparity bit for bit."""
import functools

import numpy as np
import pytest
import torch

import _camera_np as N
import _stereo_np as S

pytestmark = pytest.mark.gpu

SENSORS = ((1, 1), (2, 3), (7, 9), (33, 131), (70, 259))
COUNTS = (0, 1, 63, 64, 65, 257, 4097)
EVENT_COUNTS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 10_000)
RADTAN = (-0.21, 0.06, 0.0011, -0.0007, 0.003)
EQUI = (-0.05, 0.012, -0.02, 0.009)
BOUND = 1e-9                                                # px: equidistant coordinates, derived in tests/test_cpu_camera.py


def camera_matrix(size):
    h, w = size
    return np.array([[0.9 * max(w, 8), 0.0, (w - 1) / 2 + 0.3], [0.0, 0.85 * max(w, 8), (h - 1) / 2 - 0.2], [0.0, 0.0, 1.0]])


def rectified(size, out):
    """a rotation of two degrees, a new_K of another focal length centred in the out view"""
    K = camera_matrix(size)
    new_K = np.array([[K[0, 0] * 0.9, 0.0, (out[1] - 1) / 2], [0.0, K[0, 0] * 0.9, (out[0] - 1) / 2], [0.0, 0.0, 1.0]])
    return N.rodrigues(np.radians([1.2, -1.4, 0.8])), new_K


def calibrations():
    """(name, K, model, distortion, sensor) of the exact models: every sensor, and the divergent corner"""
    for size in SENSORS:
        yield "radtan %dx%d" % size, camera_matrix(size), "radtan", RADTAN, size
    yield "radtan4 33x131", camera_matrix((33, 131)), "radtan", RADTAN[:4], (33, 131)
    yield "none 7x9", camera_matrix((7, 9)), "none", None, (7, 9)
    yield "none 70x259", camera_matrix((70, 259)), "none", None, (70, 259)
    c = N.DIVERGENT
    yield "divergent", c["K"], c["model"], c["distortion"], c["sensor_size"]


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError("%s: %d of %d values differ, the first at %s: %r, expected %r" % (
            what, len(bad), w.size, tuple(bad[0]), np.asarray(got.cpu() if isinstance(got, torch.Tensor) else got)[tuple(bad[0])],
            np.asarray(want)[tuple(bad[0])]))


def same_flags(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.bool_ and np.array_equal(got, want), what


def points_for(rng, size, n):
    """pixel coordinates on and around the sensor; from 65 points on also NaN and +-inf"""
    h, w = size
    p = np.stack((rng.uniform(-0.2 * w - 1, 1.2 * w + 1, n), rng.uniform(-0.2 * h - 1, 1.2 * h + 1, n)), axis=1)
    if n >= 65:
        p[3, 0], p[17, 1], p[40], p[41, 0], p[64, 1] = np.nan, np.inf, (-np.inf, np.nan), -np.inf, np.nan
        p[5], p[6] = (0.0, 0.0), (w - 1.0, h - 1.0)
    return p


# ---- points: the exact models ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", list(calibrations()), ids=lambda c: c[0])
def test_points_are_the_restatements_bits(case):
    import event_utils_amd as E
    name, K, model, dist, size = case
    cam = E.CameraModel(K, dist, model, size)
    d = N.coefficients(model, dist)
    rng = np.random.default_rng(len(name) + size[1])
    R, new_K = rectified(size, size)
    for n in COUNTS:
        P = points_for(rng, size, n)
        for kw in ({}, {"R": R, "new_K": new_K}, {"iterations": 3, "tolerance": 1e-3}):
            u, v, ok = N.forward_points(P[:, 0], P[:, 1], K, model, d, kw.get("R"), kw.get("new_K"), kw.get("iterations", 20),
                                        kw.get("tolerance", 1e-6))
            got, valid = E.undistort_points(cam, P, return_valid=True, **kw)
            assert isinstance(got, np.ndarray) and got.shape == (n, 2) and got.dtype == np.float64 and valid.shape == (n,)
            same_bits(got, np.stack((u, v), axis=1), "%s undistort n=%d %s" % (name, n, sorted(kw)))
            same_flags(valid, ok, "%s undistort flags n=%d" % (name, n))
            dgot, dvalid = E.undistort_points(cam, torch.from_numpy(P).cuda(), return_valid=True, **kw)
            assert dgot.is_cuda and dvalid.is_cuda and dvalid.dtype == torch.bool
            same_bits(dgot, got, "device tensor in")
            assert not isinstance(E.undistort_points(cam, P, **kw), tuple)
        x, y, ok = N.inverse_points(P[:, 0], P[:, 1], K, model, d)
        got = E.distort_points(cam, P)
        assert isinstance(got, np.ndarray) and got.shape == (n, 2)
        same_bits(got, np.stack((x, y), axis=1), "%s distort n=%d" % (name, n))
        assert np.array_equal(np.isnan(got[:, 0]), ~ok)
        same_bits(E.distort_points(cam, torch.from_numpy(P).cuda()), got, "device tensor in")
    same_bits(E.undistort_points(cam, P.astype(np.float32)), E.undistort_points(cam, P.astype(np.float32).astype(np.float64)), "float32 points")


@pytest.mark.parametrize("case", list(calibrations()), ids=lambda c: c[0])
def test_maps_are_the_restatements_bits(case):
    import event_utils_amd as E
    name, K, model, dist, size = case
    cam = E.CameraModel(K, dist, model, size)
    d = N.coefficients(model, dist)
    out = (size[0] + 3, max(size[1] - 2, 1))
    R, new_K = rectified(size, out)
    for kw in ({}, {"R": R, "new_K": new_K, "out_size": out}, {"out_size": out, "iterations": 5, "tolerance": 1e-4}):
        want = N.maps(K, model, d, size, kw.get("R"), kw.get("new_K"), kw.get("out_size"), kw.get("iterations", 20), kw.get("tolerance", 1e-6))
        m = E.rectification_maps(cam, **kw)
        assert isinstance(m, E.RectificationMaps) and all(t.is_cuda for t in m[:4]) and m.out_size == kw.get("out_size", size)
        assert m.forward.dtype == torch.float64 and m.forward_valid.dtype == torch.bool and np.array_equal(m.new_K, kw.get("new_K", K))
        for got, ref, what in zip(m[:4], want, ("forward", "forward_valid", "inverse", "inverse_valid")):
            assert tuple(got.shape) == ref.shape, what
            (same_flags if ref.dtype == np.bool_ else same_bits)(got, ref, "%s %s %s" % (name, what, sorted(kw)))
    if name == "divergent":
        assert not bool(m.forward_valid[0, 0]) and bool(torch.isnan(m.forward[:, 0, 0]).all()) and 0.3 < float(m.forward_valid.double().mean()) < 0.9


# ---- points and maps: equidistant ----------------------------------------------------------------------------------------------------

def test_equidistant_is_within_the_bound():
    """the largest difference seen is printed (DESIGN.md section 6 records it)"""
    import event_utils_amd as E
    worst = 0.0
    for size in SENSORS:
        K = camera_matrix(size)
        cam = E.CameraModel(K, EQUI, "equidistant", size)
        d = N.coefficients("equidistant", EQUI)
        out = (size[0] + 3, max(size[1] - 2, 1))
        R, new_K = rectified(size, out)
        rng = np.random.default_rng(size[1])
        for kw in ({}, {"R": R, "new_K": new_K, "out_size": out}):
            want = N.maps(K, "equidistant", d, size, kw.get("R"), kw.get("new_K"), kw.get("out_size"))
            m = E.rectification_maps(cam, **kw)
            for got, flags, ref, rv in ((m.forward, m.forward_valid, want[0], want[1]), (m.inverse, m.inverse_valid, want[2], want[3])):
                same_flags(flags, rv, "flags %r" % (size,))
                g = got.cpu().numpy()
                assert np.isnan(g[:, ~rv]).all() and rv.mean() > 0.5
                worst = max(worst, float(np.abs(g[:, rv] - ref[:, rv]).max()))
        for n in COUNTS:
            P = points_for(rng, size, n)
            u, v, ok = N.forward_points(P[:, 0], P[:, 1], K, "equidistant", d, R, new_K)
            got, valid = E.undistort_points(cam, P, R=R, new_K=new_K, return_valid=True)
            same_flags(valid, ok, "undistort flags %r n=%d" % (size, n))
            x, y, ok2 = N.inverse_points(P[:, 0], P[:, 1], K, "equidistant", d)
            dist = E.distort_points(cam, P)
            assert np.array_equal(np.isnan(dist[:, 0]), ~ok2) and np.isnan(got[~ok]).all()
            if ok.any():
                worst = max(worst, float(np.abs(got[ok] - np.stack((u, v), axis=1)[ok]).max()))
            if ok2.any():
                worst = max(worst, float(np.abs(dist[ok2] - np.stack((x, y), axis=1)[ok2]).max()))
    print("equidistant: largest difference %.3e px" % worst)
    assert worst <= BOUND


# ---- rectify_events on supplied maps ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def supplied(model):
    """maps from the restatement for a 33 x 131 sensor and a 36 x 120 view: (cam arguments, the four arrays, new_K, out)"""
    size, out = (33, 131), (36, 120)
    K = camera_matrix(size)
    dist = {"radtan": RADTAN, "equidistant": EQUI, "none": None}[model]
    R, new_K = rectified(size, out)
    arrays = N.maps(K, model, N.coefficients(model, dist), size, R, new_K, out)
    for a in arrays:
        a.setflags(write=False)
    return (K, dist, model, size), arrays, new_K, out


def supplied_maps(E, model):
    args, (fwd, fv, inv, iv), new_K, out = supplied(model)
    m = E.RectificationMaps.from_tensors(E.CameraModel(*args), fwd.copy(), inv.copy(), fv.copy(), iv.copy(), new_K)
    assert m.out_size == out and m.forward.is_cuda and m.inverse_valid.dtype == torch.bool
    return m, (fwd, fv, inv, iv), args[3], out


def events_for(rng, size, n, dtype):
    h, w = size
    return (rng.integers(0, w, n).astype(dtype), rng.integers(0, h, n).astype(dtype), np.sort(rng.uniform(0.0, 1.0, n)),
            (rng.integers(0, 2, n) * 2 - 1).astype(np.int8))


def check_events(E, cols, kind, maps, arrays, out, mode, what):
    """rectify_events of the columns in one input kind against the restatement, return_index included -> the kept count"""
    xs, ys, ts, ps = cols
    want = N.rectify_events(xs, ys, ts, ps, arrays[0], arrays[1], out, mode)
    if kind == "numpy":
        got, index = E.rectify_events(xs, ys, ts, ps, maps, mode=mode, return_index=True)
        assert all(isinstance(c, np.ndarray) for c in got) and isinstance(index, np.ndarray)
    elif kind == "tensors":
        got, index = E.rectify_events(*(torch.from_numpy(c).cuda() for c in cols), maps, mode=mode, return_index=True)
        assert all(c.is_cuda for c in got) and index.is_cuda
        got, index = tuple(c.cpu().numpy() for c in got), index.cpu().numpy()
    else:
        prec = kind.split("_")[1]
        ev = E.DeviceEvents.from_arrays(xs, ys, ts, ps, precision=prec)
        res, index = E.rectify_events(ev, None, None, None, maps, mode=mode, return_index=True)
        assert isinstance(res, E.DeviceEvents) and index.is_cuda
        ft = np.float32 if prec == "f32" else np.float64
        assert res.dtype == (torch.float32 if prec == "f32" else torch.float64)
        got, index = tuple(c.cpu().numpy() for c in (res.x, res.y, res.t, res.p)), index.cpu().numpy()
        want = tuple(np.asarray(c).astype(ft) for c in (want[0], want[1], ts.astype(ft)[want[4]], ps.astype(ft)[want[4]])) + (want[4],)
        if len(index):
            assert res.t_at(0) == float(want[2][0]) and res.t_at(-1) == float(want[2][-1])
    assert index.dtype == np.int64 and np.array_equal(index, want[4]), what
    for g, w_, name in zip(got, want[:4], "xytp"):
        assert g.dtype == w_.dtype and g.shape == w_.shape and np.array_equal(g.view(np.uint8), w_.view(np.uint8)), (what, name)
    assert (np.diff(index) > 0).all()                       # stream order
    return len(index)


@pytest.mark.parametrize("mode", ["nearest", "subpixel"])
@pytest.mark.parametrize("model", ["radtan", "equidistant", "none"])
def test_rectify_events_on_supplied_maps(model, mode):
    import event_utils_amd as E
    maps, arrays, size, out = supplied_maps(E, model)
    rng = np.random.default_rng(7)
    kept = 0
    for n in EVENT_COUNTS:
        for kind, dtype in (("numpy", np.int16), ("numpy", np.int32), ("tensors", np.int64), ("tensors", np.float32), ("numpy", np.float64),
                            ("events_f64", np.float64), ("events_f32", np.float32)):
            if n in (63, 65, 4095) and dtype in (np.int32, np.float32):
                continue                                    # (the coordinate kinds are each seen at every chunk boundary)
            cols = events_for(rng, size, n, dtype)
            kept += check_events(E, cols, kind, maps, arrays, out, mode, "%s %s n=%d %s %s" % (model, mode, n, kind, np.dtype(dtype).name))
    assert kept > 10_000
    # two calls, the same bits; ts and ps may be left out
    cols = events_for(rng, size, 5000, np.int32)
    a, b = (E.rectify_events(*cols, maps, mode=mode) for _ in range(2))
    assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(a, b))
    x, y, t, p = E.rectify_events(cols[0], cols[1], None, None, maps, mode=mode)
    assert t is None and p is None and np.array_equal(x, a[0]) and np.array_equal(y, a[1])
    x, y, t, p = E.rectify_events(cols[0], cols[1], cols[2], None, maps, mode=mode)
    assert p is None and np.array_equal(t, a[2])


def test_rectify_events_all_dropped_none_dropped_and_refusals():
    import event_utils_amd as E
    maps, arrays, size, out = supplied_maps(E, "radtan")
    rng = np.random.default_rng(8)
    cols = events_for(rng, size, 4097, np.int32)
    nothing = maps._replace(forward_valid=torch.zeros_like(maps.forward_valid))
    for kind in ("numpy", "tensors", "events_f64"):
        assert check_events(E, cols, kind, nothing, (arrays[0], np.zeros_like(arrays[1])), out, "nearest", "all dropped " + kind) == 0
    # the identity camera drops nothing and moves nothing (sub-pixel: fx ((x - cx) / fx) + cx is x within a few ulp of 131)
    cam = E.CameraModel(np.array([[100.0, 0.0, 65.0], [0.0, 100.0, 16.0], [0.0, 0.0, 1.0]]), sensor_size=size)
    ident = E.rectification_maps(cam)
    for mode in ("nearest", "subpixel"):
        x, y, t, p = E.rectify_events(*cols, ident, mode=mode)
        assert len(x) == 4097 and np.array_equal(t, cols[2]) and np.array_equal(p, cols[3])
        if mode == "nearest":
            assert x.dtype == np.int32 and np.array_equal(x, cols[0]) and np.array_equal(y, cols[1])
        else:
            assert x.dtype == np.float64 and np.abs(x - cols[0]).max() < 1e-12 and np.abs(y - cols[1]).max() < 1e-12
    # NaN entries without flags count as invalid
    bare = E.RectificationMaps.from_tensors(E.CameraModel(*supplied("radtan")[0]), np.where(arrays[1], arrays[0], np.nan), arrays[2].copy())
    assert torch.equal(bare.forward_valid.cpu(), torch.from_numpy(arrays[1].copy()))
    assert check_events(E, cols, "numpy", bare, arrays, out, "nearest", "flags from NaN") > 0
    # coordinates that are no pixels of the raw sensor
    h, w = size
    for bad_x, bad_y in ((np.array([1.0, 2.5]), np.array([1.0, 1.0])), (np.array([1.0, np.nan]), np.array([1.0, 1.0])),
                         (np.array([1, w], dtype=np.int32), np.array([1, 1], dtype=np.int32)), (np.array([1, 1], dtype=np.int64), np.array([1, -1], dtype=np.int64)),
                         (np.array([1.0, 1.0], dtype=np.float32), np.array([float(h), 1.0], dtype=np.float32))):
        with pytest.raises(ValueError, match="raw sensor"):
            E.rectify_events(bad_x, bad_y, None, None, maps)
        with pytest.raises(ValueError, match="raw sensor"):
            E.rectify_events(torch.from_numpy(bad_x).cuda(), torch.from_numpy(bad_y).cuda(), None, None, maps, mode="subpixel")


# ---- remap_images ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("interpolation", ["nearest", "bilinear"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_remap_images_is_the_restatements_bits(dtype, interpolation):
    import event_utils_amd as E
    rng = np.random.default_rng(9)
    for model in ("radtan", "equidistant"):
        maps, (fwd, fv, inv, iv), size, out = supplied_maps(E, model)
        assert 0.5 < iv.mean() and not np.array_equal(size, out)
        for lead in ((), (0,), (1,), (3,), (2, 2)):
            shape = lead + size
            img = rng.integers(0, 256, shape).astype(dtype) if dtype == np.uint8 else rng.normal(0.0, 50.0, shape).astype(dtype)
            for fill in (0, 7.5, -3.0, 300.0):
                want = N.remap(img.reshape((-1,) + size), inv, iv, interpolation, fill).reshape(lead + out)
                got = E.remap_images(img, maps, interpolation, fill)
                assert isinstance(got, np.ndarray) and got.dtype == img.dtype and got.shape == want.shape
                assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), (model, lead, fill)
            dev = E.remap_images(torch.from_numpy(img).cuda(), maps, interpolation, fill)
            assert dev.is_cuda and np.array_equal(dev.cpu().numpy().view(np.uint8), want.view(np.uint8))
    # a map that is invalid everywhere gives the fill value everywhere
    nowhere = maps._replace(inverse_valid=torch.zeros_like(maps.inverse_valid))
    got = E.remap_images(img, nowhere, interpolation, 7.5)
    assert np.array_equal(got, N.remap(img.reshape((-1,) + size), inv, np.zeros_like(iv), interpolation, 7.5).reshape(got.shape))
    assert (got == np.asarray(8 if dtype == np.uint8 else 7.5, dtype=dtype)).all()
    # device-built radtan maps: the same bits end to end
    args = supplied("radtan")
    R, new_K = rectified(size, out)
    built = E.rectification_maps(E.CameraModel(*args[0]), R, new_K, out)
    img = rng.integers(0, 256, (3,) + size).astype(dtype)
    arrays = supplied("radtan")[1]
    assert np.array_equal(E.remap_images(img, built, interpolation, 1), N.remap(img, arrays[2], arrays[3], interpolation, 1))


# ---- the seeded raw scene, end to end ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def raw_scene(model):
    sc = N.raw_scene(model)
    sc["maps"] = {side: N.scene_maps(sc, side) for side in ("left", "right")}
    return sc


def device_maps(E, sc, side):
    K, model, d, R = sc["cameras"][0 if side == "left" else 1]
    dist = None if model == "none" else d[:4]
    return E.rectification_maps(E.CameraModel(K, dist, model, S.SCENE_SIZE), R, sc["new_K"])


def margins(m, size):
    """the least distance of a map's valid entries from a rounding boundary (x.5) and from the border of a `size` view"""
    h, w = size
    half = float(np.nanmin(np.abs(m - np.floor(m) - 0.5)))
    border = min(float(np.nanmin(np.abs(m[0] - e))) for e in (-0.5, w - 0.5))
    return min(half, border, min(float(np.nanmin(np.abs(m[1] - e))) for e in (-0.5, h - 0.5)))


@pytest.mark.parametrize("model", ["radtan", "equidistant"])
def test_the_seeded_raw_scene_through_both_rectifications(model):
    import event_utils_amd as E
    sc = raw_scene(model)
    for side in ("left", "right"):
        fwd, fv, inv, iv = sc["maps"][side]
        if model == "equidistant":
            # no entry of the seeded calibration lies within 1e-6 px of a rounding boundary or of the border: a coordinate that is
            # within 1e-9 px of the restatement's rounds as the restatement's does
            assert margins(fwd, S.SCENE_SIZE) > 1e-6 and margins(inv, S.SCENE_SIZE) > 1e-6
    streams, surfaces = {}, {}
    for side in ("left", "right"):
        maps = device_maps(E, sc, side)
        cols = S.stream(sc[side])
        fwd, fv, inv, iv = sc["maps"][side]
        for mode in ("nearest", "subpixel") if model == "radtan" else ("nearest",):
            for kind in ("numpy", "tensors", "events_f64"):
                check_events(E, cols, kind, maps, (fwd, fv), S.SCENE_SIZE, mode, "%s %s %s %s" % (model, side, mode, kind))
        streams[side] = E.rectify_events(*(torch.from_numpy(c).cuda() for c in cols), maps)
        q = E.quantised_time_surfaces(*cols, S.SCENE_TAU, S.SCENE_SIZE, [S.SCENE_END])
        surfaces[side] = E.remap_images(q, maps)
        assert surfaces[side].is_cuda and surfaces[side].dtype == torch.uint8 and tuple(surfaces[side].shape) == (1, 1) + S.SCENE_SIZE
    tests = dict(radius=S.SCENE_R, min_activity=S.SCENE_ACTIVITY)
    for how, res in (("events", E.stereo_disparity(streams["left"], streams["right"], S.SCENE_TAU, S.SCENE_SIZE, [S.SCENE_END], S.SCENE_D - 1, **tests)),
                     ("images", E.stereo_match(surfaces["left"], surfaces["right"], S.SCENE_D - 1, **tests))):
        QL, QR = N.scene_surfaces(sc, how)
        if how == "images":
            assert torch.equal(surfaces["left"].cpu(), torch.from_numpy(QL)) and torch.equal(surfaces["right"].cpu(), torch.from_numpy(QR))
        want = S.match(QL, QR, 0, S.SCENE_D, S.SCENE_R, S.SCENE_ACTIVITY)
        assert torch.equal(res.cost.cpu(), torch.from_numpy(want[2])), how
        assert torch.equal(res.index.cpu(), torch.from_numpy(want[1])), how
        assert torch.equal(res.mask.cpu(), torch.from_numpy(want[3])), how
        assert np.array_equal(res.disparity.cpu().numpy(), want[0], equal_nan=True), how
        assert int(res.mask.sum()) > 100
