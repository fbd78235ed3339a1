"""GPU (-m gpu): the event filters clip_events_to_bounds, get_events_from_mask and remove_hot_pixels (evk_select.hip) against the
numpy restatement of tests/test_cpu_filters.py (itself checked against the real reference there): numpy columns in their own
dtypes, device tensors, DeviceEvents in float32 / float64, 10 M events with planted hot pixels, edge sizes, a misaligned slice,
the reference's exceptions, and a voxel grid of the filtered stream."""
import numpy as np
import pytest
import torch

from oracle import reference_np as R
from test_cpu_filters import np_clip_events_to_bounds, np_get_events_from_mask, np_remove_hot_pixels

pytestmark = pytest.mark.gpu
H, W = 48, 64


@pytest.fixture(scope="module")
def E():
    import event_utils_amd as E
    assert torch.cuda.is_available()
    return E


def same(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8) if a.dtype == np.bool_ else a, b.view(np.uint8) if b.dtype == np.bool_ else b,
                          equal_nan=a.dtype.kind == "f")


def stream(rng, n, H=H, W=W, hot=(), hot_share=0.0):
    x = rng.integers(0, W, n)
    y = rng.integers(0, H, n)
    if hot:
        k = rng.random(n) < hot_share
        pick = rng.integers(0, len(hot), n)
        x = np.where(k, np.array([h[0] for h in hot])[pick], x)
        y = np.where(k, np.array([h[1] for h in hot])[pick], y)
    t = np.sort(rng.uniform(0, 1, n))
    p = rng.integers(0, 2, n) * 2 - 1
    if hot:
        p = np.where(k, 1, p)                                  # a stuck pixel fires one polarity
    return x, y, t, p


def dev_cols(cols, dtype):
    return [None if c is None else torch.from_numpy(np.asarray(c).astype(dtype)).cuda() for c in cols]


def events_out(ev):
    return [c.cpu().numpy() for c in (ev.x, ev.y, ev.t, ev.p)]


# ---- reference dtypes in, the same out ------------------------------------------------------------------------------------

@pytest.mark.parametrize("num_hot", [0, 1, 7, 50, H * W + 5])
def test_remove_hot_pixels_numpy_reference_dtypes(E, num_hot):
    rng = np.random.default_rng(num_hot)
    x, y, t, p = stream(rng, 20_000, hot=[(3, 4), (10, 20), (63, 47)], hot_share=0.1)
    for pc in (p, p > 0, p.astype(np.float64)):
        got = E.remove_hot_pixels(x, y, t, pc, sensor_size=(H, W), num_hot=num_hot)
        want = np_remove_hot_pixels(x, y, t, pc, sensor_size=(H, W), num_hot=num_hot)
        for g, w in zip(got, want):
            same(g, w)


def test_remove_hot_pixels_edge_images(E):
    """zero-sum pixels picked as the extra one, an all-negative image, ties, events at x == W / y == H (legal, never hot)."""
    x = np.array([0, 0, 2, 5, 5, W, 3, 3, 1], np.int64)
    y = np.array([0, 0, 1, 3, 3, 0, H, 2, 1], np.int64)
    t = np.arange(9.0)
    for p in (np.array([-1, -1, 1, 1, -1, 5, 5, 1, 1]), -np.ones(9, np.int64), np.array([1, -1, 1, 1, -1, 3, 3, 1, 1])):
        for k in range(0, 8):
            for g, w in zip(E.remove_hot_pixels(x, y, t, p, (H, W), k), np_remove_hot_pixels(x, y, t, p, (H, W), k)):
                same(g, w)
    # a NaN weight ranks above every number
    pf = np.array([1.0, 1.0, 2.0, np.nan, 4.0, 1.0, 1.0, 3.0, 0.5])
    for k in (1, 2, 3):
        for g, w in zip(E.remove_hot_pixels(x, y, t, pf, (H, W), k), np_remove_hot_pixels(x, y, t, pf, (H, W), k)):
            same(g, w)


@pytest.mark.parametrize("bounds", [(20, 30), (5, 40, 10, 50), (5.5, 40.25, 10.7, 50.1)])
@pytest.mark.parametrize("set_zero", [False, True])
def test_clip_numpy_reference_dtypes(E, bounds, set_zero):
    rng = np.random.default_rng(1)
    x, y, t, p = stream(rng, 10_001)
    for cols in ((x, y, t, p > 0), (x.astype(np.float32), y.astype(np.float32), t.astype(np.float32), p.astype(np.float32)),
                 (x.astype(np.int16), y.astype(np.int16), t, p.astype(np.int8)), (x, y, None, None)):
        got = E.clip_events_to_bounds(*cols, bounds, set_zero)
        want = np_clip_events_to_bounds(*cols, bounds, set_zero)
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            if w is not None:
                same(g, w)


def test_clip_float32_columns_compare_in_float32(E):
    b = 0.7                                                     # float32(0.7) < 0.7: kept in float32, not in float64
    xs = np.array([np.float32(b), 0.5, 0.8, 1.0], np.float32)
    ys = np.zeros(4, np.float32)
    got = E.clip_events_to_bounds(xs, ys, None, None, [0.0, 1.0, b, 1.0])
    want = np_clip_events_to_bounds(xs, ys, None, None, [0.0, 1.0, b, 1.0])
    same(got[0], want[0])
    assert got[0].shape[0] == 2


def test_clip_bounds_of_length_3_raise(E):
    x = np.arange(4)
    with pytest.raises(Exception):
        E.clip_events_to_bounds(x, x, x, x, [1, 2, 3])


def test_get_events_from_mask_numpy(E):
    rng = np.random.default_rng(2)
    x = rng.uniform(-W, W - 0.01, 30_000)
    y = rng.uniform(-H, H - 0.01, 30_000)
    for mask in (rng.uniform(0, 0.02, (H, W)), rng.uniform(0, 0.02, (H, W)).astype(np.float32), rng.integers(0, 2, (H, W)),
                 np.full((H, W), np.float32(0.01), np.float32), rng.uniform(0, 1, (H, W)) > 0.5):
        same(E.get_events_from_mask(mask, x, y), np_get_events_from_mask(mask, x, y))
        xi, yi = x.astype(np.int64), y.astype(np.int16)
        same(E.get_events_from_mask(mask, xi, yi), np_get_events_from_mask(mask, xi, yi))
    m = np.zeros((H, W), np.float32)
    m[1, 2] = np.float32(0.01)
    r = E.get_events_from_mask(m, np.array([2.7, 0.0, 3.0]), np.array([1.2, 0.0, 2.0]))
    assert r.shape == () and r.dtype == np.int64 and int(r) == 0


def test_errors_where_the_reference_raises(E):
    x, y, t, p = np.array([1, W + 1]), np.array([0, 0]), np.arange(2.0), np.ones(2, np.int64)
    with pytest.raises(ValueError):
        E.remove_hot_pixels(x, y, t, p, (H, W), 3)
    with pytest.raises(TypeError):
        E.remove_hot_pixels(x * 1.0, y * 1.0, t, p, (H, W), 3)
    xd = torch.tensor([1.0, 2.5], device="cuda")
    with pytest.raises(TypeError):
        E.remove_hot_pixels(xd, xd, xd, xd, (H, W), 3)
    ev = E.DeviceEvents.from_arrays(np.array([1.0, 2.5]), np.array([1.0, 2.0]), np.arange(2.0), np.ones(2), precision="f32")
    with pytest.raises(TypeError):
        E.remove_hot_pixels(ev, None, None, None, (H, W), 3)
    m = np.ones((H, W))
    for xb, yb in ((np.array([-W - 1.0]), np.array([0.0])), (np.array([float(W)]), np.array([0.0])),
                   (np.array([0.0]), np.array([float(H)])), (np.array([np.nan]), np.array([0.0]))):
        with pytest.raises(IndexError):
            E.get_events_from_mask(m, xb, yb)
    # the device stays usable after a reported error
    same(E.get_events_from_mask(m, np.array([-1.0, 0.0]), np.array([-1.0, 0.0])), np.array([0, 1]))


# ---- device tensors and DeviceEvents -----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_tensors_and_device_events(E, dtype):
    rng = np.random.default_rng(4)
    x, y, t, p = stream(rng, 50_003, hot=[(7, 7), (40, 30)], hot_share=0.05)
    cols = [a.astype(dtype) for a in (x, y, t, p)]
    want = np_remove_hot_pixels(x, y, cols[2], cols[3], (H, W), 9)
    got = E.remove_hot_pixels(*dev_cols(cols, dtype), sensor_size=(H, W), num_hot=9)
    for g, w in zip(got, want):
        assert g.is_cuda
        same(g, w.astype(dtype))
    prec = "f32" if dtype == np.float32 else "f64"
    ev = E.DeviceEvents.from_arrays(*cols, precision=prec)
    r = E.remove_hot_pixels(ev, None, None, None, sensor_size=(H, W), num_hot=9)
    assert isinstance(r, E.DeviceEvents) and r.t_offset == ev.t_offset and r.p_scale == ev.p_scale
    for g, w in zip(events_out(r), want):
        same(g, w.astype(dtype))
    assert r._t_ends == (float(want[2][0].astype(dtype)), float(want[2][-1].astype(dtype)))

    b = (5.5, 40.0, 10.0, 50.5)
    want = np_clip_events_to_bounds(*cols, b)
    for g, w in zip(E.clip_events_to_bounds(*dev_cols(cols, dtype), b), want):
        same(g, w)
    r = E.clip_events_to_bounds(ev, None, None, None, b)
    for g, w in zip(events_out(r), want):
        same(g, w)
    assert r._t_ends == (float(want[2][0]), float(want[2][-1]))
    z = E.clip_events_to_bounds(ev, None, None, None, b, set_zero=True)
    for g, w in zip(events_out(z), np_clip_events_to_bounds(*cols, b, set_zero=True)):
        same(g, w)

    mask = rng.uniform(0, 0.02, (H, W)).astype(np.float32)
    want = np_get_events_from_mask(mask, cols[0], cols[1])
    same(E.get_events_from_mask(torch.from_numpy(mask).cuda(), *dev_cols(cols[:2], dtype)), want)
    same(E.get_events_from_mask(mask, ev, None), want)


def test_relative_time_stamps_keep_their_offset(E):
    rng = np.random.default_rng(8)
    x, y, _, p = stream(rng, 10_000)
    t = 1.6e9 + np.sort(rng.uniform(0, 1, 10_000)).round(6)
    ev = E.DeviceEvents.from_arrays(x.astype(np.float64), y.astype(np.float64), t, p.astype(np.float64), relative_time=True)
    assert ev.t_offset != 0.0
    r = E.clip_events_to_bounds(ev, None, None, None, (30, 40))
    assert r.t_offset == ev.t_offset
    z = E.clip_events_to_bounds(ev, None, None, None, (30, 40), set_zero=True)
    want = np_clip_events_to_bounds(x.astype(np.float64), y.astype(np.float64), ev.t.double().cpu().numpy() + ev.t_offset, p, (30, 40),
                                    set_zero=True)
    same(z.t.cpu().numpy(), want[2])
    assert z.t_offset == 0.0


# ---- sizes -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 3, 255, 4095, 4096, 4097, 12_345])
def test_sizes_empty_and_all_removed(E, n):
    rng = np.random.default_rng(n)
    x, y, t, p = stream(rng, n)
    for b in ((H, W), (0, 0), (10, 20, 5, 60)):
        for g, w in zip(E.clip_events_to_bounds(x, y, t, p, b), np_clip_events_to_bounds(x, y, t, p, b)):
            same(g, w)
    for k in (0, 3, H * W):
        for g, w in zip(E.remove_hot_pixels(x, y, t, p, (H, W), k), np_remove_hot_pixels(x, y, t, p, (H, W), k)):
            same(g, w)
    if n:
        mask = rng.uniform(0, 0.02, (H, W))
        same(E.get_events_from_mask(mask, x * 1.0, y * 1.0), np_get_events_from_mask(mask, x * 1.0, y * 1.0))
    # every event on one pixel: all removed
    xs, ys = np.full(n, 5), np.full(n, 6)
    for g, w in zip(E.remove_hot_pixels(xs, ys, t, p * 0 + 1, (H, W), 1), np_remove_hot_pixels(xs, ys, t, p * 0 + 1, (H, W), 1)):
        same(g, w)
        assert g.shape[0] == 0


def test_misaligned_slice(E):
    rng = np.random.default_rng(6)
    x, y, t, p = stream(rng, 30_000, hot=[(1, 2)], hot_share=0.2)
    cols = [a.astype(np.float32) for a in (x, y, t, p)]
    ev = E.DeviceEvents.from_arrays(*cols, precision="f32")
    a, b = 3, 29_001
    s = ev.slice(a, b)
    assert s.x.data_ptr() % 16 != 0
    sub = [c[a:b] for c in cols]
    for g, w in zip(events_out(E.remove_hot_pixels(s, None, None, None, (H, W), 4)),
                    np_remove_hot_pixels(x[a:b], y[a:b], sub[2], sub[3], (H, W), 4)):
        same(g, w.astype(np.float32))
    for g, w in zip(events_out(E.clip_events_to_bounds(s, None, None, None, (10, 30, 5, 50))),
                    np_clip_events_to_bounds(*sub, (10, 30, 5, 50))):
        same(g, w)


# ---- 10 M events ---------------------------------------------------------------------------------------------------------

def test_ten_million_events_with_planted_hot_pixels(E):
    rng = np.random.default_rng(10)
    n, HH, WW = 10_000_000, 480, 640
    hot = [(int(rng.integers(0, WW)), int(rng.integers(0, HH))) for _ in range(40)]
    x, y, t, p = stream(rng, n, HH, WW, hot=hot, hot_share=0.02)
    want = np_remove_hot_pixels(x, y, t, p, (HH, WW), 50)
    got = E.remove_hot_pixels(x, y, t, p, (HH, WW), 50)
    for g, w in zip(got, want):
        same(g, w)
    assert want[0].shape[0] < n - 0.02 * n * 0.9
    cols = [a.astype(np.float32) for a in (x, y, t, p)]
    ev = E.DeviceEvents.from_arrays(*cols, precision="f32")
    r = E.remove_hot_pixels(ev, None, None, None, (HH, WW), 50)
    for g, w in zip(events_out(r), want):
        same(g, w.astype(np.float32))
    # end to end: the voxel grid of the filtered resident stream equals the oracle's of the restatement's output
    vox = E.events_to_voxel_torch(r, None, None, None, 5, sensor_size=(HH, WW)).cpu().numpy().astype(np.float64)
    wf = [a.astype(np.float32) for a in want]
    ref = R.events_to_voxel_torch(*wf, 5, sensor_size=(HH, WW), accum="f64")
    assert np.abs(vox - ref).max() <= 1e-5 * np.abs(ref).max()
    b = (100, 340, 50, 600)
    for g, w in zip(events_out(E.clip_events_to_bounds(ev, None, None, None, b)), np_clip_events_to_bounds(*cols, b)):
        same(g, w)
