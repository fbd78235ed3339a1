"""GPU (-m gpu): neighbour_support, background_activity_filter and refractory_filter (evk_denoise.hip) against the host
restatements of tests/_denoise_np.py (seq_*: the definition; fast_*: pinned to it in tests/test_cpu_denoise.py).  Every comparison
of support bytes, kept columns and dtypes is exact: the definition has no rounding freedom."""
import numpy as np
import pytest
import torch

import _denoise_np as N
from oracle import reference_np as R

pytestmark = pytest.mark.gpu
H, W = 48, 64
SEL_CHUNK = 4096          # evk_select.hip: events per compaction chunk


@pytest.fixture(scope="module")
def E():
    import event_utils_amd as E
    assert torch.cuda.is_available()
    return E


def same(a, b):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8) if a.dtype == np.bool_ else a, b.view(np.uint8) if b.dtype == np.bool_ else b)


def scene(rng, n, H=H, W=W, span=50_000, shuffle=False):
    """Uniform noise plus a vertical edge that sweeps the sensor; integer-microsecond times (ties occur), int64 / float64 / int64."""
    t = np.sort(rng.integers(0, span, n)).astype(np.float64)
    noise = rng.random(n) < 0.5
    x = np.where(noise, rng.integers(0, W, n), np.minimum(W - 1, (t / span * W).astype(np.int64)))
    y = rng.integers(0, H, n)
    p = rng.integers(0, 2, n) * 2 - 1
    if shuffle:
        t = rng.permutation(t)
    return x.astype(np.int64), y.astype(np.int64), t, p.astype(np.int64)


def events_out(ev):
    return [c.cpu().numpy() for c in (ev.x, ev.y, ev.t, ev.p)]


def check_baf(E, cols, size, dt, sup_fn=N.seq_support, support=1, want=None, **kw):
    """neighbour_support and background_activity_filter (with return_support) on numpy columns against the restatement."""
    if want is None:
        want = sup_fn(*cols, dt, size, **kw)
    same(E.neighbour_support(*cols, dt, sensor_size=size, **kw), want)
    keep = want >= support
    out = E.background_activity_filter(*cols, dt, sensor_size=size, support=support, return_support=True, **kw)
    assert len(out) == 5
    for g, c in zip(out[:4], cols):
        same(g, np.asarray(c)[keep])
    same(out[4], want)
    return want


def check_refractory(E, cols, size, refractory, per_polarity=False, keep_fn=N.seq_refractory):
    keep = keep_fn(*cols, refractory, size, per_polarity)
    out = E.refractory_filter(*cols, refractory, sensor_size=size, per_polarity=per_polarity)
    for g, c in zip(out, cols):
        same(g, np.asarray(c)[keep])
    return keep


# ---- mixed scene ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mixed():
    return scene(np.random.default_rng(100), 20_000)


@pytest.mark.parametrize("radius,support,include_self,same_polarity,dt", [
    (1, 1, False, False, 300.0), (1, 2, False, True, 300.0), (1, 1, False, False, 0.0), (1, 4, True, False, 1e6),
    (2, 2, True, False, 300.0), (2, 4, False, False, 1e6), (2, 1, False, True, 0.0),
    (3, 4, False, True, 300.0), (3, 1, True, True, 0.0), (3, 2, False, False, 1e6)])
def test_mixed_scene_support_and_filter(E, mixed, radius, support, include_self, same_polarity, dt):
    want = check_baf(E, mixed, (H, W), dt, support=support, radius=radius, include_self=include_self, same_polarity=same_polarity)
    assert 0 < (want >= support).sum() < len(want) or dt in (0.0, 1e6)


@pytest.mark.parametrize("per_polarity", [False, True])
@pytest.mark.parametrize("refractory", [0.0, 1.0, 2_000.0])
def test_mixed_scene_refractory(E, mixed, per_polarity, refractory):
    keep = check_refractory(E, mixed, (H, W), refractory, per_polarity)
    assert keep.all() if refractory == 0.0 else not keep.all()


# ---- geometry and sizes --------------------------------------------------------------------------------------------------

def test_corners_and_edges(E):
    """every corner and edge pixel fires twice, neighbours of each fire in between: the window is clipped, never wrapped"""
    pts = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W // 2, H - 1), (0, H // 2), (W - 1, H // 2)]
    xs, ys = [], []
    for (px, py) in pts:
        for dx, dy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (0, 0)):
            qx, qy = px + dx, py + dy
            if 0 <= qx < W and 0 <= qy < H:
                xs.append(qx), ys.append(qy)
    x, y = np.array(xs * 3), np.array(ys * 3)
    n = len(x)
    t = np.arange(n, dtype=np.float64) // 2
    p = (np.arange(n) % 3 == 0) * 2 - 1
    cols = (x, y, t, p)
    for radius in (1, 2, 3):
        for include_self in (False, True):
            check_baf(E, cols, (H, W), 20.0, radius=radius, include_self=include_self, same_polarity=bool(radius & 1))
    check_refractory(E, cols, (H, W), 5.0)
    check_refractory(E, cols, (H, W), 5.0, per_polarity=True)


@pytest.mark.parametrize("size", [(1, 1), (1, 37), (29, 1)])
def test_degenerate_sensors(E, size):
    rng = np.random.default_rng(size[0] * 100 + size[1])
    cols = scene(rng, 700, size[0], size[1], span=400)
    for radius in (1, 3):
        check_baf(E, cols, size, 6.0, radius=radius, include_self=True, support=2 if size != (1, 1) else 1)
        check_baf(E, cols, size, 6.0, radius=radius, same_polarity=True)
    check_refractory(E, cols, size, 3.0)
    check_refractory(E, cols, size, 3.0, per_polarity=True)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 2 * SEL_CHUNK + 1])
def test_sizes(E, n):
    rng = np.random.default_rng(n)
    cols = scene(rng, n, 8, 9, span=max(2, n // 3))
    want = check_baf(E, cols, (8, 9), 4.0, radius=2)
    assert want.shape == (n,)
    check_refractory(E, cols, (8, 9), 2.0, per_polarity=True)
    out = E.background_activity_filter(*cols, 4.0, sensor_size=(8, 9))
    assert len(out) == 4 and all(o.dtype == c.dtype for o, c in zip(out, cols))


@pytest.mark.parametrize("seed", [0, 1])
def test_unsorted_timestamps(E, seed):
    cols = scene(np.random.default_rng(200 + seed), 8_000, 20, 24, span=3_000, shuffle=True)
    assert (np.diff(cols[2]) < 0).any()
    check_baf(E, cols, (20, 24), 100.0, radius=1 + seed, same_polarity=bool(seed), support=2)
    check_refractory(E, cols, (20, 24), 40.0, per_polarity=bool(seed))


# ---- long runs -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def hot():
    rng = np.random.default_rng(300)
    n = 200_000
    x, y, t, p = scene(rng, n, span=2_000_000)
    stuck = rng.random(n) < 0.3
    x[stuck], y[stuck], p[stuck] = 17, 23, 1
    return x, y, t, p


def test_hot_pixel_support(E, hot):
    check_baf(E, hot, (H, W), 400.0, sup_fn=N.fast_support, radius=1, include_self=True, support=2)
    check_baf(E, hot, (H, W), 50.0, sup_fn=N.fast_support, radius=2, same_polarity=True, support=3)


@pytest.mark.parametrize("refractory", [0.0, 30.0, 1e5])
def test_hot_pixel_refractory(E, hot, refractory):
    keep = check_refractory(E, hot, (H, W), refractory, keep_fn=N.fast_refractory)
    check_refractory(E, hot, (H, W), refractory, per_polarity=True, keep_fn=N.fast_refractory)
    on_hot = (hot[0] == 17) & (hot[1] == 23)
    assert on_hot.sum() > 50_000 and (refractory == 0.0 or not keep[on_hot].all())


def test_runs_around_the_switch_to_a_wave(E):
    """runs just below, at and just above the length from which a wave walks a run, and around the wave's 64- and 256-event steps"""
    from event_utils_amd import _lib
    wr = _lib.EVK_DENOISE_WAVE_RUN
    lengths = sorted({1, 2, 63, 64, 65, 255, 256, 257, 513, wr - 1, wr, wr + 1, wr + 257})
    rng = np.random.default_rng(301)
    x = np.concatenate([np.full(m, k % 9) for k, m in enumerate(lengths)])
    y = np.concatenate([np.full(m, k // 9) for k, m in enumerate(lengths)])
    n = len(x)
    perm = rng.permutation(n)
    x, y = x[perm], y[perm]
    t = np.sort(rng.integers(0, 3 * n, n)).astype(np.float64)
    p = rng.integers(0, 2, n) * 2 - 1
    for refractory in (0.0, 3.0, 40.0, 1e9):
        check_refractory(E, (x, y, t, p), (3, 9), refractory)
    t = rng.permutation(t)
    check_refractory(E, (x, y, t, p), (3, 9), 10.0)
    check_refractory(E, (x, y, t, np.ones(n)), (3, 9), 10.0, per_polarity=True)
    check_baf(E, (x, y, t, p), (3, 9), 25.0, radius=1, include_self=True)


# ---- input kinds ---------------------------------------------------------------------------------------------------------

def test_numpy_dtypes_round_trip(E):
    x, y, t, p = scene(np.random.default_rng(400), 5_000, 16, 20, span=2_000)
    kinds = [(x, y, t, p > 0),                                                        # int64 / float64 / bool
             (x.astype(np.int16), y.astype(np.int16), (t.astype(np.int64) + 1_600_000_000_000_000), p.astype(np.int8)),
             (x.astype(np.int32), y.astype(np.int32), t.astype(np.float32), p.astype(np.float32)),
             (x.astype(np.float64), y.astype(np.float32), t, p.astype(np.float64))]
    for cols in kinds:
        check_baf(E, cols, (16, 20), 30.0, radius=2, same_polarity=True, support=2)
        check_refractory(E, cols, (16, 20), 25.0, per_polarity=True)
    # ps = None: the other three columns come back, the fourth stays None
    keep = N.seq_support(x, y, t, None, 30.0, (16, 20)) >= 1
    out = E.background_activity_filter(x, y, t, None, 30.0, sensor_size=(16, 20))
    assert out[3] is None
    for g, c in zip(out[:3], (x, y, t)):
        same(g, c[keep])
    keep = N.seq_refractory(x, y, t, None, 25.0, (16, 20))
    out = E.refractory_filter(x, y, t, None, 25.0, sensor_size=(16, 20))
    assert out[3] is None
    same(out[2], t[keep])
    same(E.neighbour_support(x, y, t, None, 30.0, sensor_size=(16, 20)), N.seq_support(x, y, t, None, 30.0, (16, 20)))


def test_device_tensors_float32(E):
    cols = [c.astype(np.float32) for c in scene(np.random.default_rng(401), 6_000, 16, 20, span=2_000)]
    dev = [torch.from_numpy(c).cuda() for c in cols]
    want = N.seq_support(*cols, 30.0, (16, 20), radius=1, same_polarity=True)
    s = E.neighbour_support(*dev, 30.0, sensor_size=(16, 20), same_polarity=True)
    assert isinstance(s, torch.Tensor) and s.is_cuda and s.dtype == torch.uint8
    same(s, want)
    out = E.background_activity_filter(*dev, 30.0, sensor_size=(16, 20), same_polarity=True, return_support=True)
    assert all(o.is_cuda for o in out)
    for g, c in zip(out[:4], cols):
        same(g, c[want >= 1])
    same(out[4], want)
    keep = N.seq_refractory(*cols, 25.0, (16, 20))
    for g, c in zip(E.refractory_filter(*dev, 25.0, sensor_size=(16, 20)), cols):
        assert g.is_cuda
        same(g, c[keep])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_device_events(E, dtype):
    cols = [c.astype(dtype) for c in scene(np.random.default_rng(402), 30_000, span=100_000)]
    ev = E.DeviceEvents.from_arrays(*cols, precision="f32" if dtype == np.float32 else "f64")
    want = N.fast_support(*cols, 200.0, (H, W), radius=2)
    r, s = E.background_activity_filter(ev, None, None, None, 200.0, sensor_size=(H, W), radius=2, support=2, return_support=True)
    assert isinstance(r, E.DeviceEvents) and r.t_offset == ev.t_offset and r.p_scale == ev.p_scale
    same(s, want)
    kept = [c[want >= 2] for c in cols]
    for g, w in zip(events_out(r), kept):
        same(g, w)
    assert r.t_at(0) == float(kept[2][0]) and r.t_at(-1) == float(kept[2][-1])
    keep = N.fast_refractory(*cols, 150.0, (H, W), per_polarity=True)
    r = E.refractory_filter(ev, None, None, None, 150.0, sensor_size=(H, W), per_polarity=True)
    assert isinstance(r, E.DeviceEvents)
    for g, c in zip(events_out(r), cols):
        same(g, c[keep])
    # a view that starts off a 16-byte boundary is read in place
    a, b = 3, 29_001
    sl = ev.slice(a, b)
    assert sl.x.data_ptr() % 16 != 0
    sub = [c[a:b] for c in cols]
    want = N.fast_support(*sub, 200.0, (H, W), same_polarity=True)
    for g, c in zip(events_out(E.background_activity_filter(sl, None, None, None, 200.0, sensor_size=(H, W), same_polarity=True)), sub):
        same(g, c[want >= 1])
    keep = N.fast_refractory(*sub, 150.0, (H, W))
    for g, c in zip(events_out(E.refractory_filter(sl, None, None, None, 150.0, sensor_size=(H, W))), sub):
        same(g, c[keep])


def test_relative_time_offset_cancels(E):
    x, y, t, p = scene(np.random.default_rng(403), 10_000, span=1_000_000)
    t = 1.6e9 + t * 1e-6
    ev = E.DeviceEvents.from_arrays(x.astype(np.float64), y.astype(np.float64), t, p.astype(np.float64), relative_time=True)
    assert ev.t_offset != 0.0
    stored = ev.t.cpu().numpy()
    want = N.fast_support(x, y, stored, p, 0.02, (H, W))
    r, s = E.background_activity_filter(ev, None, None, None, 0.02, sensor_size=(H, W), return_support=True)
    same(s, want)
    assert r.t_offset == ev.t_offset
    same(r.t, stored[want >= 1])


def test_return_support_agrees_with_neighbour_support(E, mixed):
    s = E.neighbour_support(*mixed, 300.0, sensor_size=(H, W), radius=2)
    for k in (1, 3):
        out = E.background_activity_filter(*mixed, 300.0, sensor_size=(H, W), radius=2, support=k, return_support=True)
        same(out[4], s)
        for g, c in zip(out[:4], mixed):
            same(g, c[s >= k])


def test_both_walk_orders_of_the_support_pass_agree(E, mixed, hot):
    """the support kernel takes the events in pixel order by default; its stream-order form counts the same"""
    from event_utils_amd import _lib
    from event_utils_amd import _grouping as G
    from event_utils_amd.util.event_util import _In
    for cols, dt, radius, fn in ((mixed, 300.0, 2, N.seq_support), (hot, 400.0, 1, N.fast_support)):
        want = fn(*cols, dt, (H, W), radius=radius, same_polarity=True)
        g = G.Grouped(_In(*cols), (H, W), True, "test")
        for walk in (_lib.EVK_DENOISE_WALK_STREAM, _lib.EVK_DENOISE_WALK_PIXEL, _lib.EVK_DENOISE_WALK_DEFAULT):
            sup, keep = g.support(dt, radius, False, 2, True, walk)
            same(sup, want)
            same(keep, (want >= 2).astype(np.uint8))


KINDS = [np.int16, np.int32, np.int64, np.float32, np.float64]            # the five EVK_SELECT_* kinds of a time column


@pytest.fixture(scope="module")
def run_lengths():
    """the run-length scene and its exact flags for every refractory period of the test below"""
    x, y, t, p, size = N.run_length_scene()
    return (x, y, t, p), size, {r: N.seq_refractory(x, y, t, p, r, size) for r in (0.0, 1.0, 40.0)}


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.__name__)
@pytest.mark.parametrize("refractory", [0.0, 1.0, 40.0])
@pytest.mark.parametrize("wave_run", [1, 64, 0, 1 << 30])
def test_refractory_on_runs_that_straddle_the_wave_steps(E, run_lengths, wave_run, refractory, kind):
    """runs of 1, 63 .. 65, 255 .. 257, 511 .. 513 and 769 events and an empty pixel, every kind of time column; wave_run 1:
    every run on the wave path (one, two and three steps of 256, the pipeline's depth); 64: the runs from 64 on; 0: the default
    and 2^30: every run on the lane path.  The flags are exact."""
    from event_utils_amd import _grouping as G
    from event_utils_amd.util.event_util import _In
    (x, y, t, p), size, want = run_lengths
    assert 0 < (~want[1.0]).sum() < (~want[40.0]).sum() and want[0.0].all()
    g = G.Grouped(_In(x, y, t.astype(kind), p), size, False, "test")
    same(g.refractory(refractory, wave_run), want[refractory].astype(np.uint8))


# ---- larger streams ------------------------------------------------------------------------------------------------------

def test_medium_stream(E):
    rng = np.random.default_rng(500)
    HH, WW, n = 480, 640, 1_000_000
    cols = scene(rng, n, HH, WW, span=2_000_000)
    want = check_baf(E, cols, (HH, WW), 20_000.0, sup_fn=N.fast_support)
    assert 0.05 * n < (want >= 1).sum() < 0.95 * n
    keep = check_refractory(E, cols, (HH, WW), 300_000.0, keep_fn=N.fast_refractory)
    assert 0.05 * n < keep.sum() < 0.999 * n


def test_voxel_grid_of_the_filtered_stream(E):
    """composition: the voxel grid of the filtered resident stream against the oracle's of the restatement's kept events"""
    x, y, t, p = scene(np.random.default_rng(501), 30_000, span=1 << 20)
    cols = [c.astype(np.float32) for c in (x, y, t / float(1 << 20), p)]
    dt = 2.0 ** -8
    ev = E.DeviceEvents.from_arrays(*cols, precision="f32")
    sup = N.fast_support(*cols, dt, (H, W))
    r = E.background_activity_filter(ev, None, None, None, dt, sensor_size=(H, W))
    r = E.refractory_filter(r, None, None, None, dt / 4, sensor_size=(H, W))
    kept = [c[sup >= 1] for c in cols]
    kept = [c[N.fast_refractory(*kept, dt / 4, (H, W))] for c in kept]
    assert 1_000 < len(kept[0]) < 29_000
    for g, w in zip(events_out(r), kept):
        same(g, w)
    vox = E.events_to_voxel_torch(r, None, None, None, 5, sensor_size=(H, W)).cpu().numpy().astype(np.float64)
    ref = R.events_to_voxel_torch(*kept, 5, sensor_size=(H, W), accum="f64")
    assert np.abs(vox - ref).max() <= 1e-5 * np.abs(ref).max()      # (the bound of the filters' own composition test)


# ---- errors --------------------------------------------------------------------------------------------------------------

def test_errors(E):
    x, y, t, p = scene(np.random.default_rng(600), 100, 8, 9, span=50)
    size = (8, 9)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            E.neighbour_support(x, y, t, p, bad, sensor_size=size)
        with pytest.raises(ValueError):
            E.background_activity_filter(x, y, t, p, bad, sensor_size=size)
        with pytest.raises(ValueError):
            E.refractory_filter(x, y, t, p, bad, sensor_size=size)
    for radius in (0, 4, -1):
        with pytest.raises(ValueError):
            E.neighbour_support(x, y, t, p, 1.0, sensor_size=size, radius=radius)
        with pytest.raises(ValueError):
            E.background_activity_filter(x, y, t, p, 1.0, sensor_size=size, radius=radius)
    for radius, include_self, support in ((1, False, 0), (1, False, 9), (1, True, 10), (2, False, 25), (3, True, 50)):
        with pytest.raises(ValueError):
            E.background_activity_filter(x, y, t, p, 1.0, sensor_size=size, radius=radius, include_self=include_self, support=support)
    E.background_activity_filter(x, y, t, p, 1.0, sensor_size=size, radius=1, include_self=True, support=9)      # the largest allowed
    with pytest.raises(TypeError):
        E.neighbour_support(x + 0.5, y.astype(np.float64), t, p, 1.0, sensor_size=size)
    with pytest.raises(TypeError):
        E.refractory_filter(torch.tensor([1.0, 2.5], device="cuda"), torch.tensor([1.0, 2.0], device="cuda"),
                            torch.tensor([0.0, 1.0], device="cuda"), None, 1.0, sensor_size=size)
    with pytest.raises(TypeError):
        E.background_activity_filter(x, y, t, None, 1.0, sensor_size=size, same_polarity=True)
    with pytest.raises(TypeError):
        E.refractory_filter(x, y, t, None, 1.0, sensor_size=size, per_polarity=True)
    for bx, by in ((9, 0), (0, 8), (-1, 0), (0, -1), (2 ** 40, 0)):
        xb, yb = x.copy(), y.copy()
        xb[50], yb[50] = bx, by
        with pytest.raises(ValueError):
            E.neighbour_support(xb, yb, t, p, 1.0, sensor_size=size)
        with pytest.raises(ValueError):
            E.refractory_filter(xb, yb, t, p, 1.0, sensor_size=size)
    # the calls after a rejected one are unaffected
    check_baf(E, (x, y, t, p), size, 5.0)


# ---- random slice --------------------------------------------------------------------------------------------------------

def test_random_configurations(E):
    master = np.random.default_rng(700)
    for case in range(200):
        rng = np.random.default_rng(master.integers(1 << 62))
        Hc, Wc = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        n = int(rng.integers(0, 5_001)) if case % 8 == 0 else int(rng.integers(0, 600))
        span = int(rng.integers(2, 4 * n + 3))
        cols = scene(rng, n, Hc, Wc, span=span, shuffle=bool(rng.integers(0, 4) == 0))
        radius, include_self, same_polarity = int(rng.integers(1, 4)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        most = (2 * radius + 1) ** 2 - (0 if include_self else 1)
        support = int(rng.integers(1, min(most, 6) + 1))
        dt = float(rng.choice([0.0, 1.0, span / 50.0, span / 5.0, 10.0 * span]))
        refractory = float(rng.choice([0.0, 1.0, span / 50.0, span / 5.0, 10.0 * span]))
        if rng.integers(0, 3) == 0:
            cols = (cols[0].astype(np.int16), cols[1].astype(np.int32), cols[2].astype(np.int64), cols[3] > 0)
        try:
            check_baf(E, cols, (Hc, Wc), dt, support=support, radius=radius, include_self=include_self, same_polarity=same_polarity)
            check_refractory(E, cols, (Hc, Wc), refractory, per_polarity=same_polarity)
        except AssertionError as e:
            raise AssertionError("case %d: sensor %dx%d n %d radius %d self %s polarity %s support %d dt %g refractory %g: %s" % (
                case, Hc, Wc, n, radius, include_self, same_polarity, support, dt, refractory, e))
