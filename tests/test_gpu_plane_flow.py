"""GPU (-m gpu): local_plane_flow and plane_flow_field (evk_planeflow.hip) against the host restatements of
tests/_plane_flow_np.py (seq_*: the definition; fast_*: pinned to it bit for bit in tests/test_cpu_plane_flow.py).

The definition fixes every double operation and its order, so both sides do the same float64 arithmetic: `valid` and `count` must be
EQUAL to the oracle's and NaN must stand in the same places.  Flow, lifetime and field: |gpu - oracle| <= 2^-23 |oracle| + 1e-10, the
bound of test_gpu_corners.py::scores_close -- the one rounding to float32 that the definition leaves.  No event is left out of any
comparison."""
import numpy as np
import pytest
import torch

import _plane_flow_np as N

pytestmark = pytest.mark.gpu
SIZE = (24, 32)


@pytest.fixture(scope="module")
def E():
    import event_utils_amd as E
    assert torch.cuda.is_available()
    return E


@pytest.fixture(scope="module")
def edge():
    return N.edge_scene()


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def values_close(got, want):
    got = host(got)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN in other places"
    ok = ~np.isnan(want)
    err = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))
    tol = 2.0 ** -23 * np.abs(want[ok].astype(np.float64)) + 1e-10
    assert (err <= tol).all(), "max error %g of the bound" % (err / tol).max()


def flags_equal(got, want):
    got = host(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), "%d of %d differ (%d set in the oracle)" % ((got != want).sum(), want.size, (want != 0).sum())


def check(E, args, cols, size, dt, tensors=None, fields=True, select=None, **kw):
    """both functions on one input (`args`: what the caller passes; `cols`: the values the device holds, as numpy); -> the oracle's
    (flow, valid, lifetime)"""
    want = N.fast_local_plane_flow(*cols, dt, size, select=select, **kw)
    got = E.local_plane_flow(*args, dt, sensor_size=size, select=select, return_valid=True, return_lifetime=True, **kw)
    assert len(got) == 3
    if tensors is not None:
        assert all((isinstance(g, torch.Tensor) and g.is_cuda) if tensors else isinstance(g, np.ndarray) for g in got)
    flags_equal(got[1], want[1])
    values_close(got[0], want[0])
    values_close(got[2], want[2])
    assert np.array_equal(np.isnan(host(got[0])[:, 0]), ~want[1]) and np.array_equal(np.isnan(host(got[2])), ~want[1])
    if fields and select is None:
        wf, wc = N.fast_field_of_flow(cols[0], cols[1], cols[3], want[0], want[1], size, kw.get("polarity", "same"))
        gf, gc = E.plane_flow_field(*args, dt, sensor_size=size, return_count=True, **kw)
        flags_equal(gc, wc)
        values_close(gf, wf)
        assert host(gf).shape == (2,) + tuple(size) and not host(gf)[:, wc == 0].any()
    return want


def stream(seed, n, H, W, ticks, shuffle=False):
    """uniform noise and a moving column on integer ticks (ties occur): int64 pixels and polarities, float64 times"""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(0, ticks, n)).astype(np.float64)
    edge = rng.random(n) < 0.6
    x = np.where(edge, np.clip((t * W / max(ticks, 1)).astype(np.int64) + rng.integers(-1, 2, n), 0, W - 1), rng.integers(0, W, n))
    y = rng.integers(0, H, n)
    if shuffle:
        t = rng.permutation(t)
    return x.astype(np.int64), y.astype(np.int64), t, (rng.integers(0, 2, n) * 2 - 1).astype(np.int64)


# ---- the moving edge -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("polarity", ["same", "ignore"])
@pytest.mark.parametrize("radius", [1, 2, 3, 4])
def test_edge_scene(E, edge, radius, polarity):
    for kw in (dict(), dict(outlier_threshold=N.EDGE_TH), dict(outlier_threshold=N.EDGE_TH, iterations=0),
               dict(outlier_threshold=N.EDGE_TH, iterations=1), dict(outlier_threshold=15.0, iterations=2, max_speed=0.03),
               dict(max_speed=0.05, min_samples=3)):
        want = check(E, edge, edge, SIZE, N.EDGE_DT, tensors=False, radius=radius, polarity=polarity, **kw)
        assert 0.05 * len(edge[0]) < want[1].sum() < 0.99 * len(edge[0])      # both outcomes are populated


def test_edge_scene_against_the_definition_itself(E, edge):
    part = tuple(c[:600] for c in edge)
    for kw in (dict(radius=2, outlier_threshold=N.EDGE_TH), dict(radius=3, polarity="ignore", outlier_threshold=15.0, max_speed=0.05)):
        want = N.seq_local_plane_flow(*part, N.EDGE_DT, SIZE, **kw)
        got = E.local_plane_flow(*part, N.EDGE_DT, sensor_size=SIZE, return_valid=True, return_lifetime=True, **kw)
        flags_equal(got[1], want[1])
        values_close(got[0], want[0])
        values_close(got[2], want[2])
        wf, wc = N.seq_plane_flow_field(*part, N.EDGE_DT, SIZE, **kw)
        gf, gc = E.plane_flow_field(*part, N.EDGE_DT, sensor_size=SIZE, return_count=True, **kw)
        flags_equal(gc, wc)
        values_close(gf, wf)


def test_return_kinds(E, edge):
    flow = E.local_plane_flow(*edge, N.EDGE_DT, sensor_size=SIZE)
    assert isinstance(flow, np.ndarray) and flow.shape == (3000, 2) and flow.dtype == np.float32
    flow2, valid = E.local_plane_flow(*edge, N.EDGE_DT, sensor_size=SIZE, return_valid=True)
    flow3, life = E.local_plane_flow(*edge, N.EDGE_DT, sensor_size=SIZE, return_lifetime=True)
    assert valid.dtype == np.bool_ and life.dtype == np.float32 and flow.tobytes() == flow2.tobytes() == flow3.tobytes()
    field = E.plane_flow_field(*edge, N.EDGE_DT, sensor_size=SIZE)
    assert isinstance(field, np.ndarray) and field.shape == (2, 24, 32) and field.dtype == np.float32


# ---- sizes and geometry --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_event_counts_around_the_step_of_64(E, n):
    cols = stream(100 + n, n, 8, 8, 40)
    for radius in (1, 2, 4):
        check(E, cols, cols, (8, 8), 30.0, radius=radius, min_samples=3, outlier_threshold=4.0)
    sel = np.arange(n)[::-1].copy()
    check(E, cols, cols, (8, 8), 30.0, radius=3, min_samples=3, select=sel)


def test_no_events(E):
    e = np.zeros(0)
    for args in ((e, e, e, e), tuple(torch.zeros(0, device="cuda") for _ in range(4))):
        flow, valid, life = E.local_plane_flow(*args, 1.0, sensor_size=(16, 16), return_valid=True, return_lifetime=True)
        assert flow.shape == (0, 2) and valid.shape == (0,) and life.shape == (0,)
        assert host(flow).dtype == np.float32 and host(valid).dtype == np.bool_ and host(life).dtype == np.float32
        assert E.local_plane_flow(*args, 1.0, sensor_size=(16, 16), select=[]).shape == (0, 2)
        field, count = E.plane_flow_field(*args, 1.0, sensor_size=(6, 7), return_count=True)
        assert field.shape == (2, 6, 7) and count.shape == (6, 7) and not host(field).any() and not host(count).any()
        assert host(field).dtype == np.float32 and host(count).dtype == np.int32
        with pytest.raises(IndexError):
            E.local_plane_flow(*args, 1.0, sensor_size=(16, 16), select=[0])


@pytest.mark.parametrize("size", [(1, 1), (2, 5), (5, 2)])
def test_sensors_smaller_than_the_window(E, size):
    cols = stream(size[1], 500, size[0], size[1], 100)
    for radius in (1, 2, 4):
        for polarity in ("same", "ignore"):
            want = check(E, cols, cols, size, 30.0, radius=radius, polarity=polarity, min_samples=3, outlier_threshold=6.0)
            assert size != (1, 1) or not want[1].any()
    assert size == (1, 1) or check(E, cols, cols, size, 30.0, radius=2, polarity="ignore", min_samples=3)[1].any()


def test_a_hot_pixel(E):
    """a third of 6000 events on one pixel: a run of 2000 in the searches of its neighbours and in one lane of the field pass"""
    x, y, t, p = stream(11, 6_000, 10, 12, 9_000)
    hot = np.arange(6_000) % 3 == 0
    x[hot], y[hot], p[hot] = 6, 4, 1
    assert ((x == 6) & (y == 4)).sum() >= 2_000
    for radius in (2, 4):
        check(E, (x, y, t, p), (x, y, t, p), (10, 12), 60.0, radius=radius, outlier_threshold=8.0)


def test_heavy_ties(E):
    cols = stream(12, 3_000, 10, 11, 1)
    assert len(np.unique(cols[2])) == 1               # all times equal: every tau is 0, every gradient is 0
    want = check(E, cols, cols, (10, 11), 0.0, radius=2)
    assert not want[1].any()
    cols = stream(13, 3_000, 10, 11, 6)
    assert len(np.unique(cols[2])) == 6
    for dt in (0.0, 1.0, 3.0):
        check(E, cols, cols, (10, 11), dt, radius=2, outlier_threshold=1.0)


def test_unsorted_times(E):
    cols = stream(14, 3_000, 12, 14, 2_000, shuffle=True)
    assert (np.diff(cols[2]) < 0).any()
    for radius in (1, 3):
        check(E, cols, cols, (12, 14), 150.0, radius=radius, outlier_threshold=30.0)


# ---- input kinds ---------------------------------------------------------------------------------------------------------

def test_time_columns_int64_float32_float64(E, edge):
    x, y, t, p = edge
    big = t.astype(np.int64) + 1_600_000_000_000_000  # beyond 2^24, inside 2^53: exact in double, ties only where the ticks tie
    for tcol in (big, t.astype(np.float32), t):
        cols = (x.astype(np.int16), y.astype(np.int32), tcol, p > 0)
        check(E, cols, cols, SIZE, N.EDGE_DT, tensors=False, outlier_threshold=N.EDGE_TH)


def test_device_tensors(E, edge):
    cols = [c.astype(np.float32) for c in edge]
    dev = [torch.from_numpy(c).cuda() for c in cols]
    check(E, dev, cols, SIZE, N.EDGE_DT, tensors=True, outlier_threshold=N.EDGE_TH)
    got = E.local_plane_flow(dev[0], dev[1], dev[2], None, N.EDGE_DT, sensor_size=SIZE, polarity="ignore")
    values_close(got, N.fast_local_plane_flow(cols[0], cols[1], cols[2], None, N.EDGE_DT, SIZE, polarity="ignore")[0])
    field, count = E.plane_flow_field(*dev, N.EDGE_DT, sensor_size=SIZE, return_count=True)
    assert field.is_cuda and count.is_cuda and field.dtype == torch.float32 and count.dtype == torch.int32


def test_device_events_with_a_time_offset(E, edge):
    x, y, t, p = edge
    t = t + 123_456.0
    ev = E.DeviceEvents.from_native(x.astype(np.int16), y.astype(np.int16), t, (p > 0).astype(np.uint8))
    assert ev.t_offset == t[0]
    stored = (t - t[0]).astype(np.float32)
    cols = (x.astype(np.float32), y.astype(np.float32), stored, p.astype(np.float32))
    check(E, (ev, None, None, None), cols, SIZE, N.EDGE_DT, tensors=True, outlier_threshold=N.EDGE_TH)


def test_device_events_with_a_negative_polarity_scale(E, edge):
    cols = [c.astype(np.float32) for c in edge]
    ev = E.DeviceEvents.from_arrays(*cols, precision="f32").scaled(-2.0)
    assert ev.p_scale < 0
    flipped = (cols[0], cols[1], cols[2], -cols[3])    # the classes swap: the field sums the other class first
    check(E, (ev, None, None, None), flipped, SIZE, N.EDGE_DT, tensors=True, outlier_threshold=N.EDGE_TH)


# ---- selections ----------------------------------------------------------------------------------------------------------

def test_select(E, edge):
    n = len(edge[0])
    rng = np.random.default_rng(7)
    kw = dict(sensor_size=SIZE, outlier_threshold=N.EDGE_TH, return_valid=True, return_lifetime=True)
    full = [host(a) for a in E.local_plane_flow(*edge, N.EDGE_DT, **kw)]
    for select in ([], [n - 1], [5, 5, 5, 0, n - 1, 5], np.arange(n)[::-1].copy(), rng.integers(0, n, 1_000),
                   torch.from_numpy(rng.integers(0, n, 300)).cuda()):
        idx = host(select).astype(np.int64)
        got = [host(a) for a in E.local_plane_flow(*edge, N.EDGE_DT, select=select, **kw)]
        assert got[0].shape == (len(idx), 2) and got[1].shape == got[2].shape == (len(idx),)
        for g, f in zip(got, full):                    # the same kernel arithmetic: bit for bit
            assert g.dtype == f.dtype and g.tobytes() == f[idx].tobytes()
        check(E, edge, edge, SIZE, N.EDGE_DT, select=idx, outlier_threshold=N.EDGE_TH)
    for bad in ([-1], [n], [0, 5, n], [1.5], [[1, 2]], torch.tensor([n], device="cuda")):
        with pytest.raises(IndexError):
            E.local_plane_flow(*edge, N.EDGE_DT, sensor_size=SIZE, select=bad)


# ---- the hand-worked cases of tests/test_cpu_plane_flow.py, on the kernel -------------------------------------------------------

def test_hand_worked_cases(E):
    def last(cols, dt=1000.0, **kw):
        flow, valid, life = E.local_plane_flow(*cols, dt, sensor_size=N.HAND_SIZE, return_valid=True, return_lifetime=True, **kw)
        want = N.seq_local_plane_flow(*cols, dt, N.HAND_SIZE, **kw)
        flags_equal(valid, want[1])
        values_close(flow, want[0])
        values_close(life, want[2])
        return float(flow[-1, 0]), float(flow[-1, 1]), float(life[-1]), bool(valid[-1])
    assert last(N.window_stream(N.plane_taus(4.0, 0.0))) == (0.25, 0.0, 4.0, True)
    assert last(N.window_stream(N.plane_taus(0.0, -2.0))) == (0.0, -0.5, 2.0, True)
    for r in (1, 3, 4):
        assert last(N.window_stream(N.plane_taus(4.0, 0.0, r), r), radius=r) == (0.25, 0.0, 4.0, True)
    cols = N.window_stream(N.plane_taus(4.0, 0.0))    # the other polarity
    cols[3][:-1] = -1
    assert not last(cols)[3] and last(cols, polarity="ignore") == (0.25, 0.0, 4.0, True)
    taus = [[None] * 5 for _ in range(5)]              # a single row of samples: D == 0
    taus[2] = [4.0 * dx for dx in range(-2, 3)]
    assert not last(N.window_stream(taus), min_samples=3)[3]
    taus = [[None] * 5 for _ in range(5)]              # n = min_samples - 1, and a sample that dt takes away
    taus[2][3], taus[3][2], taus[1][1], taus[3][4] = 4.0, 0.0, -4.0, 8.0
    cols = N.window_stream(taus)
    assert last(cols, min_samples=5) == (0.25, 0.0, 4.0, True) and not last(cols, min_samples=6)[3]
    assert not last(cols, dt=3.5, min_samples=5)[3] and last(cols, dt=4.0, min_samples=5)[3]
    taus = N.plane_taus(4.0, 0.0)                      # one gross outlier
    taus[0][4] = 500.0
    cols = N.window_stream(taus)
    plain = last(cols)
    assert plain[3] and plain[:3] != (0.25, 0.0, 4.0)
    assert last(cols, outlier_threshold=100.0, iterations=1) == (0.25, 0.0, 4.0, True)
    assert last(cols, outlier_threshold=100.0, iterations=2) == (0.25, 0.0, 4.0, True)
    assert last(cols, outlier_threshold=100.0, iterations=0) == plain and last(cols, outlier_threshold=1000.0) == plain
    assert not last(cols, outlier_threshold=100.0, iterations=1, min_samples=25)[3]      # a failed refit
    assert not last(N.window_stream(N.plane_taus(0.0, 0.0)))[3]      # a zero gradient
    cols = N.window_stream(N.plane_taus(4.0, 0.0))    # max_speed on either side of 1 / sqrt(g) = 0.25
    assert last(cols, max_speed=0.25) == (0.25, 0.0, 4.0, True)
    assert not last(cols, max_speed=float(np.nextafter(0.25, 0.0)))[3]
    x, y, t, p = cols                                  # the window clipped at x = 1
    keep = x - 4 >= 0
    assert last(((x - 4)[keep], y[keep], t[keep], p[keep])) == (0.25, 0.0, 4.0, True)


# ---- the field -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("polarity", ["same", "ignore"])
def test_the_field_is_the_average_of_the_per_event_flow(E, edge, polarity):
    """plane_flow_field against local_plane_flow's OWN output averaged per pixel in the defined order: the same float32 inputs and the
    same float64 sums on both sides, so the fields are equal bit for bit"""
    kw = dict(sensor_size=SIZE, polarity=polarity, outlier_threshold=N.EDGE_TH)
    flow, valid = E.local_plane_flow(*edge, N.EDGE_DT, return_valid=True, **kw)
    field, count = E.plane_flow_field(*edge, N.EDGE_DT, return_count=True, **kw)
    for fn in (N.field_of_flow, N.fast_field_of_flow):
        wf, wc = fn(edge[0], edge[1], edge[3], flow, valid, SIZE, polarity)
        flags_equal(count, wc)
        assert field.tobytes() == wf.tobytes()
    assert count.sum() == valid.sum() and count.max() >= 3 and (count == 0).any()
    if polarity == "same":                             # a pixel where the class order matters exists in the scene
        both = np.zeros(SIZE, dtype=np.int64)
        for cls in (edge[3] > 0, edge[3] <= 0):
            seen = np.zeros(SIZE, dtype=bool)
            seen[edge[1][cls & valid], edge[0][cls & valid]] = True
            both += seen
        assert (both == 2).any()


def test_the_field_feeds_the_flow_field_functions(E, edge):
    cols = [torch.from_numpy(c.astype(np.float32)).cuda() for c in edge]
    field = E.plane_flow_field(*cols, N.EDGE_DT, sensor_size=SIZE, outlier_threshold=N.EDGE_TH)
    assert field.is_cuda and field.shape == (2, 24, 32) and field.dtype == torch.float32 and bool(torch.isfinite(field).all())
    iwe = E.flow_field_iwe(field, *cols)               # (the sensor size is the field's)
    assert tuple(iwe.shape) == (SIZE[0] + 1, SIZE[1] + 1) and bool(torch.isfinite(iwe).all())
    zero = E.flow_field_iwe(torch.zeros_like(field), *cols)
    assert not torch.equal(iwe, zero)                  # the field moves events
    for loss_fn in (E.flow_field_contrast_loss, E.flow_field_timestamp_loss):
        loss, grad = loss_fn(field, *cols, compute_gradient=True)
        assert bool(torch.isfinite(loss).all()) and grad.shape == field.shape and bool(torch.isfinite(grad).all())
    ev = E.DeviceEvents.from_arrays(*(c.cpu().numpy() for c in cols), precision="f32")
    field_ev = E.plane_flow_field(ev, None, None, None, N.EDGE_DT, sensor_size=SIZE, outlier_threshold=N.EDGE_TH)
    assert torch.equal(field_ev, field) and bool(torch.isfinite(E.flow_field_contrast_loss(field_ev, ev)).all())
    from event_utils_amd.transforms.optic_flow import warp_events_flow_torch
    moved = warp_events_flow_torch(*cols, field)
    assert len(moved) >= 2 and moved[0].shape == cols[0].shape and bool(torch.isfinite(moved[0]).all())


# ---- repeatability and errors --------------------------------------------------------------------------------------------

def test_results_repeat_bit_for_bit(E, edge):
    calls = [lambda: E.local_plane_flow(*edge, N.EDGE_DT, sensor_size=SIZE, radius=4, outlier_threshold=N.EDGE_TH),
             lambda: E.local_plane_flow(*edge, N.EDGE_DT, sensor_size=SIZE, polarity="ignore", return_lifetime=True)[1],
             lambda: E.plane_flow_field(*edge, N.EDGE_DT, sensor_size=SIZE, outlier_threshold=N.EDGE_TH)]
    for call in calls:
        a, b, c = call(), call(), call()
        assert a.tobytes() == b.tobytes() == c.tobytes()


def test_errors(E):
    x, y, t, p = stream(18, 100, 12, 13, 50)
    size = (12, 13)
    calls = (lambda c, **kw: E.local_plane_flow(*c, 10.0, sensor_size=size, **kw),
             lambda c, **kw: E.plane_flow_field(*c, 10.0, sensor_size=size, **kw))
    for bx, by in ((13, 0), (0, 12), (-1, 0), (0, -1), (2 ** 40, 0)):      # a pixel off the sensor
        xb, yb = x.copy(), y.copy()
        xb[50], yb[50] = bx, by
        for call in calls:
            with pytest.raises(ValueError):
                call((xb, yb, t, p))
    for call in calls:
        with pytest.raises(TypeError):
            call((x + 0.5, y.astype(np.float64), t, p))      # pixels with fractions
        with pytest.raises(TypeError):
            call((x, y, t, None))                      # classes without ps
        with pytest.raises(TypeError):
            call((x, y, None, p))
        with pytest.raises(ValueError):
            call((x, y, t, p), polarity="split")
        with pytest.raises(ValueError):
            call((x, y, t, p), radius=5)
        with pytest.raises(ValueError):
            call((x, y, t, p), min_samples=26)
    with pytest.raises(ValueError):
        E.local_plane_flow(x, y, t, p, 10.0, sensor_size=(0, 5))
    # the calls after a rejected one are unaffected; ps may be None with one class
    check(E, (x, y, t, None), (x, y, t, None), size, 10.0, polarity="ignore", min_samples=3)
