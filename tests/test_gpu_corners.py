"""GPU (-m gpu): fast_corners, harris_scores, harris_corners and corner_events (evk_corner.hip) against the host restatements of
tests/_corners_np.py (seq_*: the definition; fast_*: pinned to it in tests/test_cpu_corners.py).

eFAST uses only comparisons of float64 times: the flags must be EQUAL to the oracle's.  Harris scores:
|gpu - oracle| <= 2^-23 |oracle| + 1e-10 with NaN in the same places: the first term is the rounding to float32, the second covers
the order of the float64 sums (A + B <= 32, so those errors are about 1e-13).  harris_corners is checked against the scores the
GPU itself returned, so no event near the threshold has to be left out."""
import numpy as np
import pytest
import torch

import _corners_np as N

pytestmark = pytest.mark.gpu
WINDOWS = (dict(n_last=200), dict(dt=15.0))


@pytest.fixture(scope="module")
def E():
    import event_utils_amd as E
    assert torch.cuda.is_available()
    return E


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def flags_equal(got, want):
    got = host(got)
    assert got.dtype == np.bool_ and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), "%d of %d flags differ (%d corners wanted)" % ((got != want).sum(), want.size, want.sum())


def scores_close(got, want):
    got = host(got)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN in other places"
    ok = ~np.isnan(want)
    err = np.abs(got[ok].astype(np.float64) - want[ok].astype(np.float64))
    tol = 2.0 ** -23 * np.abs(want[ok].astype(np.float64)) + 1e-10
    assert (err <= tol).all(), "max error %g of the bound" % (err / tol).max()


def check(E, args, cols, size, tensors=None, polarities=("same", "ignore"), windows=WINDOWS, select=None):
    """the three functions on one input (`args`: what the caller passes; `cols`: the values the device holds, as numpy)"""
    for polarity in polarities:
        kw = dict(polarity=polarity, select=select)
        got = E.fast_corners(*args, sensor_size=size, **kw)
        if tensors is not None:
            assert (isinstance(got, torch.Tensor) and got.is_cuda) if tensors else isinstance(got, np.ndarray)
        flags_equal(got, N.fast_fast_corners(*cols, size, **kw))
        for window in windows:
            got = E.harris_scores(*args, sensor_size=size, **window, **kw)
            scores_close(got, N.fast_harris_scores(*cols, size, **window, **kw))
            flags_equal(E.harris_corners(*args, sensor_size=size, threshold=1.0, **window, **kw), host(got) > 1.0)


def stream(seed, n, H, W, ticks, shuffle=False):
    """a few blobs and uniform noise on integer ticks (ties occur): int64 pixels and polarities, float64 times"""
    rng = np.random.default_rng(seed)
    blob = rng.random(n) < 0.7
    cx, cy = rng.integers(0, W, 3), rng.integers(0, H, 3)
    which = rng.integers(0, 3, n)
    x = np.where(blob, np.clip(cx[which] + rng.integers(-3, 4, n), 0, W - 1), rng.integers(0, W, n))
    y = np.where(blob, np.clip(cy[which] + rng.integers(-3, 4, n), 0, H - 1), rng.integers(0, H, n))
    t = np.sort(rng.integers(0, ticks, n)).astype(np.float64)
    if shuffle:
        t = rng.permutation(t)
    return x.astype(np.int64), y.astype(np.int64), t, (rng.integers(0, 2, n) * 2 - 1).astype(np.int64)


@pytest.fixture(scope="module")
def mixed():
    return N.mixed_scene()


# ---- the mixed scene -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("polarity", ["same", "ignore"])
def test_mixed_scene_fast(E, mixed, polarity):
    x, y, t, p, size = mixed
    want = N.fast_fast_corners(x, y, t, p, size, polarity)
    el = N._eligible(x, y, *size)
    assert want.sum() >= 20 and (el & ~want).sum() >= 20
    got = E.fast_corners(x, y, t, p, sensor_size=size, polarity=polarity)
    assert isinstance(got, np.ndarray)
    flags_equal(got, want)
    part = slice(0, 600)                               # the definition itself on the first events
    flags_equal(got[part], N.seq_fast_corners(x[part], y[part], t[part], p[part], size, polarity))


@pytest.mark.parametrize("window", WINDOWS, ids=["n_last", "dt"])
@pytest.mark.parametrize("polarity", ["same", "ignore"])
def test_mixed_scene_harris(E, mixed, polarity, window):
    x, y, t, p, size = mixed
    want = N.fast_harris_scores(x, y, t, p, size, polarity=polarity, **window)
    el = N._eligible(x, y, *size)
    assert (want > 8.0).sum() >= 20 and (el & ~(want > 8.0)).sum() >= 20
    got = E.harris_scores(x, y, t, p, sensor_size=size, polarity=polarity, **window)
    scores_close(got, want)
    flags_equal(E.harris_corners(x, y, t, p, sensor_size=size, polarity=polarity, **window), got > 8.0)
    flags_equal(E.harris_corners(x, y, t, p, sensor_size=size, polarity=polarity, threshold=-1.0, **window), got > -1.0)
    scores_close(E.harris_scores(x, y, t, p, sensor_size=size, polarity=polarity, k=0.0, **window),
                 N.fast_harris_scores(x, y, t, p, size, polarity=polarity, k=0.0, **window))
    part = slice(0, 300)
    scores_close(got[part], N.seq_harris_scores(x[part], y[part], t[part], p[part], size, polarity=polarity, **window))


# ---- sizes and geometry --------------------------------------------------------------------------------------------------

def test_long_runs_and_a_hot_pixel(E):
    """12 x 12 with 60 000 events, a third of them on one pixel that every eligible event has in its patch or on a circle"""
    x, y, t, p = stream(11, 60_000, 12, 12, 90_000)
    hot = np.arange(60_000) % 3 == 0
    x[hot], y[hot], p[hot] = 6, 4, 1
    assert ((x == 6) & (y == 4)).sum() >= 20_000
    check(E, (x, y, t, p), (x, y, t, p), (12, 12), windows=(dict(n_last=40), dict(dt=25.0)))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 63, 64, 65, 257])
def test_event_counts_around_the_step_of_64(E, n):
    cols = stream(100 + n, n, 16, 16, 40)
    check(E, cols, cols, (16, 16), windows=(dict(n_last=30), dict(dt=10.0)))
    sel = np.arange(n)[::-1].copy()
    check(E, cols, cols, (16, 16), polarities=("same",), windows=(dict(n_last=30),), select=sel)


def test_no_events(E):
    e = np.zeros(0)
    for args in ((e, e, e, e), tuple(torch.zeros(0, device="cuda") for _ in range(4))):
        got = E.fast_corners(*args, sensor_size=(16, 16))
        assert got.shape == (0,) and host(got).dtype == np.bool_
        got = E.harris_scores(*args, sensor_size=(16, 16), dt=1.0)
        assert got.shape == (0,) and host(got).dtype == np.float32
        assert E.harris_corners(*args, sensor_size=(16, 16), n_last=3).shape == (0,)
        assert E.fast_corners(*args, sensor_size=(16, 16), select=[]).shape == (0,)
        out = E.corner_events(*args, sensor_size=(16, 16), return_index=True)
        assert len(out) == 5 and all(len(c) == 0 for c in out) and host(out[4]).dtype == np.int64
        with pytest.raises(IndexError):
            E.fast_corners(*args, sensor_size=(16, 16), select=[0])


@pytest.mark.parametrize("size", [(1, 1), (8, 40), (40, 8)])
def test_sensors_without_an_eligible_pixel(E, size):
    x, y, t, p = stream(size[1], 500, size[0], size[1], 100)
    for polarity in ("same", "ignore"):
        assert not host(E.fast_corners(x, y, t, p, sensor_size=size, polarity=polarity)).any()
        assert np.isnan(host(E.harris_scores(x, y, t, p, sensor_size=size, polarity=polarity, n_last=50))).all()
        assert not host(E.harris_corners(x, y, t, p, sensor_size=size, polarity=polarity, dt=5.0, threshold=-100.0)).any()


def test_a_sensor_with_one_eligible_pixel(E):
    x, y, t, p = stream(9, 3_000, 9, 9, 500)
    assert ((x == 4) & (y == 4)).sum() >= 20
    check(E, (x, y, t, p), (x, y, t, p), (9, 9), windows=(dict(n_last=60), dict(dt=12.0)))
    assert np.array_equal(~np.isnan(host(E.harris_scores(x, y, t, p, sensor_size=(9, 9), n_last=60))), (x == 4) & (y == 4))


def test_heavy_ties(E):
    cols = stream(12, 4_000, 14, 15, 8)
    assert len(np.unique(cols[2])) == 8
    check(E, cols, cols, (14, 15), windows=(dict(n_last=100), dict(dt=0.0), dict(dt=1.0)))


def test_unsorted_times(E):
    cols = stream(13, 5_000, 14, 18, 3_000, shuffle=True)
    assert (np.diff(cols[2]) < 0).any()
    check(E, cols, cols, (14, 18), windows=(dict(n_last=100), dict(dt=200.0)))


# ---- input kinds ---------------------------------------------------------------------------------------------------------

def test_time_columns_int64_float32_float64(E):
    x, y, t, p = stream(14, 5_000, 16, 20, 6_000)
    big = t.astype(np.int64) + 1_600_000_000_000_000  # beyond 2^24, inside 2^53: exact in double, ties only where the ticks tie
    for tcol in (big, t.astype(np.float32), t):
        cols = (x.astype(np.int16), y.astype(np.int32), tcol, p > 0)
        check(E, cols, cols, (16, 20), tensors=False, windows=(dict(n_last=150), dict(dt=40.0)))


def test_device_tensors(E):
    cols = [c.astype(np.float32) for c in stream(15, 6_000, 16, 20, 6_000)]
    check(E, [torch.from_numpy(c).cuda() for c in cols], cols, (16, 20), tensors=True, windows=(dict(n_last=150), dict(dt=40.0)))
    dev = [torch.from_numpy(c).cuda() for c in cols]
    flags_equal(E.fast_corners(dev[0], dev[1], dev[2], None, sensor_size=(16, 20), polarity="ignore"),
                N.fast_fast_corners(cols[0], cols[1], cols[2], None, (16, 20), "ignore"))


def test_device_events_with_a_time_offset(E):
    x, y, t, p = stream(16, 6_000, 16, 20, 6_000)
    t = t + 123_456.0
    ev = E.DeviceEvents.from_native(x.astype(np.int16), y.astype(np.int16), t, (p > 0).astype(np.uint8))
    assert ev.t_offset == t[0]
    stored = (t - t[0]).astype(np.float32)
    cols = (x.astype(np.float32), y.astype(np.float32), stored, p.astype(np.float32))
    check(E, (ev, None, None, None), cols, (16, 20), tensors=True, windows=(dict(n_last=150), dict(dt=40.0)))


def test_device_events_with_a_negative_polarity_scale(E):
    cols = [c.astype(np.float32) for c in stream(17, 6_000, 16, 20, 6_000)]
    ev = E.DeviceEvents.from_arrays(*cols, precision="f32").scaled(-2.0)
    assert ev.p_scale < 0
    flipped = (cols[0], cols[1], cols[2], -cols[3])
    check(E, (ev, None, None, None), flipped, (16, 20), tensors=True, windows=(dict(n_last=150),))


# ---- selections ----------------------------------------------------------------------------------------------------------

def test_select(E, mixed):
    x, y, t, p, size = mixed
    n = len(x)
    rng = np.random.default_rng(7)
    full_f = host(E.fast_corners(x, y, t, p, sensor_size=size))
    full_h = host(E.harris_scores(x, y, t, p, sensor_size=size, n_last=200))
    for select in ([], [n - 1], [5, 5, 5, 0, n - 1, 5], np.arange(n)[::-1].copy(), rng.integers(0, n, 1_000),
                   torch.from_numpy(rng.integers(0, n, 300)).cuda()):
        idx = host(select).astype(np.int64)
        got = E.fast_corners(x, y, t, p, sensor_size=size, select=select)
        flags_equal(got, N.fast_fast_corners(x, y, t, p, size, select=idx))
        assert np.array_equal(host(got), full_f[idx])
        got = host(E.harris_scores(x, y, t, p, sensor_size=size, n_last=200, select=select))
        assert got.shape == (len(idx),) and got.tobytes() == full_h[idx].tobytes()      # the same kernel arithmetic: bit for bit
        flags_equal(E.harris_corners(x, y, t, p, sensor_size=size, n_last=200, select=select), got > 8.0)
    for bad in ([-1], [n], [0, 5, n], [1.5], [[1, 2]], torch.tensor([n], device="cuda")):
        with pytest.raises(IndexError):
            E.fast_corners(x, y, t, p, sensor_size=size, select=bad)
        with pytest.raises(IndexError):
            E.harris_scores(x, y, t, p, sensor_size=size, dt=3.0, select=bad)


# ---- corner_events -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("detector,kw", [("fast", {}), ("harris", dict(n_last=200)), ("harris", dict(dt=15.0, threshold=4.0))])
def test_corner_events_are_the_flagged_events_in_stream_order(E, mixed, detector, kw):
    x, y, t, p, size = mixed
    flag_kw = dict(kw)
    flags = host(E.fast_corners(x, y, t, p, sensor_size=size) if detector == "fast"
                 else E.harris_corners(x, y, t, p, sensor_size=size, **flag_kw))
    assert 20 <= flags.sum() < len(x)
    want_index = np.flatnonzero(flags)
    # numpy in -> numpy out, the dtypes of the input
    out = E.corner_events(x, y, t, p, detector=detector, sensor_size=size, return_index=True, **kw)
    assert len(out) == 5 and all(isinstance(c, np.ndarray) for c in out)
    for got, col in zip(out[:4], (x, y, t, p)):
        assert got.dtype == col.dtype and np.array_equal(got, col[flags])
    assert out[4].dtype == np.int64 and np.array_equal(out[4], want_index)
    plain = E.corner_events(x, y, t, p, detector=detector, sensor_size=size, **kw)
    assert len(plain) == 4 and all(np.array_equal(a, b) for a, b in zip(plain, out[:4]))
    # device tensors
    cols32 = [c.astype(np.float32) for c in (x, y, t, p)]
    dev = [torch.from_numpy(c).cuda() for c in cols32]
    out = E.corner_events(*dev, detector=detector, sensor_size=size, return_index=True, **kw)
    assert len(out) == 5 and all(isinstance(c, torch.Tensor) and c.is_cuda for c in out)
    for got, col in zip(out[:4], cols32):
        assert np.array_equal(host(got), col[flags])
    assert out[4].dtype == torch.int64 and np.array_equal(host(out[4]), want_index)
    # a DeviceEvents
    ev = E.DeviceEvents.from_arrays(*cols32, precision="f32")
    kept, index = E.corner_events(ev, None, None, None, detector=detector, sensor_size=size, return_index=True, **kw)
    assert isinstance(kept, E.DeviceEvents) and len(kept) == flags.sum() and np.array_equal(host(index), want_index)
    for got, col in zip(kept._columns(), cols32):
        assert np.array_equal(host(got), col[flags])
    assert isinstance(E.corner_events(ev, None, None, None, detector=detector, sensor_size=size, **kw), E.DeviceEvents)
    # the indices select the rows of the full local time surfaces
    full = E.local_time_surfaces(*dev, 40.0, sensor_size=size, radius=2)
    rows = E.local_time_surfaces(*dev, 40.0, sensor_size=size, radius=2, select=out[4])
    assert rows.shape[0] == flags.sum() and torch.equal(rows, full[out[4]])


# ---- the hand-built cases of tests/test_cpu_corners.py, on the kernel ----------------------------------------------------------

def gpu_flag(E, cols, **kw):
    return bool(host(E.fast_corners(*cols, sensor_size=N.HAND_SIZE, **kw))[-1])


def test_hand_built_arcs(E):
    good3, good4 = N.arc(16, 2, 4), N.arc(20, 5, 6)
    for length, want in ((2, False), (3, True), (6, True), (7, False)):
        for start in (0, 5, 11, 14):
            assert gpu_flag(E, N.circle_stream(N.arc(16, start, length), good4)) is want, (length, start)
    for length, want in ((3, False), (4, True), (8, True), (9, False)):
        for start in (0, 7, 13, 17):
            assert gpu_flag(E, N.circle_stream(good3, N.arc(20, start, length))) is want, (length, start)
    assert gpu_flag(E, N.circle_stream(N.arc(16, 15, 3), N.arc(20, 19, 4)))       # both wrap past element 0
    assert gpu_flag(E, N.circle_stream([None if v == 1.0 else v for v in good3], good4))      # the rest unfired
    for hole in range(5):                              # an unfired pixel inside an arc
        v3 = N.arc(16, 4, 5)
        v3[4 + hole] = None
        assert gpu_flag(E, N.circle_stream(v3, good4)) is (hole in (0, 4))
    assert not gpu_flag(E, N.circle_stream([None] * 16, good4)) and not gpu_flag(E, N.circle_stream(good3, [None] * 20))
    v3 = N.arc(16, 6, 3)                               # ties
    tied = list(v3)
    tied[12] = v3[6]
    assert gpu_flag(E, N.circle_stream(v3, good4)) and not gpu_flag(E, N.circle_stream(tied, good4))
    v4 = N.arc(20, 9, 4)
    v4[0] = v4[9]
    assert not gpu_flag(E, N.circle_stream(good3, v4))
    cols = N.circle_stream(good3, good4, p3=-1)        # the other polarity
    assert not gpu_flag(E, cols, polarity="same") and gpu_flag(E, cols, polarity="ignore")
    x, y, t, p = N.circle_stream(good3, good4)         # the border: x = 3
    keep = x - 3 >= 0
    assert not host(E.fast_corners((x - 3)[keep], y[keep], t[keep], p[keep], sensor_size=N.HAND_SIZE))[-1]


def test_hand_worked_patches(E):
    def score(cols, **kw):
        return float(host(E.harris_scores(*cols, sensor_size=N.HAND_SIZE, **kw))[-1])

    def near(got, want):
        return abs(got - want) <= 2.0 ** -23 * abs(want) + 1e-10
    for b in (N.lone_patch(), N.edge_patch(), N.l_patch(), N.edge_patch().T, np.ones((9, 9), dtype=np.int64)):
        for k in (0.04, 0.0):
            assert near(score(N.patch_stream(b), n_last=1000, k=k), N.harris_score_of_patch(b, k))
    assert score(N.patch_stream(N.edge_patch()), n_last=1000) < 0 < score(N.patch_stream(N.l_patch()), n_last=1000)
    b = N.lone_patch()
    b[4, 6] = 1
    lone, pair = N.harris_score_of_patch(N.lone_patch()), N.harris_score_of_patch(b)
    x, y = np.array([8, 15, 15, 15, 15, 6]), np.array([6, 6, 6, 6, 6, 6])
    t, p = np.array([3.0, 4.0, 5.0, 6.0, 7.0, 10.0]), np.ones(6, dtype=np.int64)
    assert near(score((x, y, t, p), n_last=5), pair) and near(score((x, y, t, p), n_last=4), lone)
    assert near(score((x, y, t, p), dt=7.0), pair) and near(score((x, y, t, p), dt=np.nextafter(7.0, 0.0)), lone)
    t[0] = 10.0
    assert near(score((x, y, t, p), dt=0.0), pair)
    p[0] = -1
    assert near(score((x, y, t, p), dt=0.0), lone) and near(score((x, y, t, p), dt=0.0, polarity="ignore"), pair)
    assert np.isnan(score((x - 3, y, t, p), dt=0.0))


# ---- repeatability and errors --------------------------------------------------------------------------------------------

def test_results_repeat_bit_for_bit(E, mixed):
    x, y, t, p, size = mixed
    calls = [lambda: E.fast_corners(x, y, t, p, sensor_size=size),
             lambda: E.harris_scores(x, y, t, p, sensor_size=size, n_last=200),
             lambda: E.harris_scores(x, y, t, p, sensor_size=size, dt=15.0, polarity="ignore"),
             lambda: E.corner_events(x, y, t, p, detector="harris", dt=15.0, sensor_size=size, return_index=True)[4]]
    for call in calls:
        a, b, c = call(), call(), call()
        assert a.tobytes() == b.tobytes() == c.tobytes()


def test_errors(E):
    x, y, t, p = stream(18, 100, 12, 13, 50)
    size = (12, 13)
    calls = (lambda c, **kw: E.fast_corners(*c, sensor_size=size, **kw),
             lambda c, **kw: E.harris_scores(*c, sensor_size=size, n_last=10, **kw),
             lambda c, **kw: E.corner_events(*c, sensor_size=size, **kw))
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
        E.fast_corners(x, y, t, p, sensor_size=(0, 5))
    with pytest.raises(TypeError):
        E.harris_scores(x, y, t, p, sensor_size=size)
    with pytest.raises(ValueError):
        E.harris_scores(x, y, t, p, sensor_size=size, n_last=0)
    with pytest.raises(ValueError):
        E.harris_corners(x, y, t, p, sensor_size=size, dt=-1.0)
    with pytest.raises(ValueError):
        E.corner_events(x, y, t, p, detector="arc", sensor_size=size)
    with pytest.raises(TypeError):
        E.corner_events(x, y, t, p, sensor_size=size, select=[1])
    # the calls after a rejected one are unaffected; ps may be None with one class
    flags_equal(E.fast_corners(x, y, t, None, sensor_size=size, polarity="ignore"), N.fast_fast_corners(x, y, t, None, size, "ignore"))
    scores_close(E.harris_scores(x, y, t, p, sensor_size=size, dt=5.0), N.fast_harris_scores(x, y, t, p, size, dt=5.0))
