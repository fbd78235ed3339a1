"""GPU (-m gpu): time_surfaces, local_time_surfaces and averaged_time_surfaces (evk_tsurf.hip) against the host restatements of
tests/_time_surface_np.py (seq_*: the definition; fast_*: pinned to it in tests/test_cpu_time_surface.py).

Tolerances are derived, not tuned.  Ages (decay=None) are differences of two stored values in float64: exact.  Zero elements
(empty pixels, pixels off the sensor, HATS cells without events) are exact and in the same places.  The device evaluates exp,
the linear decay and the HATS sums in double, where the double-precision exp and sums of fewer than 2^20 terms in (0, 1] are off
by relative errors many orders below 2^-24; so only the final rounding to float32 can land on the other side of a rounding
boundary: |got - want| <= np.spacing(float32(want)).  Counts are exact."""
import numpy as np
import pytest
import torch

import _time_surface_np as N

pytestmark = pytest.mark.gpu
H, W = 48, 64
DECAYS = ("exp", "linear", None)


@pytest.fixture(scope="module")
def E():
    import event_utils_amd as E
    assert torch.cuda.is_available()
    return E


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def close(got, want):
    got, want = host(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if want.dtype != np.float32:                       # ages and counts: exact (inf == inf)
        assert np.array_equal(got, want), "%d of %d elements differ" % ((got != want).sum(), want.size)
        return
    assert np.array_equal(got == 0, want == 0), "zeros in other places"
    assert np.isfinite(want).all()
    err, tol = np.abs(got.astype(np.float64) - want.astype(np.float64)), np.spacing(np.abs(want)).astype(np.float64)
    assert (err <= tol).all(), "max error %g float32 spacings" % (err / tol).max()


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


@pytest.fixture(scope="module")
def mixed():
    return scene(np.random.default_rng(100), 20_000)


@pytest.fixture(scope="module")
def hot():
    """one pixel holds 3 000 of 6 000 events on an 8 x 8 sensor: runs long enough for the searches and the HATS window walk"""
    rng = np.random.default_rng(300)
    x, y, t, p = scene(rng, 6_000, 8, 8, span=60_000)
    stuck = np.arange(6_000) % 2 == 0
    x[stuck], y[stuck], p[stuck] = 5, 3, 1
    return x, y, t, p


TAU = 4_000.0                                          # ages reach 50 000: exp(-12.5) stays a normal float32


# ---- mixed scene ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("polarity", ["split", "ignore"])
@pytest.mark.parametrize("decay", DECAYS)
def test_mixed_scene_surfaces_of_active_events(E, mixed, decay, polarity):
    x, y, t, p = mixed
    n = len(x)
    cuts = [0, n, 13_001, 64, 7_777]                   # K = 5: the two ends and unsorted cuts between them
    kw = dict(decay=decay, polarity=polarity)
    got = E.time_surfaces(x, y, t, p, TAU, sensor_size=(H, W), indices=cuts, **kw)
    assert isinstance(got, np.ndarray) and got.shape == (5, 2 if polarity == "split" else 1, H, W)
    close(got, N.fast_time_surfaces(x, y, t, p, TAU, (H, W), indices=cuts, **kw))
    tied = t[np.flatnonzero(np.diff(t) == 0)[5]]
    assert (t == tied).sum() >= 2
    refs = [t[0] - 1.0, t[-1] + 1.0, tied, t[0], 25_000.5]      # before the first event, after the last, on a tied stamp
    got = E.time_surfaces(x, y, t, p, TAU, sensor_size=(H, W), t_refs=refs, **kw)
    want = N.fast_time_surfaces(x, y, t, p, TAU, (H, W), t_refs=refs, **kw)
    close(got, want)
    assert not np.isfinite(host(got)[0]).any() if decay is None else not host(got)[0].any()
    close(E.time_surfaces(x, y, t, p, TAU, sensor_size=(H, W), t_refs=[refs[2]], **kw), want[2:3])      # K = 1
    close(E.time_surfaces(x, y, t, p, TAU, sensor_size=(H, W), indices=np.array([n]), **kw),
          N.fast_time_surfaces(x, y, t, p, TAU, (H, W), indices=[n], **kw))


@pytest.mark.parametrize("radius,decay,polarity,include_self", [
    (1, "exp", "same", True), (1, None, "split", False), (1, "linear", "ignore", True),
    (2, "linear", "split", True), (2, None, "same", False), (2, "exp", "ignore", False),
    (3, "exp", "split", True), (3, "linear", "same", False), (3, None, "ignore", True),
    (4, None, "split", True), (4, "exp", "same", False), (4, "linear", "ignore", False), (4, "exp", "split", False)])
def test_mixed_scene_local_surfaces(E, mixed, radius, decay, polarity, include_self):
    kw = dict(radius=radius, decay=decay, polarity=polarity, include_self=include_self)
    got = E.local_time_surfaces(*mixed, TAU, sensor_size=(H, W), **kw)
    P = 2 * radius + 1
    assert got.shape == (20_000, 2 if polarity == "split" else 1, P, P)
    close(got, N.fast_local_time_surfaces(*mixed, TAU, (H, W), **kw))


@pytest.mark.parametrize("radius,normalise,cell_size", [(1, True, 10), (2, False, 10), (3, True, 10), (4, False, 10), (4, True, 7)])
def test_mixed_scene_hats(E, mixed, radius, normalise, cell_size):
    kw = dict(cell_size=cell_size, radius=radius, normalise=normalise)
    got, counts = E.averaged_time_surfaces(*mixed, 500.0, 1_500.0, sensor_size=(H, W), return_counts=True, **kw)
    P = 2 * radius + 1
    assert got.shape == (-(-H // cell_size), -(-W // cell_size), 2, P, P) and counts.sum() == 20_000
    want, wc = N.fast_averaged_time_surfaces(*mixed, 500.0, 1_500.0, (H, W), return_counts=True, **kw)
    close(counts, wc)
    close(got, want)
    assert (want > 0).mean() > 0.5
    close(E.averaged_time_surfaces(*mixed, 500.0, 1_500.0, sensor_size=(H, W), **kw), want)


# ---- input kinds ---------------------------------------------------------------------------------------------------------

def check_all(E, args, cols, size, refs_shift=0.0, tensors=True):
    """the three functions on one input (`args`: what the caller passes; `cols`: the values the device holds, as numpy)"""
    n = len(cols[0])
    cuts = [n // 3, n]
    refs = np.array([cols[2][n // 2], cols[2][-1] + 1.0])
    outs = [(E.time_surfaces(*args, 900.0, sensor_size=size, indices=cuts),
             N.fast_time_surfaces(*cols, 900.0, size, indices=cuts)),
            (E.time_surfaces(*args, 900.0, sensor_size=size, t_refs=refs + refs_shift, decay=None, polarity="ignore"),
             N.fast_time_surfaces(*cols, 900.0, size, t_refs=refs, decay=None, polarity="ignore")),
            (E.local_time_surfaces(*args, 900.0, sensor_size=size, radius=2, polarity="split"),
             N.fast_local_time_surfaces(*cols, 900.0, size, radius=2, polarity="split")),
            (E.local_time_surfaces(*args, 900.0, sensor_size=size, radius=1, decay=None, select=[n - 1, 0, n - 1]),
             N.fast_local_time_surfaces(*cols, 900.0, size, radius=1, decay=None, select=[n - 1, 0, n - 1]))]
    h = E.averaged_time_surfaces(*args, 300.0, 800.0, sensor_size=size, cell_size=6, radius=2, return_counts=True)
    wh = N.fast_averaged_time_surfaces(*cols, 300.0, 800.0, size, cell_size=6, radius=2, return_counts=True)
    outs += list(zip(h, wh))
    for got, want in outs:
        assert (isinstance(got, torch.Tensor) and got.is_cuda) if tensors else isinstance(got, np.ndarray)
        close(got, want)


def test_numpy_columns(E):
    x, y, t, p = scene(np.random.default_rng(400), 5_000, 16, 20, span=8_000)
    check_all(E, (x, y, t, p), (x, y, t, p), (16, 20), tensors=False)
    cols = (x.astype(np.int16), y.astype(np.int32), t.astype(np.int64) + 1_600_000_000_000_000, p > 0)
    check_all(E, cols, cols, (16, 20), tensors=False)
    cols = (x.astype(np.float64), y.astype(np.float32), t.astype(np.float32), p.astype(np.float32))
    check_all(E, cols, cols, (16, 20), tensors=False)


def test_device_tensors_float32(E):
    cols = [c.astype(np.float32) for c in scene(np.random.default_rng(401), 6_000, 16, 20, span=8_000)]
    check_all(E, [torch.from_numpy(c).cuda() for c in cols], cols, (16, 20))


def test_native_columns_and_a_time_offset(E):
    x, y, t, p = scene(np.random.default_rng(402), 6_000, 16, 20, span=8_000)
    t = t + 123_456.0
    ev = E.DeviceEvents.from_native(x.astype(np.int16), y.astype(np.int16), t, (p > 0).astype(np.uint8))
    assert ev.t_offset == t[0]
    stored = (t - t[0]).astype(np.float32)
    assert np.array_equal(ev.t.cpu().numpy(), stored)
    cols = (x.astype(np.float32), y.astype(np.float32), stored, p.astype(np.float32))
    check_all(E, (ev, None, None, None), cols, (16, 20), refs_shift=ev.t_offset)      # t_refs are absolute times


def test_device_events_with_a_negative_polarity_scale(E):
    cols = [c.astype(np.float32) for c in scene(np.random.default_rng(403), 6_000, 16, 20, span=8_000)]
    ev = E.DeviceEvents.from_arrays(*cols, precision="f32").scaled(-2.0)
    assert ev.p_scale < 0
    flipped = (cols[0], cols[1], cols[2], -cols[3])
    check_all(E, (ev, None, None, None), flipped, (16, 20))


def test_unsorted_timestamps(E):
    cols = scene(np.random.default_rng(404), 8_000, 20, 24, span=3_000, shuffle=True)
    assert (np.diff(cols[2]) < 0).any()
    for decay, polarity in (("exp", "same"), (None, "split"), ("linear", "ignore")):
        kw = dict(radius=2, decay=decay, polarity=polarity)
        got = E.local_time_surfaces(*cols, 2_000.0, sensor_size=(20, 24), **kw)
        close(got, N.fast_local_time_surfaces(*cols, 2_000.0, (20, 24), **kw))
    cuts = [8_000, 1, 4_321]
    for decay in DECAYS:
        got = E.time_surfaces(*cols, 2_000.0, sensor_size=(20, 24), indices=cuts, decay=decay)
        close(got, N.fast_time_surfaces(*cols, 2_000.0, (20, 24), indices=cuts, decay=decay))
    assert (host(E.local_time_surfaces(*cols, 2_000.0, sensor_size=(20, 24), decay=None, include_self=False)) < 0).any()


# ---- geometry and sizes --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(1, 1), (1, 7)])
def test_degenerate_sensors(E, size):
    rng = np.random.default_rng(size[1])
    cols = scene(rng, 300, size[0], size[1], span=200)
    for radius in (1, 4):
        for polarity in ("ignore", "same", "split"):
            kw = dict(radius=radius, decay=None, polarity=polarity, include_self=radius == 1)
            close(E.local_time_surfaces(*cols, 50.0, sensor_size=size, **kw), N.seq_local_time_surfaces(*cols, 50.0, size, **kw))
        kw = dict(cell_size=3, radius=radius, return_counts=True)
        for g, w in zip(E.averaged_time_surfaces(*cols, 50.0, 20.0, sensor_size=size, **kw),
                        N.seq_averaged_time_surfaces(*cols, 50.0, 20.0, size, **kw)):
            close(g, w)
    for decay in DECAYS:
        kw = dict(decay=decay, indices=[300, 0, 150])
        close(E.time_surfaces(*cols, 50.0, sensor_size=size, **kw), N.seq_time_surfaces(*cols, 50.0, size, **kw))
        kw = dict(decay=decay, t_refs=[100.0, 1e9], polarity="ignore")
        close(E.time_surfaces(*cols, 50.0, sensor_size=size, **kw), N.seq_time_surfaces(*cols, 50.0, size, **kw))


@pytest.mark.parametrize("n", [0, 1])
def test_no_event_and_one_event(E, n):
    size = (5, 6)
    cols = (np.full(n, 2), np.full(n, 3), np.full(n, 7.0), np.ones(n))
    for decay in DECAYS:
        kw = dict(decay=decay)
        close(E.time_surfaces(*cols, 2.0, sensor_size=size, indices=[0, n], **kw),
              N.seq_time_surfaces(*cols, 2.0, size, indices=[0, n], **kw))
        close(E.time_surfaces(*cols, 2.0, sensor_size=size, t_refs=[8.0], polarity="ignore", **kw),
              N.seq_time_surfaces(*cols, 2.0, size, t_refs=[8.0], polarity="ignore", **kw))
        for polarity in ("ignore", "same", "split"):
            got = E.local_time_surfaces(*cols, 2.0, sensor_size=size, radius=2, polarity=polarity, **kw)
            close(got, N.seq_local_time_surfaces(*cols, 2.0, size, radius=2, polarity=polarity, **kw))
            assert got.shape == (n, 2 if polarity == "split" else 1, 5, 5)
    for g, w in zip(E.averaged_time_surfaces(*cols, 2.0, 1.0, sensor_size=size, cell_size=4, radius=1, return_counts=True),
                    N.seq_averaged_time_surfaces(*cols, 2.0, 1.0, size, cell_size=4, radius=1, return_counts=True)):
        close(g, w)
        assert g.shape[:3] == (2, 2, 2)
    dev = [torch.from_numpy(np.asarray(c, dtype=np.float32)).cuda() for c in cols]
    got = E.time_surfaces(*dev, 2.0, sensor_size=size, indices=[n], decay=None)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (1, 2, 5, 6)


def test_select(E, mixed):
    n = len(mixed[0])
    rng = np.random.default_rng(7)
    for select in ([], [n - 1], [5, 5, 5, 0, n - 1, 5], rng.integers(0, n, 1_000), torch.from_numpy(rng.integers(0, n, 300)).cuda()):
        for polarity, decay in (("same", "exp"), ("split", None)):
            kw = dict(radius=3, decay=decay, polarity=polarity)
            got = E.local_time_surfaces(*mixed, TAU, sensor_size=(H, W), select=select, **kw)
            close(got, N.fast_local_time_surfaces(*mixed, TAU, (H, W), select=host(select), **kw))
            assert got.shape[0] == len(select)


def test_corners_clip_the_window(E):
    """events on the four corner pixels and next to them: the window is clipped at all four borders, never wrapped"""
    pts = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (1, 1), (W - 2, 1), (1, H - 2), (W - 2, H - 2), (W - 1, 1), (0, H - 2)]
    x = np.array([q[0] for q in pts] * 6)
    y = np.array([q[1] for q in pts] * 6)
    n = len(x)
    t = (np.arange(n) // 2).astype(np.float64)
    p = (np.arange(n) % 3 == 0) * 2 - 1
    for radius in (1, 2, 3, 4):
        for polarity in ("ignore", "split"):
            kw = dict(radius=radius, decay=None, polarity=polarity, include_self=False)
            close(E.local_time_surfaces(x, y, t, p, 10.0, sensor_size=(H, W), **kw),
                  N.seq_local_time_surfaces(x, y, t, p, 10.0, (H, W), **kw))
        kw = dict(cell_size=5, radius=radius, normalise=False)
        close(E.averaged_time_surfaces(x, y, t, p, 10.0, 12.0, sensor_size=(H, W), **kw),
              N.seq_averaged_time_surfaces(x, y, t, p, 10.0, 12.0, (H, W), **kw))
    close(E.time_surfaces(x, y, t, p, 10.0, sensor_size=(H, W), indices=[n // 2, n], decay="linear"),
          N.seq_time_surfaces(x, y, t, p, 10.0, (H, W), indices=[n // 2, n], decay="linear"))


@pytest.mark.parametrize("cell_size", [5, 17, 100])
def test_hats_edge_cells_and_one_cell(E, cell_size):
    cols = scene(np.random.default_rng(500 + cell_size), 4_000, 13, 17, span=6_000)
    for radius, normalise in ((1, True), (3, False), (4, True)):
        kw = dict(cell_size=cell_size, radius=radius, normalise=normalise, return_counts=True)
        got = E.averaged_time_surfaces(*cols, 200.0, 600.0, sensor_size=(13, 17), **kw)
        want = N.fast_averaged_time_surfaces(*cols, 200.0, 600.0, (13, 17), **kw)
        assert got[0].shape[:2] == ((3, 4) if cell_size == 5 else (1, 1))
        close(got[1], want[1])
        close(got[0], want[0])


def test_hats_window_limits(E):
    cols = scene(np.random.default_rng(510), 3_000, 9, 11, span=2_000)
    for dt in (0.0, 1.0, 1e30):                        # exact ties only; one tick; everything
        close(E.averaged_time_surfaces(*cols, 100.0, dt, sensor_size=(9, 11), cell_size=4, radius=2),
              N.fast_averaged_time_surfaces(*cols, 100.0, dt, (9, 11), cell_size=4, radius=2))
    small = tuple(c[:250] for c in cols)
    close(E.averaged_time_surfaces(*small, 100.0, 30.0, sensor_size=(9, 11), cell_size=4, radius=2),
          N.seq_averaged_time_surfaces(*small, 100.0, 30.0, (9, 11), cell_size=4, radius=2))


# ---- long runs -----------------------------------------------------------------------------------------------------------

def test_hot_pixel(E, hot):
    x, y, t, p = hot
    size = (8, 8)
    on_hot = (x == 5) & (y == 3)
    assert on_hot.sum() >= 3_000
    dt = 50 * 60_000 / 3_000                            # about 50 events of the hot pixel
    for radius, cell_size in ((1, 4), (3, 8), (4, 3)):
        kw = dict(cell_size=cell_size, radius=radius, return_counts=True)
        got = E.averaged_time_surfaces(x, y, t, p, 400.0, dt, sensor_size=size, **kw)
        want = N.fast_averaged_time_surfaces(x, y, t, p, 400.0, dt, size, **kw)
        close(got[1], want[1])
        close(got[0], want[0])
    assert want[0].max() > 10.0                        # the hot pixel's own window: tens of terms per event
    for polarity in ("same", "split"):
        kw = dict(radius=2, polarity=polarity, decay=None)
        close(E.local_time_surfaces(x, y, t, p, 400.0, sensor_size=size, **kw), N.fast_local_time_surfaces(x, y, t, p, 400.0, size, **kw))
    cuts = [6_000, 2_999, 3_000, 1]
    close(E.time_surfaces(x, y, t, p, 400.0, sensor_size=size, indices=cuts), N.fast_time_surfaces(x, y, t, p, 400.0, size, indices=cuts))
    close(E.time_surfaces(x, y, t, p, 400.0, sensor_size=size, t_refs=[30_000.0], decay=None),
          N.fast_time_surfaces(x, y, t, p, 400.0, size, t_refs=[30_000.0], decay=None))


# ---- repeatability -------------------------------------------------------------------------------------------------------

def test_results_repeat_bit_for_bit(E, mixed, hot):
    calls = [lambda: E.time_surfaces(*mixed, TAU, sensor_size=(H, W), indices=[20_000, 9_000]),
             lambda: E.local_time_surfaces(*mixed, TAU, sensor_size=(H, W), radius=3, polarity="split"),
             lambda: E.averaged_time_surfaces(*mixed, 500.0, 1_500.0, sensor_size=(H, W), radius=3),
             lambda: E.averaged_time_surfaces(*hot, 400.0, 1_000.0, sensor_size=(8, 8), cell_size=4, radius=4, normalise=False)]
    for call in calls:
        a, b = call(), call()
        assert a.tobytes() == b.tobytes()


# ---- errors --------------------------------------------------------------------------------------------------------------

def test_errors(E):
    x, y, t, p = scene(np.random.default_rng(600), 100, 8, 9, span=50)
    size = (8, 9)
    cols = (x, y, t, p)

    def each(exc, glob=None, local=None, hats=None, c=cols):
        """every function that takes the argument raises `exc`"""
        if glob is not None:
            with pytest.raises(exc):
                E.time_surfaces(*c, **dict(dict(tau=5.0, sensor_size=size, indices=[50]), **glob))
        if local is not None:
            with pytest.raises(exc):
                E.local_time_surfaces(*c, **dict(dict(tau=5.0, sensor_size=size), **local))
        if hats is not None:
            with pytest.raises(exc):
                E.averaged_time_surfaces(*c, **dict(dict(tau=5.0, dt=3.0, sensor_size=size), **hats))
    for bx, by in ((9, 0), (0, 8), (-1, 0), (0, -1), (2 ** 40, 0)):      # a pixel off the sensor
        xb, yb = x.copy(), y.copy()
        xb[50], yb[50] = bx, by
        each(ValueError, {}, {}, {}, c=(xb, yb, t, p))
    each(TypeError, {}, {}, {}, c=(x + 0.5, y.astype(np.float64), t, p))      # pixels with fractions
    with pytest.raises(TypeError):
        E.local_time_surfaces(torch.tensor([1.0, 2.5], device="cuda"), torch.tensor([1.0, 2.0], device="cuda"),
                              torch.tensor([0.0, 1.0], device="cuda"), None, 5.0, sensor_size=size, polarity="ignore")
    for tau in (0.0, -1.0, float("nan")):
        each(ValueError, dict(tau=tau), dict(tau=tau), dict(tau=tau))
    for radius in (0, 5, -1, 1.5):
        each(ValueError, None, dict(radius=radius), dict(radius=radius))
    each(ValueError, dict(decay="gauss"), dict(decay="gauss"))
    each(ValueError, dict(polarity="same"), dict(polarity="both"))
    each(ValueError, None, None, dict(dt=-1.0))
    each(ValueError, None, None, dict(dt=float("nan")))
    each(ValueError, None, None, dict(cell_size=0))
    each(TypeError, dict(indices=None))                                      # neither t_refs nor indices
    each(TypeError, dict(t_refs=[10.0]))                                     # both
    each(TypeError, {}, dict(polarity="same"), {}, c=(x, y, t, None))         # classes without ps
    for bad in ([-1], [101], [3, 1000]):
        each(IndexError, dict(indices=bad))
    for bad in ([-1], [100], [0, 5, 100], [1.5], [[1, 2]], torch.tensor([100], device="cuda")):
        each(IndexError, None, dict(select=bad))
    shuffled = np.random.default_rng(1).permutation(t)
    assert (np.diff(shuffled) < 0).any()
    each(ValueError, dict(indices=None, t_refs=[10.0]), None, {}, c=(x, y, shuffled, p))
    # the calls after a rejected one are unaffected, and what is allowed on unsorted times still runs
    close(E.local_time_surfaces(x, y, shuffled, p, 5.0, sensor_size=size), N.fast_local_time_surfaces(x, y, shuffled, p, 5.0, size))
    close(E.time_surfaces(x, y, shuffled, p, 5.0, sensor_size=size, indices=[100]),
          N.fast_time_surfaces(x, y, shuffled, p, 5.0, size, indices=[100]))
    close(E.averaged_time_surfaces(*cols, 5.0, 3.0, sensor_size=size), N.fast_averaged_time_surfaces(*cols, 5.0, 3.0, size))
