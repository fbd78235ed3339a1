"""GPU (-m gpu): leaky_integrator and complementary_filter (evk_reconstruct.hip) against the literal float64 loop of
tests/_reconstruct_np.py (seq_reconstruct, pinned on hand-worked cases in tests/test_cpu_reconstruct.py).

The tolerance is derived, not tuned: |got - want| <= spacing(float32(want)) + 2^-36 A + 2^-126 per element, none excluded, with
A = |initial| + max_f |frames[f]| + sum_j |c_j| exp(-alpha (T_k - t_j)) over the counted events (returned by the oracle).
  spacing    the one float32 rounding may land on either side of a rounding boundary;
  2^-36 A    the device evaluates L = P + E (event-free solution plus an order-fixed sum of independent event terms, chained from
             query to query) where the oracle runs the dependent recurrence: float64 reassociation and the rounding of the exp
             arguments, at most about (events of the pixel + K + F) 2^-53 A plus about 2^-43 relative per exp whose argument reaches
             745.  The runs here stay below 2^14 events, so the factor is about 2^-39; 2^-36 leaves an eightfold margin;
  2^-126     keeps the comparison independent of how float32 subnormals are handled.
The streaming test widens the middle term to 2^-23 A: the state handed over as float32 adds at most 2^-24 |initial|, decayed."""
import numpy as np
import pytest
import torch

import _reconstruct_np as N

pytestmark = pytest.mark.gpu
H, W = 48, 64
ALPHA, C_ON, C_OFF = 1.0 / 4000.0, 0.23, 0.17
KW = dict(c_on=C_ON, c_off=C_OFF)


@pytest.fixture(scope="module")
def E():
    import event_utils_amd as E
    assert torch.cuda.is_available()
    return E


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def close(got, want, bound, factor=N.TOL_REASSOC):
    got = host(got)
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    assert np.isfinite(want).all()
    err, tol = np.abs(got.astype(np.float64) - want.astype(np.float64)), N.tolerance(want, bound, factor)
    print("max error / tolerance: %.3g" % (err / tol).max())
    assert (err <= tol).all(), "max error %g tolerances at %d of %d elements" % ((err / tol).max(), (err > tol).sum(), err.size)


def scene(rng, n, H=H, W=W, span=50_000):
    """Uniform noise plus a vertical edge that sweeps the sensor; integer-microsecond times (ties occur), int64 / float64 / int64."""
    t = np.sort(rng.integers(0, span, n)).astype(np.float64)
    noise = rng.random(n) < 0.5
    x = np.where(noise, rng.integers(0, W, n), np.minimum(W - 1, (t / span * W).astype(np.int64)))
    y = rng.integers(0, H, n)
    p = rng.integers(0, 2, n) * 2 - 1
    return x.astype(np.int64), y.astype(np.int64), t, p.astype(np.int64)


@pytest.fixture(scope="module")
def mixed():
    return scene(np.random.default_rng(100), 20_000)


@pytest.fixture(scope="module")
def hot():
    """one pixel holds 3 000 of 6 000 events on an 8 x 8 sensor; two other pixels are given runs of exactly 64 and 65 events"""
    rng = np.random.default_rng(300)
    x, y, t, p = scene(rng, 6_000, 8, 8, span=60_000)
    stuck = np.arange(6_000) % 2 == 0
    x[stuck], y[stuck], p[stuck] = 5, 3, 1
    free = np.flatnonzero(~stuck & ~((x == 0) & (y == 0)) & ~((x == 1) & (y == 0)))
    have = [int(((x == q) & (y == 0)).sum()) for q in (0, 1)]
    assert have[0] <= 64 and have[1] <= 65
    a, b = free[:64 - have[0]], free[100:100 + 65 - have[1]]
    x[a], y[a], x[b], y[b] = 0, 0, 1, 0
    return x, y, t, p


def mixed_refs(t):
    tied = float(t[np.flatnonzero(np.diff(t) == 0)[5]])
    assert (t == tied).sum() >= 2
    return [tied, 25_000.5, float(t[-1]) + 1.0]           # K = 3: on a tied stamp, between stamps, after the last event


@pytest.fixture(scope="module")
def mixed_want(mixed):
    x, y, t, p = mixed
    return N.seq_reconstruct(x, y, t, p, ALPHA, (H, W), t_refs=mixed_refs(t), **KW)


# ---- mixed scene: every input kind ---------------------------------------------------------------------------------------------

def test_mixed_scene_numpy_columns(E, mixed, mixed_want):
    x, y, t, p = mixed
    refs = mixed_refs(t)
    got = E.leaky_integrator(x, y, t, p, ALPHA, sensor_size=(H, W), t_refs=refs, **KW)
    assert isinstance(got, np.ndarray) and got.shape == (3, H, W)
    close(got, *mixed_want)
    assert (mixed_want[0] > 0).any() and (mixed_want[0] < 0).any()
    empty = np.ones((H, W), dtype=bool)
    empty[y, x] = False
    assert empty.any() and not got[:, empty].any()         # pixels without events
    close(E.leaky_integrator(x.astype(np.int16), y.astype(np.int32), t.astype(np.int64), p > 0, ALPHA, sensor_size=(H, W),
                             t_refs=np.array(refs), **KW), *mixed_want)
    close(E.leaky_integrator(x, y, t, p, ALPHA, sensor_size=(H, W), t_refs=refs[1:2], **KW), mixed_want[0][1:2], mixed_want[1][1:2])


def test_mixed_scene_device_tensors_float32(E, mixed, mixed_want):
    cols = [torch.from_numpy(c.astype(np.float32)).cuda() for c in mixed]      # (integers below 2^24: the same values)
    got = E.leaky_integrator(*cols, ALPHA, sensor_size=(H, W), t_refs=torch.tensor(mixed_refs(mixed[2]), dtype=torch.float64), **KW)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32
    close(got, *mixed_want)


def test_mixed_scene_device_events(E, mixed, mixed_want):
    cols = [c.astype(np.float32) for c in mixed]
    refs = mixed_refs(mixed[2])
    ev = E.DeviceEvents.from_arrays(*cols, precision="f32")
    got = E.leaky_integrator(ev, None, None, None, ALPHA, sensor_size=(H, W), t_refs=refs, **KW)
    assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32
    close(got, *mixed_want)
    # a negative p_scale turns the polarity round: the contrasts change places and the image changes sign
    neg = E.leaky_integrator(ev.scaled(-2.0), None, None, None, ALPHA, sensor_size=(H, W), t_refs=refs, c_on=C_OFF, c_off=C_ON)
    close(-neg, *mixed_want)


def test_mixed_scene_native_columns_and_a_time_offset(E, mixed, mixed_want):
    x, y, t, p = mixed
    shift = 123_456.0
    ev = E.DeviceEvents.from_native(x.astype(np.int16), y.astype(np.int16), t + shift, (p > 0).astype(np.uint8))
    assert ev.t_offset == t[0] + shift
    stored = ((t + shift) - ev.t_offset).astype(np.float32)
    assert np.array_equal(ev.t.cpu().numpy(), stored)
    refs = np.array(mixed_refs(t))
    got = E.leaky_integrator(ev, None, None, None, ALPHA, sensor_size=(H, W), t_refs=refs + shift, **KW)      # absolute times
    assert isinstance(got, torch.Tensor) and got.is_cuda
    close(got, *N.seq_reconstruct(x, y, stored, p, ALPHA, (H, W), t_refs=refs + shift - ev.t_offset, **KW))
    # t_start and the frame times are absolute as well
    frames = np.random.default_rng(5).normal(size=(2, H, W))
    fts = np.array([2.0, 30_000.0])
    start = float(t[3])                                    # the events before it do not count
    assert t[0] < start <= refs[0]
    got = E.complementary_filter(ev, None, None, None, ALPHA, frames, fts + shift, sensor_size=(H, W), t_refs=refs + shift,
                                 t_start=start + shift, **KW)
    close(got, *N.seq_reconstruct(x, y, stored, p, ALPHA, (H, W), t_refs=refs + shift - ev.t_offset, frames=frames,
                                  frame_ts=fts + shift - ev.t_offset, t_start=start + shift - ev.t_offset, **KW))


def test_indices_in_place_of_t_refs(E, mixed):
    x, y, t, p = mixed
    cuts = [0, 64, 7_777, 7_777, 20_000]
    want = N.seq_reconstruct(x, y, t, p, ALPHA, (H, W), indices=cuts, **KW)
    close(E.leaky_integrator(x, y, t, p, ALPHA, sensor_size=(H, W), indices=cuts, **KW), *want)
    assert not want[0][0].any()
    dev = [torch.from_numpy(c).cuda() for c in mixed]
    close(E.leaky_integrator(*dev, ALPHA, sensor_size=(H, W), indices=torch.tensor(cuts).cuda(), **KW), *want)


# ---- hot scene: the wave path and the lane path ----------------------------------------------------------------------------------

def hot_refs(x, y, t):
    on_hot = np.flatnonzero((x == 5) & (y == 3))
    mid = float(t[on_hot[1_500]])                          # an event time of the hot run, in its middle
    # K = 5: before any counted event; cutting the hot run at an event time; two equal queries; after the last event
    return [float(t[0]), mid, 45_000.5, 45_000.5, float(t[-1]) + 10.0]


@pytest.fixture(scope="module")
def hot_want(hot):
    x, y, t, p = hot
    return N.seq_reconstruct(x, y, t, p, 1.0 / 2000.0, (8, 8), t_refs=hot_refs(x, y, t), **KW)


@pytest.mark.parametrize("wave_run", [1, 1 << 30, 0])
def test_hot_scene_on_every_path(E, hot, hot_want, wave_run):
    """wave_run 1: every run on the wave path, runs of 1, 64 and 65 included; 2^30: every run on the lane path; 0: the default"""
    from event_utils_amd.representations import reconstruction as R
    x, y, t, p = hot
    lens = np.bincount(y * 8 + x, minlength=64)
    assert lens.max() >= 3_000 and (lens == 64).any() and (lens == 65).any() and lens.max() < 1 << 14
    assert not hot_want[0][0].any() and hot_want[0][1:, 3, 5].min() > 1.0
    got = R._reconstruct("test", x, y, t, p, 1.0 / 2000.0, (8, 8), hot_refs(x, y, t), None, C_ON, C_OFF, None, None, None, None,
                         wave_run=wave_run)
    close(got, *hot_want)
    if wave_run == 0:
        close(E.leaky_integrator(x, y, t, p, 1.0 / 2000.0, sensor_size=(8, 8), t_refs=hot_refs(x, y, t), **KW), *hot_want)


def test_a_run_of_one_on_the_wave_path(E):
    from event_utils_amd.representations import reconstruction as R
    x, y, t, p = np.array([2, 0]), np.array([1, 0]), np.array([3.0, 5.0]), np.array([1, -1])
    want = N.seq_reconstruct(x, y, t, p, 0.5, (2, 3), t_refs=[4.0, 9.0], **KW)
    for wave_run in (1, 2):
        close(R._reconstruct("test", x, y, t, p, 0.5, (2, 3), [4.0, 9.0], None, C_ON, C_OFF, None, None, None, None, wave_run=wave_run),
              *want)


@pytest.fixture(scope="module")
def run_lengths():
    """the run-length scene of tests/_denoise_np.py, K = 3 queries -- before the first event of the longest run (769 events),
    inside that run, after the last event -- and the oracle's values and bound"""
    import _denoise_np
    x, y, t, p, size = _denoise_np.run_length_scene()
    pix = y * size[1] + x
    run = np.flatnonzero(pix == np.bincount(pix).argmax())
    refs = [float(t[run[0]]), float(t[run[len(run) // 2]]) + 0.5, float(t[-1]) + 1.0]
    assert len(run) == 769 and t[0] <= refs[0] < refs[1] < refs[2]
    return (x, y, t, p), size, refs, N.seq_reconstruct(x, y, t, p, ALPHA, size, t_refs=refs, **KW)


@pytest.mark.parametrize("kind", [np.int16, np.int32, np.int64, np.float32, np.float64], ids=lambda k: k.__name__)
@pytest.mark.parametrize("wave_run", [1, 64, 0, 1 << 30])
def test_runs_that_straddle_the_wave_steps(E, run_lengths, wave_run, kind):
    """runs of 1, 63 .. 65, 255 .. 257, 511 .. 513 and 769 events and an empty pixel, every kind of time column; wave_run 1:
    every run on the wave path (one, two and three steps of 256, the pipeline's depth; a query's part of a run is shorter still);
    64: the runs from 64 on; 0: the default and 2^30: every run on the lane path"""
    from event_utils_amd.representations import reconstruction as R
    (x, y, t, p), size, refs, want = run_lengths
    assert (p > 0).any() and (p < 0).any() and want[0][0].any() and (want[0][2] != want[0][1]).any()
    got = R._reconstruct("test", x, y, t.astype(kind), p, ALPHA, size, refs, None, C_ON, C_OFF, None, None, None, None,
                         wave_run=wave_run)
    close(got, *want)


def test_results_repeat_bit_for_bit(E, hot):
    x, y, t, p = hot
    refs = hot_refs(x, y, t)
    frames = np.random.default_rng(9).normal(size=(2, 8, 8))
    calls = [lambda: E.leaky_integrator(x, y, t, p, 1.0 / 2000.0, sensor_size=(8, 8), t_refs=refs, **KW),
             lambda: E.complementary_filter(x, y, t, p, 1.0 / 2000.0, frames, [0.0, 30_000.0], sensor_size=(8, 8), t_refs=refs, **KW)]
    for call in calls:
        assert call().tobytes() == call().tobytes()


# ---- complementary filter ------------------------------------------------------------------------------------------------------

def test_complementary_filter(E, mixed):
    x, y, t, p = mixed
    rng = np.random.default_rng(7)
    frames = rng.normal(scale=2.0, size=(4, H, W))
    at_event = float(t[9_000])
    fts = [5_000.0, at_event, 30_000.0, 42_000.25]         # one on an event time; 30 000 lies between two queries
    assert fts[1] > fts[0] and fts[1] < 28_000
    refs = [5_000.0, at_event - 100.0, 28_000.0, 33_000.0, float(t[-1]) + 1.0]      # the second before frame_ts[1], the last after frame_ts[3]
    assert refs[1] < fts[1] and refs[2] < fts[2] < refs[3] and refs[4] > fts[3]
    got = E.complementary_filter(x, y, t, p, ALPHA, frames, fts, sensor_size=(H, W), t_refs=refs, **KW)      # default initial, t_start
    assert isinstance(got, np.ndarray)
    want = N.seq_reconstruct(x, y, t, p, ALPHA, (H, W), t_refs=refs, frames=frames, frame_ts=fts, **KW)
    close(got, *want)
    assert np.array_equal(want[0], N.seq_reconstruct(x, y, t, p, ALPHA, (H, W), t_refs=refs, frames=frames, frame_ts=fts,
                                                     initial=frames[0], t_start=fts[0], **KW)[0])
    # an explicit pair: a start before the first frame, float32 frames and start state on the device
    initial = rng.normal(size=(H, W)).astype(np.float32)
    f32 = frames.astype(np.float32)
    dev = [torch.from_numpy(c).cuda() for c in mixed]
    got = E.complementary_filter(*dev, ALPHA, torch.from_numpy(f32).cuda(), fts, sensor_size=(H, W), t_refs=refs,
                                 initial=torch.from_numpy(initial).cuda(), t_start=1_000.0, **KW)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    close(got, *N.seq_reconstruct(x, y, t, p, ALPHA, (H, W), t_refs=refs, frames=f32, frame_ts=fts, initial=initial, t_start=1_000.0,
                                  **KW))
    # one frame; and a faster filter, which forgets its start
    close(E.complementary_filter(x, y, t, p, 0.01, frames[:1], fts[:1], sensor_size=(H, W), t_refs=refs, **KW),
          *N.seq_reconstruct(x, y, t, p, 0.01, (H, W), t_refs=refs, frames=frames[:1], frame_ts=fts[:1], **KW))


# ---- exact integration, underflow, streaming --------------------------------------------------------------------------------------

def test_direct_integration_is_exact(E, mixed):
    x, y, t, p = mixed
    n = len(x)
    got = E.leaky_integrator(x, y, t, p, 0.0, sensor_size=(H, W), indices=[n // 3, n], c_on=1.0, c_off=1.0)
    for k, m in enumerate((n // 3, n)):
        img = E.events_to_image(x[:m], y[:m], p[:m], sensor_size=(H, W))
        assert np.array_equal(got[k], np.asarray(img).astype(np.float32))
    assert np.abs(got[1]).max() >= 3
    # the frames have no influence, the start state stays
    frames = np.random.default_rng(3).normal(size=(2, H, W))
    with_frames = E.complementary_filter(x, y, t, p, 0.0, frames, [0.0, 20_000.0], sensor_size=(H, W), indices=[n], c_on=1.0, c_off=1.0)
    close(with_frames, *N.seq_reconstruct(x, y, t, p, 0.0, (H, W), indices=[n], c_on=1.0, c_off=1.0, frames=frames,
                                          frame_ts=[0.0, 20_000.0]))


def test_old_terms_underflow(E, mixed):
    x, y, t, p = mixed
    refs = mixed_refs(t)
    want, bound = N.seq_reconstruct(x, y, t, p, 0.05, (H, W), t_refs=refs, **KW)      # ages of 15 000 and more: exp(-750) == 0.0
    got = E.leaky_integrator(x, y, t, p, 0.05, sensor_size=(H, W), t_refs=refs, **KW)
    close(got, want, bound)
    last = np.full((H, W), -np.inf)
    np.maximum.at(last, (y, x), t)
    recent = refs[2] - last < 200.0                        # the last term is at least 0.17 exp(-10)
    assert recent.sum() > 20 and (got[2][recent] != 0).all() and (want[2] == 0).any()


def test_streaming_continues_a_reconstruction(E, mixed):
    x, y, t, p = mixed
    n = len(x)
    t_mid = float(t[n // 2]) + 0.5
    m = int(np.searchsorted(t, t_mid))
    t_end = float(t[-1]) + 1.0
    first = E.leaky_integrator(x[:m], y[:m], t[:m], p[:m], ALPHA, sensor_size=(H, W), t_refs=[10_000.0, t_mid], **KW)
    second = E.leaky_integrator(x[m:], y[m:], t[m:], p[m:], ALPHA, sensor_size=(H, W), t_refs=[40_000.0, t_end], initial=first[-1],
                                t_start=t_mid, **KW)
    want, bound = N.seq_reconstruct(x, y, t, p, ALPHA, (H, W), t_refs=[10_000.0, t_mid, 40_000.0, t_end], **KW)
    close(first, want[:2], bound[:2])
    close(second, want[2:], bound[2:], factor=2.0 ** -23)
    # the same with frames: the second window gets the same frames
    frames = np.random.default_rng(8).normal(size=(3, H, W))
    fts = [0.0, 20_000.0, 35_000.0]
    first = E.complementary_filter(x[:m], y[:m], t[:m], p[:m], ALPHA, frames, fts, sensor_size=(H, W), t_refs=[t_mid], **KW)
    second = E.complementary_filter(x[m:], y[m:], t[m:], p[m:], ALPHA, frames, fts, sensor_size=(H, W), t_refs=[t_end],
                                    initial=first[-1], t_start=t_mid, **KW)
    want, bound = N.seq_reconstruct(x, y, t, p, ALPHA, (H, W), t_refs=[t_mid, t_end], frames=frames, frame_ts=fts, **KW)
    close(second, want[1:], bound[1:], factor=2.0 ** -23)


# ---- no events, errors -----------------------------------------------------------------------------------------------------------

def test_no_events(E):
    size = (5, 6)
    none = (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0, dtype=np.int64))
    got = E.leaky_integrator(*none, 0.5, sensor_size=size, t_refs=[3.0, 4.0])
    assert got.shape == (2, 5, 6) and got.dtype == np.float32 and not got.any()
    initial = np.random.default_rng(1).normal(size=size)
    close(E.leaky_integrator(*none, 0.5, sensor_size=size, t_refs=[3.0, 4.0], initial=initial),      # t_start: the first query
          *N.seq_reconstruct(*none, 0.5, size, t_refs=[3.0, 4.0], initial=initial))
    close(E.leaky_integrator(*none, 0.5, sensor_size=size, indices=[0], initial=initial),
          *N.seq_reconstruct(*none, 0.5, size, indices=[0], initial=initial))
    frames = np.random.default_rng(2).normal(size=(3, 5, 6))
    fts = [1.0, 2.0, 3.5]
    close(E.complementary_filter(*none, 0.5, frames, fts, sensor_size=size, t_refs=[1.0, 3.0, 3.5, 9.0]),
          *N.seq_reconstruct(*none, 0.5, size, t_refs=[1.0, 3.0, 3.5, 9.0], frames=frames, frame_ts=fts))
    dev = [torch.from_numpy(c).cuda() for c in none]
    got = E.complementary_filter(*dev, 0.5, frames, fts, sensor_size=size, t_refs=[2.5])
    assert got.is_cuda and got.shape == (1, 5, 6)
    close(got, *N.seq_reconstruct(*none, 0.5, size, t_refs=[2.5], frames=frames, frame_ts=fts))


def test_errors(E):
    x, y, t, p = scene(np.random.default_rng(600), 100, 8, 9, span=50)
    size = (8, 9)
    ok = E.leaky_integrator(x, y, t, p, 0.1, sensor_size=size, t_refs=[60.0])
    shuffled = np.random.default_rng(1).permutation(t)
    assert (np.diff(shuffled) < 0).any()
    for kw in (dict(t_refs=[60.0]), dict(indices=[100])):
        with pytest.raises(ValueError, match="non-decreasing"):
            E.leaky_integrator(x, y, shuffled, p, 0.1, sensor_size=size, **kw)
    with pytest.raises(ValueError, match="before"):          # before the first event, the default t_start
        E.leaky_integrator(x, y, t + 5.0, p, 0.1, sensor_size=size, t_refs=[4.0])
    with pytest.raises(ValueError, match="before"):          # ts[m - 1] lies before an explicit t_start
        E.leaky_integrator(x, y, t, p, 0.1, sensor_size=size, indices=[3], t_start=float(t[50]) + 0.5)
    with pytest.raises(IndexError):
        E.leaky_integrator(x, y, t, p, 0.1, sensor_size=size, indices=[101])
    with pytest.raises(TypeError):
        E.leaky_integrator(x, y, t, None, 0.1, sensor_size=size, t_refs=[60.0])
    xb = x.copy()
    xb[50] = 9                                             # a pixel off the sensor
    with pytest.raises(ValueError):
        E.leaky_integrator(xb, y, t, p, 0.1, sensor_size=size, t_refs=[60.0])
    # the calls after a rejected one are unaffected
    assert E.leaky_integrator(x, y, t, p, 0.1, sensor_size=size, t_refs=[60.0]).tobytes() == ok.tobytes()
