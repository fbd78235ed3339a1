"""GPU (-m gpu): simulate_events (evk_simulate.hip) against the literal float64 walk of tests/_simulate_np.py (seq_simulate, pinned
on hand-worked cases in tests/test_cpu_simulate.py).

The comparison is EXACT: the four columns and the state are np.array_equal to the oracle's.  There is no tolerance, because the
definition fixes every rounding (IEEE float64, one rounding per operation, no contraction) and the order of the output.

Event counts of the shared scenes (from the oracle): scene A (9, 48, 64), c_on 0.11, c_off 0.13: 102 985 events, up to 56 per
pixel, 21 228 with refractory 300; scene B (6, 12, 70): 23 801; the tie scene (5, 8, 70): 9 226 events, 8 914 equal-time neighbours,
1 559 exactly on a frame time; its burst: 13 162 events, 3 312 of them clamped to frame_ts[0]."""
import numpy as np
import pytest
import torch

import _reconstruct_np as RN
import _simulate_np as N

pytestmark = pytest.mark.gpu
C_ON, C_OFF = 0.11, 0.13


@pytest.fixture(scope="module")
def E():
    import event_utils_amd as E
    assert torch.cuda.is_available()
    return E


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def same(got, want):
    """got: (xs, ys, ts, ps, state) of the device; want: seq_simulate's seven values -- equal bit for bit, overflow 0"""
    assert want[6] == 0
    xs, ys, ts, ps, state = got
    for g, w, dtype in zip((xs, ys, ts, ps), want[:4], (np.int64, np.int64, np.float64, np.int64)):
        g = host(g)
        assert g.dtype == dtype and g.shape == w.shape, (g.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), "%d of %d differ, first at %d" % ((g != w).sum(), len(w), int(np.flatnonzero(g != w)[0]))
    # (equal_nan: a pixel whose frames[0] is NaN keeps that NaN as its level)
    assert np.array_equal(host(state.reference), want[4], equal_nan=True) and np.array_equal(host(state.last_event_ts), want[5])
    assert host(state.reference).dtype == host(state.last_event_ts).dtype == np.float64


@pytest.fixture(scope="module")
def a():
    return N.scene_a()


@pytest.fixture(scope="module")
def a_want(a):
    return N.seq_simulate(*a, C_ON, C_OFF)


@pytest.fixture(scope="module")
def b():
    return N.scene_b()


@pytest.fixture(scope="module")
def b_want(b):
    return N.seq_simulate(*b, C_ON, C_OFF)


@pytest.fixture(scope="module")
def tie():
    return N.tie_scene()


# ---- scene A: every input kind -------------------------------------------------------------------------------------------------

def test_scene_a_numpy(E, a, a_want):
    frames, fts = a
    assert len(a_want[2]) > 50_000 and np.bincount(a_want[1] * 64 + a_want[0]).max() > 40
    got = E.simulate_events(frames, fts, C_ON, C_OFF, return_state=True)
    assert all(isinstance(v, np.ndarray) for v in got[:4] + tuple(got[4]))
    same(got, a_want)
    four = E.simulate_events(frames, list(fts), c_on=C_ON, c_off=C_OFF)
    assert len(four) == 4 and all(np.array_equal(u, v) for u, v in zip(four, a_want[:4]))


def test_scene_a_refractory(E, a, a_want):
    frames, fts = a
    want = N.seq_simulate(frames, fts, C_ON, C_OFF, 300.0)
    assert 10_000 < len(want[2]) < len(a_want[2]) - 30_000                 # tens of thousands are dropped
    assert np.array_equal(want[4], a_want[4]) and np.array_equal(want[5], a_want[5])      # a dropped crossing still moves the state
    same(E.simulate_events(frames, fts, C_ON, C_OFF, 300.0, return_state=True), want)


def test_scene_a_device_tensors(E, a, a_want):
    frames, fts = a
    got = E.simulate_events(torch.from_numpy(frames).cuda(), torch.from_numpy(fts), C_ON, C_OFF, return_state=True)
    assert all(isinstance(v, torch.Tensor) and v.is_cuda for v in got[:4] + tuple(got[4]))
    same(got, a_want)


def test_scene_a_float32_frames(E, a):
    frames, fts = a
    f32 = frames.astype(np.float32)
    want = N.seq_simulate(f32.astype(np.float64), fts, C_ON, C_OFF)
    same(E.simulate_events(f32, fts, C_ON, C_OFF, return_state=True), want)
    got = E.simulate_events(torch.from_numpy(f32), fts, C_ON, C_OFF, return_state=True)       # a host tensor: device tensors out
    assert got[0].is_cuda and got[4].reference.is_cuda
    same(got, want)


def test_two_calls_give_identical_bytes(E, a):
    frames = torch.from_numpy(a[0]).cuda()
    one = E.simulate_events(frames, a[1], C_ON, C_OFF, 300.0, return_state=True)
    two = E.simulate_events(frames, a[1], C_ON, C_OFF, 300.0, return_state=True)
    for u, v in zip(one[:4] + tuple(one[4]), two[:4] + tuple(two[4])):
        assert host(u).tobytes() == host(v).tobytes()


# ---- scene B: a partial wave and a partial block; the wide sort values; contrast maps --------------------------------------------

def test_scene_b(E, b, b_want):
    assert b[0].shape == (6, 12, 70) and len(b_want[2]) > 10_000
    same(E.simulate_events(*b, C_ON, C_OFF, return_state=True), b_want)


def test_scene_b_with_64_bit_sort_values(E, b, b_want):
    from event_utils_amd.simulation import event_simulator as S
    same(S._simulate(b[0], b[1], C_ON, C_OFF, 0.0, None, None, True, wide=1), b_want)


def test_per_pixel_contrast_maps(E, b):
    rng = np.random.default_rng(7)
    on, off = rng.uniform(0.05, 0.3, size=(12, 70)), rng.uniform(0.05, 0.3, size=(12, 70))      # bounded away from 0
    want = N.seq_simulate(*b, on, off, 150.0)
    assert len(want[2]) > 5_000
    same(E.simulate_events(*b, on, off, 150.0, return_state=True), want)
    same(E.simulate_events(torch.from_numpy(b[0]).cuda(), b[1], torch.from_numpy(on).cuda(), off.astype(np.float32), 150.0,
                           return_state=True), N.seq_simulate(*b, on, off.astype(np.float32), 150.0))
    same(E.simulate_events(*b, on, C_OFF, return_state=True), N.seq_simulate(*b, on, C_OFF))
    # the maps' values are checked on the device, in the read-back of the count pass
    for value in (0.0, -0.1, float("nan"), float("inf")):
        broken = on.copy()
        broken[3, 5] = value
        with pytest.raises(ValueError, match="1 pixels of the maps"):
            E.simulate_events(*b, broken, off)


# ---- ties: what pins the order -------------------------------------------------------------------------------------------------

def test_tie_scene(E, tie):
    frames, fts = tie
    want = N.seq_simulate(frames, fts, 0.5, 0.25)
    x, y, t, p = want[:4]
    assert int((np.diff(t) == 0).sum()) >= 1000 and int(np.isin(t, fts).sum()) >= 500
    by_txyp = np.lexsort((p, y, x, t))                     # the defined order is NOT the (t, x, y, p) order
    assert not np.array_equal(x[by_txyp], x) and not np.array_equal(p[by_txyp], p)
    same(E.simulate_events(frames, fts, 0.5, 0.25, return_state=True), want)


def test_burst_at_the_first_frame_time(E, tie):
    frames, fts = tie
    want = N.seq_simulate(frames, fts, 0.5, 0.25, reference=frames[0] + 3)
    assert int((want[2] == fts[0]).sum()) >= 3000
    same(E.simulate_events(frames, fts, 0.5, 0.25, reference=frames[0] + 3, return_state=True), want)
    same(E.simulate_events(torch.from_numpy(frames).cuda(), fts, 0.5, 0.25, reference=torch.from_numpy(frames[0] + 3).cuda(),
                           return_state=True), want)


def test_negative_times_and_a_frame_at_zero(E, tie):
    frames = tie[0]
    fts = np.array([-2048.0, -1024.0, -0.0, 512.0, 2048.0])            # the keys cross the sign; -0.0 counts as +0.0
    want = N.seq_simulate(frames, fts, 0.5, 0.25)
    assert (want[2] < 0).any() and (want[2] == 0).any() and (want[2] > 0).any()
    same(E.simulate_events(frames, fts, 0.5, 0.25, return_state=True), want)


# ---- a hot pixel -------------------------------------------------------------------------------------------------------------------

def test_hot_pixel_below_and_above_the_step_limit(E):
    frames = np.zeros((3, 8, 8))
    frames[1, 3, 5] = 300.0
    frames[2, 3, 5] = 300.0
    fts = [0.0, 1000.0, 2000.0]
    want = N.seq_simulate(frames, fts, 0.01, 0.01)
    assert 29_000 < len(want[2]) <= 30_000 and (want[0] == 5).all() and (want[1] == 3).all()      # its neighbours have none
    same(E.simulate_events(frames, fts, 0.01, 0.01, return_state=True), want)
    frames[1:, 3, 5] = 700.0
    frames[2, 0, 0] = -700.0
    assert N.seq_simulate(frames, fts, 0.01, 0.01)[6] == 2
    with pytest.raises(ValueError, match=r"2 pixel-intervals exceeded 65536 crossings.*contrast is too small"):
        E.simulate_events(frames, fts, 0.01, 0.01)


# ---- degenerate shapes -----------------------------------------------------------------------------------------------------------

def test_one_pixel_and_two_frames(E):
    frames = np.array([0.3, 1.9, -0.4]).reshape(3, 1, 1)
    same(E.simulate_events(frames, [5.0, 6.0, 9.0], C_ON, C_OFF, return_state=True), N.seq_simulate(frames, [5.0, 6.0, 9.0], C_ON, C_OFF))
    frames, fts = N.scene_b()
    same(E.simulate_events(frames[:2], fts[:2], C_ON, C_OFF, return_state=True), N.seq_simulate(frames[:2], fts[:2], C_ON, C_OFF))


def test_constant_frames_give_four_empty_columns(E):
    frames = np.full((3, 5, 7), 0.7)
    for inp, kind in ((frames, np.ndarray), (torch.from_numpy(frames).cuda(), torch.Tensor)):
        xs, ys, ts, ps, state = E.simulate_events(inp, [0.0, 1.0, 2.0], return_state=True)
        for v, dtype in zip((xs, ys, ts, ps), (np.int64, np.int64, np.float64, np.int64)):
            assert isinstance(v, kind) and tuple(v.shape) == (0,) and host(v).dtype == dtype
            assert kind is np.ndarray or v.is_cuda
        assert np.array_equal(host(state.reference), frames[0]) and np.isneginf(host(state.last_event_ts)).all()


def test_inf_and_nan_pixels_emit_nothing_in_their_intervals(E):
    frames, fts = N.scene_b()
    frames = frames.copy()
    frames[2, 4, 9] = np.nan
    frames[3, 5, 60] = np.inf
    frames[1, 0, 0] = -np.inf
    frames[:, 11, 69] = np.nan
    want = N.seq_simulate(frames, fts, C_ON, C_OFF)
    assert len(want[2]) > 10_000 and np.isfinite(want[2]).all()
    same(E.simulate_events(frames, fts, C_ON, C_OFF, return_state=True), want)


# ---- many blocks, mostly empty ---------------------------------------------------------------------------------------------------

def test_many_blocks_with_sparse_activity(E):
    rng = np.random.default_rng(11)
    F, H, W = 3, 130, 131
    frames = np.zeros((F, H, W))
    active = rng.random((H, W)) < 0.03
    for f in (1, 2):
        frames[f][active] = rng.normal(0.0, 1.5, size=int(active.sum()))
    fts = [10.0, 20.5, 33.0]
    want = N.seq_simulate(frames, fts, C_ON, C_OFF)
    counts = np.bincount(want[1] * W + want[0], minlength=H * W)
    assert (counts == 0).mean() > 0.9 and len(want[2]) > 3_000
    same(E.simulate_events(frames, fts, C_ON, C_OFF, return_state=True), want)


# ---- streaming and the round trip ------------------------------------------------------------------------------------------------

def test_streaming_continues_a_video(E, a, a_want):
    frames, fts = a
    second = N.seq_simulate(frames[4:], fts[4:], C_ON, C_OFF, 0.0, *N.seq_simulate(frames[:5], fts[:5], C_ON, C_OFF)[4:6])
    assert not (second[2] == fts[4]).any()                 # the condition under which concatenation and the tie rule agree
    dev = torch.from_numpy(frames).cuda()
    x1, y1, t1, p1, s1 = E.simulate_events(dev[:5], fts[:5], C_ON, C_OFF, return_state=True)
    x2, y2, t2, p2, s2 = E.simulate_events(dev[4:], fts[4:], C_ON, C_OFF, reference=s1.reference, last_event_ts=s1.last_event_ts,
                                           return_state=True)
    assert len(t1) > 10_000 and len(t2) > 10_000
    same((torch.cat((x1, x2)), torch.cat((y1, y2)), torch.cat((t1, t2)), torch.cat((p1, p2)), s2), a_want)
    x1, y1, t1, p1, s1 = E.simulate_events(frames[:5], fts[:5], C_ON, C_OFF, 300.0, return_state=True)      # numpy, with a refractory period
    x2, y2, t2, p2, s2 = E.simulate_events(frames[4:], fts[4:], C_ON, C_OFF, 300.0, *s1, return_state=True)
    want = N.seq_simulate(frames, fts, C_ON, C_OFF, 300.0)
    same((np.concatenate((x1, x2)), np.concatenate((y1, y2)), np.concatenate((t1, t2)), np.concatenate((p1, p2)), s2), want)


def test_the_reconstruction_integrates_the_events_back_to_the_level(E, a, a_want):
    frames, fts = a
    H, W = frames.shape[1:]
    xs, ys, ts, ps, state = E.simulate_events(frames, fts, C_ON, C_OFF, return_state=True)
    got = E.leaky_integrator(xs, ys, ts, ps, 0.0, sensor_size=(H, W), t_refs=[float(fts[-1]) + 1.0], c_on=C_ON, c_off=C_OFF,
                             initial=frames[0], t_start=float(fts[0]))
    assert got.shape == (1, H, W) and got.dtype == np.float32
    steps = np.zeros((H, W))
    np.add.at(steps, (a_want[1], a_want[0]), np.where(a_want[3] > 0, C_ON, C_OFF))
    bound = np.abs(frames[0]) + steps                      # A = |frames[0]| + sum |c_j|
    assert np.array_equal(state.reference, a_want[4])
    want = state.reference[None]                           # float64: the one float32 rounding of the integrator is inside `spacing`
    err, tol = np.abs(got.astype(np.float64) - want), RN.tolerance(want, bound[None])
    print("max error / tolerance: %.3g" % (err / tol).max())
    assert (err <= tol).all()
