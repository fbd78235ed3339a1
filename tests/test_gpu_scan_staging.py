"""GPU (-m gpu): the partition's scan phase (wave scans, wave totals, cursors, the plan's block scan) and its staging of
exact weights, at the sizes where they change shape: tile counts around the 64-tile wave and the 1024-tile round, event
counts around the 8 K-event sub-chunk and the second pass of a workgroup, weights that are all units, all wide, or one wide
one among units, and scenes whose tile counts are empty or cut.

Voxel grids are compared with the float64 oracle at 1e-5 of the grid's maximum; with unit polarities (the counting mode:
integer accumulators) the grid of a permuted copy of the events must also have the same bits -- a wrong prefix or cursor
loses or doubles a record and breaks both."""
import functools

import numpy as np
import pytest
import torch

from oracle import reference_np as R

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture()
def E(monkeypatch):
    import event_utils_amd as E
    monkeypatch.setenv("EVK_IMPL", "tiled")
    return E


def close(a, ref, tol=TOL):
    """|a - ref| <= tol * max |ref| over the cells where the oracle is finite; where it is not, the same NaN / +-inf."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape
    fin = np.isfinite(ref)
    assert np.array_equal(np.isnan(a), np.isnan(ref)), "NaN cells differ: %d vs %d" % (np.isnan(a).sum(), np.isnan(ref).sum())
    inf = np.isinf(ref)
    assert np.array_equal(a[inf], ref[inf])
    if fin.any():
        scale = max(np.max(np.abs(ref[fin])), 1e-30)
        err = np.max(np.abs(a[fin] - ref[fin]))
        print("max err %.3e, bar %.3e" % (err, tol * scale))
        assert err <= tol * scale, "max err %.3e vs tol %.3e" % (err, tol * scale)


@functools.lru_cache(maxsize=None)
def _events(seed, n, H, W):
    """Time-sorted events on integer pixels, polarities +-1 (read-only: shared between tests)."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, W, n).astype(np.float32)
    y = rng.integers(0, H, n).astype(np.float32)
    t = np.sort(rng.uniform(0, 0.1, n)).astype(np.float32)
    p = (rng.integers(0, 2, n) * 2 - 1).astype(np.float32)
    for a in (x, y, t, p):
        a.setflags(write=False)
    return x, y, t, p


def _voxel(E, cols, B, H, W):
    return E.events_to_voxel_torch(*(torch.from_numpy(np.array(a)).cuda() for a in cols), B,
                                   sensor_size=(H, W)).cpu().numpy()


def _permuted(cols, seed=11):
    """The same events in another order; the first and the last one (ts[0], ts[-1] of the call) stay where they are."""
    n = cols[0].shape[0]
    idx = np.arange(n)
    if n > 3:
        idx[1:-1] = np.random.default_rng(seed).permutation(idx[1:-1])
    return tuple(a[idx] for a in cols)


def _check_voxel(E, cols, B, H, W, unit):
    with np.errstate(all="ignore"):   # (one event: dt == 0; weights that are not finite)
        ref = R.events_to_voxel_torch(*cols, B, sensor_size=(H, W), accum="f64")
    got = _voxel(E, cols, B, H, W)
    close(got, ref)
    if unit:   # counting mode: integer adds commute
        again = _voxel(E, _permuted(cols), B, H, W)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    E.check_errors()


# (tiles, sensor H x W, tile w x h): one wave of 64 tiles and its neighbours, half a round, a whole round of 1024 tiles, and
# 1056 tiles = a second round of the scan with 32 tiles in it
TILINGS = [(1, 16, 16, 16, 16), (63, 28, 36, 4, 4), (64, 32, 32, 4, 4), (65, 20, 52, 4, 4), (512, 64, 128, 4, 4),
           (1024, 128, 128, 4, 4), (1056, 128, 132, 4, 4)]


@pytest.mark.parametrize("ntiles,H,W,tw,th", TILINGS, ids=[str(c[0]) for c in TILINGS])
def test_tile_counts_around_the_scan_seams(E, monkeypatch, ntiles, H, W, tw, th):
    from event_utils_amd import tiled
    monkeypatch.setitem(tiled.FORCE, "tile", (tw, th))
    B = 5
    assert tiled.voxel2_shape(H, W, B) == (tw, th), "the library refuses this tiling"
    assert (-(-H // th)) * (-(-W // tw)) == ntiles
    _check_voxel(E, _events(ntiles, 20_003, H, W), B, H, W, unit=True)


@pytest.mark.parametrize("n", [1, 63, 8191, 8193, 20_003, 2_200_001])
def test_event_counts_around_the_sub_chunk_seams(E, n):
    """20 003: three workgroups, the last one partial; 2 200 001: two passes per workgroup (the deferred write-out, the
    histogram left zero by the first pass's scan).  One event: ts[0] == ts[-1], its cell is NaN in every bin, as upstream."""
    H, W, B = 48, 64, 5
    _check_voxel(E, _events(n, n, H, W), B, H, W, unit=True)


def _arbitrary_f32(rng, n):
    """Finite float32 values of any sign, mantissa and magnitude from the denormals to 2^73: each needs all its 32 bits."""
    bits = (rng.integers(0, 2, n).astype(np.uint32) << 31) | (rng.integers(0, 201, n).astype(np.uint32) << 23) | \
        rng.integers(0, 1 << 23, n).astype(np.uint32)
    return bits.view(np.float32)


def _weights(pattern, p):
    """The staging patterns over the unit polarities `p` of 20 003 events (sub-chunks of ~6.7 K: the middle one is [6668, 13336))."""
    n = p.shape[0]
    rng = np.random.default_rng(5)
    w = p.copy()
    if pattern == "one_wide":
        w[n // 2] = np.float32(0.3)
    elif pattern == "arbitrary":
        w = _arbitrary_f32(rng, n)
    elif pattern == "nan_inf":
        w[n // 2] = np.nan
        w[n // 2 + 777] = np.inf
    elif pattern == "zeros":
        w[rng.integers(0, 3, n) == 0] = np.float32(0.0)
    else:
        assert pattern == "units"
    return w


PATTERNS = ["units", "one_wide", "arbitrary", "nan_inf", "zeros"]


@pytest.mark.parametrize("pattern", PATTERNS)
def test_staged_polarities_of_the_voxel_grid(E, pattern):
    """The exact polarities reach the side run only when one is wide: none, one in the middle sub-chunk (the runs of the
    other two are not written), all of them, values that are not finite, and +0.0 (a code of its own, not wide)."""
    H, W, B = 48, 64, 5
    x, y, t, p = _events(20_003, 20_003, H, W)
    _check_voxel(E, (x, y, t, _weights(pattern, p)), B, H, W, unit=pattern in ("units", "zeros"))


@pytest.mark.parametrize("interpolation", [None, "bilinear"])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_staged_weights_of_the_event_images(E, pattern, interpolation):
    H, W = 48, 64
    x, y, t, p = _events(20_003, 20_003, H, W)
    w = _weights(pattern, p)
    if interpolation == "bilinear":   # fractional positions inside the image
        rng = np.random.default_rng(6)
        x = np.clip(x + rng.uniform(0, 1, x.shape[0]).astype(np.float32), 0, W - 1.001).astype(np.float32)
        y = np.clip(y + rng.uniform(0, 1, y.shape[0]).astype(np.float32), 0, H - 1.001).astype(np.float32)
    kw = dict(interpolation=interpolation, padding=interpolation is not None)
    with np.errstate(all="ignore"):
        ref = R.events_to_image_torch(x, y, w, sensor_size=(H, W), accum="f64", **kw)
    got = E.events_to_image_torch(*(torch.from_numpy(np.array(a)).cuda() for a in (x, y, w)), sensor_size=(H, W), **kw)
    close(got.cpu().numpy(), ref)
    E.check_errors()


def test_all_events_in_one_tile(E, monkeypatch):
    """Every tile count but one is zero: empty runs, zero wave totals, and a tile the plan cuts into pieces."""
    from event_utils_amd import tiled
    monkeypatch.setitem(tiled.FORCE, "tile", (16, 16))
    H, W, B, n = 48, 64, 5, 20_003
    assert tiled.voxel2_shape(H, W, B) == (16, 16)
    x, y, t, p = _events(20_003, n, H, W)
    _check_voxel(E, ((x % 4) + 18, (y % 4) + 18, t, p), B, H, W, unit=True)   # pixels [18, 22) x [18, 22): tile (1, 1)


def test_hot_tile_that_the_plan_cuts(E):
    """Half of 200 000 events in 10 x 10 pixels: the plan's block scan hands the hot tiles several work items each."""
    H, W, B, n = 48, 64, 5, 200_000
    x, y, t, p = _events(7, n, H, W)
    x, y = x.copy(), y.copy()
    x[::2] = 30 + (x[::2] % 10)
    y[::2] = 20 + (y[::2] % 10)
    _check_voxel(E, (x, y, t, p), B, H, W, unit=True)
