"""GPU (-m gpu): the event augmentation (evk_augment.hip, the subset select of evk_select.hip) against the numpy restatement of
tests/test_cpu_augment.py (itself checked against the real reference there): Philox words, random events and the sort bit for
bit, numpy / device tensors / DeviceEvents, 10 M events, ranges and a chi-square of the draws, the uniform subset of
remove_events, correlated events, flip / crop / rotate, and a voxel grid of an augmented resident stream."""
import numpy as np
import pytest
import torch

from test_cpu_augment import (PURPOSE, np_add_random_events, np_random_events, np_remove_events, np_rotate_events,
                              np_sort_events, np_subset, philox_words)

pytestmark = pytest.mark.gpu
H, W = 48, 64


@pytest.fixture(scope="module")
def A():
    from event_utils_amd.augmentation import event_augmentation as A
    assert torch.cuda.is_available()
    return A


def host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def same(a, b):
    a, b = host(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def stream(rng, n, ids=False):
    x = rng.integers(0, W, n)
    y = rng.integers(0, H, n)
    t = np.sort(rng.uniform(0, 1, n))
    p = np.arange(n, dtype=np.int64) if ids else rng.integers(0, 2, n) * 2 - 1
    return x, y, t, p


def kinds(cols):
    """The same columns as numpy, as device tensors and as a float64 DeviceEvents."""
    from event_utils_amd import DeviceEvents
    dev = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in cols]
    ev = DeviceEvents(*[torch.from_numpy(np.asarray(c, dtype=np.float64)).cuda() for c in cols])
    return {"numpy": cols, "torch": dev, "events": (ev, None, None, None)}


def outs(r):
    from event_utils_amd import DeviceEvents
    if isinstance(r, DeviceEvents):
        return [r.x, r.y, r.t, r.p]
    return list(r)


def test_philox_words_equal_the_restatement():
    from event_utils_amd import _lib
    from event_utils_amd import _device as D
    for seed, purpose, offset, n in ((0, 0, 0, 1000), (0x123456789ABCDEF, 3, (1 << 32) - 500, 1000), (7, 5, 5 << 40, 77)):
        out = torch.empty(4 * n, dtype=torch.int32, device="cuda")
        _lib.call("evk_philox4x32", seed, purpose, offset, n, D.ptr(out), D.stream())
        got = out.cpu().numpy().view(np.uint32).reshape(n, 4)
        want = np.stack(philox_words(seed, purpose, np.arange(n, dtype=np.uint64) + np.uint64(offset)), axis=1)
        assert np.array_equal(got, want)


def test_philox_known_answer_on_the_device():
    """Random123's first kat vector (counter 0, key 0) through the device entry point; the kernels' Philox function is checked
    against all three vectors at compile time (static_assert in evk_philox.h)."""
    from event_utils_amd import _lib
    from event_utils_amd import _device as D
    out = torch.empty(4, dtype=torch.int32, device="cuda")
    _lib.call("evk_philox4x32", 0, 0, 0, 1, D.ptr(out), D.stream())
    assert [int(v) for v in out.cpu().numpy().view(np.uint32)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


def test_subset_of_the_largest_candidate_count(A):
    """2^32 - 1 candidates, the largest the subset takes: the select's walk over the keys ends (a 32-bit index would wrap on its
    last stride) and the subset has exactly k members, the ones with the smallest keys."""
    import time
    n, k = (1 << 32) - 1, 1000
    t0 = time.perf_counter()
    _, idx, result = A._subset(1234, PURPOSE["corr_choice"], n, k, torch.device("cuda"), want_index=True)
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 60
    assert int(result[0]) == k
    idx = idx.cpu().numpy()
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    w = philox_words(1234, PURPOSE["corr_choice"], idx.astype(np.uint64))
    r = (w[0].astype(np.uint64) | (w[1].astype(np.uint64) << np.uint64(32))).astype(np.float64) / 2.0 ** 64
    assert r.max() < 4e-7                           # the 1000th smallest of 2^32 uniforms lies near 2.3e-7 (sd 3 %)


def test_empty_draws_and_nan_coordinates(A):
    x, y, t, p = np.array([-5, -3, -4]), np.array([-1, -2, -1]), np.array([0.1, 0.2, 0.3]), np.array([1, -1, 1])
    for g, w in zip(A.add_random_events(x, y, t, p, 0, seed=1), np_add_random_events(x, y, t, p, 0, seed=1)):
        same(g, w)
    assert len(A.add_correlated_events(x, y, t, p, 2, seed=1)[0]) == 2
    with pytest.raises(ValueError):
        A.add_random_events(x, y, t, p, 1, seed=1)
    xn = np.array([1.0, np.nan, 2.0])
    assert np.isnan(A.add_correlated_events(xn, y, t, p, 2, xy_std=0, ts_std=0, seed=1)[0]).all()


def test_sample_on_device_stamps(A):
    cdf = np.array([0.0, 0.5, 3.0])
    for ts in (np.array([0, 1, 2, 3]), np.array([0.1, 0.5, 0.9, 2.5], np.float32), np.array([0.2, 1.7, 2.9])):
        for s in range(20):
            np.random.seed(s)
            want = np.searchsorted(ts, np.random.uniform(cdf[0], cdf[-1]))
            np.random.seed(s)
            assert A.sample(cdf, torch.from_numpy(ts).cuda()) == want
            np.random.seed(s)
            assert A.sample(cdf, ts) == want


@pytest.mark.parametrize("mode", ["numpy", "torch", "events"])
def test_add_random_events_zero_and_noise_paths_are_exact(A, mode):
    rng = np.random.default_rng(1)
    cols = stream(rng, 5000)
    args = kinds(cols)[mode]
    for got, want in zip(outs(A.add_random_events(*args, 0, seed=3)), np_add_random_events(*cols, 0, seed=3)):
        same(got, want)
    for kw in (dict(sort=False, return_merged=False), dict(sort=True, return_merged=False), dict(sort=False, return_merged=True),
               dict()):
        got = outs(A.add_random_events(*args, 700, seed=9, **kw))
        want = np_add_random_events(*cols, 700, seed=9, **kw)
        for g, w in zip(got, want):
            if mode == "events":
                w = w.astype(np.float64)
            same(g, w)
    for got, want in zip(outs(A.remove_events(*args, 1200, add_noise=300, seed=4)),
                         np_remove_events(*cols, 1200, add_noise=300, seed=4)):
        same(got, want)
    for got, want in zip(outs(A.remove_events(*args, 1200, seed=4)), np_remove_events(*cols, 1200, seed=4)):
        same(got, want.astype(np.float64) if mode == "events" else want)


def test_sorted_merge_at_10m_equals_the_restatement(A):
    rng = np.random.default_rng(2)
    n, m = 10_000_000, 1_000_000
    x = rng.integers(0, 640, n).astype(np.int16)
    y = rng.integers(0, 480, n).astype(np.int16)
    t = np.sort(rng.uniform(0, 5, n))
    t[::97] = t[::97].round(3)                                   # ties in t
    p = (rng.integers(0, 2, n) * 2 - 1).astype(np.int8)
    dev = [torch.from_numpy(c).cuda() for c in (x, y, t, p)]
    new = [host(c) for c in A.add_random_events(*dev, m, sort=False, return_merged=False, seed=21)]
    got = A.add_random_events(*dev, m, seed=21)
    want = np_sort_events(*[np.concatenate((a, b)).astype(np.float64) for a, b in zip(new, (x, y, t, p))])
    for g, w in zip(got, want):
        same(g, w)


@pytest.mark.parametrize("n", [8, 5000, 100_003])
def test_sort_orders_polarities_of_events_equal_in_t_x_y(A, n):
    """Events equal in t, x and y are ordered by p, numpy's last field.  +-1 polarities differ only in the sign bit: above a
    merge sort's worth of events the radix sort was asked for the bit range [63, 64) and left them in stream order
    (tools/fuzz_parity.py --kinds augment)."""
    rng = np.random.default_rng(n)
    x, y = rng.integers(0, 3, n), rng.integers(0, 2, n)
    t = np.sort(rng.integers(0, 3, n)) * 0.5
    p = rng.integers(0, 2, n) * 2 - 1
    for cols in ((x, y, t, p), (np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n), p), (p, y, t, np.ones(n))):
        for mode, args in kinds(cols).items():
            got = outs(A.add_random_events(*args, 0, seed=1))
            for g, w in zip(got, np_add_random_events(*cols, 0, seed=1)):
                same(g, w)
        got = A.add_random_events(*cols, 3 * n, seed=2)
        for g, w in zip(got, np_add_random_events(*cols, 3 * n, seed=2)):
            same(g, w)


def test_random_event_ranges_dtypes_and_chi_square(A):
    rng = np.random.default_rng(3)
    x, y, t, p = stream(rng, 1000)
    x[0], y[0] = 99, 17
    nx, ny, nt, npol = A.add_random_events(x, y, t, p, 400_000, sort=False, return_merged=False, seed=12345)
    assert [a.dtype for a in (nx, ny, nt, npol)] == [np.int64, np.int64, np.float64, np.int64]
    assert nx.min() >= 0 and nx.max() <= 99 and ny.min() >= 0 and ny.max() <= max(H - 1, 17)
    assert nt.min() >= t.min() and nt.max() < t.max() and set(np.unique(npol)) == {-1, 1}
    for v, k in ((nx, 100), (ny, int(y.max()) + 1), ((npol + 1) // 2, 2)):
        c = np.bincount(v, minlength=k)
        e = len(v) / k
        chi = ((c - e) ** 2 / e).sum()
        assert chi < k - 1 + 6 * np.sqrt(2 * (k - 1)), (k, chi)
    with pytest.raises(ValueError):
        A.add_random_events(x[:0], y[:0], t[:0], p[:0], 5, seed=1)
    tn = t.copy()
    tn[5] = np.nan
    with pytest.raises(OverflowError):
        A.add_random_events(x, y, tn, p, 5, seed=1)
    xn = x.astype(np.float64)
    xn[3] = np.nan
    with pytest.raises(ValueError):
        A.add_random_events(xn, y, t, p, 5, seed=1)


def test_remove_events_subset(A):
    rng = np.random.default_rng(4)
    cols = stream(rng, 100_003, ids=True)
    for mode, args in kinds(cols).items():
        got = outs(A.remove_events(*args, 40_000, seed=77))
        ids = host(got[3]).astype(np.int64)
        assert len(ids) == 60_003 and np.all(np.diff(ids) > 0)           # exactly n - to_remove, in stream order
        for g, c in zip(got, cols):
            assert np.array_equal(host(g), np.asarray(c)[ids].astype(host(g).dtype))
        assert np.array_equal(ids, np_subset(77, PURPOSE["subset"], 100_003, 60_003))
    a = A.remove_events(*cols, 500, seed=5)[3]
    assert np.array_equal(a, A.remove_events(*cols, 500, seed=5)[3])
    assert not np.array_equal(a, A.remove_events(*cols, 500, seed=6)[3])
    np.random.seed(8)
    b = A.remove_events(*cols, 500)[3]
    np.random.seed(8)
    assert np.array_equal(b, A.remove_events(*cols, 500)[3])
    # inclusion frequencies over seeds at n = 1000
    small = stream(rng, 1000, ids=True)
    hits = np.zeros(1000)
    for s in range(300):
        hits[A.remove_events(*small, 700, seed=s)[3]] += 1
    e = 300 * 300 / 1000
    assert ((hits - e) ** 2 / e).sum() < 999 + 6 * np.sqrt(2 * 999)
    # edge cases
    for r in (A.remove_events(*small, 1001, seed=1), A.remove_events(*small, 1001, add_noise=5, seed=1)):
        assert all(c.dtype == np.float64 and c.shape == (0,) for c in r)
    with pytest.raises(ValueError):
        A.remove_events(*small, -1, seed=1)
    assert all(len(c) == 0 for c in A.remove_events(*small, 1000, seed=1))
    assert [len(c) for c in A.remove_events(*small, 0, seed=1)] == [1000] * 4
    got = A.remove_events(*small, 1000, add_noise=20, seed=1)
    assert all(c.dtype == np.float64 and len(c) == 20 for c in got)


def test_correlated_events(A):
    rng = np.random.default_rng(5)
    n = 10_000
    x, y, t, p = stream(rng, n)
    ids = np.arange(n)
    t = t + ids * 1e-3                                           # distinct t: t identifies the event
    for to_add in (3_000, 25_000):
        iters = int(to_add / n) + 1
        gx, gy, gt, gp = A.add_correlated_events(x, y, t, p, to_add, xy_std=0, ts_std=0, seed=3)
        assert all(c.dtype == np.float64 and len(c) == to_add for c in (gx, gy, gt, gp))
        blk = np.stack((gt, gx, gy, gp), 1).view(np.int64)
        assert np.all((blk[1:, 0] > blk[:-1, 0]) | (blk[1:, 0] == blk[:-1, 0]))   # sorted (positive t: int order)
        e = np.searchsorted(t, gt)
        assert np.array_equal(t[e], gt) and np.array_equal(x[e], gx) and np.array_equal(y[e], gy) and np.array_equal(p[e], gp)
        assert np.bincount(e, minlength=n).max() <= iters
    # sigma > 0: moments of the jitter (chosen events keep their t order inside a copy: unsorted output is candidate order)
    xs = np.full(n, 30)
    ys = np.full(n, 20)
    xs[0], ys[0] = 60, 40                                         # clip range far from the mean (its copies left out below)
    gx, gy, gt, gp = A.add_correlated_events(xs, ys, t, p, 200_000, sort=False, return_merged=False, xy_std=3.0,
                                             ts_std=0.01, seed=4)
    dx, dy = gx - 30, gy - 20
    for d in (dx[np.abs(dx) < 15], dy[np.abs(dy) < 15]):
        want = np.trunc(3.0 * np.random.default_rng(0).standard_normal(2_000_000))
        assert abs(d.mean()) < 0.03 and abs(d.var() - want.var()) < 0.1
    # the time jitter: nearest original time is within ~6 sigma
    assert np.abs(gt - t[np.clip(np.searchsorted(t, gt), 0, n - 1)]).max() < 0.1
    # merged with noise, no originals
    r = A.add_correlated_events(x, y, t, p, 500, add_noise=50, seed=2)
    assert all(len(c) == 550 for c in r)
    with pytest.raises(ValueError):
        A.add_correlated_events(x, y, t, p, -1, seed=2)


def test_flip_crop_rotate_are_exact(A):
    from event_utils_amd import DeviceEvents
    rng = np.random.default_rng(6)
    x, y, t, p = stream(rng, 3000)
    dev = [torch.from_numpy(c).cuda() for c in (x, y, t, p)]
    for f in (A.flip_events_x, A.flip_events_y):
        for g, w in zip(f(*dev, sensor_resolution=(H, W)), f(x, y, t, p, sensor_resolution=(H, W))):
            same(g, w)
    ev = DeviceEvents(*[c.to(torch.float64) for c in dev])
    fe = A.flip_events_x(ev, None, None, None, (H, W))
    same(fe.x, (W - x).astype(np.float64))
    got = A.crop_events(dev[0], dev[1], (H, W), (20, 30))
    keep = (x < 30) & (y < 20)
    same(got[0], x[keep])
    same(got[1], y[keep])
    for theta, centre in ((1.4, (90, 120)), (None, None), (0.7, (2.5, -3.0))):
        for cx, cy in ((x, y), (x.astype(np.float32), y.astype(np.float32)), (x.astype(np.int16), y.astype(np.int16))):
            np.random.seed(3)
            want = np_rotate_events(cx, cy, (H, W), theta, centre)
            np.random.seed(3)
            got = A.rotate_events(torch.from_numpy(cx).cuda(), torch.from_numpy(cy).cuda(), (H, W), theta, centre)
            same(got[0], want[0])
            same(got[1], want[1])
            assert got[2] == want[2] and tuple(got[3]) == tuple(want[3])
        np.random.seed(3)
        want = np_rotate_events(x, y, (H, W), theta, centre)
        np.random.seed(3)
        got = A.rotate_events(x, y, (H, W), theta, centre, clip_to_range=True)
        k = (want[0] >= 0) & (want[0] < W) & (want[1] >= 0) & (want[1] < H)
        same(got[0], want[0][k])
        same(got[1], want[1][k])


def test_voxel_grid_of_augmented_device_events(A):
    import event_utils_amd as E
    from event_utils_amd import DeviceEvents
    rng = np.random.default_rng(7)
    x, y, t, p = stream(rng, 200_000)
    ev = DeviceEvents(*[torch.from_numpy(np.asarray(c, dtype=np.float64)).cuda() for c in (x, y, t, p)])
    aug = A.add_random_events(ev, None, None, None, 30_000, seed=5)
    aug = A.remove_events(aug, None, None, None, 50_000, seed=6)
    hx = np_add_random_events(x, y, t, p, 30_000, seed=5)
    hx = np_remove_events(*hx, 50_000, seed=6)
    for g, w in zip((aug.x, aug.y, aug.t, aug.p), hx):
        same(g, w)
    # (the voxel grid takes float32 columns, as the reference's index_put_ does)
    got = E.events_to_voxel_torch(*[c.float() for c in (aug.x, aug.y, aug.t, aug.p)], 5, sensor_size=(H, W))
    want = E.events_to_voxel_torch(*[torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).cuda() for c in hx], 5,
                                   sensor_size=(H, W))
    assert torch.equal(got, want)
