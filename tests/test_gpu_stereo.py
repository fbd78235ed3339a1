"""GPU: event stereo (event_utils_amd/depth/stereo.py, evk_stereo.hip) against its restatement (tests/_stereo_np.py), bit for bit:
the quantised surfaces, the cost volume, index, cost and mask are torch.equal, the disparity is equal NaNs included.  Every cost is
an integer, so no comparison here has a tolerance."""
import functools

import numpy as np
import pytest
import torch

import _stereo_np as N

pytestmark = pytest.mark.gpu


def check_volume(E, QL, QR, d_min, D, r):
    vol = E.stereo_cost_volume(torch.from_numpy(QL).cuda(), torch.from_numpy(QR).cuda(), d_min + D - 1, radius=r, min_disparity=d_min)
    want = N.cost_volume(QL, QR, d_min, D, r)
    assert vol.dtype == torch.int32 and vol.is_cuda and tuple(vol.shape) == want.shape
    got = vol.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%d of %d costs differ, the first at (k, i, y, x) = %s: %d, expected %d" % (
            len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))
    return want


def check_match(E, QL, QR, d_min, D, r, volume=None, **kw):
    """stereo_match against the restatement -> (Disparity, the restatement's results)"""
    res = E.stereo_match(torch.from_numpy(QL).cuda(), torch.from_numpy(QR).cuda(), d_min + D - 1, radius=r, min_disparity=d_min, **kw)
    want = N.match(QL, QR, d_min, D, r, volume=volume, **kw)
    assert isinstance(res, E.Disparity) and all(t.is_cuda and tuple(t.shape) == want[1].shape for t in res)
    assert (res.disparity.dtype, res.index.dtype, res.cost.dtype, res.mask.dtype) == (torch.float32, torch.int32, torch.int32, torch.bool)
    assert torch.equal(res.cost.cpu(), torch.from_numpy(want[2])), "cost"
    assert torch.equal(res.index.cpu(), torch.from_numpy(want[1])), "index"
    assert torch.equal(res.mask.cpu(), torch.from_numpy(want[3])), "mask"
    assert np.array_equal(res.disparity.cpu().numpy(), want[0], equal_nan=True), "disparity"
    return res, want


# ---- the seeded scene, end to end ------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scene():
    return N.scene()


def as_kind(E, cols, kind):
    xs, ys, ts, ps = N.stream(cols)
    if kind == "numpy":
        return (xs, ys, ts, ps)
    if kind == "tensors":
        return tuple(torch.from_numpy(c).cuda() for c in (xs, ys, ts, ps))
    return (E.DeviceEvents.from_arrays(xs, ys, ts, ps, **({"precision": "f32"} if kind == "events_f32" else {})), None, None, None)


@pytest.mark.parametrize("t_refs", [(N.SCENE_END,), (0.012, 0.016, N.SCENE_END)], ids=["K1", "K3"])
@pytest.mark.parametrize("polarity", ["ignore", "split"])
@pytest.mark.parametrize("kind", ["numpy", "tensors", "events_f64", "events_f32"])
def test_the_seeded_scene(kind, polarity, t_refs):
    import event_utils_amd as E
    sc = scene()
    left, right = as_kind(E, sc["left"], kind), as_kind(E, sc["right"], kind)
    K, C = len(t_refs), 2 if polarity == "split" else 1
    Q, host = [], []
    for cols, raw in ((left, sc["left"]), (right, sc["right"])):
        q = E.quantised_time_surfaces(*cols, N.SCENE_TAU, N.SCENE_SIZE, list(t_refs), polarity=polarity)
        assert q.dtype == torch.uint8 and q.is_cuda and tuple(q.shape) == (K, C) + N.SCENE_SIZE
        a = E.time_surfaces(*cols, N.SCENE_TAU, N.SCENE_SIZE, t_refs=list(t_refs), decay=None, polarity=polarity)
        a = a.cpu().numpy() if isinstance(a, torch.Tensor) else a
        if kind != "events_f32":                            # float64 stamps: the ages are those of the restatement itself
            assert np.array_equal(a, N.ages(*N.stream(raw), N.SCENE_SIZE, t_refs, polarity))
        host.append(N.quantise(a, N.SCENE_TAU))
        assert torch.equal(q.cpu(), torch.from_numpy(host[-1]))
        Q.append(q)
    streams = [c[0] if kind.startswith("events") else c for c in (left, right)]
    res = E.stereo_disparity(streams[0], streams[1], N.SCENE_TAU, N.SCENE_SIZE, list(t_refs), N.SCENE_D - 1, radius=N.SCENE_R,
                             polarity=polarity, min_activity=N.SCENE_ACTIVITY)
    want = N.match(host[0], host[1], 0, N.SCENE_D, N.SCENE_R, N.SCENE_ACTIVITY)
    assert torch.equal(res.index.cpu(), torch.from_numpy(want[1])) and torch.equal(res.cost.cpu(), torch.from_numpy(want[2]))
    assert torch.equal(res.mask.cpu(), torch.from_numpy(want[3]))
    assert np.array_equal(res.disparity.cpu().numpy(), want[0], equal_nan=True)
    assert want[3][-1].sum() > 100 and (want[1][-1][want[3][-1]] == 4).sum() > 20 and (want[1][-1][want[3][-1]] == 9).sum() > 20
    again = E.stereo_match(Q[0], Q[1], N.SCENE_D - 1, radius=N.SCENE_R, min_activity=N.SCENE_ACTIVITY)
    assert all(torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
               for a, b in zip(again, res))
    if kind == "numpy" and polarity == "ignore":
        dm = E.disparity_depth_map(res, K - 1, 200.0, 0.1)
        assert isinstance(dm, E.DepthMap) and torch.equal(dm.mask, res.mask[-1] & (res.disparity[-1] > 0)) and dm.depth.dtype == torch.float64
        assert np.array_equal(dm.depth.cpu().numpy(), N.disparity_to_depth(want[0][-1], 200.0, 0.1), equal_nan=True)
        assert torch.equal(dm.confidence, -res.cost[-1].to(torch.float32))
        pts = E.depth_to_points(dm, np.array([[200.0, 0, 48.0], [0, 200.0, 24.0], [0, 0, 1.0]]), (np.zeros(3), np.array([0.0, 0, 0, 1.0])))
        assert tuple(pts.shape) == (int(dm.mask.sum()), 3) and bool((pts[:, 2] > 0).all())


def test_unsorted_stamps_in_either_stream_are_refused():
    import event_utils_amd as E
    sc = scene()
    left, right = N.stream(sc["left"]), N.stream(sc["right"])
    shuffled = tuple(c[::-1].copy() for c in right)
    for a, b in ((left, shuffled), (shuffled, left)):
        with pytest.raises(ValueError, match="non-decreasing"):
            E.stereo_disparity(a, b, N.SCENE_TAU, N.SCENE_SIZE, [N.SCENE_END], 15)


# ---- random surfaces at the shapes where packing and tiling can go wrong ---------------------------------------------------------

SHAPES = [
    # (H, W), D, d_min, radius, C, K
    ((7, 9), 16, 0, 3, 1, 1),                               # W < D, H = 2 r + 1
    ((7, 9), 16, 3, 3, 2, 2),
    ((5, 6), 5, 0, 7, 1, 1),                                # H < 2 r + 1
    ((5, 6), 1, 3, 7, 2, 1),
    ((33, 131), 64, 0, 1, 2, 2),                            # widths that are no multiple of 4, one past two tiles of 64
    ((33, 131), 5, 3, 7, 1, 1),
    ((33, 131), 256, 3, 3, 2, 1),
    ((33, 131), 16, 0, 2, 1, 1),                            # every other radius: each has its own window tail
    ((33, 131), 16, 3, 4, 2, 1),
    ((33, 131), 16, 0, 5, 1, 1),
    ((33, 131), 16, 3, 6, 1, 1),
    ((70, 259), 256, 0, 1, 1, 1),                           # one past four tiles of 64; nine row tiles
    ((70, 259), 64, 3, 7, 2, 1),
    ((70, 259), 1, 0, 3, 1, 3),
    ((70, 259), 5, 0, 1, 2, 1),
]


@pytest.mark.parametrize("size,D,d_min,r,C,K", SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_random_surfaces(size, D, d_min, r, C, K):
    import event_utils_amd as E
    rng = np.random.default_rng([size[0], size[1], D, d_min, r, C, K])
    QL, QR = N.random_pair(rng, K, C, size[0], size[1], density=0.6, noise=0.1)
    vol = check_volume(E, QL, QR, d_min, D, r)
    check_match(E, QL, QR, d_min, D, r, volume=vol, min_activity=64)
    check_match(E, QL, QR, d_min, D, r, volume=vol, min_activity=1, uniqueness=0, lr_tolerance=0, max_mean_cost=60.0)


def test_a_shift_known_in_advance_is_found():
    import event_utils_amd as E
    rng = np.random.default_rng(5)
    QL, QR = N.random_pair(rng, 1, 1, 40, 150, density=0.5, shift=11, noise=0.0)
    res, want = check_match(E, QL, QR, 2, 30, 3, min_activity=1)
    index, cost = res.index[0, 4:-4, 11 + 4:-4], res.cost[0, 4:-4, 11 + 4:-4]
    lit = cost >= 0                                         # (a dark left pixel is no candidate)
    assert int(lit.sum()) > 1000 and bool((index[lit] == 11).all()) and bool((cost[lit] == 0).all())


# ---- adversarial surfaces --------------------------------------------------------------------------------------------------------

def test_empty_surfaces_have_no_candidates():
    import event_utils_amd as E
    Z = np.zeros((2, 2, 20, 70), dtype=np.uint8)
    res, _ = check_match(E, Z, Z, 0, 16, 3)
    assert bool((res.cost == -1).all()) and bool((res.index == -1).all()) and not bool(res.mask.any()) and bool(res.disparity.isnan().all())
    assert bool((check_volume(E, Z, Z, 0, 16, 3)[:, 0] == 0).all())


def test_the_largest_cost():
    import event_utils_amd as E
    L, R = np.full((1, 2, 20, 70), 255, dtype=np.uint8), np.zeros((1, 2, 20, 70), dtype=np.uint8)
    vol = check_volume(E, L, R, 0, 8, 7)
    assert vol.max() == 2 * 15 * 15 * 255 and vol[0, 3, 10, 30] == 2 * 15 * 15 * 255
    res, _ = check_match(E, L, R, 0, 8, 7, volume=vol, uniqueness=0, lr_tolerance=None)
    assert int(res.cost.max()) == 2 * 15 * 15 * 255


def test_a_periodic_pattern_ties():
    """period 8 in x and a right surface 3 higher everywhere: d = 0, 8 and 16 cost the same, 3 per window pixel; the smallest wins,
    and with a rival as good as the winner the uniqueness test rejects"""
    import event_utils_amd as E
    pattern = np.array([10, 200, 60, 120, 5, 250, 30, 90], dtype=np.uint8)          # (no zero: every pixel is a candidate)
    QL = np.tile(pattern, (1, 1, 12, 10))                   # (1, 1, 12, 80)
    QR = QL + 3
    res, want = check_match(E, QL, QR, 0, 24, 2, min_activity=1, uniqueness=0, lr_tolerance=None)
    assert bool((res.index[0, 2:-2, 18:-2] == 0).all()) and bool((res.cost[0, 2:-2, 18:-2] == 75).all())
    res, want = check_match(E, QL, QR, 0, 24, 2, min_activity=1, uniqueness=10, lr_tolerance=None)
    assert bool((res.index[0, 2:-2, 18:-2] == -1).all()) and bool((res.cost[0, 2:-2, 18:-2] == 75).all())
    assert bool((res.index[0, 2:-2, 2:8] == 0).all())       # x < 8: d = 8 is not admissible, nothing rivals d = 0


SWITCHES = [dict(uniqueness=25), dict(max_mean_cost=20.0), dict(lr_tolerance=0), dict(subpixel=True)]


def test_every_switch_on_its_own():
    import event_utils_amd as E
    rng = np.random.default_rng(11)
    QL, QR = N.random_pair(rng, 2, 2, 37, 133, density=0.4, noise=0.15)
    vol = N.cost_volume(QL, QR, 1, 40, 2)
    off = dict(min_activity=32, uniqueness=0, max_mean_cost=None, lr_tolerance=None, subpixel=False)
    base, _ = check_match(E, QL, QR, 1, 40, 2, volume=vol, **off)
    assert bool(base.mask.any()) and torch.equal(base.mask, base.cost >= 0) and torch.equal(base.disparity[base.mask], base.index[base.mask].float())
    for switch in SWITCHES:
        res, _ = check_match(E, QL, QR, 1, 40, 2, volume=vol, **dict(off, **switch))
        assert torch.equal(res.cost, base.cost)
        if "subpixel" in switch:
            assert torch.equal(res.mask, base.mask) and bool((res.disparity[res.mask] != base.disparity[res.mask]).any())
        else:
            assert bool((res.mask <= base.mask).all()) and 0 < int(res.mask.sum()) < int(base.mask.sum()), switch
    check_match(E, QL, QR, 1, 40, 2, volume=vol, min_activity=32, uniqueness=25, max_mean_cost=20.0, lr_tolerance=0, subpixel=True)


def test_two_calls_give_identical_bits():
    import event_utils_amd as E
    rng = np.random.default_rng(13)
    QL, QR = (torch.from_numpy(q).cuda() for q in N.random_pair(rng, 3, 2, 70, 259, density=0.3))
    a, b = (E.stereo_match(QL, QR, 63, min_activity=32) for _ in range(2))
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u, v.view(torch.int32) if v.dtype == torch.float32 else v)
    assert int(a.mask.sum()) > 100
    assert torch.equal(E.stereo_cost_volume(QL, QR, 63), E.stereo_cost_volume(QL, QR, 63))
    # host arrays are taken as well
    c = E.stereo_match(QL.cpu().numpy(), QR.cpu().numpy(), 63, min_activity=32)
    assert torch.equal(c.index, a.index) and c.index.is_cuda
