"""GPU: semi-global matching (event_utils_amd/depth/sgm.py, evk_sgm.hip) against its restatement (tests/_sgm_np.py), bit for bit:
the aggregated volume, index, cost and mask are torch.equal, the disparity is equal NaNs included.  Everything is integers, so no
comparison here has a tolerance."""
import functools

import numpy as np
import pytest
import torch

import _sgm_np as G
import _stereo_np as N

pytestmark = pytest.mark.gpu


def random_volume(seed, K, D, H, W, holes=0.0, pixels=0.0, high=2000, big=0.0):
    """(K, D, H, W) int32 costs 0 .. high - 1; a share `holes` of the cells and `pixels` of the whole pixels absent (-1 .. -9); a
    share `big` of the cells past 2^22"""
    rng = np.random.default_rng(seed)
    vol = rng.integers(0, high, (K, D, H, W), dtype=np.int64)
    if big:
        up = rng.random(vol.shape) < big
        vol[up] = rng.integers(G.MAX_COST - 2, 2 ** 31, int(up.sum()))
    vol[rng.random(vol.shape) < holes] = -1
    gone = rng.random((K, 1, H, W)) < pixels
    vol = np.where(gone, -rng.integers(1, 10, vol.shape), vol)
    return vol.astype(np.int32)


def check_aggregate(E, vol, p1, p2, paths, want=None):
    got = E.sgm_aggregate(torch.from_numpy(vol).cuda(), p1, p2, paths)
    want = G.aggregate(vol, p1, p2, paths) if want is None else want
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == vol.shape
    if not torch.equal(got.cpu(), torch.from_numpy(want)):
        got = got.cpu().numpy()
        bad = np.argwhere(got != want)
        raise AssertionError("%d of %d sums differ, the first at (k, i, y, x) = %s: %d, expected %d" % (
            len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))
    return want


def check_match(E, vol, A, d_min, **kw):
    res = E.match_cost_volume(torch.from_numpy(vol).cuda(), torch.from_numpy(A).cuda(), d_min, **kw)
    want = G.match_volume(vol, A, d_min, **kw)
    assert isinstance(res, E.Disparity) and all(t.is_cuda and tuple(t.shape) == want[1].shape for t in res)
    assert (res.disparity.dtype, res.index.dtype, res.cost.dtype, res.mask.dtype) == (torch.float32, torch.int32, torch.int32, torch.bool)
    assert torch.equal(res.cost.cpu(), torch.from_numpy(want[2])), "cost"
    assert torch.equal(res.index.cpu(), torch.from_numpy(want[1])), "index"
    assert torch.equal(res.mask.cpu(), torch.from_numpy(want[3])), "mask"
    assert np.array_equal(res.disparity.cpu().numpy(), want[0], equal_nan=True), "disparity"
    return res, want


def same_bits(a, b):
    return all(torch.equal(s.view(torch.int32) if s.dtype == torch.float32 else s, t.view(torch.int32) if t.dtype == torch.float32 else t)
               for s, t in zip(a, b))


# ---- sgm_aggregate ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def directions_case():
    """one volume with holes and absent pixels, two lines of 64-wide tiles and a bit, and the L_r of each direction on its own"""
    vol = random_volume(11, 1, 16, 33, 131, holes=0.15, pixels=0.05)
    return vol, {r: G.path_costs(vol, 40, 300, r) for r in G.DIRECTIONS}


@pytest.mark.parametrize("paths", list(G.DIRECTIONS) + [4, 8, ((-1, 1), (0, -1), (1, 0))], ids=str)
def test_each_direction_and_their_sums(paths):
    import event_utils_amd as E
    vol, L = directions_case()
    if isinstance(paths, tuple) and isinstance(paths[0], int):
        paths = (paths,)                                    # one direction on its own
    want = np.where(vol >= 0, sum(L[r] for r in G.directions(paths)), -1).astype(np.int32)
    check_aggregate(E, vol, 40, 300, paths, want)


@pytest.mark.parametrize("D", [1, 2, 5, 16, 63, 64, 65, 256])
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (7, 1), (5, 6), (33, 131)], ids=str)
def test_shapes_and_disparity_counts(shape, D):
    import event_utils_amd as E
    K = 3 if shape == (5, 6) else 1
    check_aggregate(E, random_volume(D + shape[1], K, D, *shape, holes=0.1, pixels=0.05), 25, 200, 8)


@pytest.mark.parametrize("D", [5, 65])
def test_five_tiles_of_pixels_and_lines_longer_than_a_wave(D):
    import event_utils_amd as E
    check_aggregate(E, random_volume(D, 1, D, 70, 259, holes=0.1, pixels=0.02), 25, 200, 8)


def test_three_slices_at_once():
    import event_utils_amd as E
    vol = random_volume(5, 3, 16, 33, 131, holes=0.1, pixels=0.05)
    want = check_aggregate(E, vol, 25, 200, 4)
    for k in range(3):                                      # a slice does not see its neighbours
        check_aggregate(E, vol[k:k + 1].copy(), 25, 200, 4, want[k:k + 1])


@pytest.mark.parametrize("d_min", [0, 3])
@pytest.mark.parametrize("C", [1, 2])
def test_volumes_of_stereo_cost_volume(C, d_min):
    import event_utils_amd as E
    QL, QR = N.random_pair(np.random.default_rng(7 + d_min), 1, C, 33, 131, density=0.3)
    vol = E.stereo_cost_volume(torch.from_numpy(QL).cuda(), torch.from_numpy(QR).cuda(), d_min + 15, radius=2, min_disparity=d_min)
    host = vol.cpu().numpy()
    assert np.array_equal(host, N.cost_volume(QL, QR, d_min, 16, 2))
    want = G.aggregate(host, 100, 800, 8)
    got = E.sgm_aggregate(vol, 100, 800)
    assert torch.equal(got.cpu(), torch.from_numpy(want)) and torch.equal(vol.cpu(), torch.from_numpy(host))        # the input is left alone
    assert torch.equal(E.sgm_aggregate(host, 100, 800, 8).cpu(), torch.from_numpy(want))                             # a numpy volume


def test_an_absent_volume_and_absent_pixels():
    import event_utils_amd as E
    gone = -np.ones((2, 5, 9, 70), dtype=np.int32)
    assert np.array_equal(check_aggregate(E, gone, 3, 9, 8), gone)
    vol = random_volume(3, 1, 20, 9, 70, holes=0.5, pixels=0.5)           # half of the pixels absent: most paths start again
    check_aggregate(E, vol, 3, 9, 8)
    check_aggregate(E, random_volume(4, 1, 70, 9, 70, holes=0.9), 3, 9, 8)    # nearly empty, two registers a lane


@pytest.mark.parametrize("p1,p2", [(0, 0), (0, 500), (77, 77), (1000, G.MAX_PENALTY), (G.MAX_PENALTY, G.MAX_PENALTY)])
def test_the_penalties_at_their_ends_and_costs_past_the_clamp(p1, p2):
    import event_utils_amd as E
    vol = random_volume(p1 + p2, 2, 33, 12, 67, holes=0.1, pixels=0.05, high=G.MAX_COST + 1000, big=0.2)
    want = check_aggregate(E, vol, p1, p2, 8)
    assert want.max() > 8 * (G.MAX_COST - 1)
    if p2 == 0:
        assert np.array_equal(want, np.where(vol >= 0, 8 * np.minimum(vol.astype(np.int64), G.MAX_COST), -1))


# ---- match_cost_volume -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def match_case(C, d_min):
    QL, QR = N.random_pair(np.random.default_rng(20 + C + d_min), 2, C, 33, 131, density=0.4)
    raw = N.cost_volume(QL, QR, d_min, 16, 1).astype(np.int32)
    return QL, QR, raw, G.aggregate(raw, 60, 480, 8)


SWITCHES = [dict(), dict(uniqueness=0), dict(uniqueness=50), dict(uniqueness=99), dict(max_cost=150), dict(max_cost=0), dict(lr_tolerance=None),
            dict(lr_tolerance=0), dict(lr_tolerance=3), dict(subpixel=False), dict(min_activity=1), dict(min_activity=255),
            dict(uniqueness=0, lr_tolerance=None, subpixel=False)]


@pytest.mark.parametrize("kw", SWITCHES, ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()) or "defaults")
@pytest.mark.parametrize("C,d_min", [(1, 0), (2, 3)])
def test_the_winner_of_raw_and_aggregated_volumes(C, d_min, kw):
    import event_utils_amd as E
    QL, _, raw, agg = match_case(C, d_min)
    _, want = check_match(E, raw, QL, d_min, **kw)
    scaled = dict(kw, max_cost=8 * kw["max_cost"] + 2000) if "max_cost" in kw else kw
    _, want_agg = check_match(E, agg, QL, d_min, **scaled)
    if not kw:
        assert want[3].sum() > 100 and want_agg[3].sum() > 100 and (~want[3] & want[4]).sum() > 100


def test_the_winner_of_a_volume_with_holes_ties_and_large_values():
    import event_utils_amd as E
    rng = np.random.default_rng(5)
    A = rng.integers(0, 256, (2, 2, 9, 70)).astype(np.uint8)
    large = random_volume(7, 2, 40, 9, 70, holes=0.1, high=2 ** 31 - 1)                  # products past 2^32, keys past 2^32
    for vol in (random_volume(6, 2, 7, 9, 70, holes=0.4, pixels=0.2, high=6),           # ties everywhere
                large, -np.ones((2, 3, 9, 70), dtype=np.int32), random_volume(8, 2, 1, 9, 70, holes=0.3),
                random_volume(9, 2, 256, 9, 70, holes=0.3)):
        for d_min in (0, 5):
            check_match(E, vol, A, d_min, min_activity=100)
            _, want = check_match(E, vol, A, d_min, min_activity=100, uniqueness=30, lr_tolerance=0, max_cost=2 ** 30)
            if vol is large:
                # valid winners of 2^24 and more, each past the uniqueness test against a runner-up that is no smaller: a 32-bit
                # key (cost << 8 | i) would have wrapped for both
                assert ((want[2] >= 2 ** 24) & want[3]).sum() > 100


@pytest.mark.parametrize("C", [1, 2])
def test_on_the_block_matching_volume_it_is_stereo_match(C):
    import math
    import event_utils_amd as E
    for d_min, r, limit in ((0, 3, None), (3, 1, 21.5), (0, 2, 40.0)):
        QL, QR = N.random_pair(np.random.default_rng(30 + r), 2, C, 33, 131, density=0.4)
        tl, tr = torch.from_numpy(QL).cuda(), torch.from_numpy(QR).cuda()
        vol = E.stereo_cost_volume(tl, tr, d_min + 15, radius=r, min_disparity=d_min)
        for kw in (dict(), dict(uniqueness=0, lr_tolerance=None), dict(lr_tolerance=0, subpixel=False)):
            a = E.stereo_match(tl, tr, d_min + 15, radius=r, min_disparity=d_min, max_mean_cost=limit, **kw)
            b = E.match_cost_volume(vol, tl, d_min, max_cost=None if limit is None else math.floor(limit * C * (2 * r + 1) ** 2), **kw)
            assert same_bits(a, b) and int(a.mask.sum()) > 50


# ---- sgm_match and sgm_disparity -------------------------------------------------------------------------------------------------

_PIPELINE = {}


def pipeline(QL, QR, D, r, p1, p2, paths, **kw):
    """the restatement of sgm_match, kept per input"""
    key = (QL.tobytes(), QR.tobytes(), QL.shape, D, r, p1, p2, paths, tuple(sorted(kw.items())))
    if key not in _PIPELINE:
        S = G.aggregate(N.cost_volume(QL, QR, 0, D, r), p1, p2, paths)
        _PIPELINE[key] = (S, G.match_volume(S, QL, 0, **kw))
    return _PIPELINE[key]


def assert_result(res, want):
    assert torch.equal(res.index.cpu(), torch.from_numpy(want[1])) and torch.equal(res.cost.cpu(), torch.from_numpy(want[2]))
    assert torch.equal(res.mask.cpu(), torch.from_numpy(want[3]))
    assert np.array_equal(res.disparity.cpu().numpy(), want[0], equal_nan=True)


@pytest.mark.parametrize("paths", [4, 8])
def test_the_structured_pair_end_to_end(paths):
    import event_utils_amd as E
    QL, QR, truth = G.structured_pair(1)
    S, want = pipeline(QL, QR, G.PAIR_D, G.PAIR_R, G.PAIR_P1, G.PAIR_P2, paths, min_activity=G.PAIR_ACTIVITY)
    res = E.sgm_match(QL, QR, G.PAIR_D - 1, G.PAIR_P1, G.PAIR_P2, paths, radius=G.PAIR_R, min_activity=G.PAIR_ACTIVITY)
    assert_result(res, want)
    again = E.sgm_match(torch.from_numpy(QL).cuda(), torch.from_numpy(QR).cuda(), G.PAIR_D - 1, G.PAIR_P1, G.PAIR_P2, paths, radius=G.PAIR_R,
                        min_activity=G.PAIR_ACTIVITY)
    assert same_bits(res, again)
    plain = E.sgm_match(QL, QR, G.PAIR_D - 1, G.PAIR_P1, G.PAIR_P2, paths, radius=G.PAIR_R, uniqueness=0, lr_tolerance=None)
    raw = E.stereo_match(QL, QR, G.PAIR_D - 1, radius=G.PAIR_R, uniqueness=0, lr_tolerance=None)
    frac = [G.pair_fraction(None, QL, truth, winners=r.index[0].cpu().numpy())[1] for r in (raw, plain)]
    assert frac[1] - frac[0] >= 0.07                        # (half the gain test_cpu_sgm.py measures on this seed)


@pytest.mark.parametrize("polarity", ["ignore", "split"])
@pytest.mark.parametrize("kind", ["numpy", "tensors", "events_f64", "events_f32"])
def test_the_dots_scene_end_to_end(kind, polarity):
    import event_utils_amd as E
    from test_gpu_stereo import as_kind, scene
    sc = scene()
    t_refs = [0.016, N.SCENE_END]
    left, right = as_kind(E, sc["left"], kind), as_kind(E, sc["right"], kind)
    QL, QR = (E.quantised_time_surfaces(*cols, N.SCENE_TAU, N.SCENE_SIZE, t_refs, polarity=polarity).cpu().numpy() for cols in (left, right))
    streams = [c[0] if kind.startswith("events") else c for c in (left, right)]
    res = E.sgm_disparity(streams[0], streams[1], N.SCENE_TAU, N.SCENE_SIZE, t_refs, N.SCENE_D - 1, 784, 6272, radius=N.SCENE_R,
                          polarity=polarity, min_activity=N.SCENE_ACTIVITY)
    _, want = pipeline(QL, QR, N.SCENE_D, N.SCENE_R, 784, 6272, 8, min_activity=N.SCENE_ACTIVITY)
    assert_result(res, want)
    assert want[3][-1].sum() > 100
    again = E.sgm_disparity(streams[0], streams[1], N.SCENE_TAU, N.SCENE_SIZE, t_refs, N.SCENE_D - 1, 784, 6272, radius=N.SCENE_R,
                            polarity=polarity, min_activity=N.SCENE_ACTIVITY)
    assert same_bits(res, again)
    if kind == "numpy" and polarity == "ignore":
        dm = E.disparity_depth_map(res, 1, 200.0, 0.1)
        assert isinstance(dm, E.DepthMap) and torch.equal(dm.mask, res.mask[1] & (res.disparity[1] > 0))
        assert np.array_equal(dm.depth.cpu().numpy(), N.disparity_to_depth(want[0][1], 200.0, 0.1), equal_nan=True)


def test_the_c_entry_may_write_the_sums_over_its_input():
    """include/evk.h: out may be volume (the costs are copied out before the first sum is written back)"""
    from event_utils_amd import _device as Dv
    from event_utils_amd import _lib
    K, D, H, W = 2, 70, 12, 67
    vol = random_volume(21, K, D, H, W, holes=0.1, pixels=0.05)
    want = G.aggregate(vol, 25, 200, 8)
    t = torch.from_numpy(vol).cuda()
    scratch = torch.empty(int(_lib.lib().evk_sgm_scratch_bytes(_lib.EVK_SGM_AGGREGATE, K, D, H, W)), dtype=torch.uint8, device="cuda")
    _lib.call("evk_sgm_aggregate", Dv.ptr(t), K, D, H, W, 25, 200, 255, Dv.ptr(scratch), Dv.ptr(t), Dv.stream())
    assert torch.equal(t.cpu(), torch.from_numpy(want))
