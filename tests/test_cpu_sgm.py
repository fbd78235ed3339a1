"""CPU (no GPU): the host restatement of semi-global matching (tests/_sgm_np.py, the literal definition) on hand-worked cases and
its symmetries; what aggregation gains on the seeded structured pair; the evk_sgm_* entry points are declared, bound and exported
and refuse bad arguments before they touch the device; the Python argument errors; the public surface; the kernels of evk_sgm.hip
compile for gfx950 without register spills and without scratch memory."""
import ctypes
import os
import re

import numpy as np
import pytest

import _header
import _sgm_np as G
import _stereo_np as N

ENTRIES = {"evk_sgm_aggregate", "evk_sgm_match_volume"}
PUBLIC = ("sgm_aggregate", "match_cost_volume", "sgm_match", "sgm_disparity")


def row(cells):
    """(1, D, 1, W) volume of a one-row image from a list of W pixels of D costs each"""
    return np.array(cells, dtype=np.int64).T[None, :, None, :]


# ---- hand-worked cases of the restatement --------------------------------------------------------------------------------------------

def test_three_pixels_and_three_disparities_by_hand():
    """P1 = 2, P2 = 5, direction (1, 0); C(0) = [4, 1, 6], C(1) = [3, 7, 2], C(2) = [5, 5, 0].
    L(0) = C(0) = [4, 1, 6], m = 1.
    L(1, 0) = 3 + min(4, -, 1 + 2, 1 + 5) - 1 = 5;  L(1, 1) = 7 + min(1, 4 + 2, 6 + 2, 6) - 1 = 7;
    L(1, 2) = 2 + min(6, 1 + 2, -, 6) - 1 = 4;  m = 4.
    L(2, 0) = 5 + min(5, -, 7 + 2, 4 + 5) - 4 = 6;  L(2, 1) = 5 + min(7, 5 + 2, 4 + 2, 9) - 4 = 7;
    L(2, 2) = 0 + min(4, 7 + 2, -, 9) - 4 = 0."""
    vol = row([[4, 1, 6], [3, 7, 2], [5, 5, 0]])
    L = G.path_costs(vol, 2, 5, (1, 0))
    assert L.shape == (1, 3, 1, 3) and L[0, :, 0, :].T.tolist() == [[4, 1, 6], [5, 7, 4], [6, 7, 0]]
    back = G.path_costs(vol[..., ::-1], 2, 5, (-1, 0))     # the same walk from the other end
    assert back[0, :, 0, ::-1].T.tolist() == [[4, 1, 6], [5, 7, 4], [6, 7, 0]]
    S = G.aggregate(vol, 2, 5, ((1, 0),))
    assert S.dtype == np.int32 and np.array_equal(S, L)
    # a one-row image: the vertical and diagonal paths have no predecessor on the sensor, L = C
    assert np.array_equal(G.aggregate(vol, 2, 5, ((0, 1), (1, 1), (-1, 1))), 3 * vol)
    assert np.array_equal(G.aggregate(vol, 2, 5, 4), L + G.path_costs(vol, 2, 5, (-1, 0)) + 2 * vol)


def test_a_path_starts_again_behind_a_pixel_without_a_present_cell():
    vol = row([[4, 1, 6], [-1, -1, -1], [5, 5, 0], [1, 9, 9]])
    L = G.path_costs(vol, 2, 5, (1, 0))
    assert L[0, :, 0, 2].tolist() == [5, 5, 0]            # q has no present cell: L = C
    assert L[0, :, 0, 3].tolist() == [1 + 5, 9 + 2, 9]    # m = 0: min(5, 5 + 2, 0 + 5), min(5, 5 + 2, 0 + 2, 5), min(0, 5 + 2, 5)
    S = G.aggregate(vol, 2, 5, ((1, 0),))
    assert S[0, :, 0, 1].tolist() == [-1, -1, -1] and S[0, :, 0, 0].tolist() == [4, 1, 6]


def test_neighbour_terms_that_do_not_exist_or_are_absent():
    """C(0) = [4, -, 6], m = 4, P1 = 2, P2 = 5.  L(1, 0) = 3 + min(4, [i + 1 absent], 9) - 4 = 3;
    L(1, 1) = 7 + min([i absent], 4 + 2, 6 + 2, 9) - 4 = 9;  L(1, 2) = 2 + min(6, [i - 1 absent], [no i + 1], 9) - 4 = 4.
    A cell of p that is absent has no L: pixel 2 = [-, 5, -] gets L(2, 1) = 5 + min(9, 3 + 2, 4 + 2, 3 + 5) - 3 = 7 only."""
    vol = row([[4, -1, 6], [3, 7, 2], [-1, 5, -7]])
    L = G.path_costs(vol, 2, 5, (1, 0))
    assert L[0, :, 0, 1].tolist() == [3, 9, 4] and L[0, :, 0, 2].tolist() == [0, 7, 0]
    assert G.aggregate(vol, 2, 5, ((1, 0),))[0, :, 0, :].T.tolist() == [[4, -1, 6], [3, 9, 4], [-1, 7, -1]]
    one = row([[5], [2], [9]])                              # D = 1: neither neighbour exists, L = C + min(L(q), m + P2) - m = C
    assert np.array_equal(G.aggregate(one, 2, 5, 8), 8 * one)


def test_a_cost_counts_up_to_two_to_the_22():
    vol = row([[G.MAX_COST + 5, 7], [2 ** 31 - 1, G.MAX_COST]])
    assert G.aggregate(vol, 0, 0, ((1, 0),))[0, :, 0, :].T.tolist() == [[G.MAX_COST, 7], [G.MAX_COST, G.MAX_COST]]
    top = G.aggregate(np.full((1, 2, 3, 3), 2 ** 31 - 1), G.MAX_PENALTY, G.MAX_PENALTY, 8)
    assert top.dtype == np.int32 and top.max() <= 8 * (G.MAX_COST + G.MAX_PENALTY) and top.min() >= 8 * G.MAX_COST


def test_without_penalties_the_sum_is_paths_times_the_cost():
    rng = np.random.default_rng(0)
    vol = rng.integers(-40, 400, (2, 5, 6, 7))
    want = lambda n: np.where(vol >= 0, n * vol, -1)
    assert np.array_equal(G.aggregate(vol, 0, 0, 8), want(8)) and np.array_equal(G.aggregate(vol, 0, 0, 4), want(4))
    assert np.array_equal(G.aggregate(vol, 0, 0, ((1, -1), (0, 1), (-1, -1))), want(3))


def test_a_path_cost_lies_between_the_cost_and_the_cost_plus_p2():
    rng = np.random.default_rng(1)
    for p1, p2 in ((0, 0), (3, 3), (5, 40), (0, 17), (G.MAX_PENALTY, G.MAX_PENALTY)):
        vol = rng.integers(-300, 1000, (1, 6, 7, 9))
        for r in G.DIRECTIONS:
            L = G.path_costs(vol, p1, p2, r)               # (asserts the bound at every pixel itself)
            pres = vol >= 0
            assert (L[pres] >= vol[pres]).all() and (L[pres] <= vol[pres] + p2).all() and (L[~pres] == 0).all()


def test_mirrors_and_the_transpose_map_the_directions_onto_each_other():
    rng = np.random.default_rng(2)
    vol = rng.integers(-60, 500, (2, 4, 5, 8))
    for a, b in (((1, 0), (-1, 0)), ((1, 1), (-1, 1)), ((1, -1), (-1, -1)), ((0, 1), (0, 1))):      # mirrored in x
        assert np.array_equal(G.aggregate(vol[..., ::-1], 7, 31, (a,))[..., ::-1], G.aggregate(vol, 7, 31, (b,)))
    for a, b in (((0, 1), (0, -1)), ((1, 1), (1, -1)), ((-1, 1), (-1, -1)), ((1, 0), (1, 0))):      # mirrored in y
        assert np.array_equal(G.aggregate(vol[:, :, ::-1], 7, 31, (a,))[:, :, ::-1], G.aggregate(vol, 7, 31, (b,)))
    for a, b in (((1, 0), (0, 1)), ((-1, 0), (0, -1)), ((1, -1), (-1, 1)), ((1, 1), (1, 1))):       # transposed
        assert np.array_equal(G.aggregate(vol.transpose(0, 1, 3, 2), 7, 31, (a,)).transpose(0, 1, 3, 2), G.aggregate(vol, 7, 31, (b,)))
    assert G.directions(4) == G.DIRECTIONS[:4] and G.directions(8) == G.DIRECTIONS
    assert G.directions(((0, -1), (1, 0))) == ((1, 0), (0, -1))


def test_the_winner_of_a_volume_needs_a_right_pixel():
    """a present cell with x - d < 0 has no right pixel and does not compete; the cost limit is the integer itself"""
    vol = np.full((1, 3, 1, 4), 9, dtype=np.int64)
    vol[0, 2, 0, 1] = 0                                     # d = 2 at x = 1
    A = np.full((1, 2, 1, 4), 200, dtype=np.uint8)
    _, idx, cost, valid, cand = G.match_volume(vol, A, 0, uniqueness=0, lr_tolerance=None)
    assert idx[0, 0].tolist() == [0, 0, 0, 0] and cost[0, 0].tolist() == [9, 9, 9, 9] and cand.all()
    assert not G.match_volume(vol, A, 1, uniqueness=0, lr_tolerance=None)[4][0, 0, 0]       # d_min = 1: nothing at x = 0
    assert G.match_volume(vol, A, 0, uniqueness=0, lr_tolerance=None, max_cost=9)[3].all()
    assert not G.match_volume(vol, A, 0, uniqueness=0, lr_tolerance=None, max_cost=8)[3].any()


# ---- the seeded structured pair ----------------------------------------------------------------------------------------------------

RAW = {1: 0.792, 2: 0.798, 3: 0.771}
AGGREGATED = {1: 0.941, 2: 0.967, 3: 0.963}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_aggregation_gains_on_continuous_contours(seed):
    """The structured pair of _sgm_np: 40 x 96, continuous contours on the planes d = 4 and d = 9 and a surface slanted from d = 3
    to 11, 35 % of the right pixels redrawn; D = 16, r = 1, P1 = 144, P2 = 1152, eight paths.  Measured with this restatement, the
    fraction of the candidates at x >= 12 (542 / 550 / 520 for seeds 1 / 2 / 3) whose plain winner is within 1 of the truth, no
    tests: block matching 0.792 / 0.798 / 0.771, aggregated 0.941 / 0.967 / 0.963 (four paths: 0.948 / 0.965 / 0.958).  With
    uniqueness = 10 and lr_tolerance = 1, seed 1: 318 valid of which 0.947 correct, against 492 of which 0.982.  The floors lie
    0.03 below the measurements, one part in thirty being the grain of such a count, and the gain asserted is half the measured.

    Not asserted: on the dots scene of _stereo_np.scene(), isolated dots smaller than its 7 x 7 window, aggregation gains nothing:
    0.744 of the 39 eligible dots before the tests with or without it; after uniqueness = 10 and lr_tolerance = 1, 0.857 of 28
    without it, 0.813 of 32 with P1 = 144, P2 = 1152 and 0.757 of 37 with P1 = 784, P2 = 6272."""
    QL, QR, truth = G.structured_pair(seed)
    vol = N.cost_volume(QL, QR, 0, G.PAIR_D, G.PAIR_R)
    S = G.aggregate(vol, G.PAIR_P1, G.PAIR_P2, 8)
    n, raw = G.pair_fraction(vol, QL, truth)
    _, agg = G.pair_fraction(S, QL, truth)
    print("seed %d: %d candidates, block matching %.3f, aggregated %.3f" % (seed, n, raw, agg))
    assert n >= 500
    assert raw >= RAW[seed] - 0.03 and agg >= AGGREGATED[seed] - 0.03
    assert agg - raw >= (AGGREGATED[seed] - RAW[seed]) / 2


def test_the_tests_keep_more_and_better_winners_after_aggregation():
    QL, QR, truth = G.structured_pair(1)
    vol = N.cost_volume(QL, QR, 0, G.PAIR_D, G.PAIR_R)
    S = G.aggregate(vol, G.PAIR_P1, G.PAIR_P2, 8)
    counted = (QL[0, 0] >= G.PAIR_ACTIVITY) & (np.arange(G.PAIR_SIZE[1])[None, :] >= G.PAIR_MARGIN)
    kept = {}
    for name, v in (("raw", vol), ("aggregated", S)):
        _, idx, _, valid, _ = G.match_volume(v, QL, 0, G.PAIR_ACTIVITY, 10, None, 1)
        ok = valid[0] & counted
        kept[name] = (int(ok.sum()), float((ok & (np.abs(idx[0] - truth) <= 1)).sum()) / int(ok.sum()))
    print(kept)
    assert kept["raw"][0] >= 318 - 16 and kept["aggregated"][0] >= 492 - 16                 # (one part in thirty)
    assert kept["raw"][1] >= 0.947 - 0.03 and kept["aggregated"][1] >= 0.982 - 0.03
    assert kept["aggregated"][0] - kept["raw"][0] >= (492 - 318) // 2


# ---- the public surface and the C ABI ------------------------------------------------------------------------------------------------

def test_the_prototypes_are_bound_with_their_arguments():
    from event_utils_amd import _lib
    text = _header.TEXT
    protos = _header.prototypes("evk_sgm_")
    assert set(protos) == ENTRIES | {"evk_sgm_scratch_bytes"}
    for name, (want, ret) in protos.items():
        assert ret is (ctypes.c_int if name in ENTRIES else ctypes.c_int64), name
        assert _lib.PROTOTYPES[name] == (want, ret), name
        assert hasattr(_lib.lib(), name)
    assert (_lib.EVK_SGM_MAX_COST, _lib.EVK_SGM_MAX_PENALTY, _lib.EVK_SGM_AGGREGATE, _lib.EVK_SGM_MATCH) == (1 << 22, 1 << 20, 0, 1)
    assert (G.MAX_COST, G.MAX_PENALTY) == (1 << 22, 1 << 20)
    for name, value in (("EVK_SGM_MAX_COST", 1 << 22), ("EVK_SGM_MAX_PENALTY", 1 << 20), ("EVK_SGM_AGGREGATE", 0), ("EVK_SGM_MATCH", 1)):
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (name, value), text, re.M)
    assert "Semi-global matching (evk_sgm.hip)" in text


def test_public_surface():
    import inspect
    import event_utils_amd as E
    import event_utils_amd.lib.depth.sgm as alias
    from event_utils_amd import depth
    from event_utils_amd.depth import sgm
    assert alias is sgm
    for name in PUBLIC:
        assert getattr(E, name) is getattr(sgm, name) is getattr(depth, name)
    assert "(no reference module)           -> event_utils_amd.depth.sgm" in E.__doc__
    assert sgm.DIRECTIONS == G.DIRECTIONS and (sgm.MAX_COST, sgm.MAX_PENALTY) == (G.MAX_COST, G.MAX_PENALTY)
    assert sgm.Disparity is E.Disparity
    empty = inspect.Parameter.empty

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    tests = [("min_activity", 128), ("uniqueness", 10), ("max_cost", None), ("lr_tolerance", 1), ("subpixel", True)]
    assert params(E.sgm_aggregate) == [("volume", empty), ("p1", empty), ("p2", empty), ("paths", 8)]
    assert params(E.match_cost_volume) == [("volume", empty), ("activity", empty), ("min_disparity", 0)] + tests
    assert params(E.sgm_match) == [(n, empty) for n in ("QL", "QR", "max_disparity", "p1", "p2")] + \
        [("paths", 8), ("radius", 3), ("min_disparity", 0)] + tests
    assert params(E.sgm_disparity) == [(n, empty) for n in ("left", "right", "tau", "sensor_size", "t_refs", "max_disparity", "p1", "p2")] + \
        [("paths", 8), ("radius", 3), ("min_disparity", 0), ("polarity", "ignore")] + tests + [("indices", None)]


def test_arguments_are_refused_before_the_device_is_touched():
    from event_utils_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)                            # never dereferenced: every call below is refused first
    einval = -1

    def aggregate(volume=fake, nk=1, nd=16, h=48, w=96, p1=10, p2=100, directions=255, scratch=fake, out=fake):
        return L.evk_sgm_aggregate(volume, nk, nd, h, w, p1, p2, directions, scratch, out, None)

    def match(volume=fake, activity=fake, nk=1, nc=1, nd=16, h=48, w=96, d_min=0, min_activity=128, uniqueness=10, max_cost=-1, lr=1,
              subpixel=1, scratch=fake, disparity=fake, index=fake, cost=fake, mask=fake):
        return L.evk_sgm_match_volume(volume, activity, nk, nc, nd, h, w, d_min, min_activity, uniqueness, max_cost, lr, subpixel, scratch,
                                      disparity, index, cost, mask, None)

    def scratch(call=0, nk=1, nd=16, h=48, w=96):
        return L.evk_sgm_scratch_bytes(call, nk, nd, h, w)
    for f in (aggregate, match, scratch):
        assert f(nk=0) == einval and f(h=0) == einval and f(w=0) == einval and f(w=-4) == einval and f(h=1 << 16, w=1 << 15) == einval
        assert f(nk=1 << 20, h=1 << 10, w=1 << 10, nd=2) == einval              # nk nd h w past 2^40
        assert f(nk=1 << 21, h=1, w=1 << 10, nd=1) == einval                    # nk (h + w) past 2^31 - 1
        assert f(nd=0) == einval and f(nd=257) == einval and f(nd=-1) == einval
    for f in (aggregate, match):
        assert f(volume=None) == einval
    for missing in ("scratch", "out"):
        assert aggregate(**{missing: None}) == einval, missing
    assert aggregate(p1=-1) == einval and aggregate(p1=101) == einval and aggregate(p2=(1 << 20) + 1) == einval
    assert aggregate(p1=(1 << 20) + 1, p2=(1 << 20) + 2) == einval
    assert aggregate(directions=0) == einval and aggregate(directions=256) == einval and aggregate(directions=-1) == einval
    for missing in ("activity", "disparity", "index", "cost", "mask", "scratch"):
        assert match(**{missing: None}) == einval, missing
    assert match(nc=0) == einval and match(nc=3) == einval
    assert match(d_min=-1) == einval and match(d_min=(1 << 30) + 1) == einval
    assert match(min_activity=0) == einval and match(min_activity=256) == einval
    assert match(uniqueness=-1) == einval and match(uniqueness=100) == einval
    assert match(subpixel=2) == einval and match(subpixel=-1) == einval
    assert scratch(0, 3, 16, 48, 96) == 2 * 3 * 16 * 48 * 96 * 4 and scratch(1, 3, 16, 48, 96) == 3 * 48 * 96 * 4
    assert scratch(2) == einval and scratch(-1) == einval


def test_python_argument_errors_come_before_any_device_work():
    """every call below is refused on its arguments alone: none of them reaches the point where a missing GPU would matter"""
    import torch
    import event_utils_amd as E
    V = torch.zeros((1, 4, 6, 8), dtype=torch.int32)
    A = torch.zeros((1, 1, 6, 8), dtype=torch.uint8)
    for kw, match in ((dict(p1=-1, p2=5), "p1"), (dict(p1=6, p2=5), "p1 must not exceed p2"), (dict(p1=1, p2=(1 << 20) + 1), "p2"),
                      (dict(p1=1.5, p2=5), "p1"), (dict(p1=True, p2=5), "p1"), (dict(p1=1, p2=5, paths=5), "paths"),
                      (dict(p1=1, p2=5, paths=()), "paths"), (dict(p1=1, p2=5, paths=True), "paths"),
                      (dict(p1=1, p2=5, paths=((1, 0), (2, 0))), "direction"), (dict(p1=1, p2=5, paths=(3,)), "direction")):
        with pytest.raises(ValueError, match=match):
            E.sgm_aggregate(V, **kw)
        with pytest.raises(ValueError, match=match):
            E.sgm_match(A, A, 5, **kw)
    for bad in (V[0], V[None], torch.zeros((1, 257, 2, 2), dtype=torch.int32), torch.zeros((1, 0, 2, 2), dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"\(K, D, H, W\)"):
            E.sgm_aggregate(bad, 1, 5)
        with pytest.raises(ValueError, match=r"\(K, D, H, W\)"):
            E.match_cost_volume(bad, A)
    for bad in (V.to(torch.int64), V.to(torch.float32), V.numpy().astype(np.int16)):
        with pytest.raises(TypeError, match="int32"):
            E.sgm_aggregate(bad, 1, 5)
        with pytest.raises(TypeError, match="int32"):
            E.match_cost_volume(bad, A)
    with pytest.raises(TypeError, match="int32"):
        E.sgm_aggregate([[1]], 1, 5)
    for bad in (A.to(torch.int32), A.numpy().astype(np.int8)):
        with pytest.raises(TypeError, match="uint8"):
            E.match_cost_volume(V, bad)
    with pytest.raises(TypeError, match="uint8"):
        E.match_cost_volume(V, None)
    for bad in (A[0], A.expand(1, 3, 6, 8), A.expand(2, 1, 6, 8), torch.zeros((1, 1, 6, 9), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="activity must be"):
            E.match_cost_volume(V, bad)
    for kw, match in ((dict(min_disparity=-1), "min_disparity"), (dict(min_activity=0), "min_activity"), (dict(min_activity=256), "min_activity"),
                      (dict(uniqueness=100), "uniqueness"), (dict(uniqueness=9.5), "uniqueness"), (dict(max_cost=-1), "max_cost"),
                      (dict(max_cost=2.5), "max_cost"), (dict(lr_tolerance=-1), "lr_tolerance"), (dict(lr_tolerance=0.5), "lr_tolerance")):
        with pytest.raises(ValueError, match=match):
            E.match_cost_volume(V, A, **kw)
        if "min_disparity" not in kw:
            with pytest.raises(ValueError, match=match):
                E.sgm_match(A, A, 5, 1, 5, **kw)
    for kw, match in ((dict(max_disparity=256), "disparities"), (dict(max_disparity=5, radius=8), "radius"),
                      (dict(max_disparity=5, min_disparity=6), "disparities")):
        with pytest.raises(ValueError, match=match):
            E.sgm_match(A, A, p1=1, p2=5, **kw)
    with pytest.raises(TypeError, match="uint8"):
        E.sgm_match(A, A.to(torch.int32), 5, 1, 5)
    with pytest.raises(ValueError, match="one shape"):
        E.sgm_match(A, torch.zeros((1, 1, 6, 9), dtype=torch.uint8), 5, 1, 5)
    cols = (np.array([1, 2]), np.array([1, 2]), np.array([0.0, 0.1]), np.array([1, -1]))
    with pytest.raises(TypeError, match="indices"):
        E.sgm_disparity(cols, cols, 0.01, (6, 8), [0.2], 5, 1, 5, indices=[1, 2])
    with pytest.raises(TypeError, match="t_refs"):
        E.sgm_disparity(cols, cols, 0.01, (6, 8), None, 5, 1, 5)
    with pytest.raises(TypeError, match="left"):
        E.sgm_disparity(cols[:3], cols, 0.01, (6, 8), [0.2], 5, 1, 5)
    with pytest.raises(TypeError, match="right"):
        E.sgm_disparity(cols, None, 0.01, (6, 8), [0.2], 5, 1, 5)
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tau"):
            E.sgm_disparity(cols, cols, tau, (6, 8), [0.2], 5, 1, 5)
    with pytest.raises(ValueError, match="polarity"):
        E.sgm_disparity(cols, cols, 0.01, (6, 8), [0.2], 5, 1, 5, polarity="both")
    for kw, match in ((dict(max_disparity=256, p1=1, p2=5), "disparities"), (dict(max_disparity=5, p1=6, p2=5), "p1"),
                      (dict(max_disparity=5, p1=1, p2=5, paths=3), "paths"), (dict(max_disparity=5, p1=1, p2=5, max_cost=-2), "max_cost"),
                      (dict(max_disparity=5, p1=1, p2=5, uniqueness=100), "uniqueness")):
        with pytest.raises(ValueError, match=match):
            E.sgm_disparity(cols, cols, 0.01, (6, 8), [0.2], **kw)


def test_the_kernels_compile_without_register_spills(tmp_path):
    """every kernel of evk_sgm.hip compiles for gfx950 without spilling registers and without scratch memory; the transposes hold
    the 16 640 bytes of LDS that DESIGN.md states, and the path kernels none; the cross-lane traffic of a path is DPP"""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    from event_utils_amd.csrc import build as B
    src = os.path.join(B.HERE, "evk_sgm.hip")
    subprocess.run([hipcc] + list(B.CFLAGS) + ["-c", src, "-o", str(tmp_path / "sgm.o"), "-save-temps=obj"], check=True, cwd=B.HERE,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert asm, os.listdir(tmp_path)
    text = open(tmp_path / asm[0]).read()
    kernels = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    seen = {n: (int(p), int(v), int(sp), int(lds)) for lds, n, p, v, sp in kernels}
    for name, count in (("k_sgm_transpose", 2), ("k_sgm_path", 10), ("k_sgm_winner", 1), ("k_sgm_right", 1), ("k_disparity_lr", 1)):
        assert sum(name in n for n in seen) == count, (name, sorted(seen))
    assert not {n: v for n, v in seen.items() if v[0] or v[2]}                   # no scratch, no spills
    assert all(v <= 128 for n, (_, v, _, _) in seen.items())                     # four waves per SIMD at least
    assert all(lds == (16640 if "k_sgm_transpose" in n else 0) for n, (_, _, _, lds) in seen.items())
    assert "wave_ror:1" in text and "wave_rol:1" in text and "row_mirror" in text and "row_bcast:31" in text
