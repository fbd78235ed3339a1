"""CPU (no GPU): the host restatement of event stereo (tests/_stereo_np.py, the literal definition) on hand-worked cases; the
restatement finds the two planes of the seeded scene; the evk_stereo_* entry points are declared, bound and exported and refuse bad
arguments before they touch the device; the Python argument errors; the public surface; the kernels of evk_stereo.hip compile for
gfx950 without register spills."""
import ctypes
import os
import re

import numpy as np
import pytest

import _header
import _stereo_np as N

ENTRIES = {"evk_stereo_quantise", "evk_stereo_cost_volume", "evk_stereo_match"}
PUBLIC = ("Disparity", "quantised_time_surfaces", "stereo_cost_volume", "stereo_match", "stereo_disparity", "disparity_to_depth",
          "disparity_depth_map")


def surfaces(rows_l, rows_r):
    """(1, 1, H, W) uint8 surfaces from lists of rows"""
    return np.array(rows_l, dtype=np.uint8)[None, None], np.array(rows_r, dtype=np.uint8)[None, None]


def from_volume(costs, **kw):
    """match on a hand-written (D, W) cost table of a one-row image whose every pixel is a candidate"""
    vol = np.asarray(costs, dtype=np.int64)[None, :, None, :]
    D, W = vol.shape[1], vol.shape[3]
    Q = np.full((1, 1, 1, W), 255, dtype=np.uint8)
    args = dict(uniqueness=0, lr_tolerance=None, subpixel=False)
    args.update(kw)
    return N.match(Q, Q, 0, D, 1, volume=vol, **args)


# ---- hand-worked cases of the restatement --------------------------------------------------------------------------------------------

def test_quantisation_at_its_edges():
    tau = 0.01
    a = np.array([0.0, tau / 256, 2 * tau / 256, tau / 2, tau, 2 * tau, np.inf, -1.0, np.nan, np.nextafter(tau, 0.0)])
    # v = 1, 255/256, 254/256, 1/2, 0, -1, -inf, 101, NaN, one ulp above 0
    assert N.quantise(a, tau).tolist() == [255, 255, 254, 128, 0, 0, 0, 255, 0, 0]
    assert N.quantise(a, tau).dtype == np.uint8
    assert N.quantise(np.array([0.75]), 1.0).tolist() == [64] and N.quantise(np.array([0.7501]), 1.0).tolist() == [63]


def test_ages_take_the_last_event_before_the_query():
    xs, ys, ts, ps = np.array([1, 1, 2, 1]), np.array([0, 0, 0, 0]), np.array([0.0, 1.0, 2.0, 3.0]), np.array([1, -1, 1, 1])
    a = N.ages(xs, ys, ts, ps, (1, 3), [2.0, 3.5])
    assert a.shape == (2, 1, 1, 3) and a[0, 0, 0].tolist() == [np.inf, 1.0, np.inf]         # t < T: the event at 2.0 is not before 2.0
    assert a[1, 0, 0].tolist() == [np.inf, 0.5, 1.5]
    s = N.ages(xs, ys, ts, ps, (1, 3), [3.5], "split")
    assert s[0, 0, 0].tolist() == [np.inf, 2.5, np.inf] and s[0, 1, 0].tolist() == [np.inf, 0.5, 1.5]


def test_a_right_surface_shifted_by_three_costs_nothing_at_three():
    left = [[0, 10, 250, 30, 77, 200, 5, 160, 90, 255, 40, 130]]
    right = [left[0][3:] + [0, 0, 0]]                       # QR[x - 3] = QL[x]
    QL, QR = surfaces(left, right)
    vol = N.cost_volume(QL, QR, 0, 6, 1)
    assert vol.shape == (1, 6, 1, 12) and vol.dtype == np.int64
    assert (vol[0, 3, 0, 4:] == 0).all()                    # from x = 4 on the whole window has its partner
    assert vol[0, 3, 0, 3] == 250                           # x = 3: QL[2] = 250 meets the right column -1, off the sensor
    disp, idx, cost, valid, cand = N.match(QL, QR, 0, 6, 1, min_activity=1, uniqueness=0, lr_tolerance=None, subpixel=False)
    assert idx[0, 0, 4:].tolist() == [3] * 8 and cost[0, 0, 4:].tolist() == [0] * 8 and valid[0, 0, 4:].all()
    assert disp.dtype == np.float32 and idx.dtype == np.int32 and cost.dtype == np.int32 and valid.dtype == bool


def test_the_cost_of_one_window_by_hand():
    QL, QR = surfaces([[10, 20, 30, 40], [1, 2, 3, 4]], [[40, 30, 20, 10], [9, 9, 9, 9]])
    vol = N.cost_volume(QL, QR, 1, 2, 1)                    # d = 1, 2
    # (x, y) = (2, 0), d = 1: rows y = -1 (all zero), 0, 1; left columns 1 .. 3, right columns 0 .. 2
    assert vol[0, 0, 0, 2] == (abs(20 - 40) + abs(30 - 30) + abs(40 - 20)) + (abs(2 - 9) + abs(3 - 9) + abs(4 - 9))
    # (3, 1), d = 2: left columns 2 .. 4 (4 is off the sensor: 0), right columns 0 .. 2
    assert vol[0, 1, 1, 3] == (abs(30 - 40) + abs(40 - 30) + abs(0 - 20)) + (abs(3 - 9) + abs(4 - 9) + abs(0 - 9))
    # (1, 0), d = 1: right column -1 is off the sensor
    assert vol[0, 0, 0, 1] == (abs(10 - 0) + abs(20 - 40) + abs(30 - 30)) + (abs(1 - 0) + abs(2 - 9) + abs(3 - 9))
    assert vol[0, 0, :, 0].tolist() == [-1, -1] and vol[0, 1, :, :2].tolist() == [[-1, -1], [-1, -1]]
    two = N.cost_volume(np.concatenate((QL, QL), axis=1), np.concatenate((QR, QR), axis=1), 1, 2, 1)
    assert np.array_equal(two, np.where(vol >= 0, 2 * vol, -1))                              # channels add


def test_a_tie_goes_to_the_smaller_disparity():
    Q = np.full((1, 1, 3, 20), 200, dtype=np.uint8)
    disp, idx, cost, valid, _ = N.match(Q, Q, 2, 5, 1, lr_tolerance=None)
    assert idx[0, 1, 10] == 2 and cost[0, 1, 10] == 0 and valid[0, 1, 10] and disp[0, 1, 10] == 2.0       # all five cost nothing
    _, idx, cost, valid, _ = from_volume([[7] * 6, [3] * 6, [3] * 6, [9] * 6])
    assert idx[0, 0, 5] == 1 and cost[0, 0, 5] == 3


def test_a_disparity_beyond_x_is_not_admissible():
    rng = np.random.default_rng(0)
    QL, QR = rng.integers(0, 256, (2, 1, 1, 4, 9)).astype(np.uint8)
    vol = N.cost_volume(QL, QR, 2, 8, 1)                    # d = 2 .. 9: nothing is admissible at x < 2, d = 9 nowhere
    for i in range(8):
        assert (vol[0, i, :, :min(2 + i, 9)] == -1).all() and (vol[0, i, :, 2 + i:] >= 0).all()
    disp, idx, cost, valid, cand = N.match(QL, QR, 2, 8, 1, min_activity=1, uniqueness=0, lr_tolerance=None)
    assert not cand[0, :, :2].any() and (cost[0, :, :2] == -1).all() and (idx[0, :, :2] == -1).all() and np.isnan(disp[0, :, :2]).all()
    assert (idx[0, :, 2] == 2).all() and (idx[0, :, 3] <= 3).all()                           # only d <= x competes


def test_the_uniqueness_boundary():
    table = lambda c2: [[500] * 5 + [90], [500] * 5 + [95], [500] * 5 + [200], [500] * 5 + [c2]]
    _, idx, cost, valid, _ = from_volume(table(100), uniqueness=10)             # c2 (100 - u) == 100 c1: passes
    assert valid[0, 0, 5] and idx[0, 0, 5] == 0 and cost[0, 0, 5] == 90
    disp, idx, cost, valid, _ = from_volume(table(99), uniqueness=10)
    assert not valid[0, 0, 5] and idx[0, 0, 5] == -1 and cost[0, 0, 5] == 90 and np.isnan(disp[0, 0, 5])
    assert from_volume(table(99), uniqueness=0)[3][0, 0, 5]                     # switched off
    # the neighbour of the winner is no rival: 95 at d* + 1 is skipped, and with two disparities there is no c2 at all
    assert from_volume([[500] * 5 + [90], [500] * 5 + [91]], uniqueness=99)[3][0, 0, 5]


def test_the_max_cost_test():
    Q = np.full((1, 2, 1, 6), 255, dtype=np.uint8)
    vol = np.full((1, 1, 1, 6), 36, dtype=np.int64)
    for limit, passes in ((2.0, True), (1.99, False)):      # floor(limit C (2 r + 1)^2), C = 2, r = 1: 36 and 35
        valid = N.match(Q, Q, 0, 1, 1, uniqueness=0, lr_tolerance=None, max_mean_cost=limit, volume=vol)[3]
        assert bool(valid.all()) == passes and bool(valid.any()) == passes


def test_the_left_right_test_rejects_an_occluded_pixel():
    costs = np.full((3, 6), 50, dtype=np.int64)
    costs[1, :1], costs[2, :2] = -1, -1                     # d > x
    costs[0, 3] = 5                                        # the left pixel 3 claims the right pixel 3 with d = 0 ...
    costs[2, 5] = 1                                         # ... which the left pixel 5 claims with d = 2 at a lower cost
    disp, idx, cost, valid, _ = from_volume(costs, lr_tolerance=1)
    assert idx[0, 0, 5] == 2 and valid[0, 0, 5]
    assert not valid[0, 0, 3] and idx[0, 0, 3] == -1 and cost[0, 0, 3] == 5 and np.isnan(disp[0, 0, 3])
    assert from_volume(costs, lr_tolerance=2)[3][0, 0, 3] and from_volume(costs, lr_tolerance=None)[3][0, 0, 3]


def test_the_parabola():
    table = [[9] * 4 + [4], [9] * 4 + [2], [9] * 4 + [6]]   # cm = 4, c1 = 2, cp = 6: den = 6, offset (4 - 6) / 12
    disp, idx, _, _, _ = from_volume(table, subpixel=True)
    assert idx[0, 0, 4] == 1 and disp[0, 0, 4] == np.float32(1.0 - 1.0 / 6.0) and disp.dtype == np.float32
    assert from_volume(table, subpixel=False)[0][0, 0, 4] == 1.0
    # a winner at the end of the range, or next to a disparity that is not admissible, stays whole
    assert from_volume([[9] * 4 + [1], [9] * 4 + [2], [9] * 4 + [6]], subpixel=True)[0][0, 0, 4] == 0.0
    assert from_volume([[9, 9], [-1, 2], [-1, -1]], subpixel=True)[0][0, 0, 1] == 1.0


def test_a_flat_cost_has_no_parabola():
    """den = cm - 2 c1 + cp is 0 only where cm == c1 == cp, and then the tie rule makes d* - 1 the winner: with cm > c1 (the
    smaller d wins ties) and cp >= c1 a winner inside the range always has den > 0.  The flat table takes the plain winner."""
    disp, idx, _, _, _ = from_volume([[2] * 5, [2] * 5, [2] * 5], subpixel=True)
    assert idx[0, 0, 4] == 0 and disp[0, 0, 4] == 0.0
    disp, idx, _, _, _ = from_volume([[3] * 5, [2] * 5, [2] * 5], subpixel=True)           # den = 3 - 4 + 2 = 1, offset 1 / 2
    assert idx[0, 0, 4] == 1 and disp[0, 0, 4] == 1.5


def test_disparity_to_depth_at_zero_and_nan():
    import event_utils_amd as E
    d = np.array([[4.0, 0.0, np.nan, -2.0, 0.5]], dtype=np.float32)
    for f in (N.disparity_to_depth, E.disparity_to_depth):
        z = f(d, 200.0, 0.1)
        assert z.dtype == np.float64 and z[0, 0] == 5.0 and z[0, 4] == 40.0 and np.isnan(z[0, 1:4]).all()
    import torch
    z = E.disparity_to_depth(torch.from_numpy(d), 200.0, 0.1)
    assert z.dtype == torch.float64 and np.array_equal(z.numpy(), N.disparity_to_depth(d, 200.0, 0.1), equal_nan=True)
    dm = E.disparity_depth_map(E.Disparity(torch.from_numpy(d)[None], torch.tensor([[[4, -1, -1, -1, 0]]], dtype=torch.int32),
                                           torch.tensor([[[7, -1, 3, 3, 9]]], dtype=torch.int32),
                                           torch.tensor([[[True, False, False, False, True]]])), 0, 200.0, 0.1)
    assert isinstance(dm, E.DepthMap) and dm.confidence.dtype == torch.float32 and dm.confidence.tolist() == [[-7.0, 1.0, -3.0, -3.0, -9.0]]
    assert dm.mask.tolist() == [[True, False, False, False, True]] and dm.depth[0, 0] == 5.0 and dm.index.tolist() == [[4, -1, -1, -1, 0]]


# ---- the seeded scene ------------------------------------------------------------------------------------------------------------

def scene_fractions(sc, match):
    """(eligible dots, valid ones, the fraction of the valid ones within one disparity of the truth) of match(**tests) results"""
    H, W = N.SCENE_SIZE
    px, d = sc["pixels"], sc["true_disparity"]
    disp, idx, cost, valid, cand = match
    inside = (px[:, 0] >= 0) & (px[:, 0] < W) & (px[:, 1] >= 0) & (px[:, 1] < H)
    el = inside.copy()
    el[inside] &= cand[0, px[inside, 1], px[inside, 0]]
    v = valid[0, px[el, 1], px[el, 0]]
    good = np.abs(idx[0, px[el, 1], px[el, 0]] - d[el]) <= 1
    return int(el.sum()), int(v.sum()), float((good & v).sum()) / max(int(v.sum()), 1)


def test_the_restatement_finds_the_two_planes_of_the_seeded_scene():
    """56 dots on the planes d = 4 and d = 9, 1 372 left and 1 351 right events, tau 10 ms, r = 3, D = 16, min_activity 128.  Of the
    39 dots whose last left pixel is a candidate, measured with this restatement: 0.744 have d* within 1 of the truth before any
    test; 0.771 of the 35 that pass uniqueness = 10; 0.857 of the 28 that pass uniqueness = 10 and lr_tolerance = 1.  The floors
    lie 0.05 below: one dot in twenty is the grain of such a scene."""
    sc = N.scene()
    assert (len(sc["left"]["ts"]), len(sc["right"]["ts"])) == (1372, 1351)
    QL = N.quantise(N.ages(*N.stream(sc["left"]), N.SCENE_SIZE, [N.SCENE_END]), N.SCENE_TAU)
    QR = N.quantise(N.ages(*N.stream(sc["right"]), N.SCENE_SIZE, [N.SCENE_END]), N.SCENE_TAU)
    vol = N.cost_volume(QL, QR, 0, N.SCENE_D, N.SCENE_R)
    run = lambda **kw: scene_fractions(sc, N.match(QL, QR, 0, N.SCENE_D, N.SCENE_R, N.SCENE_ACTIVITY, volume=vol, **kw))
    eligible, kept0, before = run(uniqueness=0, lr_tolerance=None)
    _, kept1, unique = run(uniqueness=10, lr_tolerance=None)
    _, kept2, after = run(uniqueness=10, lr_tolerance=1)
    print("eligible %d; before %.3f; uniqueness %.3f of %d; all tests %.3f of %d" % (eligible, before, unique, kept1, after, kept2))
    assert eligible == kept0 >= 30
    assert before >= 0.744 - 0.05 and unique >= 0.771 - 0.05 and after >= 0.857 - 0.05
    assert 2 * kept1 >= eligible and 2 * kept2 >= eligible


# ---- the public surface and the C ABI ------------------------------------------------------------------------------------------------

def test_the_prototypes_are_bound_with_their_arguments():
    from event_utils_amd import _lib
    text = _header.TEXT
    protos = _header.prototypes("evk_stereo_")
    assert set(protos) == ENTRIES | {"evk_stereo_scratch_bytes"}
    for name, (want, ret) in protos.items():
        assert ret is (ctypes.c_int if name in ENTRIES else ctypes.c_int64), name
        assert _lib.PROTOTYPES[name] == (want, ret), name
        assert hasattr(_lib.lib(), name)
    assert (_lib.EVK_STEREO_MAX_DISPARITIES, _lib.EVK_STEREO_MAX_RADIUS) == (256, 7)
    for name, value in (("EVK_STEREO_MAX_DISPARITIES", 256), ("EVK_STEREO_MAX_RADIUS", 7)):
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (name, value), text, re.M)
    assert "Event stereo (evk_stereo.hip)" in text


def test_public_surface():
    import inspect
    import event_utils_amd as E
    import event_utils_amd.lib.depth.stereo as alias
    from event_utils_amd import depth
    from event_utils_amd.depth import stereo
    assert alias is stereo
    for name in PUBLIC:
        assert getattr(E, name) is getattr(stereo, name) is getattr(depth, name)
    assert "(no reference module)           -> event_utils_amd.depth.stereo" in E.__doc__
    assert E.Disparity._fields == ("disparity", "index", "cost", "mask")
    empty = inspect.Parameter.empty

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    assert params(E.quantised_time_surfaces) == [(n, empty) for n in ("xs", "ys", "ts", "ps", "tau", "sensor_size", "t_refs")] + \
        [("polarity", "ignore")]
    assert params(E.stereo_cost_volume) == [("QL", empty), ("QR", empty), ("max_disparity", empty), ("radius", 3), ("min_disparity", 0)]
    tests = [("min_activity", 128), ("uniqueness", 10), ("max_mean_cost", None), ("lr_tolerance", 1), ("subpixel", True)]
    assert params(E.stereo_match) == params(E.stereo_cost_volume) + tests
    assert params(E.stereo_disparity) == [(n, empty) for n in ("left", "right", "tau", "sensor_size", "t_refs", "max_disparity")] + \
        [("radius", 3), ("min_disparity", 0), ("polarity", "ignore")] + tests + [("indices", None)]
    assert params(E.disparity_to_depth) == [(n, empty) for n in ("disparity", "fx", "baseline")]
    assert params(E.disparity_depth_map) == [(n, empty) for n in ("disp", "k", "fx", "baseline")]


def test_arguments_are_refused_before_the_device_is_touched():
    from event_utils_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)                            # never dereferenced: every call below is refused first
    einval, nan, inf = -1, float("nan"), float("inf")

    def quantise(ages=fake, n=100, tau=0.01, q=fake):
        return L.evk_stereo_quantise(ages, n, tau, q, None)
    assert quantise(ages=None) == einval and quantise(q=None) == einval and quantise(n=-1) == einval
    for bad in (0.0, -1.0, nan, inf):
        assert quantise(tau=bad) == einval
    assert quantise(n=0, ages=None, q=None) == 0            # nothing to do

    def volume(ql=fake, qr=fake, nk=1, nc=1, h=48, w=96, d_min=0, nd=16, radius=3, out=fake):
        return L.evk_stereo_cost_volume(ql, qr, nk, nc, h, w, d_min, nd, radius, out, None)

    def match(ql=fake, qr=fake, nk=1, nc=1, h=48, w=96, d_min=0, nd=16, radius=3, activity=128, uniqueness=10, max_cost=-1, lr=1, subpixel=1,
              scratch=fake, disparity=fake, index=fake, cost=fake, mask=fake):
        return L.evk_stereo_match(ql, qr, nk, nc, h, w, d_min, nd, radius, activity, uniqueness, max_cost, lr, subpixel, scratch, disparity,
                                  index, cost, mask, None)
    for f in (volume, match):
        assert f(ql=None) == einval and f(qr=None) == einval
        assert f(nk=0) == einval and f(nc=0) == einval and f(nc=3) == einval
        assert f(h=0) == einval and f(w=0) == einval and f(w=-4) == einval and f(h=1 << 16, w=1 << 15) == einval
        assert f(nk=1 << 20, h=1 << 10, w=1 << 10, nd=2) == einval              # nk nd h w past 2^40
        assert f(nd=0) == einval and f(nd=257) == einval and f(nd=-1) == einval
        assert f(d_min=-1) == einval and f(d_min=(1 << 30) + 1) == einval
        assert f(radius=0) == einval and f(radius=8) == einval and f(radius=-2) == einval
    assert volume(out=None) == einval
    for missing in ("disparity", "index", "cost", "mask", "scratch"):
        assert match(**{missing: None}) == einval, missing
    assert match(activity=0) == einval and match(activity=256) == einval
    assert match(uniqueness=-1) == einval and match(uniqueness=100) == einval
    assert match(subpixel=2) == einval and match(subpixel=-1) == einval
    assert L.evk_stereo_scratch_bytes(3, 48, 96, 1) == 3 * 48 * 96 * 4 and L.evk_stereo_scratch_bytes(3, 48, 96, 0) == 3 * 48 * 96 * 4
    assert L.evk_stereo_scratch_bytes(3, 48, 96, -1) == 0
    assert L.evk_stereo_scratch_bytes(0, 48, 96, 1) == einval and L.evk_stereo_scratch_bytes(1, 0, 96, 1) == einval
    assert L.evk_stereo_scratch_bytes(1, 1 << 16, 1 << 15, 1) == einval


def test_python_argument_errors_come_before_any_device_work():
    """every call below is refused on its arguments alone: none of them reaches the point where a missing GPU would matter"""
    import torch
    import event_utils_amd as E
    Q = torch.zeros((1, 1, 6, 8), dtype=torch.uint8)
    for f in (E.stereo_cost_volume, E.stereo_match):
        for kw, match in ((dict(max_disparity=256), "disparities"), (dict(max_disparity=-1), "disparities"),
                          (dict(max_disparity=5, min_disparity=6), "disparities"), (dict(max_disparity=300, min_disparity=44), "disparities"),
                          (dict(max_disparity=2.5), "max_disparity"), (dict(max_disparity=5, min_disparity=-1), "min_disparity"),
                          (dict(max_disparity=5, radius=0), "radius"), (dict(max_disparity=5, radius=8), "radius"),
                          (dict(max_disparity=5, radius=1.5), "radius")):
            with pytest.raises(ValueError, match=match):
                f(Q, Q, **kw)
        with pytest.raises(ValueError, match="one shape"):
            f(Q, torch.zeros((1, 1, 6, 9), dtype=torch.uint8), 5)
        with pytest.raises(ValueError, match=r"\(K, C, H, W\)"):
            f(Q[0], Q[0], 5)
        with pytest.raises(ValueError, match=r"\(K, C, H, W\)"):
            f(Q.expand(1, 3, 6, 8), Q.expand(1, 3, 6, 8), 5)
        for other in (Q.to(torch.int32), Q.to(torch.float32), Q.numpy().astype(np.int8)):
            with pytest.raises(TypeError, match="uint8"):
                f(Q, other, 5)
            with pytest.raises(TypeError, match="uint8"):
                f(other, Q, 5)
        with pytest.raises(TypeError, match="uint8"):
            f([[1]], Q, 5)
    for kw, match in ((dict(min_activity=0), "min_activity"), (dict(min_activity=256), "min_activity"), (dict(uniqueness=100), "uniqueness"),
                      (dict(uniqueness=-1), "uniqueness"), (dict(uniqueness=9.5), "uniqueness"), (dict(max_mean_cost=-1.0), "max_mean_cost"),
                      (dict(max_mean_cost=float("nan")), "max_mean_cost"), (dict(lr_tolerance=-1), "lr_tolerance"),
                      (dict(lr_tolerance=0.5), "lr_tolerance")):
        with pytest.raises(ValueError, match=match):
            E.stereo_match(Q, Q, 5, **kw)
    cols = (np.array([1, 2]), np.array([1, 2]), np.array([0.0, 0.1]), np.array([1, -1]))
    with pytest.raises(TypeError, match="indices"):
        E.stereo_disparity(cols, cols, 0.01, (6, 8), None, 5, indices=[1, 2])
    with pytest.raises(TypeError, match="indices"):
        E.stereo_disparity(cols, cols, 0.01, (6, 8), [0.2], 5, indices=[1, 2])
    with pytest.raises(TypeError, match="t_refs"):
        E.stereo_disparity(cols, cols, 0.01, (6, 8), None, 5)
    with pytest.raises(TypeError):
        E.quantised_time_surfaces(*cols, 0.01, (6, 8), [0.2], indices=[1])
    with pytest.raises(TypeError, match="t_refs"):
        E.quantised_time_surfaces(*cols, 0.01, (6, 8), None)
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tau"):
            E.quantised_time_surfaces(*cols, tau, (6, 8), [0.2])
        with pytest.raises(ValueError, match="tau"):
            E.stereo_disparity(cols, cols, tau, (6, 8), [0.2], 5)
    for polarity in ("same", "both", None):
        with pytest.raises(ValueError, match="polarity"):
            E.quantised_time_surfaces(*cols, 0.01, (6, 8), [0.2], polarity=polarity)
        with pytest.raises(ValueError, match="polarity"):
            E.stereo_disparity(cols, cols, 0.01, (6, 8), [0.2], 5, polarity=polarity)
    with pytest.raises(TypeError, match="left"):
        E.stereo_disparity(cols[:3], cols, 0.01, (6, 8), [0.2], 5)
    with pytest.raises(TypeError, match="right"):
        E.stereo_disparity(cols, None, 0.01, (6, 8), [0.2], 5)
    for kw, match in ((dict(max_disparity=256), "disparities"), (dict(max_disparity=5, radius=9), "radius"),
                      (dict(max_disparity=5, uniqueness=100), "uniqueness"), (dict(max_disparity=5, min_activity=0), "min_activity")):
        with pytest.raises(ValueError, match=match):
            E.stereo_disparity(cols, cols, 0.01, (6, 8), [0.2], **kw)
    for fx, b in ((0.0, 0.1), (200.0, -0.1), (float("nan"), 0.1), (200.0, float("inf"))):
        with pytest.raises(ValueError, match="fx and baseline"):
            E.disparity_to_depth(np.ones(3), fx, b)
    disp = E.Disparity(torch.ones((2, 3, 4)), torch.ones((2, 3, 4), dtype=torch.int32), torch.ones((2, 3, 4), dtype=torch.int32),
                       torch.ones((2, 3, 4), dtype=torch.bool))
    for k in (2, -1, 0.5):
        with pytest.raises(IndexError, match="k must be"):
            E.disparity_depth_map(disp, k, 200.0, 0.1)
    with pytest.raises(ValueError, match="Disparity"):
        E.disparity_depth_map(disp[:3], 0, 200.0, 0.1)


def test_the_kernels_compile_without_register_spills(tmp_path):
    """every kernel of evk_stereo.hip compiles for gfx950 without spilling registers and without scratch memory"""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    from event_utils_amd.csrc import build as B
    src = os.path.join(B.HERE, "evk_stereo.hip")
    subprocess.run([hipcc] + list(B.CFLAGS) + ["-c", src, "-o", str(tmp_path / "stereo.o"), "-save-temps=obj"], check=True, cwd=B.HERE,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert asm, os.listdir(tmp_path)
    text = open(tmp_path / asm[0]).read()
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n"
                         r"\s+\.vgpr_spill_count:\s+(\d+)", text)
    seen = {n: (int(p), int(v), int(sp)) for n, p, v, sp in kernels}
    for name, count in (("k_stereo_quantise", 1), ("k_stereo_scan", 12), ("k_disparity_lr", 1)):        # 4 window widths x 3 modes
        assert sum(name in n for n in seen) == count, (name, sorted(seen))
    assert not {n: v for n, v in seen.items() if v[0] or v[2]}                   # no scratch, no spills
    assert all(v <= 128 for n, (_, v, _) in seen.items())                        # four waves per SIMD at least
    assert text.count("v_sad_u8") >= 12 and "v_alignbyte_b32" in text           # the packed byte instructions are what runs
