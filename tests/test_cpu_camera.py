"""CPU (no GPU): the host restatement of camera calibration (tests/_camera_np.py, the literal definition) on hand-worked values, its
round trip, a divergent corner, the composition of both maps, the rounding rules of the event look-up and the image remap; Bouguet's
stereo_rectify (the product's host code and the restatement's) on random points; the equidistant restatement against itself in
np.longdouble; the seeded raw stereo scene; the evk_camera_* entry points are declared, bound and exported and refuse bad arguments
before they touch the device; the Python argument errors; the public surface; the kernels of evk_camera.hip compile for gfx950
without scratch memory."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _camera_np as N
import _header
import _stereo_np as S

ENTRIES = {"evk_camera_points", "evk_camera_rectify_lookup", "evk_camera_remap"}
PUBLIC = ("CameraModel", "RectificationMaps", "distort_points", "undistort_points", "rectification_maps", "rectify_events", "remap_images",
          "stereo_rectify")
K0 = np.array([[50.0, 0.0, 20.0], [0.0, 40.0, 10.0], [0.0, 0.0, 1.0]])


def rot(axis, degrees):
    om = np.zeros(3)
    om[axis] = np.radians(degrees)
    return N.rodrigues(om)


# ---- hand-worked values ------------------------------------------------------------------------------------------------------------

def test_radtan_by_hand():
    full = N.coefficients("radtan", (0.3, -0.2, 0.01, 0.02, 0.05))
    a, b = N.distort(0.0, 0.0, "radtan", full)
    assert (a, b) == (0.0, 0.0)
    # on an axis, k1 only: r2 = .25, rad = 1 + .25 (.25) = 1.0625
    a, b = N.distort(0.5, 0.0, "radtan", N.coefficients("radtan", (0.25, 0.0, 0.0, 0.0)))
    assert (a, b) == (0.53125, 0.0)
    # p1 only: ab = .125, r2 = .3125; dx = (2 .125) .125, dy = .125 (.3125 + 2 .0625)
    a, b = N.distort(0.5, 0.25, "radtan", N.coefficients("radtan", (0.0, 0.0, 0.125, 0.0)))
    assert (a, b) == (0.5 + 0.03125, 0.25 + 0.0546875)
    # k3 is the fifth coefficient, and four coefficients mean k3 = 0: r2 = .25, rad = 1 + .25 (.25 (.25 k3))
    assert N.distort(0.5, 0.0, "radtan", N.coefficients("radtan", (0.0, 0.0, 0.0, 0.0, 64.0)))[0] == 0.5 * 2.0
    assert N.coefficients("radtan", (1.0, 2.0, 3.0, 4.0)).tolist() == [1.0, 2.0, 3.0, 4.0, 0.0]


def test_equidistant_by_hand():
    d = N.coefficients("equidistant", (1e15, 0.0, 0.0, 0.0))
    assert [float(v) for v in N.distort(0.0, 0.0, "equidistant", d)] == [0.0, 0.0]
    # just below the switch the scale is 1 whatever the coefficients say; just above it is thd / r
    a, b = N.distort(0.6e-8, 0.7e-8, "equidistant", d)       # r = 0.92e-8
    assert (a, b) == (0.6e-8, 0.7e-8)
    r = 1.1e-8
    th = math.atan(r)
    s = (th * (1.0 + (th * th) * (1e15 + (th * th) * 0.0))) / r
    assert 1.12 < s < 1.13                                  # th2 k1 = 0.121: the other branch
    assert float(N.distort(r, 0.0, "equidistant", d)[0]) == r * s
    # no coefficients: the pure fisheye, r' = atan(r)
    a, b = N.distort(3.0, 4.0, "equidistant", N.coefficients("equidistant", (0.0, 0.0, 0.0, 0.0)))
    assert abs(float(np.hypot(a, b)) - math.atan(5.0)) < 1e-15 and abs(a / b - 0.75) < 1e-15


def test_zero_coefficients_are_the_identity_bit_for_bit():
    rng = np.random.default_rng(0)
    a, b = rng.uniform(-2, 2, 500), rng.uniform(-2, 2, 500)
    for model, d in (("none", N.coefficients("none", None)), ("radtan", N.coefficients("radtan", (0.0, 0.0, 0.0, 0.0, 0.0)))):
        ad, bd = N.distort(a, b, model, d)
        assert np.array_equal(ad.view(np.uint64), a.view(np.uint64)) and np.array_equal(bd.view(np.uint64), b.view(np.uint64))
        au, bu, ok = N.undistort(a, b, model, d, 100.0, 100.0)
        assert ok.all() and np.array_equal(au.view(np.uint64), a.view(np.uint64)) and np.array_equal(bu.view(np.uint64), b.view(np.uint64))
    x, y = N.grid((5, 7))
    u, v, ok = N.forward_points(x, y, K0, "none", N.coefficients("none", None))
    assert ok.all() and np.abs(u - x).max() < 1e-13 and np.abs(v - y).max() < 1e-13


# ---- round trip, divergence, maps ------------------------------------------------------------------------------------------------------

CASES = (("radtan", (-0.25, 0.08, 0.0012, -0.0008)), ("radtan", (0.1, -0.02, 0.001, 0.002, 0.004)), ("equidistant", (-0.06, 0.015, -0.006, 0.0015)),
         ("none", None))


@pytest.mark.parametrize("model,dist", CASES)
def test_round_trip(model, dist):
    d = N.coefficients(model, dist)
    fx, fy, cx, cy = N.intrinsics(K0)
    x, y = N.grid((21, 41))
    ad, bd = (x - cx) / fx, (y - cy) / fy
    for tol in (1e-6, 1e-9):
        a, b, ok = N.undistort(ad, bd, model, d, fx, fy, 20, tol)
        assert ok.all()
        ar, br = N.distort(a, b, model, d)
        assert np.abs(fx * (ar - ad)).max() <= tol and np.abs(fy * (br - bd)).max() <= tol
    # too few steps do not pass silently either
    if model == "radtan":
        a, b, ok = N.undistort(ad, bd, model, d, fx, fy, 1, 1e-9)
        assert not ok.all() and np.isnan(a[~ok]).all() and np.isfinite(a[ok]).all()


def test_a_divergent_corner_is_invalid_and_nan():
    c = N.DIVERGENT
    d = N.coefficients(c["model"], c["distortion"])
    H, W = c["sensor_size"]
    fwd, fv, inv, iv = N.maps(c["K"], c["model"], d, c["sensor_size"])
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        assert not fv[y, x] and np.isnan(fwd[:, y, x]).all()
    assert fv[H // 2 - 3:H // 2 + 3, W // 2 - 3:W // 2 + 3].all() and 0.3 < fv.mean() < 0.9
    assert np.isnan(fwd[:, ~fv]).all() and np.isfinite(fwd[:, fv]).all()
    # where it is valid it is right: distorting again gives the pixel back
    x, y, ok = N.inverse_points(fwd[0][fv], fwd[1][fv], c["K"], c["model"], d)
    gx, gy = (g.reshape(H, W)[fv] for g in N.grid((H, W)))
    assert ok.all() and np.abs(x - gx).max() <= 2e-6 and np.abs(y - gy).max() <= 2e-6


@pytest.mark.parametrize("model,dist", CASES)
def test_the_maps_compose_to_the_identity(model, dist):
    d = N.coefficients(model, dist)
    R = N.rodrigues([0.02, -0.03, 0.01])
    new_K = np.array([[45.0, 0.0, 24.0], [0.0, 45.0, 13.0], [0.0, 0.0, 1.0]])
    size, out = (21, 41), (26, 48)
    fwd, fv, inv, iv = N.maps(K0, model, d, size, R, new_K, out)
    assert fwd.shape == (2, 21, 41) and inv.shape == (2, 26, 48) and fv.all() and iv.all()
    # raw -> rectified -> raw
    x, y, ok = N.inverse_points(fwd[0].ravel(), fwd[1].ravel(), K0, model, d, R, new_K)
    gx, gy = N.grid(size)
    assert ok.all() and np.abs(x - gx).max() <= 2e-6 and np.abs(y - gy).max() <= 2e-6
    # rectified -> raw -> rectified
    u, v, ok = N.forward_points(inv[0].ravel(), inv[1].ravel(), K0, model, d, R, new_K)
    gu, gv = N.grid(out)
    assert ok.all() and np.abs(u - gu).max() <= 2e-6 and np.abs(v - gv).max() <= 2e-6


def test_a_point_behind_the_rectified_camera_is_invalid():
    d = N.coefficients("radtan", (-0.1, 0.01, 0.0, 0.0))
    R = rot(1, 100.0)
    fwd, fv, inv, iv = N.maps(K0, "radtan", d, (21, 41), R)
    # Z = cos(100 deg) - a sin(100 deg) forward (+ a sin inverse): positive only beyond |a| = 0.176, in the outer columns of one side
    assert not fv[:, 12:].any() and fv[:, :11].all() and np.isnan(fwd[:, :, 12:]).all() and np.isfinite(fwd[:, :, :11]).all()
    assert not iv[:, :29].any() and iv[:, 30:].all() and np.isnan(inv[:, :, :29]).all()
    u, v, ok = N.forward_points([20.0], [10.0], K0, "radtan", d, rot(1, 80.0))
    assert ok.all() and np.isfinite(u).all()


# ---- stereo rectification ------------------------------------------------------------------------------------------------------------

def stereo_cases():
    rng = np.random.default_rng(4)
    for _ in range(6):
        om = rng.normal(size=3)
        om *= np.radians(rng.uniform(0.0, 8.0)) / np.linalg.norm(om)
        T = np.array([-rng.uniform(0.05, 0.3), rng.uniform(-0.02, 0.02), rng.uniform(-0.02, 0.02)])
        KL = np.array([[rng.uniform(200, 600), 0.0, rng.uniform(300, 340)], [0.0, rng.uniform(200, 600), rng.uniform(220, 260)], [0.0, 0.0, 1.0]])
        KR = np.array([[rng.uniform(200, 600), 0.0, rng.uniform(300, 340)], [0.0, rng.uniform(200, 600), rng.uniform(220, 260)], [0.0, 0.0, 1.0]])
        X = np.stack((rng.uniform(-2, 2, 200), rng.uniform(-1.5, 1.5, 200), rng.uniform(1.0, 8.0, 200)))
        yield N.rodrigues(om), T, KL, KR, X
    yield np.eye(3), np.array([-0.1, 0.0, 0.0]), K0, K0, np.array([[0.0, 0.3], [0.0, -0.2], [1.0, 2.0]])


@pytest.mark.parametrize("which", ("product", "restatement"))
def test_stereo_rectify_puts_points_on_one_row(which):
    """|v_l - v_r| <= 1e-9 px and u_l - u_r = fx' b / Z within 1e-9 px.  The bound is derived: coordinates up to 1e3 px, 2^-52
    relative rounding per value, about 1e2 operations between input and output give 2e-11 px; 1e-9 leaves fifty times that."""
    import event_utils_amd as E
    for R, T, KL, KR, X in stereo_cases():
        if which == "product":
            R1, R2, new_K, base = E.stereo_rectify(E.CameraModel(KL, sensor_size=(480, 640)), E.CameraModel(KR, sensor_size=(480, 640)), R, T)
        else:
            R1, R2, new_K, base = N.stereo_rectify(KL, KR, (480, 640), R, T)
        assert abs(base - np.linalg.norm(T)) < 1e-15 and new_K[0, 0] == new_K[1, 1] and new_K[0, 1] == 0.0
        for Rk in (R1, R2):
            assert np.abs(Rk @ Rk.T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(Rk) - 1.0) < 1e-14
        XL, XR = R1 @ X, R2 @ (R @ X + T[:, None])
        assert (XL[2] > 0).all() and (XR[2] > 0).all()
        pl, pr = new_K @ (XL / XL[2]), new_K @ (XR / XR[2])
        assert np.abs(pl).max() < 1e4
        assert np.abs(pl[1] - pr[1]).max() <= 1e-9
        assert np.abs((pl[0] - pr[0]) - new_K[0, 0] * base / XL[2]).max() <= 1e-9
    Ra, Rb, Ka, ba = E.stereo_rectify(E.CameraModel(K0, sensor_size=(20, 40)), E.CameraModel(K0, sensor_size=(20, 40)), None, [-0.2, 0.0, 0.0],
                                      out_size=(30, 60))
    assert np.array_equal(Ra, np.eye(3)) and np.array_equal(Rb, np.eye(3)) and ba == 0.2
    assert Ka.tolist() == [[45.0, 0.0, 30.0], [0.0, 45.0, 15.0], [0.0, 0.0, 1.0]]


# ---- the equidistant reference against itself in extended precision ---------------------------------------------------------------------

def test_the_equidistant_restatement_against_longdouble():
    """The float64 restatement stays within 1e-9 px of the same statement in np.longdouble: the bound the GPU test then uses for the
    equidistant model, whose atan and tan are not numpy's.  Largest difference seen, over the three cases: 2.0e-13 px forward, 8.9e-14
    px inverse (x86-64, 80-bit long double)."""
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.skip("np.longdouble is no wider than float64 here")
    sc_cams = N.scene_cameras("equidistant")
    cases = [(sc_cams[0][0], sc_cams[0][2], S.SCENE_SIZE, sc_cams[0][3], sc_cams[2], None),
             (sc_cams[1][0], sc_cams[1][2], S.SCENE_SIZE, sc_cams[1][3], sc_cams[2], None),
             (np.array([[226.4, 0.0, 173.6], [0.0, 226.1, 133.7], [0.0, 0.0, 1.0]]), N.coefficients("equidistant", (-0.048, 0.0113, -0.0489, 0.0339)),
              (260, 346), N.rodrigues([0.01, -0.02, 0.015]), None, (280, 360))]         # (an MVSEC-like DAVIS 346)
    worst = [0.0, 0.0]
    for K, d, size, R, new_K, out in cases:
        ref = N.maps(K, "equidistant", d, size, R, new_K, out)
        with N.precision(np.longdouble):
            ext = N.maps(K, "equidistant", d, size, R, new_K, out)
        assert ext[0].dtype == np.longdouble
        for k, (m, mv, e, ev) in enumerate(((ref[0], ref[1], ext[0], ext[1]), (ref[2], ref[3], ext[2], ext[3]))):
            assert np.array_equal(mv, ev) and mv.mean() > 0.9
            worst[k] = max(worst[k], float(np.abs(m[:, mv] - e[:, mv]).max()))
    print("largest difference: forward %.2e px, inverse %.2e px" % tuple(worst))
    assert worst[0] <= 1e-9 and worst[1] <= 1e-9


# ---- the event look-up ---------------------------------------------------------------------------------------------------------------

def test_rounding_at_a_half_and_at_the_border():
    W_even, W_odd = 4, 5
    # one raw row of eight pixels whose entries sit on halves: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4, 4.5 -> 4, -0.5 -> -0 (kept), -0.6
    u = np.array([[0.5, 1.5, 2.5, 3.5, 4.5, -0.5, -0.6, np.nan]])
    fwd = np.stack((u, np.zeros_like(u)))
    fv = np.ones((1, 8), dtype=bool)
    xs, ys = np.arange(8, dtype=np.int32), np.zeros(8, dtype=np.int32)
    ts = np.arange(8, dtype=np.float64)
    x, y, t, p, idx = N.rectify_events(xs, ys, ts, None, fwd, fv, (1, W_even))
    assert x.dtype == np.int32 and x.tolist() == [0, 2, 2, 0] and idx.tolist() == [0, 1, 2, 5] and t.tolist() == [0.0, 1.0, 2.0, 5.0] and p is None
    x, y, t, p, idx = N.rectify_events(xs, ys, ts, None, fwd, fv, (1, W_odd))              # W' - 0.5 = 4.5 rounds to 4: inside
    assert x.tolist() == [0, 2, 2, 4, 4, 0] and idx.tolist() == [0, 1, 2, 3, 4, 5]
    x, y, t, p, idx = N.rectify_events(xs, ys, ts, None, fwd, fv, (1, W_odd), mode="subpixel")
    assert x.dtype == np.float64 and x.tolist() == [0.5, 1.5, 2.5, 3.5] and idx.tolist() == [0, 1, 2, 3]      # 4.5 > W' - 1
    fv[0, 1] = False
    assert N.rectify_events(xs, ys, ts, None, fwd, fv, (1, W_odd))[4].tolist() == [0, 2, 3, 4, 5]
    for bad in (np.array([0.5]), np.array([8.0]), np.array([-1.0]), np.array([np.nan])):
        with pytest.raises(ValueError):
            N.rectify_events(bad, np.zeros(1), None, None, fwd, fv, (1, W_odd))


# ---- the remap -----------------------------------------------------------------------------------------------------------------------

def test_remap_by_hand():
    plane = np.array([[[10.0, 20.0, 40.0], [80.0, 160.0, 200.0]]])
    mx = np.array([[0.0, 1.25, 2.5, 1.5, -0.25, 5.0, 0.5]])
    my = np.array([[0.0, 0.25, 1.0, 0.5, 0.0, 0.0, 0.5]])
    inv, iv = np.stack((mx, my)), np.ones((1, 7), dtype=bool)
    iv[0, 6] = False
    near = N.remap(plane, inv, iv, "nearest", fill=-1.0)
    # (1.25, .25) -> (1, 0); (2.5, 1) -> (2, 1); (1.5, .5) -> (2, 0): halves to even; (-.25, 0) -> (0, 0); x = 5 is off the sensor
    assert near[0, 0].tolist() == [10.0, 20.0, 200.0, 40.0, 10.0, -1.0, -1.0]
    lin = N.remap(plane, inv, iv, "bilinear", fill=-1.0)
    # a quarter offset: .75 (.75 20 + .25 40) + .25 (.75 160 + .25 200) = .75 25 + .25 170
    assert lin[0, 0, 1] == 0.75 * 25.0 + 0.25 * 170.0
    # (2.5, 1): x0 = 2, taps x = 3 and y = 2 are off the sensor: b = 0, so 1 (.5 200 + .5 -1) + 0 (...)
    assert lin[0, 0, 2] == 0.5 * 200.0 + 0.5 * -1.0
    # (-.25, 0): x0 = -1, a = .75: .25 (-1) + .75 10
    assert lin[0, 0, 4] == 0.25 * -1.0 + 0.75 * 10.0
    assert lin[0, 0, 0] == 10.0 and lin[0, 0, 5] == -1.0 and lin[0, 0, 6] == -1.0
    # uint8: one rounding, halves to even, clamped
    q = np.array([[[1, 2], [4, 255]]], dtype=np.uint8)
    mx = np.array([[0.5, 0.5, 0.0, 1.0, 1.4]])
    my = np.array([[0.0, 1.0, 0.5, 0.5, 1.0]])
    out = N.remap(q, np.stack((mx, my)), np.ones((1, 5), dtype=bool), "bilinear", fill=300.0)
    # 1.5 -> 2; (4 + 255) / 2 = 129.5 -> 130; (1 + 4) / 2 = 2.5 -> 2; (2 + 255) / 2 = 128.5 -> 128; .6 255 + .4 fill(255) = 255
    assert out.dtype == np.uint8 and out[0, 0].tolist() == [2, 130, 2, 128, 255]
    assert N.remap(q, np.full((2, 1, 2), np.nan), np.ones((1, 2), dtype=bool), "nearest", fill=300.0)[0, 0].tolist() == [255, 255]
    assert N.remap(q, np.full((2, 1, 2), -9.0), np.ones((1, 2), dtype=bool), "bilinear", fill=-3.0)[0, 0].tolist() == [0, 0]
    assert N.remap(q.astype(np.float32), np.stack((mx, my)), np.ones((1, 5), dtype=bool), "bilinear").dtype == np.float32
    assert N.remap(q[:0], np.stack((mx, my)), np.ones((1, 5), dtype=bool)).shape == (0, 1, 5)


# ---- the seeded raw scene --------------------------------------------------------------------------------------------------------------

def test_rectification_recovers_the_seeded_raw_scene():
    """The dots of the stereo scene seen through two raw cameras: focal length 130 px, a relative rotation of 1.1 degrees, lenses that
    move the corner pixels by 3.8 px (radtan) and 5.3 px (equidistant).  The share of candidate dots (last rectified left pixel)
    whose winner lies within one disparity of the truth, measured with the restatements alone (uniqueness and left-right test off):
      yardstick (no lens, no rotation)   0.744 of 39
      radtan       raw events as they are 0.333 of 12; after rectify_events 0.767 of 30; after remap of the surfaces 0.742 of 31
      equidistant  raw events as they are 0.308 of 13; after rectify_events 0.750 of 28; after remap of the surfaces 0.733 of 30
    Both rectifications must stand no more than 0.05 below the yardstick (one dot in twenty is the grain of such a scene, the
    margin of the stereo section's floors), and the raw events below both."""
    yard = N.raw_scene("none")
    n0, share0 = N.scene_share(yard, *N.scene_surfaces(yard, "raw"))
    print("yardstick %.3f of %d" % (share0, n0))
    assert n0 == 39 and abs(share0 - 29 / 39) < 1e-12       # the same dots as the rectified scene of the stereo tests
    for model in ("radtan", "equidistant"):
        sc = N.raw_scene(model)
        got = {how: N.scene_share(sc, *N.scene_surfaces(sc, how)) for how in ("raw", "events", "images")}
        print(model, " ".join("%s %.3f of %d" % (how, s, n) for how, (n, s) in got.items()))
        assert got["events"][1] >= share0 - 0.05 and got["images"][1] >= share0 - 0.05
        assert got["raw"][1] < got["events"][1] and got["raw"][1] < got["images"][1]
        assert got["events"][0] >= 20 and got["images"][0] >= 20
        # the lens moves corner pixels by several pixels; every pixel of both sensors has a place in the rectified view
        for side in ("left", "right"):
            fwd, fv, inv, iv = N.scene_maps(sc, side)
            gx, gy = (g.reshape(S.SCENE_SIZE) for g in N.grid(S.SCENE_SIZE))
            assert fv.all() and iv.all() and np.hypot(fwd[0] - gx, fwd[1] - gy).max() > 3.0


# ---- the public surface and the C ABI ------------------------------------------------------------------------------------------------

def test_the_prototypes_are_bound_with_their_arguments():
    from event_utils_amd import _lib
    text = _header.TEXT
    protos = _header.prototypes("evk_camera_")
    assert set(protos) == ENTRIES
    for name, want in protos.items():
        assert want[1] is ctypes.c_int and _lib.PROTOTYPES[name] == want, name
        assert hasattr(_lib.lib(), name)
    for name, value in (("EVK_CAMERA_NONE", 0), ("EVK_CAMERA_RADTAN", 1), ("EVK_CAMERA_EQUIDISTANT", 2), ("EVK_CAMERA_FORWARD", 0),
                        ("EVK_CAMERA_INVERSE", 1), ("EVK_CAMERA_NEAREST", 0), ("EVK_CAMERA_SUBPIXEL", 1), ("EVK_CAMERA_BILINEAR", 1),
                        ("EVK_CAMERA_U8", 0), ("EVK_CAMERA_F32", 1), ("EVK_CAMERA_F64", 2)):
        assert getattr(_lib, name) == value and re.search(r"^#define\s+%s\s+%d\b" % (name, value), text, re.M)
    assert "Camera calibration (evk_camera.hip)" in text


def test_public_surface():
    import inspect
    import event_utils_amd as E
    import event_utils_amd.lib.calibration.camera as alias
    from event_utils_amd import calibration
    from event_utils_amd.calibration import camera
    assert alias is camera
    for name in PUBLIC:
        assert getattr(E, name) is getattr(camera, name) is getattr(calibration, name)
    assert "(no reference module)           -> event_utils_amd.calibration.camera" in E.__doc__
    assert E.RectificationMaps._fields == ("forward", "forward_valid", "inverse", "inverse_valid", "new_K", "out_size")
    empty = inspect.Parameter.empty

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    solver = [("iterations", 20), ("tolerance", 1e-6)]
    assert params(E.CameraModel) == [("K", empty), ("distortion", None), ("model", "none"), ("sensor_size", None)]
    assert params(E.distort_points) == [("cam", empty), ("points", empty)]
    assert params(E.undistort_points) == [("cam", empty), ("points", empty), ("R", None), ("new_K", None)] + solver + [("return_valid", False)]
    assert params(E.rectification_maps) == [("cam", empty), ("R", None), ("new_K", None), ("out_size", None)] + solver
    assert params(E.rectify_events) == [(n, empty) for n in ("xs", "ys", "ts", "ps", "maps")] + [("mode", "nearest"), ("return_index", False)]
    assert params(E.remap_images) == [("images", empty), ("maps", empty), ("interpolation", "nearest"), ("fill", 0)]
    assert params(E.stereo_rectify) == [(n, empty) for n in ("cam_left", "cam_right", "R", "T")] + [("out_size", None)]
    cam = E.CameraModel(K0, (0.1, 0.2, 0.3, 0.4), "radtan", (20, 40))
    assert cam.coefficients.tolist() == [0.1, 0.2, 0.3, 0.4, 0.0] and cam.sensor_size == (20, 40) and cam.intrinsics == (50.0, 40.0, 20.0, 10.0)


def test_arguments_are_refused_before_the_device_is_touched():
    from event_utils_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)                            # a device pointer that is never dereferenced: every call below is refused first
    einval, nan, inf = -1, float("nan"), float("inf")
    keep = []

    def params(**kw):
        a = np.concatenate(([50.0, 40.0, 20.0, 10.0], np.zeros(5), np.eye(3).reshape(9), [45.0, 45.0, 24.0, 13.0]))
        for k, v in kw.items():
            a[int(k[1:])] = v
        keep.append(a)
        return ctypes.c_void_p(a.ctypes.data)

    def points(model=1, direction=0, pts=fake, n=100, h=0, w=0, prm="ok", iterations=20, tolerance=1e-6, out=fake, valid=fake):
        return L.evk_camera_points(model, direction, pts, n, h, w, params() if prm == "ok" else prm, iterations, tolerance, out, valid, None)
    assert points(model=3) == einval and points(model=-1) == einval and points(direction=2) == einval and points(direction=-1) == einval
    assert points(n=-1) == einval and points(h=-1) == einval and points(w=-1) == einval and points(pts=None, n=100, h=10, w=11) == einval
    assert points(pts=None, n=1 << 32, h=1 << 16, w=1 << 16) == einval
    assert points(iterations=0) == einval and points(iterations=-3) == einval and points(tolerance=-1e-6) == einval and points(tolerance=nan) == einval
    assert points(out=None) == einval and points(valid=None) == einval and points(prm=None) == einval
    for at in (0, 1, 18, 19):                               # fx, fy, fx', fy'
        for bad in (0.0, -50.0, nan, inf):
            assert points(prm=params(**{"p%d" % at: bad})) == einval, (at, bad)
    for at in (2, 3, 4, 8, 9, 17, 20, 21):
        for bad in (nan, inf, -inf):
            assert points(prm=params(**{"p%d" % at: bad})) == einval, (at, bad)
    assert points(n=0) == 0 and points(pts=None, n=0, h=0, w=7) == 0 and points(model=0, direction=1, n=0) == 0       # nothing is launched

    def lookup(kind=1, x=fake, y=fake, n=100, m=fake, mv=fake, h=10, w=12, oh=10, ow=12, mode=0, out_kind=1, ox=fake, oy=fake, kp=fake, bad=fake):
        return L.evk_camera_rectify_lookup(kind, x, y, n, m, mv, h, w, oh, ow, mode, out_kind, ox, oy, kp, bad, None)
    assert lookup(kind=-1) == einval and lookup(kind=5) == einval and lookup(out_kind=-1) == einval and lookup(out_kind=5) == einval
    assert lookup(n=-1) == einval and lookup(h=-1) == einval and lookup(w=-1) == einval and lookup(oh=-1) == einval and lookup(ow=-1) == einval
    assert lookup(h=1 << 16, w=1 << 15) == einval and lookup(mode=2) == einval and lookup(mode=-1) == einval
    assert lookup(out_kind=0, ow=32769) == einval and lookup(out_kind=0, oh=40000) == einval
    for missing in ("x", "y", "m", "mv", "ox", "oy", "kp"):
        assert lookup(**{missing: None}) == einval, missing
    assert lookup(n=0) == 0 and lookup(n=0, x=None, y=None, m=None, mv=None) == 0

    def remap(src=fake, dtype=0, planes=2, h=10, w=12, m=fake, mv=fake, oh=10, ow=12, interp=0, fill=0.0, dst=fake):
        return L.evk_camera_remap(src, dtype, planes, h, w, m, mv, oh, ow, interp, fill, dst, None)
    assert remap(dtype=-1) == einval and remap(dtype=3) == einval and remap(planes=-1) == einval and remap(interp=2) == einval and remap(interp=-1) == einval
    assert remap(h=-1) == einval and remap(w=-1) == einval and remap(oh=-1) == einval and remap(ow=-1) == einval
    assert remap(h=1 << 16, w=1 << 15) == einval and remap(oh=1 << 16, ow=1 << 15) == einval
    assert remap(src=None) == einval and remap(m=None) == einval and remap(mv=None) == einval and remap(dst=None) == einval
    assert remap(planes=0) == 0 and remap(oh=0) == 0 and remap(planes=0, src=None, m=None, mv=None) == 0


def test_python_argument_errors_come_before_any_device_work():
    """every call below is refused on its arguments alone: none of them reaches the point where a missing GPU would matter"""
    import torch
    import event_utils_amd as E
    size = (20, 40)
    with pytest.raises(ValueError, match="skew"):
        E.CameraModel(K0 + np.array([[0, 0.5, 0], [0, 0, 0], [0, 0, 0]]), sensor_size=size)
    for bad in (np.eye(4), np.eye(2), K0 * np.array([[0.0, 1, 1]] * 3), K0 * np.array([[-1.0, 1, 1]] * 3), K0 + np.array([[0, 0, 0], [1.0, 0, 0], [0, 0, 0]]),
                K0 * np.nan, K0 * 2.0):
        with pytest.raises(ValueError, match="K must"):
            E.CameraModel(bad, sensor_size=size)
    with pytest.raises(ValueError, match="model"):
        E.CameraModel(K0, model="fisheye", sensor_size=size)
    for model, dist in (("none", (0.1,)), ("radtan", (0.1, 0.2, 0.3)), ("radtan", None), ("radtan", (1, 2, 3, 4, 5, 6)), ("equidistant", (1, 2, 3, 4, 5)),
                        ("equidistant", None), ("radtan", (0.1, 0.2, np.nan, 0.4))):
        with pytest.raises(ValueError, match="coefficients"):
            E.CameraModel(K0, dist, model, size)
    for bad in (None, (20,), (0, 40), (20, -1), (2.5, 40), (1 << 16, 1 << 16)):
        with pytest.raises(ValueError, match="sensor_size"):
            E.CameraModel(K0, sensor_size=bad)
    cam = E.CameraModel(K0, (-0.1, 0.01, 0.0, 0.0), "radtan", size)
    for f in (lambda p, **kw: E.distort_points(cam, p), lambda p, **kw: E.undistort_points(cam, p, **kw)):
        for bad in (np.ones((5, 3)), np.ones(2), np.ones((2, 5)), torch.ones((2, 2, 2))):
            with pytest.raises(ValueError, match="points"):
                f(bad)
        for bad in ([[1.0, 2.0]], np.ones((5, 2), dtype=complex), torch.ones((5, 2), dtype=torch.bool)):
            with pytest.raises(TypeError, match="points"):
                f(bad)
    with pytest.raises(TypeError, match="CameraModel"):
        E.undistort_points(K0, np.ones((5, 2)))
    P = np.ones((5, 2))
    for f in (lambda **kw: E.undistort_points(cam, P, **kw), lambda **kw: E.rectification_maps(cam, **kw)):
        for bad in (np.eye(4), np.eye(3) * 2.0, np.eye(3) * np.nan, np.diag([1.0, 1.0, -1.0])):
            with pytest.raises(ValueError, match="R must"):
                f(R=bad)
        with pytest.raises(ValueError, match="new_K"):
            f(new_K=np.eye(3) * 2.0)
        with pytest.raises(ValueError, match="skew"):
            f(new_K=K0 + np.array([[0, 0.5, 0], [0, 0, 0], [0, 0, 0]]))
        for bad in (0, -1, 2.5, True):
            with pytest.raises(ValueError, match="iterations"):
                f(iterations=bad)
        for bad in (-1e-6, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="tolerance"):
                f(tolerance=bad)
    for bad in ((20,), (0, 40), (20, 2.5)):
        with pytest.raises(ValueError, match="out_size"):
            E.rectification_maps(cam, out_size=bad)
    # maps: made from tensors on the host here; the consumers check them before they ask for a device
    fwd, inv = torch.zeros((2, 20, 40), dtype=torch.float64), torch.zeros((2, 24, 48), dtype=torch.float64)
    maps = E.RectificationMaps(fwd, torch.ones((20, 40), dtype=torch.bool), inv, torch.ones((24, 48), dtype=torch.bool), K0, (24, 48))
    xs = np.zeros(3, dtype=np.int32)
    with pytest.raises(ValueError, match="mode"):
        E.rectify_events(xs, xs, xs, xs, maps, mode="bilinear")
    with pytest.raises(ValueError, match="interpolation"):
        E.remap_images(np.zeros((20, 40), dtype=np.uint8), maps, interpolation="subpixel")
    with pytest.raises(TypeError, match="RectificationMaps"):
        E.rectify_events(xs, xs, xs, xs, (fwd, inv))
    with pytest.raises(TypeError, match="RectificationMaps"):
        E.remap_images(np.zeros((20, 40), dtype=np.uint8), fwd)
    with pytest.raises(TypeError, match="float64"):
        E.rectify_events(xs, xs, xs, xs, maps._replace(forward=fwd.to(torch.float32)))
    with pytest.raises(TypeError, match="bool"):
        E.rectify_events(xs, xs, xs, xs, maps._replace(forward_valid=torch.ones((20, 40), dtype=torch.uint8)))
    with pytest.raises(ValueError, match=r"\(2, H, W\)"):
        E.rectify_events(xs, xs, xs, xs, maps._replace(forward=fwd[0]))
    with pytest.raises(ValueError, match=r"\(2, H, W\)"):
        E.remap_images(np.zeros((20, 40), dtype=np.uint8), maps._replace(inverse_valid=torch.ones((20, 40), dtype=torch.bool)))
    with pytest.raises(ValueError, match="size"):           # images of another size than the maps' camera
        E.remap_images(np.zeros((3, 24, 48), dtype=np.uint8), maps)
    with pytest.raises(ValueError, match=r"\(\.\.\., H, W\)"):
        E.remap_images(np.zeros(40, dtype=np.uint8), maps)
    for bad in (np.zeros((20, 40), dtype=np.int32), np.zeros((20, 40), dtype=np.float16), torch.zeros((20, 40), dtype=torch.int8)):
        with pytest.raises(TypeError, match="uint8, float32 or float64"):
            E.remap_images(bad, maps)
    with pytest.raises(TypeError, match="images"):
        E.remap_images([[1, 2]], maps)
    with pytest.raises(ValueError, match="fill"):
        E.remap_images(np.zeros((20, 40), dtype=np.uint8), maps, fill=float("nan"))
    with pytest.raises(ValueError, match="camera's size"):  # a map whose size is not the camera's
        E.RectificationMaps.from_tensors(cam, np.zeros((2, 24, 48)), np.zeros((2, 24, 48)))
    with pytest.raises(TypeError, match="float64"):
        E.RectificationMaps.from_tensors(cam, np.zeros((2, 20, 40), dtype=np.float32), np.zeros((2, 24, 48)))
    with pytest.raises(ValueError, match=r"\(2, H, W\)"):
        E.RectificationMaps.from_tensors(cam, np.zeros((20, 40)), np.zeros((2, 24, 48)))
    # stereo_rectify is host code
    for bad in ([1.0, 2.0], [0.0, 0.0, 0.0], [np.nan, 0.0, 0.0]):
        with pytest.raises(ValueError, match="T must"):
            E.stereo_rectify(cam, cam, np.eye(3), bad)
    with pytest.raises(ValueError, match="left"):
        E.stereo_rectify(cam, cam, np.eye(3), [0.1, 0.0, 0.0])
    with pytest.raises(ValueError, match="R must"):
        E.stereo_rectify(cam, cam, np.eye(3) * 2.0, [-0.1, 0.0, 0.0])
    with pytest.raises(TypeError, match="CameraModel"):
        E.stereo_rectify(cam, K0, np.eye(3), [-0.1, 0.0, 0.0])
    with pytest.raises(ValueError, match="out_size"):
        E.stereo_rectify(cam, cam, np.eye(3), [-0.1, 0.0, 0.0], out_size=(0, 5))


def test_the_kernels_compile_without_scratch_memory(tmp_path):
    """every kernel of evk_camera.hip compiles for gfx950 with no scratch memory, no spilled registers and no LDS, within 64 registers
    (eight waves per SIMD): read from the code object's metadata"""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    from event_utils_amd.csrc import build as B
    src = os.path.join(B.HERE, "evk_camera.hip")
    subprocess.run([hipcc] + list(B.CFLAGS) + ["-c", src, "-o", str(tmp_path / "camera.o"), "-save-temps=obj"], check=True, cwd=B.HERE,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert asm, os.listdir(tmp_path)
    text = open(tmp_path / asm[0]).read()
    kernels = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    seen = {n: dict(lds=int(l), private=int(p), sspill=int(ss), vgpr=int(v), vspill=int(vs)) for l, n, p, ss, v, vs in kernels}
    # three models x two directions; five coordinate kinds; three plane dtypes
    for name, count in (("k_camera_points", 6), ("k_rectify_lookup", 5), ("k_remap_planes", 3)):
        assert sum(name in n for n in seen) == count, (name, sorted(seen))
    assert len(seen) == 14
    assert not {n: v for n, v in seen.items() if v["private"] or v["sspill"] or v["vspill"] or v["lds"]}
    assert all(v["vgpr"] <= 64 for v in seen.values()), seen
