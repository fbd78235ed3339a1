"""CPU (no GPU): the angular-velocity and planar-flow motion models -- library entry points, the Python API surface, argument
errors, band geometry, and the numpy restatement the GPU tests compare against
(tests/_motion_models8_np.py)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import scipy.optimize as opt

import _motion_models8_np as M8
import _motion_models_np as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evk_warp_param_f64", "evk_iwe_param_f32", "evk_iwe_param_f64", "evk_iwe_param_band_rows",
       "evk_objective_gradsums_planes_f32")
K = M8.K_DEFAULT


def test_entry_points_are_declared_exported_and_bound():
    from event_utils_amd.csrc import build
    build.build(verbose=False)
    from event_utils_amd import _lib
    text = open(os.path.join(ROOT, "include", "evk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = set(_lib.PROTOTYPES)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in bound, name
    for name in ("EVK_WARP_ANGULAR_VELOCITY", "EVK_WARP_PLANAR_FLOW"):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, header)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    assert len({_lib.EVK_WARP_ROTATION, _lib.EVK_WARP_XYZTHETA, _lib.EVK_WARP_ANGULAR_VELOCITY, _lib.EVK_WARP_PLANAR_FLOW}) == 4
    assert _lib.lib().evk_version() == 100


def test_api_surface():
    import event_utils_amd as E
    from event_utils_amd import _lib
    from event_utils_amd import contrast_max as CM
    from event_utils_amd.contrast_max import warps as W
    a, f = E.angular_velocity_warp(K), E.planar_flow_warp()
    assert CM.angular_velocity_warp is W.angular_velocity_warp and CM.planar_flow_warp is W.planar_flow_warp
    assert (a.name, a.dims, f.name, f.dims) == ("angular_velocity_warp", 3, "planar_flow_warp", 8)
    assert f.center == (0.0, 0.0) and W.planar_flow_warp(center=(3, 4)).center == (3.0, 4.0)
    sig = inspect.signature(W.linvel_warp.warp)
    assert inspect.signature(W.angular_velocity_warp.warp) == sig == inspect.signature(W.planar_flow_warp.warp)
    assert np.array_equal(a.default_params((180, 240)), np.zeros(3))
    assert np.array_equal(f.default_params((480, 640)), np.zeros(8))
    assert np.array_equal(a.host_params((0.1, 0.2, 0.3)), [0.1, 0.2, 0.3, 200.0, 200.0, 120.0, 90.0])
    assert np.array_equal(W.planar_flow_warp((5, 6)).host_params(np.arange(8.0)), list(range(8)) + [5.0, 6.0])
    assert W.uses_fused_param(a) and W.uses_fused_param(f)
    assert (a.fused_model, f.fused_model) == (_lib.EVK_WARP_ANGULAR_VELOCITY, _lib.EVK_WARP_PLANAR_FLOW)

    class Sub(W.planar_flow_warp):
        pass

    class Own(W.angular_velocity_warp):
        def warp(self, xs, ys, ts, ps, t0, params, compute_grad=False):
            return None
    assert W.uses_fused_param(Sub()) and not W.uses_fused_param(Own(K))


@pytest.mark.parametrize("bad", [np.eye(2), np.zeros((3, 4)), [[200.0, 1.0, 120.0], [0.0, 200.0, 90.0], [0.0, 0.0, 1.0]],
                                 [[0.0, 0.0, 120.0], [0.0, 200.0, 90.0], [0.0, 0.0, 1.0]],
                                 [[200.0, 0.0, 120.0], [0.0, -5.0, 90.0], [0.0, 0.0, 1.0]],
                                 [[200.0, 0.0, 120.0], [0.0, 200.0, 90.0], [0.0, 0.0, 2.0]]])
def test_camera_matrix_is_validated(bad):
    from event_utils_amd.contrast_max.warps import angular_velocity_warp
    with pytest.raises(ValueError):
        angular_velocity_warp(bad)


def test_an_explicit_d_iwe_must_have_dims_channels():
    from event_utils_amd.contrast_max import objectives as O
    from event_utils_amd.contrast_max.warps import angular_velocity_warp, planar_flow_warp
    assert O._d_iwe_planes(np.zeros((3, 4, 4)), angular_velocity_warp(K)) is True
    assert O._d_iwe_planes(np.zeros((8, 4, 4)), planar_flow_warp()) is True
    for d, w in ((np.zeros((4, 4, 4)), planar_flow_warp()), (np.zeros((8, 4, 4)), angular_velocity_warp(K))):
        with pytest.raises(ValueError):
            O._d_iwe_planes(d, w)


def test_argument_errors_need_no_gpu():
    from event_utils_amd import _lib
    L = _lib.lib()
    hp = np.zeros(10)
    hpp = ctypes.c_void_p(hp.ctypes.data)
    fake = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused first
    for bad_model in (0, 5, -1):
        assert L.evk_warp_param_f64(bad_model, fake, fake, fake, 8, 0.0, hpp, fake, fake, None, None, None) == -1
        assert L.evk_iwe_param_f32(bad_model, fake, fake, fake, fake, 8, 0.0, hpp, 240.0, 180.0, 181, 241, 0, 1.0, fake, None,
                                   None) == -1
        assert L.evk_iwe_param_f64(bad_model, fake, fake, fake, fake, 8, 0.0, hpp, 240.0, 180.0, 181, 241, 0, 1.0, fake, None,
                                   None) == -1
        assert L.evk_iwe_param_band_rows(bad_model, 0, 181, 241) == 0
    F = _lib.EVK_WARP_PLANAR_FLOW
    assert L.evk_warp_param_f64(F, None, fake, fake, 8, 0.0, hpp, fake, fake, None, None, None) == -1
    assert L.evk_warp_param_f64(F, fake, fake, fake, 8, 0.0, None, fake, fake, None, None, None) == -1
    assert L.evk_warp_param_f64(F, fake, fake, fake, 8, 0.0, hpp, fake, fake, fake, None, None) == -1
    assert L.evk_warp_param_f64(F, fake, fake, fake, -1, 0.0, hpp, fake, fake, None, None, None) == -1
    assert L.evk_iwe_param_f32(F, fake, None, fake, fake, 8, 0.0, hpp, 240.0, 180.0, 181, 241, 0, 1.0, fake, None, None) == -1
    assert L.evk_iwe_param_f64(F, fake, fake, fake, None, 8, 0.0, hpp, 240.0, 180.0, 181, 241, 0, 1.0, fake, None, None) == -1
    assert L.evk_iwe_param_f32(F, fake, fake, fake, fake, 8, 0.0, hpp, 240.0, 180.0, 181, 241, _lib.EVK_IWE_GRADIENT, 1.0, fake,
                               None, None) == -1
    assert L.evk_iwe_param_f32(F, fake, fake, fake, fake, 8, 0.0, hpp, 240.0, 180.0, 181, 241, 0, 1.0, None, None, None) == -1
    assert L.evk_iwe_param_f32(F, fake, fake, fake, fake, 8, 0.0, hpp, 240.0, 180.0, 1, 241, 0, 1.0, fake, None, None) == -1
    assert L.evk_iwe_param_f32(F, fake, fake, fake, fake, 8, 0.0, None, 240.0, 180.0, 181, 241, 0, 1.0, fake, None, None) == -1
    G8 = L.evk_objective_gradsums_planes_f32
    for k in (0, 9):
        assert G8(fake, fake, k, 4, 4, 0, 0.0, fake, fake, 1 << 20, None) == -1
    assert G8(None, fake, 8, 4, 4, 0, 0.0, fake, fake, 1 << 20, None) == -1
    assert G8(fake, fake, 8, 4, 4, 4, 0.0, fake, fake, 1 << 20, None) == -1
    assert G8(fake, fake, 8, 0, 4, 0, 0.0, fake, fake, 1 << 20, None) == -1
    assert G8(fake, fake, 8, 4, 4, 0, 0.0, fake, fake, 8, None) == -2


def test_band_geometry():
    from event_utils_amd import _lib
    L = _lib.lib()
    A, F, G = _lib.EVK_WARP_ANGULAR_VELOCITY, _lib.EVK_WARP_PLANAR_FLOW, _lib.EVK_IWE_GRADIENT
    for model, flags, planes in ((A, 0, 1), (A, G, 4), (F, 0, 1), (F, G, 9)):
        for h, w in ((181, 241), (481, 641)):
            rows = L.evk_iwe_param_band_rows(model, flags, h, w)
            assert rows >= 1 and planes * rows * w * 4 <= 160 * 1024, (model, flags, h, w)
    # the sizing of DESIGN.md: 9 planes -> 18 rows (11 bands) at 240x180, 7 rows (69 bands) at 640x480, direct at 1280x720
    assert L.evk_iwe_param_band_rows(F, G, 181, 241) == 18
    assert L.evk_iwe_param_band_rows(F, G, 481, 641) == 7
    assert L.evk_iwe_param_band_rows(F, G, 721, 1281) == 0
    # 4 planes: as rotation
    R = _lib.EVK_WARP_ROTATION
    for h, w in ((181, 241), (481, 641), (721, 1281)):
        assert L.evk_iwe_param_band_rows(A, G, h, w) == L.evk_iwe_param_band_rows(R, G, h, w)
        assert L.evk_iwe_param_band_rows(F, 0, h, w) == L.evk_iwe_param_band_rows(R, 0, h, w)
    assert L.evk_iwe_param_band_rows(F, G | _lib.EVK_IWE_DIRECT, 181, 241) == 0
    assert L.evk_iwe_param_band_rows(F, G, 41, 12001) == 0          # not one row of 9 planes fits: the direct kernel


# ---- the numpy restatement itself ---------------------------------------------------------------------------------------

def _events(n=300, seed=1, duration=0.2):
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, 240, n), rng.uniform(0, 180, n)
    t = np.sort(rng.uniform(0, duration, n))
    return x, y, t


def _fd_check(model, params, center=(0.0, 0.0), rel=1e-6, tol=1e-7, x=None, y=None, t=None):
    if x is None:
        x, y, t = _events()
    _, _, jx, jy = M8.warp(model, x, y, t, t[-1], params, center)
    finite = np.isfinite(jx[0])
    for i in range(len(params)):
        h = rel * max(1.0, abs(params[i]))
        qp, qm = np.array(params, dtype=float), np.array(params, dtype=float)
        qp[i] += h
        qm[i] -= h
        xp, yp, _, _ = M8.warp(model, x, y, t, t[-1], qp, center)
        xm, ym, _, _ = M8.warp(model, x, y, t, t[-1], qm, center)
        np.testing.assert_allclose(jx[i][finite], ((xp - xm) / (2 * h))[finite], rtol=1e-6, atol=tol)
        np.testing.assert_allclose(jy[i][finite], ((yp - ym) / (2 * h))[finite], rtol=1e-6, atol=tol)
    return finite


@pytest.mark.parametrize("w", [(0.0, 0.0, 0.0), (0.6, -0.8, 1.5), (1e-7, -2e-7, 3e-7), (1e-9 / 0.2, 0.0, 0.0)])
def test_helper_angular_velocity_jacobian_matches_central_differences(w):
    finite = _fd_check(M8.ANGVEL, w, rel=1e-6, tol=1e-7)
    assert finite.all()


def test_helper_angular_velocity_at_zero_is_the_identity():
    x, y, t = _events()
    xo, yo, jx, jy = M8.warp(M8.ANGVEL, x, y, t, t[-1], (0.0, 0.0, 0.0))
    np.testing.assert_allclose(xo, x, rtol=0, atol=1e-12)
    np.testing.assert_allclose(yo, y, rtol=0, atol=1e-12)
    R, Jr = M8.so3(np.zeros((1, 3)))
    assert np.array_equal(R[0], np.eye(3)) and np.array_equal(Jr[0], np.eye(3))


def test_helper_angular_velocity_behind_the_camera():
    # |w dt| ~ 2 rad about y: the events on one side of the image turn behind the camera
    x, y, t = _events(400, seed=3, duration=1.0)
    w = (0.0, 2.2, 0.0)
    xo, yo, jx, jy = M8.warp(M8.ANGVEL, x, y, t, t[-1], w)
    bad = np.isnan(xo)
    assert bad.any() and (~bad).any()
    assert np.array_equal(bad, np.isnan(yo)) and np.isnan(jx[:, bad]).all() and np.isnan(jy[:, bad]).all()
    finite = _fd_check(M8.ANGVEL, w, rel=1e-7, tol=1e-5, x=x, y=y, t=t)
    assert np.array_equal(finite, ~bad)
    # such events reach no image
    img, d_img = M8.iwe(M8.ANGVEL, w, x, y, t, np.ones_like(x))
    assert np.isfinite(img).all() and np.isfinite(d_img).all()


@pytest.mark.parametrize("a", [np.zeros(8), M8.PF_TRUTH, np.array([-30.0, 1.2, -0.7, 12.0, -0.9, 0.4, -4e-3, 6e-3])])
def test_helper_planar_flow_jacobian_matches_central_differences(a):
    _fd_check(M8.PLANAR, a, center=(120.0, 90.0), rel=1e-6, tol=1e-7)


def test_helper_planar_flow_special_cases():
    x, y, t = _events(500, seed=4)
    c = (120.0, 90.0)
    for q in ((40.0, -25.0, 2.0, 1.0), (-300.0, 200.0, -8.0, 30.0), (0.0, 0.0, 0.0, 0.0)):
        xz, yz, jxz, jyz = M.warp(M.XYZTHETA, x, y, t, t[-1], q, center=c)
        xp, yp, jxp, jyp = M8.warp(M8.PLANAR, x, y, t, t[-1], M8.xyztheta_as_planar(q), center=c)
        np.testing.assert_allclose(xp, xz, rtol=1e-13, atol=1e-10)
        np.testing.assert_allclose(yp, yz, rtol=1e-13, atol=1e-10)
    for q in ((30.0, -20.0), (0.0, 0.0), (-150.0, 75.0)):
        xp, yp, _, _ = M8.warp(M8.PLANAR, x, y, t, t[-1], M8.linvel_as_planar(q), center=c)
        dt = t - t[-1]
        np.testing.assert_allclose(xp, x - dt * q[0], rtol=1e-14, atol=1e-12)
        np.testing.assert_allclose(yp, y - dt * q[1], rtol=1e-14, atol=1e-12)


def test_helper_angular_velocity_about_z_is_pure_rotation():
    x, y, t = _events(500, seed=5)
    for wz in (0.0, 0.3, -2.5, 1e-8):
        xa, ya, jxa, jya = M8.warp(M8.ANGVEL, x, y, t, t[-1], (0.0, 0.0, wz))
        xr, yr, jxr, jyr = M.warp(M.ROTATION, x, y, t, t[-1], (K[0, 2], K[1, 2], -wz))
        np.testing.assert_allclose(xa, xr, rtol=1e-13, atol=1e-10)
        np.testing.assert_allclose(ya, yr, rtol=1e-13, atol=1e-10)
        # d/dwz = -d/domega
        np.testing.assert_allclose(jxa[2], -jxr[2], rtol=1e-9, atol=1e-10)
        np.testing.assert_allclose(jya[2], -jyr[2], rtol=1e-9, atol=1e-10)


def test_helper_synthetic_scenes_map_back_onto_their_points():
    for model, truth, c in ((M8.ANGVEL, M8.AV_TRUTH, (0.0, 0.0)), (M8.PLANAR, M8.PF_TRUTH, M8.PF_CENTER)):
        x, y, t, p = M8.scene(model, n=5000, seed=0)
        xs, ys, _, _ = M8.scene(model, n=5000, seed=0, duration=1e-300)        # every event at its point (dt ~ 0)
        xw, yw, _, _ = M8.warp(model, x, y, t, t[-1], truth, c)
        np.testing.assert_allclose(xw, xs, atol=1e-9)
        np.testing.assert_allclose(yw, ys, atol=1e-9)


@pytest.mark.parametrize("model", [M8.ANGVEL, M8.PLANAR])
def test_helper_scipy_bfgs_recovers_the_synthetic_scene(model):
    x, y, t, p = M8.scene(model)
    truth, start = (M8.AV_TRUTH, M8.AV_START) if model == M8.ANGVEL else (M8.PF_TRUTH, M8.PF_START)
    center = (0.0, 0.0) if model == M8.ANGVEL else M8.PF_CENTER
    f, g = M8.objective(model, x, y, t, p, center=center, reference_exact=False)
    assert f(truth) < f(start)
    res = opt.fmin_bfgs(f, start, fprime=g, disp=False)
    assert np.all(np.abs(res - truth) <= M8.TOL[model]), (res, truth)
