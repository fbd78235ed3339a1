"""GPU (-m gpu): angular_velocity_warp and planar_flow_warp -- warp(), the fused IWE (LDS band and direct kernels, up to 9
planes), the variance objective and the other objectives' gradients over 3 / 8 derivative planes, the special cases (planar
flow as xyztheta and linvel, angular velocity as pure rotation), events behind the camera, optimize_contrast on the synthetic
scenes and a 10 M-event evaluation, all against tests/_motion_models8_np.py."""
import numpy as np
import pytest
import torch

import _motion_models8_np as M8

pytestmark = pytest.mark.gpu

MODELS = [M8.ANGVEL, M8.PLANAR]
K = M8.K_DEFAULT
CENTER = {M8.ANGVEL: (0.0, 0.0), M8.PLANAR: M8.PF_CENTER}
POINTS = {M8.ANGVEL: [(0.0, 0.0, 0.0), (0.8, -0.6, 1.2), (-4.0, 3.0, 25.0)],        # zero, moderate, large
          M8.PLANAR: [np.zeros(8), M8.PF_TRUTH, np.array([-300.0, 1.2, -0.7, 200.0, -0.9, 0.4, -4e-3, 6e-3])]}


@pytest.fixture(scope="module")
def E():
    import event_utils_amd as E
    assert torch.cuda.is_available()
    return E


def warp_of(E, model, center=None):
    if model == M8.ANGVEL:
        return E.angular_velocity_warp(K)
    return E.planar_flow_warp(center=CENTER[model] if center is None else center)


def events(n, seed=0, lo=-20.0, hi_x=260.0, hi_y=200.0, duration=0.1):
    """Random events, a part of them out of the image before and after warping; +-1 polarities."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(lo, hi_x, n), rng.uniform(lo, hi_y, n)
    t = np.sort(rng.uniform(0.0, duration, n))
    p = (rng.integers(0, 2, n) * 2 - 1).astype(np.float64)
    return x, y, t, p


def close(got, ref, tol=1e-5):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all()
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(got - ref).max()
    assert err <= tol * scale, (err, scale)


# ---- warp() ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("on_device", [False, True])
def test_warp_matches_the_helper(E, model, on_device):
    x, y, t, _ = events(5000, seed=3)
    w = warp_of(E, model)
    for q in POINTS[model] + ([(0.0, 2.2, 0.0)] if model == M8.ANGVEL else []):
        tt = t * 10.0 if model == M8.ANGVEL and q[1] == 2.2 else t          # (1 s: a part of the events turns behind)
        args = [torch.from_numpy(a).cuda() for a in (x, y, tt)] if on_device else [x, y, tt]
        xo, yo, jx, jy = w.warp(*args, None, tt[-1], q, compute_grad=True)
        if on_device:
            assert xo.is_cuda and jx.is_cuda
            xo, yo, jx, jy = (a.cpu().numpy() for a in (xo, yo, jx, jy))
        assert jx.shape == jy.shape == (w.dims, len(x))
        rx, ry, rjx, rjy = M8.warp(model, x, y, tt, tt[-1], q, CENTER[model])
        for g, r in ((xo, rx), (yo, ry), (jx, rjx), (jy, rjy)):
            assert np.array_equal(np.isnan(g), np.isnan(r))
            ok = np.isfinite(r)
            np.testing.assert_allclose(g[ok], r[ok], rtol=1e-10, atol=1e-10 * max(1.0, np.abs(r[ok]).max()))
        xo2, yo2, jx2, jy2 = w.warp(x, y, tt, None, tt[-1], q)
        assert jx2 is None and jy2 is None


# ---- get_iwe ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("use_polarity", [True, False])
@pytest.mark.parametrize("kind", ["numpy", "device_f32", "device_f64"])
def test_get_iwe_matches_the_helper(E, model, use_polarity, kind):
    x, y, t, p = events(30000, seed=4)
    if kind == "device_f32":
        x, y, t = (np.float32(a).astype(np.float64) for a in (x, y, t))
    w = warp_of(E, model)
    for q in POINTS[model]:
        if kind == "numpy":
            src = (x, y, t, p)
        else:
            ev = E.DeviceEvents.from_arrays(x, y, t, p, precision="f32" if kind == "device_f32" else "f64")
            src = (ev, None, None, None)
        iwe, d_iwe = E.get_iwe(q, *src, w, (180, 240), compute_gradient=True, use_polarity=use_polarity)
        ri, rd = M8.iwe(model, q, x, y, t, p, use_polarity=use_polarity, center=CENTER[model])
        assert iwe.shape == (181, 241) and d_iwe.shape == (w.dims, 181, 241)
        close(iwe, ri)
        close(d_iwe, rd)
        only, none = E.get_iwe(q, *src, w, (180, 240), compute_gradient=False, use_polarity=use_polarity)
        assert none is None
        close(only, ri)


@pytest.mark.parametrize("model", MODELS)
def test_get_iwe_sensor_size_return_events_and_tiny_inputs(E, model):
    w = warp_of(E, model)
    q = POINTS[model][1]
    x, y, t, p = events(40000, seed=5, hi_x=660.0, hi_y=500.0)
    iwe, d_iwe = E.get_iwe(q, x, y, t, p, w, (480, 640), compute_gradient=True, sensor_size=(480, 640))
    ri, rd = M8.iwe(model, q, x, y, t, p, img_size=(480, 640), sensor_size=(480, 640), center=CENTER[model])
    assert d_iwe.shape == (w.dims, 481, 641)
    close(iwe, ri)
    close(d_iwe, rd)
    iwe2, d2, (xw, yw) = E.get_iwe(q, x[:5000], y[:5000], t[:5000], p[:5000], w, (180, 240), compute_gradient=True,
                                   return_events=True)
    ri, rd = M8.iwe(model, q, x[:5000], y[:5000], t[:5000], p[:5000], center=CENTER[model])
    close(iwe2, ri)
    close(d2, rd)
    rx, ry, _, _ = M8.warp(model, x[:5000], y[:5000], t[:5000], t[4999], q, CENTER[model])
    keep = (rx > 0) & (rx <= 240) & (ry > 0) & (ry <= 180)
    np.testing.assert_allclose(xw, np.where(keep, rx, 0.0), rtol=1e-10, atol=1e-9)
    np.testing.assert_allclose(yw, np.where(keep, ry, 0.0), rtol=1e-10, atol=1e-9)
    for n in (0, 1):
        xs, ys, ts, ps = (np.array([110.3]), np.array([80.7]), np.array([0.05]), np.array([1.0]))
        xs, ys, ts, ps = xs[:n], ys[:n], ts[:n], ps[:n]
        ev = E.DeviceEvents.from_arrays(xs, ys, ts, ps, precision="f32")
        iwe, d_iwe = E.get_iwe(q, ev, None, None, None, w, (180, 240), compute_gradient=True)
        ri, rd = M8.iwe(model, q, xs, ys, ts, ps, center=CENTER[model])
        assert d_iwe.shape == (w.dims, 181, 241)
        assert np.allclose(iwe, ri, atol=1e-6) and np.allclose(d_iwe, rd, atol=1e-6)
        assert (np.abs(iwe).sum() > 0) == (n == 1)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_band_and_direct_kernels_agree(E, model, precision, monkeypatch):
    from event_utils_amd import _lib
    w = warp_of(E, model)
    q = POINTS[model][1]
    for ss in ((180, 240), (480, 640)):
        x, y, t, p = events(200000, seed=6, hi_x=ss[1] + 20.0, hi_y=ss[0] + 20.0)
        if precision == "f32":
            x, y, t = (np.float32(a).astype(np.float64) for a in (x, y, t))
        assert _lib.lib().evk_iwe_param_band_rows(w.fused_model, _lib.EVK_IWE_GRADIENT, ss[0] + 1, ss[1] + 1) > 0
        ev = E.DeviceEvents.from_arrays(x, y, t, p, precision=precision)
        band = E.get_iwe(q, ev, None, None, None, w, ss, compute_gradient=True, sensor_size=ss)
        monkeypatch.setenv("EVK_IMPL", "direct")
        direct = E.get_iwe(q, ev, None, None, None, w, ss, compute_gradient=True, sensor_size=ss)
        monkeypatch.delenv("EVK_IMPL")
        for a, b in zip(band, direct):
            close(a, b, 1e-5)
        ri, rd = M8.iwe(model, q, x, y, t, p, img_size=ss, sensor_size=ss, center=CENTER[model])
        close(band[0], ri)
        close(band[1], rd)
    # a canvas too wide for one band row of 1 + dims planes: the direct kernel runs without being asked
    ss = (40, 12000)
    assert _lib.lib().evk_iwe_param_band_rows(w.fused_model, _lib.EVK_IWE_GRADIENT, ss[0] + 1, ss[1] + 1) == 0
    rng = np.random.default_rng(7)
    xw, yw = rng.uniform(0, ss[1], 50000), rng.uniform(0, ss[0], 50000)
    tw = np.sort(rng.uniform(0, 0.01, 50000))
    pw = np.ones(50000)
    for grad in (True, False):
        iwe, d_iwe = E.get_iwe(q, xw, yw, tw, pw, w, ss, compute_gradient=grad, sensor_size=ss)
        ri, rd = M8.iwe(model, q, xw, yw, tw, pw, img_size=ss, sensor_size=ss, center=CENTER[model], compute_gradient=grad)
        close(iwe, ri)
        if grad:
            close(d_iwe, rd)


def test_planar_flow_equals_xyztheta_and_linvel(E):
    """planar_flow_warp at the mapped parameters gives xyztheta's and linvel's images and gradients."""
    x, y, t, p = events(50000, seed=8)
    ev = E.DeviceEvents.from_arrays(x, y, t, p, precision="f32")
    c = (120.0, 90.0)
    pf = E.planar_flow_warp(center=c)
    o = E.variance_objective()
    o.reference_exact = False
    for q in ((40.0, -25.0, 2.0, 1.0), (-150.0, 75.0, -3.0, 5.0), (0.0, 0.0, 0.0, 0.0)):
        qp = M8.xyztheta_as_planar(q)
        i8, d8 = E.get_iwe(qp, ev, None, None, None, pf, (180, 240), compute_gradient=True)
        i4, d4 = E.get_iwe(q, ev, None, None, None, E.xyztheta_warp(center=c), (180, 240), compute_gradient=True)
        close(i8, i4, 1e-5)
        # chain rule: d/dvx = d/da1, d/dvy = d/da4, d/dvz = d/da2 + d/da6, d/dw = -d/da3 + d/da5
        close(np.stack([d8[0], d8[3], d8[1] + d8[5], -d8[2] + d8[4]]), d4, 1e-5)
        f8, g8 = o.evaluate_function_and_gradient(qp, ev, None, None, None, pf, (180, 240), 1.0)
        f4, g4 = o.evaluate_function_and_gradient(q, ev, None, None, None, E.xyztheta_warp(center=c), (180, 240), 1.0)
        np.testing.assert_allclose(f8, f4, rtol=1e-5)
        g8m = np.array([g8[0], g8[3], g8[1] + g8[5], -g8[2] + g8[4]])
        np.testing.assert_allclose(g8m, g4, rtol=1e-4, atol=1e-4 * np.abs(g4).max())
    for q in ((30.0, -20.0), (-150.0, 75.0)):
        i8, d8 = E.get_iwe(M8.linvel_as_planar(q), ev, None, None, None, pf, (180, 240), compute_gradient=True)
        i2, d2 = E.get_iwe(q, ev, None, None, None, E.linvel_warp(), (180, 240), compute_gradient=True)
        close(i8, i2, 1e-6)
        close(np.stack([d8[0], d8[3]]), d2, 1e-6)


def test_angular_velocity_about_z_equals_pure_rotation(E):
    x, y, t, p = events(50000, seed=9)
    ev = E.DeviceEvents.from_arrays(x, y, t, p, precision="f32")
    av = E.angular_velocity_warp(K)
    for wz in (0.0, 1.5, -20.0):
        ia, da = E.get_iwe((0.0, 0.0, wz), ev, None, None, None, av, (180, 240), compute_gradient=True)
        ir, dr = E.get_iwe((K[0, 2], K[1, 2], -wz), ev, None, None, None, E.pure_rotation_warp(), (180, 240),
                           compute_gradient=True)
        close(ia, ir, 1e-5)
        close(da[2], -dr[2], 1e-5)


def test_events_behind_the_camera_are_dropped(E):
    """About y at 2.2 rad/s over 1 s, the events on one side turn behind the camera: no NaN in any image, and the image is
    the helper's (which drops them)."""
    x, y, t, p = events(100000, seed=10, duration=1.0)
    x, y, t = (np.float32(a).astype(np.float64) for a in (x, y, t))
    av = E.angular_velocity_warp(K)
    q = (0.0, 2.2, 0.0)
    xw, _, _, _ = av.warp(x, y, t, None, t[-1], q)
    assert np.isnan(xw).sum() > 1000
    for precision in ("f32", "f64"):
        ev = E.DeviceEvents.from_arrays(x, y, t, p, precision=precision)
        for impl in ("auto", "direct"):
            from event_utils_amd.contrast_max import objectives as O
            iwe, d_iwe = O.iwe_param_device(q, ev, av, (180, 240), True, True, None, impl)
            iwe, d_iwe = iwe.cpu().numpy(), d_iwe.cpu().numpy()
            assert np.isfinite(iwe).all() and np.isfinite(d_iwe).all()
            ri, rd = M8.iwe(M8.ANGVEL, q, x, y, t, p)
            close(iwe, ri, 1e-4)
            close(d_iwe, rd, 1e-4)
    o = E.variance_objective()
    f, g = o.evaluate_function_and_gradient(q, x, y, t, p, av, (180, 240), 1.0)
    assert np.isfinite(f) and np.isfinite(g).all()
    _, _, (xe, ye) = E.get_iwe(q, x, y, t, p, av, (180, 240), return_events=True)
    assert np.isfinite(xe).all() and np.isfinite(ye).all()
    assert not xe[np.isnan(xw)].any() and not ye[np.isnan(xw)].any()


# ---- objectives ----------------------------------------------------------------------------------------------------------

def _scene_point(model):
    truth = M8.AV_TRUTH if model == M8.ANGVEL else M8.PF_TRUTH
    return np.array(truth) * 0.9


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("reference_exact", [True, False])
@pytest.mark.parametrize("sigma", [0.0, 1.0, 9.0])
def test_variance_objective_matches_the_helper(E, model, reference_exact, sigma):
    x, y, t, p = M8.scene(model, n=30000, seed=9)
    w = warp_of(E, model)
    q = _scene_point(model)
    o = E.variance_objective()
    o.reference_exact = reference_exact
    ev = E.DeviceEvents.from_arrays(x, y, t, p)
    ri, rd = M8.iwe(model, q, x, y, t, p, center=CENTER[model])
    f_ref = M8.variance_f(ri, sigma)
    g_ref = M8.variance_grad(ri, rd, sigma, reference_exact)
    f = o.evaluate_function(q, ev, None, None, None, w, (180, 240), sigma)
    g = o.evaluate_gradient(q, ev, None, None, None, w, (180, 240), sigma)
    f2, g2 = o.evaluate_function_and_gradient(q, ev, None, None, None, w, (180, 240), sigma)
    assert g.shape == g2.shape == (w.dims,)
    np.testing.assert_allclose(f, f_ref, rtol=1e-4)
    np.testing.assert_allclose(f2, f_ref, rtol=1e-4)
    np.testing.assert_allclose(g, g_ref, rtol=1e-4, atol=1e-4 * np.abs(g_ref).max())
    np.testing.assert_allclose(g2, g_ref, rtol=1e-4, atol=1e-4 * np.abs(g_ref).max())
    iwe, d_iwe = E.get_iwe(q, ev, None, None, None, w, (180, 240), compute_gradient=True)
    g3 = o.evaluate_gradient(iwe=iwe, d_iwe=d_iwe, blur_sigma=sigma, warpfunc=w)
    np.testing.assert_allclose(g3, g_ref, rtol=1e-4, atol=1e-4 * np.abs(g_ref).max())
    with pytest.raises(ValueError):
        o.evaluate_gradient(iwe=iwe, d_iwe=d_iwe[:2], blur_sigma=sigma, warpfunc=w)
    if sigma == 1.0:
        fb = o.evaluate_function_batch([q, q * 1.05, q * 0.95], ev, None, None, None, w, (180, 240), sigma)
        for qq, fv in zip((q, q * 1.05, q * 0.95), fb):
            fr = M8.variance_f(M8.iwe(model, qq, x, y, t, p, compute_gradient=False, center=CENTER[model])[0], sigma)
            np.testing.assert_allclose(fv, fr, rtol=1e-4)


@pytest.mark.parametrize("model", MODELS)
def test_other_objectives_gradients_have_dims_components(E, model):
    from event_utils_amd.contrast_max import objectives as O
    x, y, t, p = M8.scene(model, n=30000, seed=10)
    w = warp_of(E, model)
    q = _scene_point(model)
    ev = E.DeviceEvents.from_arrays(x, y, t, p)
    cases = [
        (O.sos_objective(), True, lambda i, d, s: -2.0 * M8.gradsums(i, d, s, lambda a: a, False)[0] / i.size),
        (O.rms_objective(), True, lambda i, d, s: -2.0 * M8.gradsums(i, d, s, lambda a: a, False)[0] / i.size),
        (O.soe_objective(), False, lambda i, d, s: -M8.gradsums(i, d, s, np.exp, True)[0] / i.size),
        (O.isoa_objective(), False, lambda i, d, s: -M8.gradsums(i, d, s, lambda a: (a > 0.5).astype(float), True)[0]),
        (O.sosa_objective(), False, lambda i, d, s: 3.0 * M8.gradsums(
            i, d, s, lambda a: np.exp((-3.0 * a.astype(np.float32)).astype(np.float64)), True)[0]),
    ]
    for obj, pol, ref in cases:
        s = obj.default_blur
        ri, rd = M8.iwe(model, q, x, y, t, p, use_polarity=pol, center=CENTER[model])
        g = np.asarray(obj.evaluate_gradient(q, ev, None, None, None, w, (180, 240), s), dtype=np.float64)
        gr = ref(ri, rd, s)
        assert g.shape == (w.dims,), obj.name
        loose = 1e-2 if obj.name == "isoa" else 1e-3
        np.testing.assert_allclose(g, gr, rtol=1e-4, atol=loose * np.abs(gr).max() + 1e-12, err_msg=obj.name)


def test_sharded_evaluation_is_refused(E):
    o = E.variance_objective()
    o.distributed = True
    x, y, t, p = events(100, seed=11)
    with pytest.raises(NotImplementedError):
        o.evaluate_function((0.1, 0.2, 0.3), x, y, t, p, E.angular_velocity_warp(K), (180, 240), 1.0)
    with pytest.raises(NotImplementedError):
        E.optimize_contrast(x, y, t, p, E.planar_flow_warp(), o, img_size=(180, 240))


# ---- optimisation ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("optimizer", ["scipy", "evk_bfgs"])
def test_optimize_contrast_recovers_the_synthetic_scene(E, model, optimizer):
    x, y, t, p = M8.scene(model)
    truth, start = (M8.AV_TRUTH, M8.AV_START) if model == M8.ANGVEL else (M8.PF_TRUTH, M8.PF_START)
    w = warp_of(E, model)
    o = E.variance_objective()
    o.reference_exact = False
    kw = {} if optimizer == "scipy" else {"optimizer": "evk_bfgs"}
    res = E.optimize_contrast(x, y, t, p, w, o, x0=start.copy(), numeric_grads=False, blur_sigma=1.0, img_size=(180, 240), **kw)
    assert np.all(np.abs(np.asarray(res) - truth) <= M8.TOL[model]), (res, truth)


def test_angular_velocity_from_default_params(E):
    x, y, t, p = M8.scene(M8.ANGVEL)
    o = E.variance_objective()
    o.reference_exact = False
    res = E.optimize_contrast(x, y, t, p, E.angular_velocity_warp(K), o, numeric_grads=False, blur_sigma=1.0,
                              img_size=(180, 240))
    assert np.all(np.abs(np.asarray(res) - M8.AV_TRUTH) <= M8.TOL[M8.ANGVEL]), res


# ---- size ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", MODELS)
def test_ten_million_events(E, model):
    n = 10_000_000
    rng = np.random.default_rng(12)
    x, y = rng.uniform(0, 240, n).astype(np.float32), rng.uniform(0, 180, n).astype(np.float32)
    t = np.sort(rng.uniform(0, 0.1, n)).astype(np.float32)
    p = (rng.integers(0, 2, n) * 2 - 1).astype(np.float32)
    w = warp_of(E, model)
    q = POINTS[model][1]
    ev = E.DeviceEvents.from_arrays(x, y, t, p, precision="f32")
    o = E.variance_objective()
    o.reference_exact = False
    f, g = o.evaluate_function_and_gradient(q, ev, None, None, None, w, (180, 240), 1.0)
    ri, rd = M8.iwe(model, q, x, y, t, p, center=CENTER[model])
    np.testing.assert_allclose(f, M8.variance_f(ri, 1.0), rtol=1e-4)
    gr = M8.variance_grad(ri, rd, 1.0, False)
    np.testing.assert_allclose(g, gr, rtol=1e-4, atol=1e-4 * np.abs(gr).max())
