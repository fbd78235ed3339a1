"""GPU (-m gpu): pure_rotation_warp and xyztheta_warp -- warp(), the fused IWE (LDS band and direct kernels), the variance
objective and the other objectives' gradients over 3 / 4 derivative planes, the reduction of xyztheta to the linear flow,
optimize_contrast on the synthetic scenes and a 10 M-event evaluation, all against tests/_motion_models_np.py."""
import numpy as np
import pytest
import scipy.optimize as opt
import torch

import _motion_models_np as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import event_utils_amd as E
    assert torch.cuda.is_available()
    return E


def warp_of(E, model, center=(0.0, 0.0)):
    return E.pure_rotation_warp() if model == M.ROTATION else E.xyztheta_warp(center=center)


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
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(got - ref).max()
    assert err <= tol * scale, (err, scale)


POINTS = {M.ROTATION: [(120.0, 90.0, 0.0), (110.0, 95.0, 1.5), (60.0, 150.0, -40.0)],      # omega 0, moderate, large
          M.XYZTHETA: [(0.0, 0.0, 0.0, 0.0), (40.0, -25.0, 2.0, 1.0), (-300.0, 200.0, -8.0, 30.0)]}
CENTER = {M.ROTATION: (0.0, 0.0), M.XYZTHETA: (120.0, 90.0)}


# ---- warp() ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", [M.ROTATION, M.XYZTHETA])
@pytest.mark.parametrize("on_device", [False, True])
def test_warp_matches_the_helper(E, model, on_device):
    x, y, t, _ = events(5000, seed=3)
    w = warp_of(E, model, CENTER[model])
    for q in POINTS[model]:
        args = [torch.from_numpy(a).cuda() for a in (x, y, t)] if on_device else [x, y, t]
        xo, yo, jx, jy = w.warp(*args, None, t[-1], q, compute_grad=True)
        if on_device:
            assert xo.is_cuda and jx.is_cuda
            xo, yo, jx, jy = (a.cpu().numpy() for a in (xo, yo, jx, jy))
        assert jx.shape == jy.shape == (w.dims, len(x))
        rx, ry, rjx, rjy = M.warp(model, x, y, t, t[-1], q, CENTER[model])
        for g, r in ((xo, rx), (yo, ry), (jx, rjx), (jy, rjy)):
            np.testing.assert_allclose(g, r, rtol=1e-12, atol=1e-12 * max(1.0, np.abs(r).max()))
        xo2, yo2, jx2, jy2 = w.warp(x, y, t, None, t[-1], q)
        assert jx2 is None and jy2 is None


# ---- get_iwe ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", [M.ROTATION, M.XYZTHETA])
@pytest.mark.parametrize("use_polarity", [True, False])
@pytest.mark.parametrize("kind", ["numpy", "device_f32", "device_f64"])
def test_get_iwe_matches_the_helper(E, model, use_polarity, kind):
    x, y, t, p = events(30000, seed=4)
    if kind == "device_f32":
        x, y, t = (np.float32(a).astype(np.float64) for a in (x, y, t))
    w = warp_of(E, model, CENTER[model])
    for q in POINTS[model]:
        if kind == "numpy":
            src = (x, y, t, p)
        else:
            ev = E.DeviceEvents.from_arrays(x, y, t, p, precision="f32" if kind == "device_f32" else "f64")
            src = (ev, None, None, None)
        iwe, d_iwe = E.get_iwe(q, *src, w, (180, 240), compute_gradient=True, use_polarity=use_polarity)
        ri, rd = M.iwe(model, q, x, y, t, p, use_polarity=use_polarity, center=CENTER[model])
        assert iwe.shape == (181, 241) and d_iwe.shape == (w.dims, 181, 241)
        close(iwe, ri)
        close(d_iwe, rd)
        only, none = E.get_iwe(q, *src, w, (180, 240), compute_gradient=False, use_polarity=use_polarity)
        assert none is None
        close(only, ri)


@pytest.mark.parametrize("model", [M.ROTATION, M.XYZTHETA])
def test_get_iwe_sensor_size_return_events_and_tiny_inputs(E, model):
    w = warp_of(E, model, CENTER[model])
    q = POINTS[model][1]
    x, y, t, p = events(40000, seed=5, hi_x=660.0, hi_y=500.0)
    iwe, d_iwe = E.get_iwe(q, x, y, t, p, w, (480, 640), compute_gradient=True, sensor_size=(480, 640))
    ri, rd = M.iwe(model, q, x, y, t, p, img_size=(480, 640), sensor_size=(480, 640), center=CENTER[model])
    assert d_iwe.shape == (w.dims, 481, 641)
    close(iwe, ri)
    close(d_iwe, rd)
    # return_events: the image has `dims` planes on this branch too, the events are warp() * mask
    iwe2, d2, (xw, yw) = E.get_iwe(q, x[:5000], y[:5000], t[:5000], p[:5000], w, (180, 240), compute_gradient=True,
                                   return_events=True)
    ri, rd = M.iwe(model, q, x[:5000], y[:5000], t[:5000], p[:5000], center=CENTER[model])
    close(iwe2, ri)
    close(d2, rd)
    rx, ry, _, _ = M.warp(model, x[:5000], y[:5000], t[:5000], t[4999], q, CENTER[model])
    keep = (rx > 0) & (rx <= 240) & (ry > 0) & (ry <= 180)
    np.testing.assert_allclose(xw, rx * keep, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(yw, ry * keep, rtol=1e-12, atol=1e-9)
    # n = 0 and n = 1
    for n in (0, 1):
        xs, ys, ts, ps = (np.array([110.3]), np.array([80.7]), np.array([0.05]), np.array([1.0]))
        xs, ys, ts, ps = xs[:n], ys[:n], ts[:n], ps[:n]
        ev = E.DeviceEvents.from_arrays(xs, ys, ts, ps, precision="f32")
        iwe, d_iwe = E.get_iwe(q, ev, None, None, None, w, (180, 240), compute_gradient=True)
        ri, rd = M.iwe(model, q, xs, ys, ts, ps, center=CENTER[model])
        assert d_iwe.shape == (w.dims, 181, 241)
        assert np.allclose(iwe, ri, atol=1e-6) and np.allclose(d_iwe, rd, atol=1e-6)
        assert (np.abs(iwe).sum() > 0) == (n == 1)


@pytest.mark.parametrize("model", [M.ROTATION, M.XYZTHETA])
def test_band_and_direct_kernels_agree(E, model, monkeypatch):
    from event_utils_amd import _lib
    w = warp_of(E, model, CENTER[model])
    q = POINTS[model][1]
    x, y, t, p = events(200000, seed=6)
    ev = E.DeviceEvents.from_arrays(x, y, t, p, precision="f32")
    band = E.get_iwe(q, ev, None, None, None, w, (180, 240), compute_gradient=True)
    monkeypatch.setenv("EVK_IMPL", "direct")
    direct = E.get_iwe(q, ev, None, None, None, w, (180, 240), compute_gradient=True)
    monkeypatch.delenv("EVK_IMPL")
    for a, b in zip(band, direct):
        close(a, b, 1e-5)
    # a canvas too wide for one band row of 1 + dims planes: the direct kernel runs without being asked
    ss = (40, 12000)
    assert _lib.lib().evk_iwe_param_band_rows(w.fused_model, _lib.EVK_IWE_GRADIENT, ss[0] + 1, ss[1] + 1) == 0
    assert _lib.lib().evk_iwe_param_band_rows(w.fused_model, 0, ss[0] + 1, ss[1] + 1) > 0
    rng = np.random.default_rng(7)
    xw, yw = rng.uniform(0, ss[1], 50000), rng.uniform(0, ss[0], 50000)
    tw = np.sort(rng.uniform(0, 0.01, 50000))
    pw = np.ones(50000)
    qw = (6000.0, 20.0, 0.3) if model == M.ROTATION else (50.0, 10.0, 0.0, 0.0)
    cw = (0.0, 0.0) if model == M.ROTATION else (6000.0, 20.0)
    ww = warp_of(E, model, cw)
    for grad in (True, False):
        iwe, d_iwe = E.get_iwe(qw, xw, yw, tw, pw, ww, ss, compute_gradient=grad, sensor_size=ss)
        ri, rd = M.iwe(model, qw, xw, yw, tw, pw, img_size=ss, sensor_size=ss, center=cw, compute_gradient=grad)
        close(iwe, ri)
        if grad:
            close(d_iwe, rd)


def test_xyztheta_reduces_to_the_linear_flow(E):
    """xyztheta at (vx, vy, 0, 0) is the linear flow: IWE and d_iwe[:2] equal linvel's."""
    x, y, t, p = events(50000, seed=8)
    ev = E.DeviceEvents.from_arrays(x, y, t, p, precision="f32")
    for vx, vy in ((30.0, -20.0), (0.0, 0.0), (-150.0, 75.0)):
        i4, d4 = E.get_iwe((vx, vy, 0.0, 0.0), ev, None, None, None, E.xyztheta_warp(center=(120.0, 90.0)), (180, 240),
                           compute_gradient=True)
        i2, d2 = E.get_iwe((vx, vy), ev, None, None, None, E.linvel_warp(), (180, 240), compute_gradient=True)
        close(i4, i2, 1e-6)
        close(d4[:2], d2, 1e-6)


# ---- objectives ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", [M.ROTATION, M.XYZTHETA])
@pytest.mark.parametrize("reference_exact", [True, False])
@pytest.mark.parametrize("sigma", [0.0, 1.0, 9.0])
def test_variance_objective_matches_the_helper(E, model, reference_exact, sigma):
    x, y, t, p = M.scene(model, n=30000, seed=9)
    w = warp_of(E, model, CENTER[model])
    q = np.array(POINTS[model][1]) * 0.9
    o = E.variance_objective()
    o.reference_exact = reference_exact
    ev = E.DeviceEvents.from_arrays(x, y, t, p)
    ri, rd = M.iwe(model, q, x, y, t, p, center=CENTER[model])
    f_ref = M.variance_f(ri, sigma)
    g_ref = M.variance_grad(ri, rd, sigma, reference_exact)
    f = o.evaluate_function(q, ev, None, None, None, w, (180, 240), sigma)
    g = o.evaluate_gradient(q, ev, None, None, None, w, (180, 240), sigma)
    f2, g2 = o.evaluate_function_and_gradient(q, ev, None, None, None, w, (180, 240), sigma)
    assert g.shape == g2.shape == (w.dims,)
    np.testing.assert_allclose(f, f_ref, rtol=1e-4)
    np.testing.assert_allclose(f2, f_ref, rtol=1e-4)
    np.testing.assert_allclose(g, g_ref, rtol=1e-4, atol=1e-4 * np.abs(g_ref).max())
    np.testing.assert_allclose(g2, g_ref, rtol=1e-4, atol=1e-4 * np.abs(g_ref).max())
    # explicit images: d_iwe must have dims channels for these warps
    iwe, d_iwe = E.get_iwe(q, ev, None, None, None, w, (180, 240), compute_gradient=True)
    g3 = o.evaluate_gradient(iwe=iwe, d_iwe=d_iwe, blur_sigma=sigma, warpfunc=w)
    np.testing.assert_allclose(g3, g_ref, rtol=1e-4, atol=1e-4 * np.abs(g_ref).max())
    with pytest.raises(ValueError):
        o.evaluate_gradient(iwe=iwe, d_iwe=d_iwe[:2], blur_sigma=sigma, warpfunc=w)
    if sigma == 1.0:
        fn, gn = o.evaluate_function_and_numeric_gradient(q, ev, None, None, None, w, (180, 240), sigma)
        assert gn.shape == (w.dims,)
        for i in range(w.dims):
            qi = q.copy()
            qi[i] += 1.0
            fi = M.variance_f(M.iwe(model, qi, x, y, t, p, compute_gradient=False, center=CENTER[model])[0], sigma)
            np.testing.assert_allclose(gn[i], fi - f_ref, rtol=2e-3, atol=1e-4 * abs(f_ref))


@pytest.mark.parametrize("model", [M.ROTATION, M.XYZTHETA])
def test_other_objectives_gradients_have_dims_components(E, model):
    from event_utils_amd.contrast_max import objectives as O
    x, y, t, p = M.scene(model, n=30000, seed=10)
    w = warp_of(E, model, CENTER[model])
    q = np.array(POINTS[model][1]) * 0.9
    ev = E.DeviceEvents.from_arrays(x, y, t, p)
    cases = [  # objective, reference gradient from (img, d_img) of its polarity setting
        (O.sos_objective(), True, lambda i, d, s: -2.0 * M.gradsums(i, d, s, lambda a: a, False)[0] / i.size),
        (O.rms_objective(), True, lambda i, d, s: -2.0 * M.gradsums(i, d, s, lambda a: a, False)[0] / i.size),
        (O.soe_objective(), False, lambda i, d, s: -M.gradsums(i, d, s, np.exp, True)[0] / i.size),
        (O.isoa_objective(), False, lambda i, d, s: -M.gradsums(i, d, s, lambda a: (a > 0.5).astype(float), True)[0]),
        (O.sosa_objective(), False, lambda i, d, s: 3.0 * M.gradsums(
            i, d, s, lambda a: np.exp((-3.0 * a.astype(np.float32)).astype(np.float64)), True)[0]),
    ]
    for obj, pol, ref in cases:
        s = obj.default_blur
        ri, rd = M.iwe(model, q, x, y, t, p, use_polarity=pol, center=CENTER[model])
        g = np.asarray(obj.evaluate_gradient(q, ev, None, None, None, w, (180, 240), s), dtype=np.float64)
        gr = ref(ri, rd, s)
        assert g.shape == (w.dims,), obj.name
        # (isoa's step at 0.5 may flip a pixel or two between the float32 and the float64 blur)
        loose = 1e-2 if obj.name == "isoa" else 1e-3
        np.testing.assert_allclose(g, gr, rtol=1e-4, atol=loose * np.abs(gr).max() + 1e-12, err_msg=obj.name)


def test_sharded_evaluation_is_refused(E):
    o = E.variance_objective()
    o.distributed = True
    x, y, t, p = events(100, seed=11)
    with pytest.raises(NotImplementedError):
        o.evaluate_function((1.0, 2.0, 0.1), x, y, t, p, E.pure_rotation_warp(), (180, 240), 1.0)
    with pytest.raises(NotImplementedError):
        E.optimize_contrast(x, y, t, p, E.xyztheta_warp(), o, img_size=(180, 240))


# ---- optimisation ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", [M.ROTATION, M.XYZTHETA])
@pytest.mark.parametrize("optimizer", ["scipy", "evk_bfgs"])
def test_optimize_contrast_recovers_the_synthetic_scene(E, model, optimizer):
    x, y, t, p = M.scene(model)
    truth, start = (M.ROT_TRUTH, M.ROT_START) if model == M.ROTATION else (M.XYZ_TRUTH, M.XYZ_START)
    w = warp_of(E, model, CENTER[model])
    o = E.variance_objective()
    o.reference_exact = False
    kw = {} if optimizer == "scipy" else {"optimizer": "evk_bfgs"}
    res = E.optimize_contrast(x, y, t, p, w, o, x0=start.copy(), numeric_grads=False, blur_sigma=1.0, img_size=(180, 240), **kw)
    assert np.all(np.abs(np.asarray(res) - truth) <= M.TOL[model]), (res, truth)


def test_pure_rotation_from_default_params(E):
    x, y, t, p = M.scene(M.ROTATION)
    o = E.variance_objective()
    o.reference_exact = False
    res = E.optimize_contrast(x, y, t, p, E.pure_rotation_warp(), o, numeric_grads=False, blur_sigma=1.0, img_size=(180, 240))
    assert np.all(np.abs(np.asarray(res) - M.ROT_TRUTH) <= M.TOL[M.ROTATION]), res


# ---- size ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model", [M.ROTATION, M.XYZTHETA])
def test_ten_million_events(E, model):
    n = 10_000_000
    rng = np.random.default_rng(12)
    x, y = rng.uniform(0, 240, n).astype(np.float32), rng.uniform(0, 180, n).astype(np.float32)
    t = np.sort(rng.uniform(0, 0.1, n)).astype(np.float32)
    p = (rng.integers(0, 2, n) * 2 - 1).astype(np.float32)
    w = warp_of(E, model, CENTER[model])
    q = POINTS[model][1]
    ev = E.DeviceEvents.from_arrays(x, y, t, p, precision="f32")
    o = E.variance_objective()
    o.reference_exact = False
    f, g = o.evaluate_function_and_gradient(q, ev, None, None, None, w, (180, 240), 1.0)
    ri, rd = M.iwe(model, q, x, y, t, p, center=CENTER[model])
    np.testing.assert_allclose(f, M.variance_f(ri, 1.0), rtol=1e-4)
    gr = M.variance_grad(ri, rd, 1.0, False)
    np.testing.assert_allclose(g, gr, rtol=1e-4, atol=1e-4 * np.abs(gr).max())
