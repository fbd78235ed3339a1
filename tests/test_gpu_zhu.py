"""GPU: the average-timestamp (Zhu) objective against its float64 numpy restatement (tests/_zhu_np.py, pinned to the
reference's timestamp images by tests/test_cpu_zhu.py).  Tolerances are those tests/test_gpu_motion_models.py uses for float32
images against a float64 restatement: planes and images atol = 1e-6 x the plane's maximum, loss rtol = 1e-4, gradient
rtol = 1e-4 with atol = 1e-4 max|g_ref|."""
import numpy as np
import pytest
import scipy.optimize as opt
import torch

import _motion_models8_np as M8
import _zhu_np as Z

pytestmark = pytest.mark.gpu

IMG = (180, 240)


def _warp(model):
    import event_utils_amd as E
    return {Z.LINVEL: lambda: E.linvel_warp(), Z.ROTATION: lambda: E.pure_rotation_warp(),
            Z.XYZTHETA: lambda: E.xyztheta_warp(center=Z.CENTER[Z.XYZTHETA]),
            Z.ANGVEL: lambda: E.angular_velocity_warp(M8.K_DEFAULT),
            Z.PLANAR: lambda: E.planar_flow_warp(center=Z.CENTER[Z.PLANAR])}[model]()


def _f32(cols):
    return tuple(np.asarray(a, dtype=np.float32) for a in cols)


def _scene_partly_outside(model, n=6000):
    """The model's scene with a tenth of its events moved across the image borders (dropped by the mask)."""
    x, y, t, p = Z.scene(model, n=n)
    x, y = x.copy(), y.copy()
    x[::20] += 200.0
    y[7::20] -= 170.0
    return x, y, t, p


def _close_planes(got, ref):
    got = got.cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape
    for c in range(ref.shape[0]):
        np.testing.assert_allclose(got[c], ref[c], rtol=0, atol=1e-6 * max(np.abs(ref[c]).max(), 1e-30), err_msg="plane %d" % c)


def _close_grad(g, ref):
    np.testing.assert_allclose(np.asarray(g, dtype=np.float64), ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


# ---- the images --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", Z.MODELS)
def test_timestamp_images_match_the_restatement(model):
    """numpy (float64 and float32 columns), tensor and DeviceEvents inputs and a misaligned slice, events partly out of bounds."""
    import event_utils_amd as E
    from event_utils_amd.contrast_max import objectives as O
    warp, q = _warp(model), Z.START[model]
    kw = dict(img_size=IMG, center=Z.CENTER[model], f32_coords=True)
    cols64 = _scene_partly_outside(model)
    cols32 = _f32(cols64)
    assert not Z.mask(model, q, *cols32, img_size=IMG, center=Z.CENTER[model]).all()
    ref64, ref32 = Z.images(model, q, *cols64, **kw), Z.images(model, q, *cols32, **kw)
    out = E.get_timestamp_images(q, *cols64, warp, IMG)
    assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (2, 181, 241)
    _close_planes(out, ref64)                                                                   # float64 columns
    _close_planes(E.get_timestamp_images(q, *cols32, warp, IMG), ref32)                         # float32 columns
    tens = tuple(torch.from_numpy(a).cuda() for a in cols32)
    _close_planes(E.get_timestamp_images(q, *tens, warp, IMG), ref32)
    ev = E.DeviceEvents.from_arrays(*cols32)
    assert ev.dtype == torch.float32
    _close_planes(E.get_timestamp_images(q, ev, None, None, None, warp, IMG), ref32)
    _close_planes(O.timestamp_planes_device(q, ev, warp, IMG, sensor_size=IMG), Z.planes(model, q, *cols32, **kw))
    n = len(ev)
    part = ev.slice(1, n - 4)                                                                   # columns off 16-byte alignment
    assert part.x.data_ptr() % 16 != 0
    _close_planes(E.get_timestamp_images(q, part, None, None, None, warp, IMG),
                  Z.images(model, q, *(a[1:n - 4] for a in cols32), **kw))


def test_angular_velocity_events_behind_the_camera_are_dropped():
    import event_utils_amd as E
    x, y, t, p = _f32(Z.scene(Z.ANGVEL, n=4000, duration=1.0))
    w = np.array([0.0, 3.0, 0.0])
    xw = Z.warp(Z.ANGVEL, x, y, t, float(t[-1]), w)[0]
    assert np.isnan(xw).any()
    out = E.get_timestamp_images(w, x, y, t, p, _warp(Z.ANGVEL), IMG)
    assert bool(torch.isfinite(out).all())
    _close_planes(out, Z.images(Z.ANGVEL, w, x, y, t, p, img_size=IMG, f32_coords=True))


@pytest.mark.parametrize("case", ["positive", "negative", "empty", "one"])
def test_one_sided_and_tiny_streams(case):
    import event_utils_amd as E
    x, y, t, p = _f32(Z.scene(Z.LINVEL, n=3000))
    if case == "positive":
        p = np.ones_like(p)
    elif case == "negative":
        p = -np.ones_like(p)
    elif case == "empty":
        x, y, t, p = (a[:0] for a in (x, y, t, p))
    else:
        x, y, t, p = (a[:1] for a in (x, y, t, p))
    q = Z.LV_START
    out = E.get_timestamp_images(q, x, y, t, p, E.linvel_warp(), IMG)
    _close_planes(out, Z.images(Z.LINVEL, q, x, y, t, p, img_size=IMG, f32_coords=True))
    if case == "positive":
        assert float(out[1].abs().max()) == 0.0 and float(out[0].max()) > 0.0
    if case == "negative":
        assert float(out[0].abs().max()) == 0.0 and float(out[1].max()) > 0.0
    obj = E.zhu_timestamp_objective()
    f, g = obj.evaluate_function_and_gradient(q, x, y, t, p, E.linvel_warp(), IMG)
    assert f == pytest.approx(Z.loss(Z.LINVEL, q, x, y, t, p, img_size=IMG, f32_coords=True), rel=1e-4, abs=1e-12)
    assert g.shape == (2,) and np.all(np.isfinite(g))
    if case == "empty":
        assert f == 0.0 and not g.any()


@pytest.mark.parametrize("route", ["fused", "plugin"])
@pytest.mark.parametrize("factor", [100.0, 0.5, -1.0, 0.0])
def test_scaled_events_are_classified_by_the_scaled_polarity(route, factor):
    """DeviceEvents.scaled(f) behaves exactly like columns holding p f, as in get_iwe: f < 0 swaps the two classes (zeros stay
    non-positive), f = 0 puts every event into the non-positive class; images, loss and gradient, bit for bit."""
    import event_utils_amd as E
    x, y, t, p = _f32(_scene_partly_outside(Z.LINVEL))
    p = p.copy()
    p[::7] = 0.0
    p[3::11] *= 2.0
    warp = _plugin_flow() if route == "plugin" else E.linvel_warp()
    q = Z.LV_START
    ev = E.DeviceEvents.from_arrays(x, y, t, p).scaled(factor)
    same_cols = E.DeviceEvents.from_arrays(x, y, t, (p * np.float32(factor)).astype(np.float32))
    got = E.get_timestamp_images(q, ev, None, None, None, warp, IMG)
    want = E.get_timestamp_images(q, same_cols, None, None, None, warp, IMG)
    assert torch.equal(got, want)
    _close_planes(got, Z.images(Z.LINVEL, q, x, y, t, p.astype(np.float64) * factor, img_size=IMG, f32_coords=True))
    if factor <= 0:
        plain = E.get_timestamp_images(q, E.DeviceEvents.from_arrays(x, y, t, p), None, None, None, warp, IMG)
        assert not torch.equal(got, plain)
    if factor == 0:
        assert float(got[0].abs().max()) == 0.0 and float(got[1].max()) > 0.0
    obj = E.zhu_timestamp_objective()
    f, g = obj.evaluate_function_and_gradient(q, ev, None, None, None, warp, IMG)
    f2, g2 = obj.evaluate_function_and_gradient(q, same_cols, None, None, None, warp, IMG)
    assert f == f2 and np.array_equal(g, g2)
    kw = dict(img_size=IMG, f32_coords=True)
    assert f == pytest.approx(Z.loss(Z.LINVEL, q, x, y, t, p.astype(np.float64) * factor, **kw), rel=1e-4)
    _close_grad(g, Z.grad(Z.LINVEL, q, x, y, t, p.astype(np.float64) * factor, **kw))


@pytest.mark.parametrize("sensor", [(180, 240), (480, 640), (2000, 640)])
@pytest.mark.parametrize("model", [Z.LINVEL, Z.PLANAR])
def test_band_and_direct_splats_agree(model, sensor):
    """A canvas of several bands whose height is not a multiple of the band (181 = 8 x 21 + 13, 481 = 68 x 7 + 5) and one for
    which the geometry function returns 0 (the direct kernel runs either way): the same planes within float32 summation order."""
    import event_utils_amd as E
    from event_utils_amd import _lib
    from event_utils_amd.contrast_max import objectives as O
    rows = _lib.lib().evk_tsimg_band_rows(0, sensor[0] + 1, sensor[1] + 1)
    assert (rows == 0) == (sensor == (2000, 640))
    if rows:
        assert (sensor[0] + 1) % rows != 0 and rows < sensor[0] + 1
    x, y, t, p = Z.scene(model, n=8000)
    sx, sy = sensor[1] / 240.0, sensor[0] / 180.0
    cols = _f32((x * sx, y * sy, t, p))
    q = Z.START[model].copy()
    warp = _warp(model) if model == Z.LINVEL else E.planar_flow_warp(center=(120.0 * sx, 90.0 * sy))
    if model == Z.PLANAR:
        q[6:] = 0.0
    ev = E.DeviceEvents.from_arrays(*cols)
    band = O.timestamp_planes_device(q, ev, warp, sensor, sensor_size=sensor)
    direct = O.timestamp_planes_device(q, ev, warp, sensor, sensor_size=sensor, impl="direct")
    ref = Z.planes(model, q, *cols, img_size=sensor, center=(120.0 * sx, 90.0 * sy), f32_coords=True)
    assert ref[1].sum() + ref[3].sum() > 0.9 * len(cols[0])
    _close_planes(band, ref)
    _close_planes(direct, ref)
    _close_planes(band, direct.cpu().numpy().astype(np.float64))


def test_zero_flow_equals_the_timestamp_image_of_the_package():
    """Ties the fused kernel to the fixture-pinned events_to_timestamp_image_torch: zero flow, events inside the image."""
    import event_utils_amd as E
    rng = np.random.default_rng(5)
    n = 20000
    x, y = rng.uniform(0.5, 239.5, n).astype(np.float32), rng.uniform(0.5, 179.5, n).astype(np.float32)
    t = np.sort(rng.uniform(2.0, 2.5, n)).astype(np.float32)
    p = rng.choice([-1.0, 1.0], n).astype(np.float32)
    tens = tuple(torch.from_numpy(a).cuda() for a in (x, y, t, p))
    pos, neg = E.events_to_timestamp_image_torch(*tens)
    out = E.get_timestamp_images([0.0, 0.0], *tens, E.linvel_warp(), IMG)
    for ours, theirs in ((out[0], pos), (out[1], neg)):
        theirs = theirs.cpu().numpy().astype(np.float64)
        np.testing.assert_allclose(ours.cpu().numpy().astype(np.float64), theirs, rtol=0, atol=1e-6 * np.abs(theirs).max())


# ---- value and gradient ------------------------------------------------------------------------------------------------
class _plugin_flow:
    """A user plugin (not one of the package's classes): linear flow in whatever array type it is handed."""

    def __new__(cls):
        import event_utils_amd as E

        class plugin_flow(E.warp_function):
            def __init__(self):
                E.warp_function.__init__(self, "plugin_flow", 2)

            def warp(self, xs, ys, ts, ps, t0, params, compute_grad=False):
                dt = ts - t0
                xo, yo = xs - dt * params[0], ys - dt * params[1]
                if not compute_grad:
                    return xo, yo, None, None
                z = dt * 0
                stack = torch.stack if isinstance(dt, torch.Tensor) else np.stack
                return xo, yo, stack([-dt, z]), stack([z, -dt])
        return plugin_flow()


@pytest.mark.parametrize("sigma", [0, 1.0, 2.0, 9.0])
@pytest.mark.parametrize("model", Z.MODELS + ("plugin",))
def test_value_and_gradient_match_the_restatement(model, sigma):
    """sigma 9 has radius 36 > EVK_MAX_RADIUS: the wide blur.  The one-call and the two-call forms agree bitwise."""
    import event_utils_amd as E
    from event_utils_amd import _lib
    from event_utils_amd.contrast_max.objectives import _blur_kernel
    assert (_blur_kernel(sigma)[1] > _lib.EVK_MAX_RADIUS) == (sigma == 9.0)
    np_model = Z.LINVEL if model == "plugin" else model
    warp = _plugin_flow() if model == "plugin" else _warp(model)
    q = Z.START[np_model]
    cols = _f32(_scene_partly_outside(np_model))
    kw = dict(sigma=sigma, img_size=IMG, center=Z.CENTER[np_model], f32_coords=True)
    f_ref, g_ref = Z.loss(np_model, q, *cols, **kw), Z.grad(np_model, q, *cols, **kw)
    obj = E.zhu_timestamp_objective()
    f = obj.evaluate_function(q, *cols, warp, IMG, sigma)
    g = obj.evaluate_gradient(q, *cols, warp, IMG, sigma)
    f2, g2 = obj.evaluate_function_and_gradient(q, *cols, warp, IMG, sigma)
    print("%s sigma %g: f %.9g (ref %.9g, rel %.2e)  max |g - g_ref| / max |g_ref| %.2e" % (
        model, sigma, f, f_ref, abs(f - f_ref) / abs(f_ref), np.abs(g - g_ref).max() / np.abs(g_ref).max()))
    assert f == pytest.approx(f_ref, rel=1e-4)
    _close_grad(g, g_ref)
    assert f2 == f and np.array_equal(g2, g)
    assert isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == (warp.dims,)
    if model != "plugin":
        ev = E.DeviceEvents.from_arrays(*cols)
        f3, g3 = obj.evaluate_function_and_gradient(q, ev, None, None, None, warp, IMG, sigma)
        assert f3 == f and np.array_equal(g3, g)
        # `iwe` is ignored: not a function of the image of warped events
        assert obj.evaluate_function(q, ev, None, None, None, warp, IMG, sigma, iwe=np.ones((181, 241), np.float32)) == f


def test_default_blur_and_float64_columns():
    import event_utils_amd as E
    cols = _scene_partly_outside(Z.XYZTHETA)            # float64 values that are not float32 values: the _f64 entries
    warp, q = _warp(Z.XYZTHETA), Z.START[Z.XYZTHETA]
    ev = E.DeviceEvents.from_arrays(*cols)
    assert ev.dtype == torch.float64
    obj = E.zhu_timestamp_objective()
    f, g = obj.evaluate_function_and_gradient(q, ev, None, None, None, warp, IMG)
    kw = dict(sigma=2.0, img_size=IMG, center=Z.CENTER[Z.XYZTHETA], f32_coords=True)
    assert f == pytest.approx(Z.loss(Z.XYZTHETA, q, *cols, **kw), rel=1e-4)
    _close_grad(g, Z.grad(Z.XYZTHETA, q, *cols, **kw))
    part = ev.slice(1, len(ev) - 3)                     # 8-byte aligned, not 16
    f, g = obj.evaluate_function_and_gradient(q, part, None, None, None, warp, IMG)
    sub = tuple(a[1:len(ev) - 3] for a in cols)
    assert f == pytest.approx(Z.loss(Z.XYZTHETA, q, *sub, **kw), rel=1e-4)
    _close_grad(g, Z.grad(Z.XYZTHETA, q, *sub, **kw))


@pytest.mark.parametrize("model", Z.MODELS)
def test_gradient_is_bitwise_repeatable(model):
    """The same inputs give the same bits, call after call (the gather reduces in a fixed order, without atomics)."""
    import event_utils_amd as E
    ev = E.DeviceEvents.from_arrays(*_f32(Z.scene(model, n=60000)))
    obj, warp, q = E.zhu_timestamp_objective(), _warp(model), Z.START[model]
    runs = [obj.evaluate_gradient(q, ev, None, None, None, warp, IMG) for _ in range(5)]
    print(model, [np.abs(g - runs[0]).max() / np.abs(runs[0]).max() for g in runs])
    assert all(np.array_equal(runs[0], g) for g in runs[1:])


@pytest.mark.parametrize("model", Z.MODELS)
def test_gather_alone_is_bitwise_repeatable(model):
    """evk_tsobj_grad_* on fixed adjoint images: no atomics, a grid that depends on n alone -- the same bits every time, and
    nothing written past the model's dims."""
    import event_utils_amd as E
    from event_utils_amd import _device as D
    from event_utils_amd import _lib
    from event_utils_amd.contrast_max import objectives as O
    ev = E.DeviceEvents.from_arrays(*_f32(Z.scene(model, n=60000)))
    warp, q = _warp(model), Z.START[model]
    dev = ev.device
    adj = torch.rand((4, 181, 241), dtype=torch.float32, device=dev)
    args, hp, suffix = O._ts_fused_args(q, ev, warp, IMG, None, None)
    scratch, nbytes = D.reduce_scratch(dev)
    outs = []
    for _ in range(5):
        out = torch.zeros(8, dtype=torch.float64, device=dev)
        _lib.call("evk_tsobj_grad_" + suffix, *args, D.ptr(adj), D.ptr(out), D.ptr(scratch), nbytes, D.stream())
        outs.append(out.cpu().numpy())
    assert all(np.array_equal(outs[0], o) for o in outs[1:])
    assert np.abs(outs[0][:warp.dims]).min() > 0 and not outs[0][warp.dims:].any()


def test_gradient_matches_differences_of_the_gpu_value():
    """Value and gradient belong together: central differences of evaluate_function itself.  The float32 planes and the kinks
    of the interpolant limit the agreement; the allowance is THREE TIMES the error of the same difference quotient taken on
    the CPU from the restatement's loss with its planes rounded to float32 (measured for this scene and step 0.1 px/s:
    9.7e-5 and 3.6e-4 of max |g|, so the bound is about 1.1e-3 max |g|)."""
    import event_utils_amd as E
    cols = _f32(Z.scene(Z.LINVEL))
    q, h = Z.LV_START, 0.1
    kw = dict(img_size=IMG, f32_coords=True)
    g_ref = Z.grad(Z.LINVEL, q, *cols, **kw)

    def f_cpu(v):
        return Z.loss_of_planes(Z.planes(Z.LINVEL, v, *cols, **kw).astype(np.float32).astype(np.float64))
    obj, warp = E.zhu_timestamp_objective(), E.linvel_warp()
    ev = E.DeviceEvents.from_arrays(*cols)
    g = obj.evaluate_gradient(q, ev, None, None, None, warp, IMG)
    cpu_err, gpu_err = 0.0, 0.0
    for k in range(2):
        e = np.zeros(2)
        e[k] = h
        cpu_err = max(cpu_err, abs((f_cpu(q + e) - f_cpu(q - e)) / (2 * h) - g_ref[k]))
        fd = (obj.evaluate_function(q + e, ev, None, None, None, warp, IMG) -
              obj.evaluate_function(q - e, ev, None, None, None, warp, IMG)) / (2 * h)
        gpu_err = max(gpu_err, abs(fd - g[k]))
    print("difference quotient vs gradient: cpu %.3e gpu %.3e (max |g| %.3e)" % (cpu_err, gpu_err, np.abs(g_ref).max()))
    assert cpu_err <= 1e-3 * np.abs(g_ref).max()          # (the measurement above still holds)
    assert gpu_err <= 3.0 * cpu_err


# ---- optimisation ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer", ["scipy", "evk_bfgs"])
@pytest.mark.parametrize("model", Z.MODELS)
def test_optimize_contrast_recovers_the_scene(model, optimizer):
    """The analytic gradient drives both optimisers from the perturbed start of the motion-model tests to within their
    acceptance radii of the generating parameters (tests/test_cpu_zhu.py's scenes; scipy on the restatement reaches them from
    the same start).  Parameters that push every event off the canvas give loss 0, the global minimum: the starts keep the
    events on the canvas."""
    import event_utils_amd as E
    cols = Z.scene(model)
    obj, warp = E.zhu_timestamp_objective(), _warp(model)
    kw = {} if optimizer == "scipy" else {"optimizer": "evk_bfgs"}
    q = E.optimize_contrast(*cols, warp, obj, x0=Z.START[model].copy(), numeric_grads=False, img_size=IMG, **kw)
    err = np.abs(np.asarray(q) - Z.TRUTH[model]) / Z.TOL[model]
    print(model, optimizer, q, "err / radius", err.max())
    assert np.all(err <= 1.0), (q, Z.TRUTH[model])


@pytest.mark.parametrize("optimizer", ["scipy", "evk_bfgs"])
def test_optimize_contrast_with_numeric_gradients(optimizer):
    import event_utils_amd as E
    cols = Z.scene(Z.LINVEL)
    kw = {} if optimizer == "scipy" else {"optimizer": "evk_bfgs"}
    q = E.optimize_contrast(*cols, E.linvel_warp(), E.zhu_timestamp_objective(), x0=Z.LV_START.copy(), numeric_grads=True,
                            img_size=IMG, **kw)
    assert np.all(np.abs(q - Z.LV_TRUTH) <= Z.TOL[Z.LINVEL]), q


def test_cpu_scipy_reaches_the_radius_from_the_same_start():
    """The basin is the loss's own: scipy on the restatement's loss and gradient, same scene, same start (linear flow here;
    tests/test_cpu_zhu.py's scenes are the same for every model)."""
    cols = Z.scene(Z.LINVEL)
    q = opt.fmin_bfgs(lambda v: Z.loss(Z.LINVEL, v, *cols), Z.LV_START, fprime=lambda v: Z.grad(Z.LINVEL, v, *cols), disp=False)
    assert np.all(np.abs(q - Z.LV_TRUTH) <= Z.TOL[Z.LINVEL]), q


def test_optimize_with_default_start_and_optimize_wrapper():
    """x0=None: the warp's defaults (xyztheta: zeros); optimize() forwards has_derivative = True (analytic gradient, blur 1)."""
    import event_utils_amd as E
    from event_utils_amd.contrast_max import events_cmax as C
    cols = Z.scene(Z.LINVEL)
    q = C.optimize(*cols, E.linvel_warp(), E.zhu_timestamp_objective(), numeric_grads=False, img_size=IMG)
    assert np.all(np.abs(q - Z.LV_TRUTH) <= Z.TOL[Z.LINVEL]), q
    x, y, t, p = Z.scene(Z.XYZTHETA, n=4000)
    q = E.optimize_contrast(x, y, t, p, _warp(Z.XYZTHETA), E.zhu_timestamp_objective(), img_size=IMG)
    assert q.shape == (4,) and np.all(np.isfinite(q))


def test_batch_landscape_and_grid_search_agree_with_single_evaluations():
    import event_utils_amd as E
    from event_utils_amd.contrast_max import events_cmax as C
    cols = _f32(Z.scene(Z.LINVEL, n=5000))
    obj, warp = E.zhu_timestamp_objective(), E.linvel_warp()
    pts = [np.array([40.0, -25.0]), np.array([0.0, 0.0]), np.array([-60.0, 80.0]), np.array([41.0, -25.0])]
    ev = E.DeviceEvents.from_arrays(*cols)
    single = [obj.evaluate_function(q, ev, None, None, None, warp, IMG, 1.0) for q in pts]
    for got in (obj.evaluate_function_batch(pts, ev, None, None, None, warp, IMG, 1.0),
                obj.evaluate_function_batch(pts, *cols, warp, IMG, 1.0)):
        np.testing.assert_allclose(got, single, rtol=1e-6)
    for q, f in zip(pts, single):
        assert f == pytest.approx(Z.loss(Z.LINVEL, q, *cols, sigma=1.0, img_size=IMG, f32_coords=True), rel=1e-4)
    xr, yr, res = (-60, 60), (-60, 60), 30
    img = C.objective_landscape(*cols, objective=obj, warpfunc=warp, x_range=xr, y_range=yr, resolution=res, img_size=IMG)
    vals = np.array([[-obj.evaluate_function(np.array([xx * res + xr[0], yy * res + yr[0]], dtype=np.float64), ev, None, None, None,
                                             warp, IMG, 0) for xx in range(4)] for yy in range(4)])
    np.testing.assert_allclose(img, (vals - vals.min()) / ((vals.max() - vals.min()) + 1e-6), rtol=1e-5, atol=1e-6)
    out = C.grid_search_initial(*cols, warp, obj, IMG, param_ranges=[[-80, 80], [-80, 80]], log_scale=False)
    assert len(out["params"]) == len(out["eval"]) == 25
    one = [obj.evaluate_function(np.array(q, dtype=np.float64), ev, None, None, None, warp, IMG, 1.0) for q in out["params"]]
    np.testing.assert_allclose(out["eval"], one, rtol=1e-6)
    # the loss is never below 0: the smallest sample is kept (upstream's start value would keep none)
    k = int(np.argmin(out["eval"]))
    assert tuple(out["min_params"]) == tuple(out["params"][k]) and out["min_func_eval"] == out["eval"][k]
    assert tuple(out["min_params"]) == (40.0, -40.0)            # the sample nearest the truth (40, -25)
