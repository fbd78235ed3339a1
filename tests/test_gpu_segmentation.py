"""GPU: motion segmentation (cluster images, loss and gradient, assignment step, alternating loop) against its float64 numpy
restatement (tests/_segmentation_np.py, pinned by tests/test_cpu_segmentation.py) and against the package's own single-motion
code.  Tolerances are those tests/test_gpu_zhu.py uses for float32 planes against a float64 restatement: planes atol = 1e-6 x
the plane's maximum, loss rtol = 1e-4, gradient rtol = 1e-4 with atol = 1e-4 max|g_ref|."""
import functools

import numpy as np
import pytest
import torch

import _motion_models8_np as M8
import _segmentation_np as S
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


@functools.lru_cache(maxsize=None)
def _scene_partly_outside(model, n=6000):
    """The model's scene of tests/_zhu_np.py with a tenth of its events moved across the image borders."""
    x, y, t, p = Z.scene(model, n=n)
    x, y = x.copy(), y.copy()
    x[::20] += 200.0
    y[7::20] -= 170.0
    return x, y, t, p


def _cluster_params(model, L):
    """L sets of parameters between the scene's start and its truth (and a little beyond)."""
    a, b = np.asarray(Z.START[model], dtype=np.float64), np.asarray(Z.TRUTH[model], dtype=np.float64)
    return np.stack([a + (b - a) * f for f in np.linspace(-0.3, 1.3, L)]) if L > 1 else b[None].copy()


def _dirichlet(L, n, seed=0):
    return np.ascontiguousarray(np.random.default_rng(seed).dirichlet(np.ones(L), n).T, dtype=np.float32)


def _np(a):
    return a.cpu().numpy().astype(np.float64) if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)


def _close_planes(got, ref):
    got = _np(got)
    assert got.shape == ref.shape
    for c in range(ref.shape[0]):
        np.testing.assert_allclose(got[c], ref[c], rtol=0, atol=1e-6 * max(np.abs(ref[c]).max(), 1e-30), err_msg="plane %d" % c)


def _close_grad(g, ref):
    np.testing.assert_allclose(np.asarray(g, dtype=np.float64), ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


def _kw(model, img=IMG, **more):
    return dict(img_size=img, center=Z.CENTER[model], f32_coords=True, **more)


# ---- 1. the planes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", Z.MODELS)
def test_cluster_images_match_the_restatement(model):
    """numpy (float64 and float32 columns), tensor and DeviceEvents inputs and a misaligned slice; L = 3 and L = 8 (several
    bands); both polarity modes; the band and the direct form give the same bits, and so do two calls."""
    import event_utils_amd as E
    from event_utils_amd import _lib
    warp = _warp(model)
    cols64 = _scene_partly_outside(model)
    cols32 = _f32(cols64)
    n = len(cols32[0])
    ev = E.DeviceEvents.from_arrays(*cols32)
    assert ev.dtype == torch.float32
    part = ev.slice(1, n - 4)                                                                   # columns off 16-byte alignment
    assert part.x.data_ptr() % 16 != 0
    for L in (3, 8):
        rows = _lib.lib().evk_seg_band_rows(L, 0, IMG[0] + 1, IMG[1] + 1)
        assert 0 < rows and -(-(IMG[0] + 1) // rows) >= (16 if L == 8 else 2)                  # several bands
        assert _lib.lib().evk_seg_band_rows(L, _lib.EVK_IWE_DIRECT, IMG[0] + 1, IMG[1] + 1) == 0
        q, probs = _cluster_params(model, L), _dirichlet(L, n)
        assert not Z.mask(model, q[0], *cols32, img_size=IMG, center=Z.CENTER[model]).all()
        for pol in (False, True):
            ref32 = S.iwes(model, q, probs, *cols32, **_kw(model, use_polarity=pol))
            assert min(np.abs(r).max() for r in ref32) > 0
            out = E.cluster_iwes(q, probs, *cols32, warp, IMG, use_polarity=pol)
            assert isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32
            assert tuple(out.shape) == (L, 181, 241)
            _close_planes(out, ref32)
            band = E.cluster_iwes(q, torch.from_numpy(probs).cuda(), ev, None, None, None, warp, IMG, use_polarity=pol)
            direct = E.cluster_iwes(q, probs, ev, None, None, None, warp, IMG, use_polarity=pol, impl="direct")
            assert torch.equal(band, out) and torch.equal(band, direct)
            assert torch.equal(band, E.cluster_iwes(q, probs, ev, None, None, None, warp, IMG, use_polarity=pol))
            if L == 3:
                _close_planes(E.cluster_iwes(q, probs, *cols64, warp, IMG, use_polarity=pol),    # float64 columns
                              S.iwes(model, q, probs, *cols64, **_kw(model, use_polarity=pol)))
                tens = tuple(torch.from_numpy(a).cuda() for a in cols32)
                assert torch.equal(E.cluster_iwes(q, probs, *tens, warp, IMG, use_polarity=pol), out)
                sl = np.ascontiguousarray(probs[:, 1:n - 4])
                got = E.cluster_iwes(q, sl, part, None, None, None, warp, IMG, use_polarity=pol)
                _close_planes(got, S.iwes(model, q, sl, *(a[1:n - 4] for a in cols32), **_kw(model, use_polarity=pol)))
                assert torch.equal(got, E.cluster_iwes(q, sl, part, None, None, None, warp, IMG, use_polarity=pol, impl="direct"))


# ---- 2. small and odd sizes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 3, 5, 1023])
def test_small_and_odd_sizes(n):
    """L = 1 and L = 2; associations holding exact zeros; NaN polarities dropped; events that stay on the canvas for cluster 0
    only; images, loss, gradient and assignment."""
    import event_utils_amd as E
    rng = np.random.default_rng(n)
    H, W = S.CANVAS
    x, y = rng.uniform(2.0, W - 2.0, n).astype(np.float32), rng.uniform(2.0, H - 2.0, n).astype(np.float32)
    t = np.sort(rng.uniform(0.0, 0.5, n)).astype(np.float32)
    p = rng.choice([-1.0, 1.0], n).astype(np.float32)
    p[2::7] = np.nan
    warp = E.linvel_warp()
    for q in (np.array([[12.0, -9.0]]), np.array([[0.0, 0.0], [400.0, 300.0]])):                # cluster 1 pushes early events off
        L = len(q)
        probs = _dirichlet(L, n, seed=1) if L > 1 else np.ones((1, n), dtype=np.float32)
        probs[:, 1::3] = 0.0
        if L == 2 and n:
            only0 = Z.mask(Z.LINVEL, q[0], x, y, t, p, img_size=S.CANVAS, f32_coords=True) & \
                ~Z.mask(Z.LINVEL, q[1], x, y, t, p, img_size=S.CANVAS, f32_coords=True)
            assert n < 5 or only0.any()
        for pol in (False, True):
            kw = dict(img_size=S.CANVAS, f32_coords=True, use_polarity=pol)
            out = E.cluster_iwes(q, probs, x, y, t, p, warp, S.CANVAS, use_polarity=pol)
            assert tuple(out.shape) == (L, H + 1, W + 1)
            _close_planes(out, S.iwes(Z.LINVEL, q, probs, x, y, t, p, **kw))
            f, g = E.segmentation_loss(q, probs, x, y, t, p, warp, S.CANVAS, use_polarity=pol, compute_gradient=True)
            fr, gr = S.loss_and_grad(Z.LINVEL, q, probs, x, y, t, p, 1.0, **kw)
            assert f == pytest.approx(fr, rel=1e-4, abs=1e-12) and g.shape == (L, 2) and g.dtype == np.float64
            _close_grad(g, gr)
            new, labels = E.update_assignments(q, probs, x, y, t, p, warp, S.CANVAS, use_polarity=pol)
            assert tuple(new.shape) == (L, n) and new.dtype == torch.float32 and tuple(labels.shape) == (n,)
            assert labels.dtype == torch.int32
            rn, rl, rs, _, rb = S.assign(Z.LINVEL, q, probs, x, y, t, p, 1.0, **kw)
            if n == 0:
                assert float(out.abs().max()) == 0.0 and f == 0.0 and not g.any()
                continue
            keep = rs == 0
            assert np.array_equal(new.cpu().numpy()[:, keep], probs[:, keep])                      # rows kept bit for bit
            assert keep[np.isnan(p)].all()
            sure = rs >= 0.02 * rb.max()
            np.testing.assert_allclose(_np(new)[:, sure], rn[:, sure].astype(np.float64), rtol=0, atol=(1 + L) * 5e-5)
            top = np.sort(rn.astype(np.float64), axis=0)
            clear = sure & ((top[-1] - top[-2] >= 1e-3) if L > 1 else True)
            assert np.array_equal(labels.cpu().numpy()[clear | keep], rl[clear | keep])


def test_the_second_trip_of_the_event_loops():
    """1024 x 256 x 4 + 5 events, two clusters, a (16, 16) image: the adjoint gather's grid is capped at 1024 workgroups of 256
    threads with four events each, so five events are taken on a second trip of its grid-stride loop (a quad and a tail of one:
    n = 1 mod 4, the rows of probs off 16-byte alignment), and the band kernel runs many chunks.  Planes, loss, gradient and the
    assignment step by the rules of the tests above."""
    import event_utils_amd as E
    n, L, img = 1024 * 256 * 4 + 5, 2, (16, 16)
    rng = np.random.default_rng(7)
    x, y = rng.uniform(0.5, 15.5, n).astype(np.float32), rng.uniform(0.5, 15.5, n).astype(np.float32)
    t = np.sort(rng.uniform(0.0, 0.5, n)).astype(np.float32)
    p = rng.choice([-1.0, 1.0], n).astype(np.float32)
    q, probs, warp = np.array([[6.0, -4.0], [-10.0, 8.0]]), _dirichlet(L, n, seed=2), E.linvel_warp()
    ev, dprobs = E.DeviceEvents.from_arrays(x, y, t, p), torch.from_numpy(probs).cuda()
    kw = dict(img_size=img, f32_coords=True, use_polarity=True)
    keep = np.stack([Z.mask(Z.LINVEL, v, x, y, t, p, img_size=img, f32_coords=True) for v in q])
    assert keep[:, -5:].all() and 0.5 * n < keep[1].sum() < n                                   # the second trip counts; some events leave
    out = E.cluster_iwes(q, dprobs, ev, None, None, None, warp, img, use_polarity=True)
    _close_planes(out, S.iwes(Z.LINVEL, q, probs, x, y, t, p, **kw))
    assert torch.equal(out, E.cluster_iwes(q, dprobs, ev, None, None, None, warp, img, use_polarity=True, impl="direct"))
    f, g = E.segmentation_loss(q, dprobs, ev, None, None, None, warp, img, use_polarity=True, compute_gradient=True)
    fr, gr = S.loss_and_grad(Z.LINVEL, q, probs, x, y, t, p, 1.0, **kw)
    print("loss %.9g (ref %.9g), max|g - ref| / max|ref| %.3g" % (f, fr, np.abs(g - gr).max() / np.abs(gr).max()))
    assert f == pytest.approx(fr, rel=1e-4)
    _close_grad(g, gr)
    # the five events of the second trip are in the sums: without them the gradient is another
    g5 = E.segmentation_loss(q, probs[:, :-5].copy(), x[:-5], y[:-5], t[:-5], p[:-5], warp, img, use_polarity=True, compute_gradient=True)[1]
    assert not np.array_equal(g5, g)
    new, labels = E.update_assignments(q, dprobs, ev, None, None, None, warp, img, use_polarity=True)
    new, labels = new.cpu().numpy(), labels.cpu().numpy()
    rn, rl, rs, _, rb = S.assign(Z.LINVEL, q, probs, x, y, t, p, 1.0, **kw)
    on, sure = rs > 0, rs >= 0.02 * rb.max()
    assert sure.sum() >= 0.3 * n and sure[-5:].any()
    np.testing.assert_allclose(new[:, sure].astype(np.float64), rn[:, sure].astype(np.float64), rtol=0, atol=(1 + L) * 5e-5)
    top = np.sort(rn.astype(np.float64), axis=0)
    check = sure & (top[-1] - top[-2] >= 1e-3)
    assert np.array_equal(labels[check], rl[check])
    off = ~keep.any(axis=0)                                                                      # off the canvas under both motions: S = 0 for certain
    assert off.any() and not on[off].any()
    assert np.array_equal(new[:, off], probs[:, off]) and np.array_equal(labels[off], np.argmax(probs[:, off], axis=0))


# ---- 3. one cluster holding every event: the package's single-motion code -----------------------------------------------
def test_one_cluster_of_all_events_is_get_iwe_and_the_variance_objective():
    """L = 1, P = 1.  The plane is get_iwe's image: use_polarity=False there takes |p|, so the polarities are +-1.  The loss is
    variance_objective's value, which already is minus the variance (reference_exact=False; float32)."""
    import event_utils_amd as E
    x, y, t, p = _f32(_scene_partly_outside(Z.LINVEL))
    p = np.where(p > 0, 1.0, -1.0).astype(np.float32)
    q, warp = Z.LV_START, E.linvel_warp()
    ones = np.ones((1, len(t)), dtype=np.float32)
    for pol in (False, True):
        iwe = E.get_iwe(q, x, y, t, p, warp, IMG, use_polarity=pol)[0].astype(np.float64)
        assert np.abs(iwe).max() > 1
        _close_planes(E.cluster_iwes(q[None], ones, x, y, t, p, warp, IMG, use_polarity=pol), iwe[None])
        obj = E.variance_objective()
        obj.reference_exact, obj.use_polarity = False, pol
        want = float(obj.evaluate_function(q, x, y, t, p, warp, IMG, 1.0))
        got = E.segmentation_loss(q[None], ones, x, y, t, p, warp, IMG, blur_sigma=1.0, use_polarity=pol)
        assert want < 0 and got == pytest.approx(want, rel=1e-4)


# ---- 4. loss and gradient ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.0, 1.0])
@pytest.mark.parametrize("model", Z.MODELS)
def test_loss_and_gradient_match_the_restatement(model, sigma):
    import event_utils_amd as E
    warp, L = _warp(model), 3
    cols = _f32(_scene_partly_outside(model))
    q, probs = _cluster_params(model, L), _dirichlet(L, len(cols[0]))
    ev = E.DeviceEvents.from_arrays(*cols)
    for pol in (False, True):
        fr, gr = S.loss_and_grad(model, q, probs, *cols, sigma, **_kw(model, use_polarity=pol))
        f, g = E.segmentation_loss(q, probs, ev, None, None, None, warp, IMG, blur_sigma=sigma, use_polarity=pol,
                                   compute_gradient=True)
        print("%s sigma %g polarity %s: loss %.9g (ref %.9g), max|g - ref| / max|ref| %.3g"
              % (model, sigma, pol, f, fr, np.abs(g - gr).max() / np.abs(gr).max()))
        assert isinstance(f, float) and g.shape == (L, Z.DIMS[model]) and g.dtype == np.float64
        assert f == pytest.approx(fr, rel=1e-4)
        _close_grad(g, gr)
        assert f == E.segmentation_loss(q, probs, ev, None, None, None, warp, IMG, blur_sigma=sigma, use_polarity=pol)
        f2, g2 = E.segmentation_loss(q, probs, *cols, warp, IMG, blur_sigma=sigma, use_polarity=pol, compute_gradient=True)
        assert f2 == f and np.array_equal(g2, g)                                                     # the same bits


# ---- 5. assignment -----------------------------------------------------------------------------------------------------
SCENES = {2: (S.FLOWS2, 12), 3: (S.FLOWS3, 10)}


@pytest.mark.parametrize("pol", [False, True])
@pytest.mark.parametrize("clusters", [2, 3])
def test_assignment_matches_the_restatement(clusters, pol):
    """P' within (1 + L) 5e-5 where the reference's S >= 0.02 max B (each gathered value is within 1e-6 max B of the
    reference's, and is divided by S); at most 1 % of the events with S > 0 may lie below that bar; labels agree except where
    the reference's two largest probabilities differ by less than 1e-3, at most 1 % too; S = 0 keeps the row bit for bit."""
    import event_utils_amd as E
    flows, sources = SCENES[clusters]
    x, y, t, p, _ = S.scene(flows, sources, 40, seed=0, push_every=20)
    x, y, t, p = _f32((x, y, t, p))
    q, probs = S.start(flows, 0), _dirichlet(clusters, len(t), seed=4)
    rn, rl, rs, _, rb = S.assign(Z.LINVEL, q, probs, x, y, t, p, 1.0, img_size=S.CANVAS, f32_coords=True, use_polarity=pol)
    new, labels = E.update_assignments(q, probs, x, y, t, p, E.linvel_warp(), S.CANVAS, blur_sigma=1.0, use_polarity=pol)
    new, labels = new.cpu().numpy(), labels.cpu().numpy()
    on, sure = rs > 0, rs >= 0.02 * rb.max()
    assert not on[::20].any() and on.sum() >= 0.94 * len(t)
    print("below the S bar: %d of %d" % ((on & ~sure).sum(), on.sum()))
    assert (on & ~sure).sum() <= 0.01 * on.sum()
    np.testing.assert_allclose(new[:, sure].astype(np.float64), rn[:, sure].astype(np.float64), rtol=0, atol=(1 + clusters) * 5e-5)
    top = np.sort(rn.astype(np.float64), axis=0)
    tie = on & (top[-1] - top[-2] < 1e-3)
    print("near ties: %d of %d" % (tie.sum(), on.sum()))
    assert tie.sum() <= 0.01 * on.sum()
    check = sure & ~tie
    assert np.array_equal(labels[check], rl[check])
    assert np.array_equal(new[:, ~on], probs[:, ~on])
    assert np.array_equal(labels[~on], np.argmax(probs[:, ~on], axis=0))
    again = E.update_assignments(q, torch.from_numpy(probs).cuda(), x, y, t, p, E.linvel_warp(), S.CANVAS, use_polarity=pol)
    assert np.array_equal(again[0].cpu().numpy(), new) and np.array_equal(again[1].cpu().numpy(), labels)


# ---- 6. end to end ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clusters", [2, 3])
def test_segment_events_recovers_the_scene(clusters):
    """The bars of tests/test_cpu_segmentation.py on float32 columns; the final loss within 1e-3 of the restated loop's."""
    import event_utils_amd as E
    flows, sources = SCENES[clusters]
    x, y, t, p, k = S.scene(flows, sources, 40, seed=0)
    x, y, t, p = _f32((x, y, t, p))
    x0 = S.start(flows, 0)
    seen = []
    r = E.segment_events(x, y, t, p, E.linvel_warp(), x0, S.CANVAS, n_outer=6, callback=lambda *a: seen.append(a))
    ref = S.segment(Z.LINVEL, x, y, t, p, x0, S.CANVAS, n_outer=6, f32_coords=True)
    assert isinstance(r, E.SegmentationResult) and r.params.shape == flows.shape
    assert r.probs.is_cuda and tuple(r.probs.shape) == (clusters, len(t)) and r.probs.dtype == torch.float32
    assert r.labels.is_cuda and r.labels.dtype == torch.int32
    acc, err = float(np.mean(r.labels.cpu().numpy() == k)), float(np.abs(r.params - flows).max())
    print("clusters %d: accuracy %.4f, error %.3f px/s, loss %.6f (restated %.6f), history %s"
          % (clusters, acc, err, r.loss, ref.loss, np.round(r.history, 6)))
    assert acc >= 0.97
    assert err <= 2.0
    assert r.loss == pytest.approx(ref.loss, rel=1e-3)
    h = np.array(r.history)
    assert len(h) == 6 and r.loss == h[-1] and np.all(np.diff(h) <= 1e-6 * np.abs(h[:-1]))
    assert [a[0] for a in seen] == list(range(6)) and [a[2] for a in seen] == r.history
    assert np.array_equal(seen[-1][1], r.params)
    assert np.array_equal(r.labels.cpu().numpy(), r.probs.argmax(0).cpu().numpy())


# ---- 7. errors -----------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    import event_utils_amd as E
    x, y, t, p = _f32(S.scene(S.FLOWS2, 2, 10)[:4])
    n, warp = len(t), E.linvel_warp()
    with pytest.raises(ValueError):
        E.cluster_iwes(np.zeros((9, 2)), np.full((9, n), 1.0 / 9, dtype=np.float32), x, y, t, p, warp, S.CANVAS)
    with pytest.raises(ValueError):
        E.cluster_iwes(np.zeros((0, 2)), np.zeros((0, n), dtype=np.float32), x, y, t, p, warp, S.CANVAS)
    with pytest.raises(ValueError):
        E.cluster_iwes(S.FLOWS2, np.full((2, n - 1), 0.5, dtype=np.float32), x, y, t, p, warp, S.CANVAS)
    with pytest.raises(ValueError):
        E.segmentation_loss(S.FLOWS2, np.full((n, 2), 0.5, dtype=np.float32), x, y, t, p, warp, S.CANVAS)
    for bad in (1.5, -0.25, np.nan):
        probs = np.full((2, n), 0.5, dtype=np.float32)
        probs[1, 3] = bad
        with pytest.raises(ValueError):
            E.update_assignments(S.FLOWS2, probs, x, y, t, p, warp, S.CANVAS)
        with pytest.raises(ValueError):
            E.segment_events(x, y, t, p, warp, S.FLOWS2, S.CANVAS, probs0=torch.from_numpy(probs).cuda())
    with pytest.raises(ValueError):
        E.segmentation_loss(np.zeros((2, 3)), np.full((2, n), 0.5, dtype=np.float32), x, y, t, p, warp, S.CANVAS)

    class plugin(E.warp_function):
        def __init__(self):
            E.warp_function.__init__(self, "plugin", 2)

        def warp(self, xs, ys, ts, ps, t0, params, compute_grad=False):
            return xs, ys, None, None
    for call in (lambda: E.cluster_iwes(S.FLOWS2, np.full((2, n), 0.5, dtype=np.float32), x, y, t, p, plugin(), S.CANVAS),
                 lambda: E.segment_events(x, y, t, p, plugin(), S.FLOWS2, S.CANVAS)):
        with pytest.raises(NotImplementedError, match="linvel_warp"):
            call()
