"""CPU (no GPU): the float64 numpy restatement of motion segmentation (tests/_segmentation_np.py) that the GPU tests compare
the kernels with -- its gradient against central differences, its reduction to the contrast loss of a constant flow field, the
rules of the assignment step and the recovery of synthetic scenes by the alternating loop -- and the public surface."""
import ctypes
import os
import re

import numpy as np
import pytest

import _flow_contrast_np as FC
import _segmentation_np as S
import _zhu_np as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG = (30, 40)


def _small_scene(model, n=48, L=3, seed=0):
    """n events on a 30 x 40 image that stay on the canvas under L sets of parameters near zero motion, random Dirichlet P."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(8.0, 32.0, n), rng.uniform(8.0, 22.0, n)
    t = np.sort(rng.uniform(0.0, 0.1, n))
    p = rng.choice([-1.0, 1.0], n)
    if model == Z.LINVEL:
        params = rng.uniform(-30.0, 30.0, (L, 2))
    else:                                                      # xyztheta about the image centre: (vx, vy, vz, omega)
        params = np.column_stack([rng.uniform(-30, 30, L), rng.uniform(-30, 30, L), rng.uniform(-1, 1, L), rng.uniform(-2, 2, L)])
    probs = rng.dirichlet(np.ones(L), n).T
    return x, y, t, p, params, probs


@pytest.mark.parametrize("use_polarity", [False, True])
@pytest.mark.parametrize("sigma", [0.0, 1.0])
@pytest.mark.parametrize("model", [Z.LINVEL, Z.XYZTHETA])
def test_gradient_matches_central_differences(model, sigma, use_polarity):
    """<= 1e-6 max|g| (measured: <= 2e-9)."""
    x, y, t, p, params, probs = _small_scene(model)
    kw = dict(img_size=IMG, use_polarity=use_polarity, center=(20.0, 15.0))
    f, g = S.loss_and_grad(model, params, probs, x, y, t, p, sigma, **kw)
    assert f == pytest.approx(S.loss(model, params, probs, x, y, t, p, sigma, **kw), rel=1e-14)
    assert f < 0 and np.abs(g).max() > 0
    num = np.zeros_like(g)
    for i in np.ndindex(*params.shape):
        h = 1e-6 * max(1.0, abs(params[i]))
        up, dn = params.copy(), params.copy()
        up[i] += h
        dn[i] -= h
        num[i] = (S.loss(model, up, probs, x, y, t, p, sigma, **kw) - S.loss(model, dn, probs, x, y, t, p, sigma, **kw)) / (2 * h)
    err = np.abs(num - g).max() / np.abs(g).max()
    print("finite differences: relative error %.3g" % err)
    assert err <= 1e-6


def test_float32_images_cost_rounding_only():
    """f32_images of loss_and_grad (tests/_flow_contrast_np.py's, per cluster image): 1e-6 of the loss and 1e-5 of the largest
    gradient component on the small scene of 48 events (measured: 7e-10 and 1e-6); the default is float64 throughout."""
    x, y, t, p, params, probs = _small_scene(Z.LINVEL)
    f64, g64 = S.loss_and_grad(Z.LINVEL, params, probs, x, y, t, p, 1.0, img_size=IMG)
    assert (f64, g64.tolist()) == (lambda r: (r[0], r[1].tolist()))(S.loss_and_grad(Z.LINVEL, params, probs, x, y, t, p, 1.0, img_size=IMG,
                                                                                     f32_images=False))
    for mode in (True, np.random.default_rng(1)):
        f32, g32 = S.loss_and_grad(Z.LINVEL, params, probs, x, y, t, p, 1.0, img_size=IMG, f32_images=mode)
        assert f32 != f64 and abs(f32 - f64) <= 1e-6 * abs(f64) and np.abs(g32 - g64).max() <= 1e-5 * np.abs(g64).max()


@pytest.mark.parametrize("sigma", [0.0, 1.0])
def test_one_cluster_of_all_events_is_the_contrast_loss_of_a_constant_field(sigma):
    """L = 1, P = 1: the loss is minus the variance of the image tests/_flow_contrast_np.py forms for the constant field -v."""
    rng = np.random.default_rng(3)
    n, (H, W) = 400, IMG
    x, y = rng.uniform(10.0, W - 10.0, n), rng.uniform(8.0, H - 8.0, n)
    t = np.sort(rng.uniform(0.0, 0.1, n))
    p = rng.choice([-1.0, 1.0], n)
    v = np.array([35.0, -20.0])
    flow = np.empty((2, H, W))
    flow[0], flow[1] = -v[0], -v[1]
    ones = np.ones((1, n))
    assert FC.iwe(flow, x, y, t, p, use_polarity=False).sum() > 0.99 * n          # the events stay on the canvas
    for use_polarity in (True, False):
        ours = S.loss(Z.LINVEL, v[None], ones, x, y, t, p, sigma, img_size=IMG, use_polarity=use_polarity)
        img = FC.iwe(flow, x, y, t, p, use_polarity=use_polarity)
        assert ours == pytest.approx(-np.var(FC.blur(img, sigma)), rel=1e-10, abs=0)
        assert ours == pytest.approx(FC.loss(flow, x, y, t, p, sigma, "variance", use_polarity=use_polarity), rel=1e-10, abs=0)
        np.testing.assert_allclose(S.iwes(Z.LINVEL, v[None], ones, x, y, t, p, img_size=IMG, use_polarity=use_polarity)[0], img,
                                   rtol=0, atol=1e-12)


def test_assignment_rules():
    """Rows of P' sum to 1 where S > 0 and are unchanged where S = 0 (events off the canvas under every cluster, NaN
    polarities); ties go to the lowest label."""
    x, y, t, p, k = S.scene(S.FLOWS3, 6, 30, seed=1, push_every=9)
    p = p.copy()
    p[4::50] = np.nan
    rng = np.random.default_rng(2)
    probs = rng.dirichlet(np.ones(3), len(t)).T.astype(np.float32)
    new, labels, Ssum, c, _ = S.assign(Z.LINVEL, S.FLOWS3, probs, x, y, t, p, img_size=S.CANVAS)
    on = Ssum > 0
    assert on.sum() > 0.8 * len(t) and (~on).sum() >= len(t) // 9
    assert not on[::9].any() and not on[4::50].any()
    np.testing.assert_allclose(new[:, on].astype(np.float64).sum(0), 1.0, rtol=0, atol=3 * 2.0 ** -24)
    assert np.array_equal(new[:, ~on], probs[:, ~on])
    assert new.dtype == np.float32 and (new >= 0).all() and (new <= 1).all()
    assert np.array_equal(labels, np.argmax(new, axis=0))
    # two clusters with the same motion and the same associations have the same image: a tie, which goes to the lower label
    twin = np.array([S.FLOWS3[0], S.FLOWS3[0], S.FLOWS3[2]])
    halves = np.stack([probs[0], probs[0], probs[2]])
    new, labels, Ssum, c, _ = S.assign(Z.LINVEL, twin, halves, x, y, t, p, img_size=S.CANVAS)
    assert np.array_equal(new[0], new[1]) and (labels != 1).all() and (labels == 0).any()
    # the polarity flag: an event whose signed image value is negative gets nothing from that cluster
    new, labels, Ssum, c, B = S.assign(Z.LINVEL, S.FLOWS3, probs, x, y, t, p, img_size=S.CANVAS, use_polarity=True)
    assert (c >= 0).all() and (B < 0).any() and (c[:, np.nan_to_num(p) < 0] > 0).any()


SCENES = {2: (S.FLOWS2, 12), 3: (S.FLOWS3, 10)}


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("clusters", [2, 3])
def test_alternating_loop_recovers_the_scene(clusters, seed):
    """Label accuracy >= 0.97 and max|theta - truth| <= 2 px/s from truth + U(-8, 8) and uniform associations in 6 outer
    iterations (the float64 prototype gave 0.988-1.000 and 0.40-1.03 px/s; this restatement 0.991-1.000 and 0.31-1.21)."""
    flows, sources = SCENES[clusters]
    x, y, t, p, k = S.scene(flows, sources, 40, seed=seed)
    assert len(t) == clusters * sources * 40 and np.all(np.diff(t) >= 0)
    r = S.segment(Z.LINVEL, x, y, t, p, S.start(flows, seed), S.CANVAS, n_outer=6)
    acc, err = float(np.mean(r.labels == k)), float(np.abs(r.params - flows).max())
    print("clusters %d seed %d: accuracy %.4f, error %.3f px/s, history %s" % (clusters, seed, acc, err, np.round(r.history, 5)))
    assert acc >= 0.97
    assert err <= 2.0
    h = np.array(r.history)
    assert len(h) == 6 and r.loss == h[-1] and np.all(np.diff(h) <= 1e-6 * np.abs(h[:-1]))


def test_public_surface():
    """The names are exported, reachable through the reference's dotted paths, and the evk_seg_* entries are declared in the
    header and bound in _lib."""
    import event_utils_amd as E
    from event_utils_amd import _lib
    import event_utils_amd.lib.contrast_max.segmentation as alias
    from event_utils_amd.contrast_max import segmentation
    assert alias is segmentation
    for name in ("cluster_iwes", "segmentation_loss", "update_assignments", "segment_events", "SegmentationResult"):
        assert getattr(E, name) is getattr(segmentation, name)
    assert E.SegmentationResult._fields == ("params", "probs", "labels", "loss", "history")
    header = open(os.path.join(ROOT, "include", "evk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    entries = ["evk_seg_%s_%s" % (k, s) for k in ("splat", "grad", "assign") for s in ("f32", "f64")]
    for name in entries:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert _lib.PROTOTYPES[name][1] is ctypes.c_int
    assert re.search(r"\bint evk_seg_band_rows\s*\(", header) and _lib.PROTOTYPES["evk_seg_band_rows"][1] is ctypes.c_int
    assert _lib.EVK_SEG_MAX_CLUSTERS == 8 and _lib.EVK_SEG_POLARITY == 1
    L = _lib.lib()
    assert L.evk_seg_band_rows(8, 0, 181, 241) == 10 and L.evk_seg_band_rows(8, _lib.EVK_IWE_DIRECT, 181, 241) == 0
    assert L.evk_seg_band_rows(9, 0, 181, 241) == 0 and L.evk_seg_band_rows(1, 0, 181, 241) == 84


def test_arguments_are_refused_before_the_device_is_touched():
    """The C entries validate on the host: L outside 1..8, an unknown model, null pointers with n > 0, misaligned columns."""
    import ctypes
    from event_utils_amd import _lib
    L = _lib.lib()
    hp = np.zeros(16, dtype=np.float64)
    hpp = ctypes.c_void_p(hp.ctypes.data)
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every call below is refused first

    def splat(model=0, cols=fake, n=8, clusters=2, probs=fake, acc=fake, flags=0, params=hpp, x=None):
        return L.evk_seg_splat_f32(model, cols if x is None else x, cols, cols, cols, n, 0.0, params, clusters, probs, 40.0, 30.0,
                                   31, 41, flags, acc, fake, None)
    einval = L.evk_seg_splat_f32(0, None, None, None, None, -1, 0.0, None, 1, None, 0.0, 0.0, 0, 0, 0, None, None, None)
    assert einval != 0 and _lib.lib().evk_error_string(einval) == b"invalid argument"
    assert splat(clusters=0) == einval and splat(clusters=9) == einval
    assert splat(model=5) == einval and splat(model=-1) == einval
    assert splat(cols=None) == einval and splat(probs=None) == einval and splat(acc=None) == einval and splat(params=None) == einval
    assert splat(flags=2) == einval
    ealign = splat(x=ctypes.c_void_p(4098))
    assert ealign not in (0, einval)
    assert splat(probs=ctypes.c_void_p(4097)) == ealign
    assert L.evk_seg_grad_f64(0, ctypes.c_void_p(4100), fake, fake, fake, 8, 0.0, hpp, 2, fake, 40.0, 30.0, 31, 41, 0, fake, fake, fake,
                              1 << 20, None) == ealign
    assert L.evk_seg_grad_f32(0, fake, fake, fake, fake, 8, 0.0, hpp, 2, fake, 40.0, 30.0, 31, 41, 0, fake, fake, fake, 8, None) \
        not in (0, einval, ealign)                                                                    # scratch too small
    assert L.evk_seg_assign_f32(0, fake, fake, fake, fake, 8, 0.0, hpp, 2, fake, 40.0, 30.0, 31, 41, 0, fake, fake, fake, None) \
        == einval                                                                                     # probs_out is probs
    assert L.evk_seg_assign_f32(0, fake, fake, fake, fake, 8, 0.0, hpp, 9, fake, 40.0, 30.0, 31, 41, 0, fake, fake, fake, None) \
        == einval
