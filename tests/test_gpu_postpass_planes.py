"""GPU (-m gpu): the plane-generic gradient post-pass of the parametric warps (rotation and angular velocity: 3 derivative
planes, xyztheta: 4, planar flow: 8) -- k_gradsums_planes<4> / <8> and k_gradsums_planes_final (evk_warps.hip) behind
evk_objective_gradsums_planes_f32, and the 3-D channel-mixing Gaussian filter (k_blur_axis, evk_imgops.hip) on (k, H, W) stacks
-- held to what tests/test_gpu_postpass.py holds the two-plane post-pass to, with its helpers.

Part 1: gaussian_filter_device on k planes == the oracle == scipy.ndimage.gaussian_filter, bit for bit.  Along the leading axis
the reflection period is 2 k = 2 .. 16 while the radius goes to 100: the indices fold many times, and the single-plane inputs
make the weight that lands on every output plane readable.

Part 2: every output of evk_objective_gradsums_planes_f32 against math.fsum of the float64 terms of the same float32 arrays,
within REL * sum |terms|.  The kernel adds at most ceil(npix / 131072) = 3 terms per thread serially (481 x 641; one or two on
the other shapes), then a 6-level shuffle tree, 4 wave partials, at most 2 block partials per thread of the final kernel and the
same tree again: under 25 roundings of 2^-53 each, < 3e-15 * sum |terms|, and the device exp() is good to an ulp or two; REL =
1e-13 leaves the margin the two-plane file leaves.  Plane i is scaled by 2^i (exact in float32), so that a swapped or shifted
output slot is wrong by a factor and not by a rounding.

Part 3: the public objectives on a real IWE / dIWE of each parametric warp at every blur sigma, the fused ones and those wider
than EVK_MAX_RADIUS.  Values against the oracle objective on the same float32 IWE.  Gradients within 2e-5 of the largest
component (2e-4 for soe and sosa) of two references: the formulas of tests/_motion_models_np.py with the blurred images stored
as float32 -- what scipy returns for the float32 images and what the library computes bit for bit (part 1) -- and the same
formulas on float64 copies of the images (M.variance_grad, M.gradsums).  The second is further away by what the float32
rounding of the blurred images explains, and that is no small thing at a wide blur: every event's dIWE stencil sums to zero, so
sum g(a) d_i cancels the more the smoother g(blur(a)) is.  Evaluated on the CPU alone (both references, float64 sums, the
images of tests/_motion_models*_np.py for these scenes), the two lie apart by at most 4.3e-6 of the largest component up to
sigma 3.25 for every objective, but at sigma 8 / 8.25 / 20 by 1.1e-5 / 1.7e-5 / 4.9e-4 for soe, 2.6e-5 / 2.9e-5 / 1.5e-4 for
isoa, 4.1e-6 / 5.0e-6 / 3.2e-5 for sosa and 2.1e-6 / 3.8e-6 / 1.3e-5 for sos, rms and variance: more than the bound itself.
So the float64 comparison allows, on top of the bound, exactly that distance for the case at hand (float32_margin: computed
from the two references, never from the library's output); the float32-stored comparison allows nothing on top.  isoa's mask
is taken from the float32 blurred IWE, the image the kernel thresholds: a pixel within a float32 rounding of 0.5 is not the
float64 formula's to decide."""
import numpy as np
import pytest
import torch

import _motion_models8_np as M8
import _motion_models_np as M
from oracle import reference_np as R
from test_gpu_postpass import (F64, REL, SIGMAS, _close_f, _lib, _oracle_on, gfun_of, lines, make, oblur, sigma_of,  # noqa: F401
                               weights, xsum)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------- part 1: the 3-D filter on k planes
FILTER_PLANES = (1, 3, 4, 5, 8)
FILTER_RADII = (0, 1, 4, 5, 12, 13, 32, 33, 40, 100)
SENSOR_RADII = (4, 13, 40)          # the (181, 241) canvas with 3 and 8 planes: the compile-time radius, a generic one, the wide filter


def one_plane(k, plane, h, w, seed):
    """(k, h, w) zeros but for plane `plane`, which holds spikes on the rows and columns of lines()."""
    a = np.zeros((k, h, w), np.float32)
    ys, xs = lines(h), lines(w)
    a[plane, ys[:, None], xs[None, :]] = np.random.default_rng(seed).uniform(0.25, 1.5, (len(ys), len(xs))).astype(np.float32)
    return a


def filter_inputs(k, h, w, seed):
    """[(kind, (k, h, w) float32)]: noise, spikes, and one non-zero plane: the first, the last and (k >= 3) a middle one."""
    out = [(kind, make(kind, k, h, w, seed)) for kind in ("noise", "spikes")]
    for plane in sorted({0, k - 1} | ({k // 2} if k >= 3 else set())):
        out.append(("plane%d" % plane, one_plane(k, plane, h, w, seed + 1 + plane)))
    return out


def filter_shapes(k, r):
    return [(k, 1, 1), (k, 3, 5), (k, 37, 53)] + ([(k, 181, 241)] if k in (3, 8) and r in SENSOR_RADII else [])


def same_bits(got, ref, what):
    """Bit equality of two float32 stacks; the message names the output planes that differ and the first such pixel."""
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        planes = sorted({int(i) for i in np.argwhere(bad)[:, 0]})
        raise AssertionError((what, "output planes", planes, "pixels", int(bad.sum()), "first", at, float(got[at]), float(ref[at])))


@pytest.mark.parametrize("r", FILTER_RADII)
@pytest.mark.parametrize("k", FILTER_PLANES)
def test_gaussian_filter_device_k_planes_bit_exact(k, r):
    from event_utils_amd.contrast_max.objectives import gaussian_filter_device
    _lib()
    for shape in filter_shapes(k, r):
        for kind, a in filter_inputs(*shape, 100 * r + k):
            got = gaussian_filter_device(torch.from_numpy(a).cuda(), sigma_of(r)).cpu().numpy()
            same_bits(got, oblur(a, r), ("k", k, "radius", r, "shape", shape, kind))


# --------------------------------------------------------- part 2: evk_objective_gradsums_planes_f32 against exact sums
SUM_SHAPES = ((1, 1), (1, 255), (1, 256), (1, 257), (181, 241), (363, 362))     # 363 x 362 = 131 072 + 334: a second sweep
SUM_MATRIX = [(k, s) for k in range(1, 9) for s in SUM_SHAPES] + [(k, (481, 641)) for k in (3, 8)]     # 2.35 sweeps
SENTINEL = -12345.6789


def sums_inputs(kind, k, h, w):
    """a (h, w) and d (k, h, w) float32 of one kind, plane i of d scaled by 2^i."""
    img = make(kind, 1 + k, h, w, 31 * k + 7919 * h + w + len(kind))
    d = img[1:] * np.exp2(np.arange(k, dtype=np.float32))[:, None, None]
    return np.ascontiguousarray(img[0]), np.ascontiguousarray(d)


def slot_names(k):
    return ["S a", "S a^2", "S g(a)"] + ["S d%d" % i for i in range(k)] + ["S g(a) d%d" % i for i in range(k)]


def weight_functions(a):
    """(gfun, gparam): identity, exp, the step at the median and at a value that a holds (the comparison is strict), exp(-3 a)."""
    return ((0, 0.0), (1, 0.0), (2, float(np.median(a))), (2, float(np.sort(a, axis=None)[(2 * a.size) // 3])), (3, 3.0))


@pytest.mark.parametrize("kind", ("noise", "negative", "spikes"))
@pytest.mark.parametrize("k,shape", SUM_MATRIX, ids=["k%d-%dx%d" % (k, s[0], s[1]) for k, s in SUM_MATRIX])
def test_gradsums_planes_against_exact_sums(k, shape, kind):
    """All 3 + 2 k outputs [S a, S a^2, S g(a), S d_i .., S g(a) d_i ..] for every weight function; the slots past them (the
    caller's buffer has 19) are not written."""
    D, L = _lib()
    h, w = shape
    a, d = sums_inputs(kind, k, h, w)
    dev = torch.device("cuda", 0)
    ad, dd = torch.from_numpy(a).to(dev), torch.from_numpy(d).to(dev)
    out = torch.empty(19, dtype=torch.float64, device=dev)
    scratch, nbytes = D.reduce_scratch(dev)
    a64, d64 = a.astype(F64), d.astype(F64)
    base = [xsum(a64), xsum(a64 * a64)]
    sd = [xsum(d64[i]) for i in range(k)]
    names = slot_names(k)
    for gfun, gparam in weight_functions(a):
        out.fill_(SENTINEL)
        L.call("evk_objective_gradsums_planes_f32", D.ptr(ad), D.ptr(dd), k, h, w, gfun, float(gparam), D.ptr(out), D.ptr(scratch),
               nbytes, D.stream())
        got = out.cpu().numpy()
        g = gfun_of(gfun, a, gparam)
        ref = base + [xsum(g)] + sd + [xsum(g * d64[i]) for i in range(k)]
        for j, (s, scale) in enumerate(ref):
            assert abs(got[j] - s) <= REL * scale, ("slot", j, names[j], "k", k, shape, kind, "gfun", gfun, gparam, got[j], s,
                                                    got[j] - s, REL * scale)
        assert np.all(got[3 + 2 * k:] == SENTINEL), ("written past 3 + 2 k", k, shape, kind, gfun, got[3 + 2 * k:])


# ------------------------------------------------- part 3: the public objectives on k-plane images at every blur sigma
WARPS = ("rotation", "xyztheta", "angular_velocity", "planar_flow")


def warp_setup(name):
    """(warp, numpy model module, its model id, parameters, keywords of its iwe()) as the motion-model tests build them."""
    import event_utils_amd as E
    if name == "rotation":
        return E.pure_rotation_warp(), M, M.ROTATION, M.ROT_TRUTH * 0.9, {}
    if name == "xyztheta":
        return E.xyztheta_warp(center=M.XYZ_CENTER), M, M.XYZTHETA, M.XYZ_TRUTH * 0.9, {"center": M.XYZ_CENTER}
    if name == "angular_velocity":
        return E.angular_velocity_warp(M8.K_DEFAULT), M8, M8.ANGVEL, M8.AV_TRUTH * 0.9, {}
    return E.planar_flow_warp(center=M8.PF_CENTER), M8, M8.PLANAR, M8.PF_TRUTH * 0.9, {"center": M8.PF_CENTER}


def scene_events(name):
    """The model's synthetic scene, 20 000 events, with seeded +-1 polarities (so that use_polarity changes the image)."""
    _, mod, model, _, _ = warp_setup(name)
    seed = 40 + WARPS.index(name)
    x, y, t, p = mod.scene(model, n=20000, seed=seed)
    return x, y, t, p * (np.random.default_rng(seed).integers(0, 2, len(p)) * 2 - 1)


class Images:
    """IWE and dIWE of one warp for both polarity settings: float32 host arrays (get_iwe on device events), their device
    copies, and float64 copies for the formulas."""

    def __init__(self, name):
        import event_utils_amd as E
        self.name = name
        self.warp, _, _, q, _ = warp_setup(name)
        ev = E.DeviceEvents.from_arrays(*scene_events(name))
        self.host, self.dev, self.f64 = {}, {}, {}
        for pol in (True, False):
            iwe, d_iwe = E.get_iwe(q, ev, None, None, None, self.warp, (180, 240), compute_gradient=True, use_polarity=pol)
            assert iwe.dtype == d_iwe.dtype == np.float32 and iwe.shape == (181, 241) and d_iwe.shape == (self.warp.dims, 181, 241)
            assert np.abs(iwe).sum() > 100 and all(np.abs(c).sum() > 0 for c in d_iwe), name
            self.host[pol] = (iwe, d_iwe)
            self.dev[pol] = (torch.from_numpy(iwe).cuda(), torch.from_numpy(d_iwe).cuda())
            self.f64[pol] = (iwe.astype(F64), d_iwe.astype(F64))


_IMAGES = {}


@pytest.fixture(params=WARPS)
def images(request):
    _lib()
    if request.param not in _IMAGES:
        _IMAGES[request.param] = Images(request.param)
    return _IMAGES[request.param]


def close_g(g, rg, dims, what, rel=2e-5, margin=0.0):
    """_close_g of tests/test_gpu_postpass.py over `dims` components (+ `margin`, see float32_margin)."""
    g, rg = np.asarray(g, dtype=F64), np.asarray(rg, dtype=F64)
    assert g.shape == rg.shape == (dims,), (what, g.shape, rg.shape)
    err = np.abs(g - rg)
    assert err.max() <= rel * np.max(np.abs(rg)) + margin + 1e-9, (what, "component", int(err.argmax()), g, rg,
                                                                    err / np.max(np.abs(rg)), margin)


def float32_margin(rg64, rg32):
    """What the float32 rounding of the blurred images explains of the distance to the float64 formula: the distance between
    that formula on float64 blurs and on float32-stored blurs (scipy on the float32 arrays), both summed in float64."""
    return float(np.max(np.abs(np.asarray(rg64) - np.asarray(rg32))))


def variance_grad_f32(hi, hd, s, exact):
    """M.variance_grad with the blurs stored as float32 (scipy keeps the dtype of the float32 images) and float64 sums."""
    a, d = (v.astype(F64) for v in M.blurred(hi, hd, s, exact, not exact))
    return -np.array([np.mean(2.0 * (a - a.mean()) * d[i]) for i in range(d.shape[0])])


def gradsums_f32(hi, hd, s, g, blur_iwe):
    """M.gradsums with the blurs stored as float32 and float64 sums."""
    a, d = (v.astype(F64) for v in M.blurred(hi, hd, s, True, blur_iwe))
    ga = g(a)
    return np.array([np.sum(ga * d[i]) for i in range(d.shape[0])])


def gradient_refs(name, hi, hd, i64, d64, s):
    """The gradient formula of the objective `name` (the `cases` of test_other_objectives_gradients_have_dims_components) at blur
    sigma s -> (on float64 copies of the images by M.gradsums, on the float32 images with float32-stored blurs)."""
    n = i64.size
    if name in ("sos", "rms"):
        g, blur_iwe, scale = (lambda a: a), False, -2.0 / n
    elif name == "soe":
        g, blur_iwe, scale = np.exp, True, -1.0 / n
    elif name == "isoa":        # the mask of the float32 blurred IWE, the image the kernel thresholds, in both
        mask = (M.blurred(hi, hd[:1], s, True, True)[0] > np.float32(0.5)).astype(F64)
        g, blur_iwe, scale = (lambda a: mask), True, -1.0
    else:
        assert name == "sosa"
        g, blur_iwe, scale = (lambda a: np.exp((-3.0 * a.astype(np.float32)).astype(F64))), True, 3.0
    return scale * M.gradsums(i64, d64, s, g, blur_iwe)[0], scale * gradsums_f32(hi, hd, s, g, blur_iwe)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_variance_objective_on_k_planes_at_every_sigma(images, sigma):
    import event_utils_amd as E
    (di, dd), (hi, hd), (i64, d64) = images.dev[True], images.host[True], images.f64[True]
    w = images.warp
    s = 1.0 if sigma is None else sigma
    for exact in (True, False):
        o = E.variance_objective()
        o.reference_exact = exact
        f = o.evaluate_function(iwe=di, blur_sigma=sigma)
        assert isinstance(f, np.float32)
        _close_f(f, R.variance_objective().evaluate_function(iwe=hi, blur_sigma=sigma), ("variance f", images.name, sigma, exact))
        g = o.evaluate_gradient(iwe=di, d_iwe=dd, blur_sigma=sigma, warpfunc=w)
        rg, rg32 = M.variance_grad(i64, d64, s, exact), variance_grad_f32(hi, hd, s, exact)
        close_g(g, rg32, w.dims, ("variance g, float32 blurs", images.name, sigma, exact))
        close_g(g, rg, w.dims, ("variance g", images.name, sigma, exact), margin=float32_margin(rg, rg32))


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("name", ("sos", "soe", "moa", "isoa", "sosa", "r1", "rms"))
def test_other_objectives_on_k_planes_at_every_sigma(images, name, sigma):
    from event_utils_amd.contrast_max import objectives as O
    o = getattr(O, name + "_objective")()
    pol = o.use_polarity
    (di, dd), (hi, hd), (i64, d64) = images.dev[pol], images.host[pol], images.f64[pol]
    w = images.warp
    ro = _oracle_on(getattr(R, name + "_objective")(), hi, hd)
    assert ro.use_polarity == pol and ro.default_blur == o.default_blur
    f = o.evaluate_function(iwe=di, blur_sigma=sigma)
    rf = ro.evaluate_function(None, None, None, None, None, None, None, blur_sigma=sigma)
    if name == "isoa":          # a count of the same float32 values against the same threshold: exact
        assert int(f) == int(rf), (images.name, sigma, f, rf)
    else:
        _close_f(f, rf, (name, images.name, sigma))
    if o.has_derivative:
        s = o.default_blur if sigma is None else sigma
        g = o.evaluate_gradient(iwe=di, d_iwe=dd, blur_sigma=sigma, warpfunc=w)
        rel = 2e-4 if name in ("soe", "sosa") else 2e-5
        rg, rg32 = gradient_refs(name, hi, hd, i64, d64, s)
        close_g(g, rg32, w.dims, (name, "float32 blurs", images.name, sigma), rel)
        close_g(g, rg, w.dims, (name, images.name, sigma), rel, margin=float32_margin(rg, rg32))
    else:
        assert o.evaluate_gradient(iwe=di, d_iwe=dd, blur_sigma=sigma) is None
