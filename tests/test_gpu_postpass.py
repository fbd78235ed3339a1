"""GPU (-m gpu): the fused objective post-pass -- k_post_fused (evk_imgops.hip) with blur_tile_fill, blur_tiles_fill and
reflect_idx (evk_img.h) -- and the standalone blur, against a float64 oracle on the very same float32 arrays.

The blurred planes come from oracle.reference_np.gaussian_filter_reflect (pinned bit for bit to scipy.ndimage.gaussian_filter
where scipy imports); every reference sum is math.fsum over the float64 terms, i.e. exact.  The device adds its doubles in a
tree at most ~60 levels deep (error < 7e-15 * sum |terms|), so a raw sum must lie within REL * sum |terms| of the exact one.  On
the sparse inputs (a few dozen spikes) that bound is far below one float32 ulp of a single blurred pixel: a wrong tap, halo,
reflection, channel mix or tile seam fails it.  Derived values (mean, var, gradients) are held to REL times the magnitude of the
terms they are built from, since var and the gradients cancel.  The max and the count are exact.

The matrix walks every code path of the kernel: the compile-time radius 4 and the generic one; the three-planes-in-LDS layout of
the gradient modes (radius <= 12) and the one-plane-at-a-time one (13..32); single and repeated (modulo) reflection, on images
shorter than the radius; the grid-stride loop once the tiles outnumber the reduction slots; the row window of the row-sharded
entry.  Part 2 pins the public objectives at every blur sigma, including those wider than the fused kernels take
(include/evk.h: EVK_MAX_RADIUS), which the Python layer composes from the wide blur and the un-blurred reductions.

This file stops at two derivative planes.  The plane-generic sums of the parametric warps (evk_objective_gradsums_planes_f32,
1..8 planes) and the 3-D filter on (k, H, W) stacks are pinned the same way, with these helpers, in
tests/test_gpu_postpass_planes.py."""
import math

import numpy as np
import pytest
import torch

from oracle import reference_np as R

pytestmark = pytest.mark.gpu

try:
    from scipy import ndimage as _ndi
except ImportError:         # the oracle alone then
    _ndi = None

REL = 1e-13
MIX, BLUR_IWE = 1, 2
RADII = (-1, 0, 1, 4, 5, 12, 13, 32)
SHAPES = ((1, 1), (1, 300), (300, 1), (3, 5), (31, 33), (32, 32), (33, 65), (181, 241))
SENSOR_SHAPES = ((181, 241), (481, 641))      # canvases of a (180, 240) / (480, 640) sensor: also a real IWE
# every radius on the shapes above; the 481 x 641 canvas (300 k pixels, exact sums cost) at the radii that change the code path
MATRIX = [(r, s) for r in RADII for s in SHAPES] + [(r, (481, 641)) for r in (-1, 4, 12, 13, 32)]
F64 = np.float64


def _lib():
    from event_utils_amd import _device as D, _lib as L
    torch.cuda.set_device(0)
    return D, L


def sigma_of(r):
    """blur_sigma whose scipy radius int(4 sigma + 0.5) is r (r = 0: sigma 0.1, a 1-tap kernel)."""
    return 0.1 if r == 0 else r / 4.0


def weights(r):
    """(host weights, radius) of the library for radius r; (None, -1) = no blur."""
    from event_utils_amd.contrast_max.objectives import _blur_kernel
    if r < 0:
        return None, -1
    w, radius = _blur_kernel(sigma_of(r))
    assert radius == r
    return w, radius


def oblur(a, r):
    """scipy.ndimage.gaussian_filter(a, sigma_of(r)) of a float32 array by the oracle (3-D: the channel-mixing filter of the
    (2, H, W) dIWE, quirk Q4); r < 0: a itself."""
    if r < 0:
        return a
    b = R.gaussian_filter_reflect(a, sigma_of(r))
    if _ndi is not None:
        ref = _ndi.gaussian_filter(a, sigma_of(r))
        assert ref.dtype == b.dtype == np.float32 and np.array_equal(ref.view(np.uint32), b.view(np.uint32)), r
    return b


def lines(n):
    """Rows (columns) of the spikes: both edges and within a radius of them, the 32-pixel tile seams, the middle."""
    cand = {0, 1, 2, 3, 5, 8, 13, 31, 32, 63, 64, n // 2, n - 1, n - 2, n - 4, n - 9, n - 14, n - 33}
    return np.array(sorted(c for c in cand if 0 <= c < n))


def make(kind, planes, h, w, seed):
    """(planes, h, w) float32 inputs; the values keep exp(v) and exp(-3 v) finite in float64."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return (rng.normal(size=(planes, h, w)) * 0.5 + 0.75).astype(np.float32)
    if kind == "negative":
        return (-rng.uniform(0.25, 2.0, size=(planes, h, w))).astype(np.float32)
    if kind == "spikes":
        a = np.zeros((planes, h, w), np.float32)
        ys, xs = lines(h), lines(w)
        a[:, ys[:, None], xs[None, :]] = rng.uniform(0.25, 1.5, size=(planes, len(ys), len(xs))).astype(np.float32)
        a[:, 0, 0] = 4.0     # the largest value of every plane lies in the first tile
        return a
    assert kind == "iwe"
    import event_utils_amd as E
    from event_utils_amd.contrast_max.objectives import iwe_device
    n = h * w // 2
    x = rng.uniform(1, w - 2, n).astype(np.float32); y = rng.uniform(1, h - 2, n).astype(np.float32)
    t = np.sort(rng.uniform(0, 0.1, n)).astype(np.float32)
    p = (rng.integers(0, 2, n) * 2 - 1).astype(np.float32)
    iwe, diwe = iwe_device(np.array([20.0, -12.0]), E.DeviceEvents.from_arrays(x, y, t, p), (h - 1, w - 1), True, True,
                           (h - 1, w - 1))
    return torch.cat([iwe[None], diwe]).cpu().numpy()


def kinds(shape):
    return ("noise", "spikes", "negative") + (("iwe",) if shape in SENSOR_SHAPES else ())


class Case:
    """Host inputs img = (3, h, w) [iwe, d0, d1] of one kind and shape, their oracle blurs at radius r (computed on first use)
    and the exact sums taken of them (memoised: the flag combinations share most of their terms)."""

    def __init__(self, kind, h, w, r):
        self.img, self.r, self.h, self.w, self._m = make(kind, 3, h, w, 7919 * h + w + len(kind)), r, h, w, {}

    def memo(self, key, fn):
        if key not in self._m:
            self._m[key] = fn()
        return self._m[key]

    @property
    def v(self):                # blur(iwe)
        return self.memo("v", lambda: oblur(self.img[0], self.r))

    def d(self, flags):         # the blurred dIWE: one 3-D filter with EVK_POST_MIX (Q4), channel by channel without
        if self.r < 0:
            return self.img[1:]
        if flags & MIX:
            return self.memo("dm", lambda: oblur(self.img[1:], self.r))
        return self.memo("dc", lambda: np.stack([oblur(self.img[1], self.r), oblur(self.img[2], self.r)]))

    def a(self, flags):         # the IWE the gradient weights: blurred with EVK_POST_BLUR_IWE
        return self.v if flags & BLUR_IWE else self.img[0]

    def xsum(self, key, fn):
        return self.memo(("sum",) + key, lambda: xsum(fn()))

    def value_sums(self, rows=slice(None)):
        """Exact [S v, S v^2] over `rows`."""
        k = (rows.start, rows.stop)
        return [self.xsum(("v",) + k, lambda: self.v[rows].astype(F64)),
                self.xsum(("vv",) + k, lambda: self.v[rows].astype(F64) ** 2)]

    def grad_sums(self, flags, gfun=0, gparam=0.0, rows=slice(None)):
        """Exact [S g, S d0, S d1, S g d0, S g d1] over `rows` with g = gfun(a), a and d as `flags` select."""
        ka = ("a", bool(flags & BLUR_IWE), gfun, gparam, rows.start, rows.stop)
        kd = ("d", self.r >= 0 and bool(flags & MIX), rows.start, rows.stop)
        g = lambda: gfun_of(gfun, self.a(flags)[rows], gparam)          # noqa: E731
        d = lambda i: self.d(flags)[i, rows].astype(F64)                # noqa: E731
        return [self.xsum(ka, g), self.xsum(kd + (0,), lambda: d(0)), self.xsum(kd + (1,), lambda: d(1)),
                self.xsum(ka + kd + (0,), lambda: g() * d(0)), self.xsum(ka + kd + (1,), lambda: g() * d(1))]


_CACHE = {}


def case(kind, h, w, r):
    key = (kind, h, w, r)
    if key not in _CACHE:
        if len(_CACHE) > 16:
            _CACHE.clear()
        _CACHE[key] = Case(kind, h, w, r)
    return _CACHE[key]


def xsum(t):
    """(exact sum, sum of |terms|) of float64 terms."""
    t = np.asarray(t, dtype=F64).ravel()
    return math.fsum(t.tolist()), float(np.abs(t).sum())


def near(got, ref, scale, what):
    assert abs(float(got) - ref) <= REL * scale, (what, float(got), ref, float(got) - ref, REL * scale)


def check_raw(got, sums, what):
    for k, (g, (s, a)) in enumerate(zip(got, sums)):
        near(g, s, a, (what, k))


def check_value(out, sums, n, what):
    """out[0..3] = [mean v, var v, S v, S v^2] (mode 0 of the fused entries) against the exact [S v, S v^2]."""
    (s0, a0), (s1, a1) = sums
    check_raw(out[2:4], sums, (what, "raw"))
    mean = s0 / n
    near(out[0], mean, a0 / n, (what, "mean"))
    near(out[1], s1 / n - mean * mean, a1 / n + 2 * (a0 / n) ** 2, (what, "var"))


def check_mean_var(out, sums, n, what):
    """out[0], out[1] = mean v, var v (the value half of evk_objective_variance_fg_f32)."""
    (s0, a0), (s1, a1) = sums
    near(out[0], s0 / n, a0 / n, (what, "mean"))
    near(out[1], s1 / n - (s0 / n) ** 2, a1 / n + 2 * (a0 / n) ** 2, (what, "var"))


def check_grad(out, sums, n, what):
    """out[0], out[1] = 2/n (S g d_i - mean g * S d_i) against the exact sums."""
    mean, am = sums[0][0] / n, sums[0][1] / n
    for i in range(2):
        ref = 2.0 / n * (sums[3 + i][0] - mean * sums[1 + i][0])
        near(out[i], ref, 2.0 / n * (sums[3 + i][1] + 2 * am * sums[1 + i][1]), (what, "g%d" % i))
    return mean, am


def gfun_of(gfun, a, gparam):
    a64 = a.astype(F64)
    if gfun == 0:
        return a64
    if gfun == 1:
        return np.exp(a64)
    if gfun == 2:
        return np.where(a64 > gparam, 1.0, 0.0)
    return np.exp((np.float32(-gparam) * a).astype(F64))        # the reference forms -p * iwe in float32 first


# ------------------------------------------------------------------------------------------------- part 1: raw entries
def _ids(rs):
    r, s = rs
    return "r%d-%dx%d" % (r, s[0], s[1])


@pytest.mark.parametrize("r,shape", MATRIX, ids=[_ids(m) for m in MATRIX])
def test_variance_value_gradient_and_fg(r, shape):
    """evk_objective_variance_f32 / _grad_f32 / _fg_f32 at every radius and flag combination against the oracle."""
    D, L = _lib()
    h, w = shape
    n = h * w
    wts, radius = weights(r)
    wp = D.host_ptr(wts) if wts is not None else None
    dev = torch.device("cuda", 0)
    out, (scratch, nbytes) = D.out4(dev), D.reduce_scratch(dev)
    for kind in kinds(shape):
        c = case(kind, h, w, r)
        img = torch.from_numpy(c.img).to(dev)
        L.call("evk_objective_variance_f32", D.ptr(img), h, w, wp, radius, D.ptr(out), D.ptr(scratch), nbytes, D.stream())
        check_value(out.cpu().numpy(), c.value_sums(), n, (kind, "value"))
        for flags in (0, MIX, BLUR_IWE, MIX | BLUR_IWE):
            sums = c.grad_sums(flags)
            L.call("evk_objective_variance_grad_f32", D.ptr(img), D.ptr(img[1:]), h, w, wp, radius, flags, D.ptr(out),
                   D.ptr(scratch), nbytes, D.stream())
            got = out.cpu().numpy()
            mean, am = check_grad(got, sums, n, (kind, "grad", flags))
            near(got[2], mean, am, (kind, "grad mean", flags))
            near(got[3], sums[0][0], sums[0][1], (kind, "grad S a", flags))
            L.call("evk_objective_variance_fg_f32", D.ptr(img), D.ptr(img[1:]), h, w, wp, radius, flags, D.ptr(out),
                   D.ptr(scratch), nbytes, D.stream())
            got = out.cpu().numpy()
            check_grad(got, sums, n, (kind, "fg", flags))
            check_mean_var(got[2:4], c.value_sums(), n, (kind, "fg", flags))


def check_stats(D, L, img, c, p, what, radius, wp):
    """evk_objective_stats_f32 -> [mean, var, S v, S v^2, S exp v, S exp(-p v), count(v > thresh), max v]; thresh is a value
    that occurs in v, so that > and >= differ."""
    dev = img.device
    out, (scratch, nbytes) = D.out4(dev, 8), D.reduce_scratch(dev)
    v = c.v
    u = np.unique(v)
    thresh = float(u[(2 * len(u)) // 3])
    L.call("evk_objective_stats_f32", D.ptr(img), c.h, c.w, wp, radius, float(p), thresh, D.ptr(out), D.ptr(scratch), nbytes,
           D.stream())
    got = out.cpu().numpy()
    check_value(got[:4], c.value_sums(), c.h * c.w, what)
    ev = c.xsum(("exp",), lambda: np.exp(v.astype(F64)))
    enp = c.xsum(("exp-p", p), lambda: np.exp(-float(p) * v.astype(F64)))
    check_raw(got[4:6], [ev, enp], (what, "exp"))
    assert got[6] == float(np.count_nonzero(v.astype(F64) > thresh)), (what, "count", got[6], thresh)
    assert got[7] == float(v.max()), (what, "max", got[7], v.max())


def check_gradsums(D, L, img, c, flags, gfun, gparam, what, radius, wp):
    """evk_objective_gradsums_f32 -> [g0, g1, mean g, S g, S d0, S d1, S g d0, S g d1] with g = gfun(a)."""
    dev = img.device
    out, (scratch, nbytes) = D.out4(dev, 8), D.reduce_scratch(dev)
    L.call("evk_objective_gradsums_f32", D.ptr(img), D.ptr(img[1:]), c.h, c.w, wp, radius, flags, gfun, float(gparam),
           D.ptr(out), D.ptr(scratch), nbytes, D.stream())
    got = out.cpu().numpy()
    sums = c.grad_sums(flags, gfun, gparam)
    check_raw(got[3:8], sums, (what, "raw"))
    mean, am = check_grad(got, sums, c.h * c.w, what)
    near(got[2], mean, am, (what, "mean"))


@pytest.mark.parametrize("r,shape", MATRIX, ids=[_ids(m) for m in MATRIX])
def test_stats_and_gradsums(r, shape):
    """The reductions of the six other objectives: stats at p = 3 and 0.5 (exact max and count), gradsums with every weight
    function, with and without channel mixing and blurred IWE."""
    D, L = _lib()
    h, w = shape
    wts, radius = weights(r)
    wp = D.host_ptr(wts) if wts is not None else None
    for kind in kinds(shape):
        c = case(kind, h, w, r)
        img = torch.from_numpy(c.img).cuda()
        for p in (3.0, 0.5):
            check_stats(D, L, img, c, p, (kind, "stats", p), radius, wp)
        for gfun, gparam in ((0, 0.0), (1, 0.0), (2, float(np.median(c.v))), (3, 3.0)):
            for flags in (0, MIX, BLUR_IWE, MIX | BLUR_IWE):
                check_gradsums(D, L, img, c, flags, gfun, gparam, (kind, "gradsums", gfun, flags), radius, wp)


@pytest.mark.parametrize("r", (4, 13, 32))
@pytest.mark.parametrize("world", (1, 2, 3, 8))
def test_row_sharded_sums_against_the_oracle(world, r):
    """evk_objective_variance_rows_f32 on the row block (with halo) of each of `world` ranks: its raw sums are those of the
    whole image's oracle blur over the rank's OWN rows.  At radius 13 and 32 the blocks of 8 ranks are thinner than the halo."""
    from event_utils_amd import distributed as DD
    D, L = _lib()
    h, w = 181, 241
    wts, radius = weights(r)
    wp = D.host_ptr(wts)
    scratch, nbytes = D.reduce_scratch(torch.device("cuda", 0))
    sums_d = torch.zeros(8, dtype=torch.float64, device="cuda")
    for kind in ("spikes", "noise"):
        c = case(kind, h, w, r)
        img = torch.from_numpy(c.img).cuda()
        for mode, flags in ((0, 0), (1, MIX), (1, BLUR_IWE), (3, MIX), (3, MIX | BLUR_IWE)):
            for rank in range(world):
                y0, y1, lo, hi = DD.row_block(h, radius, rank, world)
                block = img[:(1 if mode == 0 else 3), lo:hi, :].contiguous()
                L.call("evk_objective_variance_rows_f32", D.ptr(block), mode, hi - lo, w, y0 - lo, y1 - lo, wp, radius, flags,
                       D.ptr(sums_d), D.ptr(scratch), nbytes, D.stream())
                got = sums_d.cpu().numpy()
                rows = slice(y0, y1)
                ref = c.value_sums(rows) if mode == 0 else c.grad_sums(flags, rows=rows)
                if mode == 3:
                    ref = ref + c.value_sums(rows)
                ref = ref + [(0.0, 0.0)] * (7 - len(ref))
                check_raw(got[:7], ref, (kind, mode, flags, rank))


@pytest.mark.parametrize("r", (4, 13))
def test_1080p_gradient_modes_and_capped_planes(r):
    """At 1081 x 1921: the gradient modes (three planes batched in LDS at radius 4, one at a time at 13), and the value of 1..8
    stacked planes (evk_objective_variance_planes_f32), whose grid is capped at 4096 / nplanes blocks and strides over the
    2074 tiles from 2 planes on."""
    D, L = _lib()
    h, w = 1081, 1921
    n = h * w
    wts, radius = weights(r)
    wp = D.host_ptr(wts)
    dev = torch.device("cuda", 0)
    out, (scratch, nbytes) = D.out4(dev), D.reduce_scratch(dev)
    c = case("spikes", h, w, r)
    img = torch.from_numpy(c.img).to(dev)
    for flags in (MIX, MIX | BLUR_IWE):
        sums = c.grad_sums(flags)
        for fn in ("evk_objective_variance_grad_f32", "evk_objective_variance_fg_f32"):
            L.call(fn, D.ptr(img), D.ptr(img[1:]), h, w, wp, radius, flags, D.ptr(out), D.ptr(scratch), nbytes, D.stream())
            got = out.cpu().numpy()
            check_grad(got, sums, n, (fn, flags))
            if fn.endswith("fg_f32"):
                check_mean_var(got[2:4], c.value_sums(), n, (fn, flags))
            else:
                near(got[3], sums[0][0], sums[0][1], (fn, "S a"))
    planes = make("spikes", 8, h, w, 11)
    planes[:, 500:540, 900:1000] += np.linspace(0.5, 2.0, 8, dtype=np.float32)[:, None, None]
    sums = []
    for k in range(8):
        v = oblur(planes[k], r).astype(F64)
        sums.append([xsum(v), xsum(v * v)])
    pd = torch.from_numpy(planes).to(dev)
    out32 = D.out4(dev, 32)
    for k in range(1, 9):
        L.call("evk_objective_variance_planes_f32", D.ptr(pd), k, h, w, wp, radius, D.ptr(out32), D.ptr(scratch), nbytes,
               D.stream())
        got = out32.cpu().numpy().reshape(8, 4)
        for j in range(k):
            check_value(got[j], sums[j], n, ("planes", k, j))


@pytest.mark.parametrize("r", (4, 13))
def test_4k_stats_and_gradsums_stride_over_8228_tiles(r):
    """2161 x 3841 has 68 x 121 = 8228 tiles against a grid cap of 4088 blocks for stats and gradsums (their finalised sums and
    running max live in the last 16 doubles of the reduction scratch, past the partial sums of the 4088 blocks)."""
    D, L = _lib()
    h, w = 2161, 3841
    wts, radius = weights(r)
    wp = D.host_ptr(wts)
    c = case("spikes", h, w, r)
    img = torch.from_numpy(c.img).cuda()
    check_stats(D, L, img, c, 3.0, ("4k stats", r), radius, wp)
    for gfun, gparam, flags in ((0, 0.0, MIX), (3, 3.0, MIX | BLUR_IWE)):
        check_gradsums(D, L, img, c, flags, gfun, gparam, ("4k gradsums", gfun, flags), radius, wp)


@pytest.mark.parametrize("r", (0, 1, 4, 5, 12, 13, 32, 33, 40, 100))
def test_gaussian_filter_device_bit_exact(r):
    """gaussian_filter_device (2-D and the 3-D channel-mixing filter) == the oracle == scipy, bit for bit, at every radius,
    past EVK_MAX_RADIUS (the wide blur) and longer than both sides of the image."""
    from event_utils_amd.contrast_max.objectives import gaussian_filter_device
    for shape in ((1, 1), (3, 5), (2, 37, 53), (181, 241), (2, 181, 241)):
        for kind in ("noise", "spikes"):
            a = make(kind, 1, shape[-2], shape[-1], r)[0] if len(shape) == 2 else make(kind, 2, shape[1], shape[2], r)
            got = gaussian_filter_device(torch.from_numpy(a).cuda(), sigma_of(r)).cpu().numpy()
            ref = oblur(a, r)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (r, shape, kind)


# ------------------------------------------------------------------------------ part 2: public objectives at every sigma
SIGMAS = (None, 0, 0.5, 2.5, 3.25, 8.0, 8.25, 20)


@pytest.fixture(scope="module")
def sensor_iwe():
    """A real (181, 241) IWE and dIWE of seeded sensor events: device tensors and their host copies."""
    img = make("iwe", 3, 181, 241, 21)
    return torch.from_numpy(img[0]).cuda(), torch.from_numpy(img[1:]).cuda(), img[0], img[1:]


def _oracle_on(robj, iwe, d_iwe):
    robj._iwe = lambda *a: (iwe, d_iwe)         # the oracle objective evaluated on exactly these arrays
    return robj


def _consistent_gradient(iwe, d_iwe, sigma):
    """reference_exact=False: mean(2 (v - mean v) blur(d_i)) with v = blur(iwe) and the channels blurred one by one."""
    if sigma > 0:
        iwe = R.gaussian_filter_reflect(iwe, sigma)
        d_iwe = np.stack([R.gaussian_filter_reflect(d_iwe[k], sigma) for k in range(2)])
    c = 2.0 * (iwe - np.mean(iwe))
    return -np.array([np.mean(c * d_iwe[k]) for k in range(2)])


def _close_f(f, rf, what):
    assert abs(float(f) - float(rf)) <= 2e-5 * abs(float(rf)) + 1e-12, (what, f, rf)


def _close_g(g, rg, what, rel=2e-5):
    g, rg = np.asarray(g, dtype=F64), np.asarray(rg, dtype=F64)
    assert g.shape == (2,) and np.max(np.abs(g - rg)) <= rel * np.max(np.abs(rg)) + 1e-9, (what, g, rg)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_variance_objective_at_every_sigma(sensor_iwe, sigma):
    import event_utils_amd as E
    di, dd, hi, hd = sensor_iwe
    s = 1.0 if sigma is None else sigma
    for exact in (True, False):
        o = E.variance_objective()
        o.reference_exact = exact
        ro = R.variance_objective()
        f = o.evaluate_function(iwe=di, blur_sigma=sigma)
        assert isinstance(f, np.float32)
        _close_f(f, ro.evaluate_function(iwe=hi, blur_sigma=sigma), ("variance f", sigma, exact))
        g = o.evaluate_gradient(iwe=di, d_iwe=dd, blur_sigma=sigma)
        rg = ro.evaluate_gradient(iwe=hi, d_iwe=hd, blur_sigma=sigma) if exact else _consistent_gradient(hi, hd, s)
        _close_g(g, rg, ("variance g", sigma, exact))


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("name", ("sos", "soe", "moa", "isoa", "sosa", "r1", "rms"))
def test_other_objectives_at_every_sigma(sensor_iwe, name, sigma):
    from event_utils_amd.contrast_max import objectives as O
    di, dd, hi, hd = sensor_iwe
    o, ro = getattr(O, name + "_objective")(), _oracle_on(getattr(R, name + "_objective")(), hi, hd)
    f = o.evaluate_function(iwe=di, blur_sigma=sigma)
    rf = ro.evaluate_function(None, None, None, None, None, None, None, blur_sigma=sigma)
    if name == "isoa":          # a count of the same float32 values against the same threshold: exact
        assert int(f) == int(rf), (sigma, f, rf)
    else:
        _close_f(f, rf, (name, sigma))
    if o.has_derivative:
        g = o.evaluate_gradient(iwe=di, d_iwe=dd, blur_sigma=sigma)
        rg = ro.evaluate_gradient(None, None, None, None, None, None, None, blur_sigma=sigma)
        _close_g(g, rg, (name, sigma), 2e-4 if name in ("soe", "sosa") else 2e-5)
    else:
        assert o.evaluate_gradient(iwe=di, d_iwe=dd, blur_sigma=sigma) is None


def test_event_driven_objectives_at_a_wide_blur():
    """blur_sigma = 10 (radius 40 > EVK_MAX_RADIUS) from the events: variance (value, gradient, both at once, the numeric
    gradient and a three-flow batch), sos and rms return the oracle's values instead of raising."""
    import event_utils_amd as E
    from event_utils_amd.contrast_max import objectives as O
    rng = np.random.default_rng(4)
    n, H, W = 60_000, 180, 240
    x = rng.uniform(1, W - 1, n).astype(np.float32); y = rng.uniform(1, H - 1, n).astype(np.float32)
    t = np.sort(rng.uniform(0, 0.1, n)).astype(np.float32)
    p = (rng.integers(0, 2, n) * 2 - 1).astype(np.float32)
    ev = E.DeviceEvents.from_arrays(x, y, t, p)
    d = [a.astype(F64) for a in (x, y, t, p)]
    prm, w, rw = np.array([30.0, -20.0]), E.linvel_warp(), R.linvel_warp()
    vo, rvo = E.variance_objective(), R.variance_objective()
    rvo.accum = "f64"
    rf = rvo.evaluate_function(prm, *d, rw, (H, W), 10.0)
    rg = rvo.evaluate_gradient(prm, *d, rw, (H, W), 10.0)
    _close_f(vo.evaluate_function(prm, ev, None, None, None, w, (H, W), 10.0), rf, "variance f")
    _close_g(vo.evaluate_gradient(prm, ev, None, None, None, w, (H, W), 10.0), rg, "variance g")
    fv, gv = vo.evaluate_function_and_gradient(prm, ev, None, None, None, w, (H, W), 10.0)
    _close_f(fv, rf, "variance fg f")
    _close_g(gv, rg, "variance fg g")
    fb = vo.evaluate_function_batch([prm, prm + 1.0, prm - 1.0], ev, None, None, None, w, (H, W), 10.0)
    _close_f(fb[0], rf, "variance batch")
    fn, gn = vo.evaluate_function_and_numeric_gradient(prm, ev, None, None, None, w, (H, W), 10.0)
    _close_f(fn, rf, "variance numeric")
    for name in ("sos", "rms"):
        o, ro = getattr(O, name + "_objective")(), getattr(R, name + "_objective")()
        ro.accum = "f64"
        _close_f(o.evaluate_function(prm, ev, None, None, None, w, (H, W), 10.0),
                 ro.evaluate_function(prm, *d, rw, (H, W), 10.0), name)
        _close_g(o.evaluate_gradient(prm, ev, None, None, None, w, (H, W), 10.0),
                 ro.evaluate_gradient(prm, *d, rw, (H, W), 10.0), name)


@pytest.mark.parametrize("sigma", (3.25, 10.0))
def test_native_bfgs_loop_at_a_wide_blur(sigma):
    """optimize_contrast(optimizer='evk_bfgs') at blur_sigma 3.25 (radius 13: the one-plane-at-a-time gradient path inside the
    library's loop) visits the points of the Python loops bit for bit; at 10 (radius 40) the library's loop declines and the
    Python loop composes the blur."""
    import bench
    import event_utils_amd as E
    from event_utils_amd.contrast_max.events_cmax import evk_bfgs, optimize_contrast
    H, W = 240, 320
    x, y, t, p = bench.structured_scene(7, 200_000, H, W)
    ev = E.DeviceEvents.from_arrays(x, y, t, p, precision="f32")
    args = (ev, None, None, None, E.linvel_warp(), (H, W), sigma)
    runs = {}
    for mode in ("native", "bound", "public"):
        o, tr = E.variance_objective(), []
        o.sensor_size, o.reference_exact, o.native_passes = (H, W), False, None
        xs = evk_bfgs(o, np.array([0.0, 0.0]), args, numeric_grads=False, trace=tr, native=mode == "native",
                      fast=mode != "public")
        assert (o.native_passes is not None) == (mode == "native" and sigma < 8.125), (mode, sigma)
        runs[mode] = (xs, tr)
    for other in ("bound", "public"):
        assert np.array_equal(runs["native"][0], runs[other][0]) and len(runs["native"][1]) == len(runs[other][1])
        for (xa, fa, ga), (xb, fb, gb) in zip(runs["native"][1], runs[other][1]):
            assert np.array_equal(xa, xb) and fa == fb and np.array_equal(ga, gb), (sigma, other)
    o = E.variance_objective()
    o.sensor_size, o.reference_exact, o.native_passes = (H, W), False, None
    a = optimize_contrast(ev, None, None, None, E.linvel_warp(), o, optimizer="evk_bfgs", numeric_grads=False,
                          blur_sigma=sigma, img_size=(H, W))
    assert bool(o.native_passes) == (sigma < 8.125) and np.array_equal(a, runs["native"][0])
