"""CPU (no GPU): the contrast (focus) loss of a dense flow field -- the numpy restatement the GPU tests compare against
(tests/_flow_contrast_np.py): its adjoint against central differences, the self-adjointness of the reflect blur that the adjoint
image rests on, a constant field against the project's linear-flow restatement (tests/_motion_models_np.py), batches; and the
library's new entry points: declared, exported, bound, plain C, refusing bad arguments."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _flow_contrast_np as C
import _motion_models_np as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evk_flowcm_warp_f32", "evk_flowcm_post_f32", "evk_flowcm_grad_f32")
TINY = (5, 6)
FD_STEP = 1e-6          # the step and the bound of tests/test_cpu_flow_loss.py
FD_TOL = 1e-5


def _tiny_scene():
    """About 40 events on a (5, 6) field, real-valued polarities so that use_polarity matters to more than the sign."""
    flow, x, y, t, p = C.scene(TINY[0], TINY[1], 40, seed=2)
    p = p * np.random.default_rng(12).uniform(0.5, 2.0, len(p))
    return flow, x, y, t, p


# ---- (a) the adjoint is the derivative -------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_polarity", (True, False), ids=("signed", "abs"))
@pytest.mark.parametrize("direction", C.DIRECTIONS)
@pytest.mark.parametrize("objective", C.OBJECTIVES)
@pytest.mark.parametrize("sigma", (0.0, 1.0))
def test_gradient_matches_central_differences(sigma, objective, direction, use_polarity):
    """Every one of the 2 x 5 x 6 components, float64, h = 1e-6: within 1e-5 of max |g|, the bound of the timestamp loss (these
    sixteen cases measured 1.7e-8 to 2.3e-7).  The loss is only piecewise smooth (an event that changes cell, or crosses the
    mask, changes the slope): no warped coordinate may come within h max |dt| of an integer, which the test asserts."""
    flow, x, y, t, p = _tiny_scene()
    xw, yw = C.warp(flow, x, y, t, direction)
    dt, _ = C.time_constants(t, direction)
    margin = min(np.abs(xw - np.round(xw)).min(), np.abs(yw - np.round(yw)).min())
    assert margin > 10 * FD_STEP * np.abs(dt).max()
    assert 10 < C.kept(flow, x, y, t, p, direction).sum() < len(t)          # some events leave, most stay
    kw = dict(sigma=sigma, objective=objective, direction=direction, use_polarity=use_polarity)
    _, g = C.loss_and_grad(flow, x, y, t, p, **kw)
    assert np.abs(g).max() > 0
    num = np.zeros_like(g)
    for k in range(flow.size):
        fp, fm = flow.copy(), flow.copy()
        fp.reshape(-1)[k] += FD_STEP
        fm.reshape(-1)[k] -= FD_STEP
        num.reshape(-1)[k] = (C.loss(fp, x, y, t, p, **kw) - C.loss(fm, x, y, t, p, **kw)) / (2 * FD_STEP)
    err = np.abs(num - g).max() / np.abs(g).max()
    print("sigma %g, %s, %s, use_polarity %s: max |fd - g| / max |g| = %.3g" % (sigma, objective, direction, use_polarity, err))
    assert err <= FD_TOL


@pytest.mark.parametrize("shape", ((6, 7), (25, 33)))
@pytest.mark.parametrize("sigma", (1.0, 8.5))
def test_the_reflect_blur_is_self_adjoint_and_keeps_constants(sigma, shape):
    """<blur(a), b> == <a, blur(b)> in float64, also where the radius (34 at sigma 8.5) exceeds the image and the reflection
    wraps several times: what step 6 rests on.  Each side sums the same products in another order: 1e-12 of sum |a| |b|."""
    rng = np.random.default_rng(5)
    a, b = rng.normal(size=shape), rng.normal(size=shape)
    lhs, rhs = np.sum(C.blur(a, sigma) * b), np.sum(a * C.blur(b, sigma))
    assert abs(lhs - rhs) <= 1e-12 * np.sum(np.abs(a)) * np.abs(b).max()
    np.testing.assert_allclose(C.blur(np.full(shape, 3.25), sigma), 3.25, rtol=1e-13)


def test_both_directions_is_the_sum():
    flow, x, y, t, p = C.scene(24, 32, 3000, seed=4)
    lf, gf = C.loss_and_grad(flow, x, y, t, p, 1.0, direction="forward")
    lb, gb = C.loss_and_grad(flow, x, y, t, p, 1.0, direction="backward")
    l2, g2 = C.loss_and_grad(flow, x, y, t, p, 1.0, direction="both")
    assert l2 == lf + lb and np.array_equal(g2, gf + gb) and lf != lb
    assert C.loss(flow, x, y, t, p, 1.0, direction="both") == l2


# ---- (b) pinned to the project's linear-flow restatement ---------------------------------------------------------------------
def _dyadic_scene(n=3000, shape=(24, 32)):
    """Coordinates on a 1/64 grid inside [0, W - 1] x [0, H - 1] and timestamps on a 2^-14 s grid: with a constant integer field
    every warped coordinate is a multiple of 2^-11 below 64, exact in float32 -- the linear-flow restatement casts the warped
    coordinates to float32 before it floors them (get_iwe's quirk Q7), the field restatement does not."""
    rng = np.random.default_rng(9)
    x = rng.integers(0, 64 * (shape[1] - 1) + 1, n) / 64.0
    y = rng.integers(0, 64 * (shape[0] - 1) + 1, n) / 64.0
    t = np.sort(rng.integers(0, 820, n)) / 16384.0
    p = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    return x, y, t, p


@pytest.mark.parametrize("sigma", (0.0, 1.0))
def test_constant_field_is_the_linear_flow(sigma):
    """A constant field (u, v) moves every event by (u, v) dt: the linear flow x' = x - dt vx at (vx, vy) = (-u, -v), t_ref =
    t_last, which tests/_motion_models_np.py has as xyztheta with vz = omega = 0.  Loss to 1e-10 relative, and sum_pixels
    dL/dflow[c] = -dL/dv_c to 1e-9 of the larger component (variance, reference_exact=False)."""
    shape = (24, 32)
    x, y, t, p = _dyadic_scene(shape=shape)
    assert x.min() >= 0 and x.max() <= shape[1] - 1 and y.min() >= 0 and y.max() <= shape[0] - 1
    u, v = 24.0, -16.0
    flow = np.empty((2,) + shape)
    flow[0], flow[1] = u, v
    params = (-u, -v, 0.0, 0.0)
    xw, yw = C.warp(flow, x, y, t)
    assert np.array_equal(xw, xw.astype(np.float32)) and np.array_equal(yw, yw.astype(np.float32))
    img, d_img = M.iwe(M.XYZTHETA, params, x, y, t, p, img_size=shape, sensor_size=shape)
    lm, gm = M.variance_f(img, sigma), M.variance_grad(img, d_img, sigma, reference_exact=False)[:2]
    lf, gf = C.loss_and_grad(flow, x, y, t, p, sigma, "variance", "forward")
    np.testing.assert_allclose(C.iwe(flow, x, y, t, p), img, rtol=0, atol=1e-12)
    assert lm < 0 and abs(lf - lm) <= 1e-10 * abs(lm)
    total = gf.sum(axis=(1, 2))
    print("loss %.12g against %.12g; summed gradient %s against %s" % (lf, lm, total, -gm))
    assert np.abs(total + gm).max() <= 1e-9 * np.abs(gm).max()


def test_f32_restatement_is_close_to_the_definition():
    """The float32 expressions move the image by float32 rounding only, apart from events that change cell: its mass agrees
    to 1e-5 relative, and the restatement fed its own float32 warp reproduces itself."""
    flow, x, y, t, p = C.scene(24, 32, 3000, seed=5)
    a, b = C.iwe(flow, x, y, t, p, use_polarity=False), C.iwe(flow, x, y, t, p, f32_coords=True, use_polarity=False)
    np.testing.assert_allclose(b.sum(), a.sum(), rtol=1e-5)
    xw, yw = C.warp(flow, x, y, t, f32_coords=True)
    assert xw.dtype == np.float32
    assert np.array_equal(C.iwe(flow, x, y, t, p, f32_coords=True, warped=(xw, yw), use_polarity=False), b)


def test_float32_images_cost_rounding_only_where_the_loss_is_measurable():
    """f32_images=True (the image, its blurs and the adjoint image stored as float32) against float64.  On the (24, 32) scene the
    difference is float32 rounding: 1e-6 of the loss and of the largest gradient component, with a Generator (values a unit in the
    last place off) as well.  Under a blur far wider than a (2, 3) field's canvas B is constant to 1e-4: what is left of var(B)
    and of the slopes of the adjoint image is of the size of that rounding, which is why the GPU fuzz takes its allowance for such
    cases from this difference (tools/fuzz_parity.py::flow_allowance)."""
    flow, x, y, t, p = C.scene(24, 32, 3000, seed=5)
    for objective in C.OBJECTIVES:
        l64, g64 = C.loss_and_grad(flow, x, y, t, p, 1.0, objective)
        for mode in (True, np.random.default_rng(1)):
            l32, g32 = C.loss_and_grad(flow, x, y, t, p, 1.0, objective, f32_images=mode)
            assert l32 != l64 and abs(l32 - l64) <= 1e-6 * abs(l64)
            assert np.abs(g32 - g64).max() <= 1e-6 * np.abs(g64).max()
    flow, x, y, t, p = C.scene(2, 3, 64, seed=6, speed=4.0)
    b = C.blur(C.iwe(flow, x, y, t, p, use_polarity=False), 8.5)
    assert np.ptp(b) <= 1e-4 * b.mean()
    l64, g64 = C.loss_and_grad(flow, x, y, t, p, 8.5, "variance", use_polarity=False)
    worst = max(np.abs(C.loss_and_grad(flow, x, y, t, p, 8.5, "variance", use_polarity=False, f32_images=mode)[1] - g64).max()
                for mode in [True] + [np.random.default_rng(2)] * 4)
    assert worst >= 1e-2 * np.abs(g64).max()
    # the plain storage changes nothing that is exactly representable: a zero image keeps a zero loss and gradient
    l0, g0 = C.loss_and_grad(flow, x, y, t, 0.0 * p, 1.0, "variance", f32_images=True)
    assert l0 == 0.0 and not g0.any()


# ---- (c) batches and the edge cases --------------------------------------------------------------------------------------------
def test_batch_of_three_with_an_empty_sample():
    flows, cols, offsets = [], [], [0]
    for n, seed in ((3001, 6), (0, 7), (517, 8)):
        flow, x, y, t, p = C.scene(24, 32, n, seed=seed)
        flows.append(flow)
        cols.append((x, y, t, p))
        offsets.append(offsets[-1] + n)
    x, y, t, p = (np.concatenate([c[k] for c in cols]) for k in range(4))
    for objective, direction in (("variance", "forward"), ("mean_square", "both")):
        losses, grads = C.batch_loss_and_grad(np.stack(flows), x, y, t, p, offsets, 1.0, objective, direction)
        for b in range(3):
            one, g = C.loss_and_grad(flows[b], *cols[b], 1.0, objective, direction)
            assert losses[b] == one and np.array_equal(grads[b], g)
        assert losses[1] == 0 and not grads[1].any() and losses[0] < 0 and losses[2] < 0
    assert not C.iwe(flows[1], *cols[1]).any()


def test_a_nan_polarity_adds_nothing_and_abs_drops_the_sign():
    flow, x, y, t, p = C.scene(24, 32, 500, seed=10)
    q = p.copy()
    q[5:300:7] = np.nan
    ok = ~np.isnan(q)
    ok[0] = ok[-1] = True                                    # the stream's ends set the time constants
    q[0], q[-1] = p[0], p[-1]
    assert np.array_equal(C.iwe(flow, x, y, t, q), C.iwe(flow, x[ok], y[ok], t[ok], q[ok]))
    assert np.array_equal(C.iwe(flow, x, y, t, p, use_polarity=False), C.iwe(flow, x, y, t, np.abs(p)))
    assert np.array_equal(C.iwe(flow, x, y, t, p, p_scale=-2.0), -2.0 * C.iwe(flow, x, y, t, p))


# ---- (d) library entry points --------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    from event_utils_amd.csrc import build
    build.build(verbose=False)
    from event_utils_amd import _lib
    text = open(os.path.join(ROOT, "include", "evk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert _lib.PROTOTYPES[name][1] is ctypes.c_int, name
    for name, value in (("EVK_FLOWCM_ABS", "1u"), ("EVK_FLOWCM_VARIANCE", "0"), ("EVK_FLOWCM_MEAN_SQUARE", "1")):
        assert re.search(r"#define %s %s\b" % (name, value), header), name
        assert getattr(_lib, name) == int(value.rstrip("u"))
    assert "bound = 2 M D Q n" in text and "|cell| <= Q n" in text          # both overflow bounds are written down


def test_prototypes_compile_from_c(tmp_path):
    """The new prototypes are plain C99 and agree with the exported symbols' names: their addresses are taken through the
    declared types, and an entry is called through its prototype with arguments it must refuse."""
    from event_utils_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "use_flowcm.c"
    src.write_text(r"""
#include <dlfcn.h>
#include <stdio.h>
#include "evk.h"
typedef int (*post_fn)(const float *, int, int, const double *, const double *, int, int, float *, float *, double *, void *,
                       int64_t, void *);
int main(int argc, char **argv) {
    void *h = dlopen(argv[1], RTLD_NOW);
    if (!h) { fprintf(stderr, "%s\n", dlerror()); return 2; }
    post_fn post = (post_fn)dlsym(h, "evk_flowcm_post_f32");
    if (!post) return 3;
    post_fn a = evk_flowcm_post_f32; (void)a;
    int (*b)(const float *, const float *, const float *, const float *, const int64_t *, int, int64_t, const float *, int, int,
             const float *, double, uint32_t, uint32_t *, uint64_t *, float *, void *) = evk_flowcm_warp_f32; (void)b;
    int (*c)(const float *, const float *, const float *, const float *, const int64_t *, int, int64_t, const float *, int, int,
             const float *, double, uint32_t, const float *, const uint32_t *, uint32_t *, int64_t *, float *, void *) =
        evk_flowcm_grad_f32; (void)c;
    printf("%d|%u|%d|%d\n", post(0, 25, 33, 0, 0, -1, EVK_FLOWCM_VARIANCE, 0, 0, 0, 0, 0, 0), EVK_FLOWCM_ABS, EVK_FLOWCM_VARIANCE,
           EVK_FLOWCM_MEAN_SQUARE);
    return 0;
}
""")
    exe = tmp_path / "use_flowcm"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-ldl",
                    "-Wl,--unresolved-symbols=ignore-all"], check=True, capture_output=True)
    out = subprocess.run([str(exe), _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout.strip().split("|")
    assert [int(v) for v in out] == [-1, 1, 0, 1]


def test_argument_errors_need_no_gpu():
    from event_utils_amd import _lib
    L = _lib.lib()
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)      # never dereferenced: every call below is refused first

    def warp(x=fake, p=fake, off=fake, batch=1, n=8, flow=fake, h=24, w=32, tcs=fake, flags=0, qmax=fake, acc=fake, out=fake):
        return L.evk_flowcm_warp_f32(x, fake, fake, p, off, batch, n, flow, h, w, tcs, 1.0, flags, qmax, acc, out, None)
    assert warp(x=None) == -1 and warp(p=None) == -1 and warp(off=None) == -1 and warp(n=-1) == -1 and warp(flow=None) == -1
    assert warp(batch=0) == -1 and warp(batch=65536) == -1 and warp(h=1) == -1 and warp(w=1) == -1 and warp(tcs=None) == -1
    assert warp(qmax=None) == -1 and warp(acc=None) == -1 and warp(out=None) == -1 and warp(flags=2) == -1
    assert warp(x=odd) == -3 and warp(p=odd) == -3

    def post(iwe=fake, h=25, w=33, hw=fake, dw=fake, radius=4, objective=0, work=fake, out=fake, scratch=fake, nbytes=1 << 20):
        return L.evk_flowcm_post_f32(iwe, h, w, hw, dw, radius, objective, work, fake, out, scratch, nbytes, None)
    assert post(iwe=None) == -1 and post(h=0) == -1 and post(w=0) == -1 and post(work=None) == -1 and post(out=None) == -1
    assert post(objective=2) == -1 and post(objective=-1) == -1 and post(scratch=None) == -1
    assert post(hw=None) == -1 and post(radius=_lib.EVK_MAX_RADIUS + 1, dw=None) == -1 and post(nbytes=64) == -2

    def grad(x=fake, t=fake, off=fake, batch=1, n=8, flow=fake, h=24, w=32, tcs=fake, flags=0, adj=fake, qmax=fake, amax=fake,
             gacc=fake, out=fake):
        return L.evk_flowcm_grad_f32(x, fake, t, fake, off, batch, n, flow, h, w, tcs, 1.0, flags, adj, qmax, amax, gacc, out, None)
    assert grad(x=None) == -1 and grad(t=None) == -1 and grad(off=None) == -1 and grad(n=-1) == -1 and grad(flow=None) == -1
    assert grad(batch=0) == -1 and grad(batch=65536) == -1 and grad(h=1) == -1 and grad(w=1) == -1 and grad(tcs=None) == -1
    assert grad(adj=None) == -1 and grad(qmax=None) == -1 and grad(amax=None) == -1 and grad(gacc=None) == -1
    assert grad(out=None) == -1 and grad(flags=2) == -1 and grad(t=odd) == -3


def test_python_surface():
    import event_utils_amd as E
    from event_utils_amd import transforms
    from event_utils_amd.lib import transforms as aliased
    from event_utils_amd.transforms import flow_loss
    for name in ("flow_field_iwe", "flow_field_contrast_loss", "flow_contrast_loss"):
        assert getattr(E, name) is getattr(transforms, name) is getattr(flow_loss, name) is getattr(aliased, name)
    flow = np.zeros((2, 24, 32), dtype=np.float32)
    cols = [np.zeros(4, dtype=np.float32)] * 4
    # refused before anything needs the device
    with pytest.raises(ValueError):
        E.flow_field_contrast_loss(flow, *cols, objective="contrast")
    with pytest.raises(ValueError):
        E.flow_field_contrast_loss(flow, *cols, direction="sideways")
    with pytest.raises(ValueError):
        E.flow_field_contrast_loss(flow[0], *cols)
    with pytest.raises(ValueError):
        E.flow_field_contrast_loss(np.zeros((2, 2, 24, 32), dtype=np.float32), *cols)          # a batch without offsets
    with pytest.raises(ValueError):
        E.flow_field_contrast_loss(flow, *cols, offsets=[0, 4])                                 # offsets without a batch
    with pytest.raises(ValueError):
        E.flow_field_iwe(flow, *cols, direction="both")
    with pytest.raises(ValueError):
        E.flow_contrast_loss(flow, *cols)                                                       # takes a device tensor
