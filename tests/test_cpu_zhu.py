"""CPU (no GPU): the average-timestamp (Zhu) objective -- the numpy restatement the GPU tests compare against
(tests/_zhu_np.py) pinned to the reference's own average-timestamp images, its gradient against central differences, the sign
of the loss, the library entry points and their argument errors, and the Python surface."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _zhu_np as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evk_tsimg_warp_f32", "evk_tsimg_warp_f64", "evk_tsimg_band_rows", "evk_tsimg_average_f32", "evk_tsobj_post_f32",
       "evk_tsobj_grad_f32", "evk_tsobj_grad_f64")


def _f11_events(golden):
    g = golden("f11_gather_timestamp")
    # the inputs of the fixture's events_to_timestamp_image_torch call (oracle/make_golden.py:203-214)
    return g, (g["ti_x"], g["ti_y"], g["ti_ts64"].astype(np.float32), g["ps"])


def _assert_images_equal_upstream(images, masked, pos, neg):
    """Every pixel outside the 2x2 block at the origin: upstream's clip quirk moves each clipped event to pixel (0, 0) with its
    fractions, the bounds mask of this definition drops exactly those events.  float32 rounding of upstream's float32
    arithmetic: rtol = atol = 1e-6."""
    assert masked == 135
    for ours, theirs in ((images[0], pos), (images[1], neg)):
        ours = ours.astype(np.float32).copy()
        theirs = np.array(theirs, dtype=np.float32)
        assert ours.shape == theirs.shape == (181, 241)
        ours[:2, :2] = theirs[:2, :2] = 0
        np.testing.assert_allclose(ours, theirs, rtol=1e-6, atol=1e-6)


def test_restatement_equals_the_reference_timestamp_images(golden):
    """With zero flow the warp is the identity, so the restatement's images of the fixture's events are upstream's own output
    of events_to_timestamp_image_torch (fixture f11)."""
    g, (x, y, t, p) = _f11_events(golden)
    outside = (x >= 240) | (y >= 180)
    keep = Z.mask(Z.LINVEL, [0.0, 0.0], x, y, t, p, img_size=(180, 240))
    assert np.array_equal(~keep, outside)        # (x >= 240 or y >= 180 is upstream's clip test too)
    images = Z.images(Z.LINVEL, [0.0, 0.0], x, y, t, p, img_size=(180, 240))
    _assert_images_equal_upstream(images, int((~keep).sum()), g["ti_t_pos_rev0"], g["ti_t_neg_rev0"])
    # the float32 view of the kernels (coordinates and normalised timestamps rounded to float32) is the same images
    images32 = Z.images(Z.LINVEL, [0.0, 0.0], x, y, t, p, img_size=(180, 240), f32_coords=True)
    _assert_images_equal_upstream(images32, int((~keep).sum()), g["ti_t_pos_rev0"], g["ti_t_neg_rev0"])


def test_restatement_equals_the_live_reference(golden):
    from oracle import ref_loader
    if not ref_loader.available():
        pytest.skip("the reference checkout is not on this machine")
    import torch
    ref = ref_loader.load()
    _, (x, y, t, p) = _f11_events(golden)
    pos, neg = ref.image.events_to_timestamp_image_torch(*(torch.from_numpy(np.asarray(v, dtype=np.float32)) for v in (x, y, t, p)))
    keep = Z.mask(Z.LINVEL, [0.0, 0.0], x, y, t, p, img_size=(180, 240))
    images = Z.images(Z.LINVEL, [0.0, 0.0], x, y, t, p, img_size=(180, 240))
    _assert_images_equal_upstream(images, int((~keep).sum()), pos.numpy(), neg.numpy())


# Central-difference steps per parameter: each moves the farthest event by about 1e-6 px (a flow of 1e-5 px/s over 0.1 s; an
# angular rate over 0.1 s at a lever arm of ~100 px, or through fx = 200; a quadratic term through 100^2 px^2), so that
# practically no event crosses a pixel edge between the two probes -- the interpolant has a kink there.
STEPS = {Z.LINVEL: [1e-5, 1e-5], Z.ROTATION: [1e-5, 1e-5, 1e-7], Z.XYZTHETA: [1e-5, 1e-5, 1e-7, 1e-7],
         Z.ANGVEL: [5e-8, 5e-8, 5e-8], Z.PLANAR: [1e-5, 1e-7, 1e-7, 1e-5, 1e-7, 1e-7, 1e-9, 1e-9]}


@pytest.mark.parametrize("where", ["near", "away"])
@pytest.mark.parametrize("model", Z.MODELS)
def test_gradient_matches_central_differences(model, where):
    """The adjoint gradient against central differences of the loss, float64 throughout, for EVERY parameter; the scenes keep
    their events well inside the bounds, and the masks at both probes must be identical (the loss is discontinuous where an
    event crosses the mask)."""
    x, y, t, p = Z.scene(model, n=6000)
    kw = dict(center=Z.CENTER[model])
    truth, start = Z.TRUTH[model], Z.START[model]
    q = truth + 0.02 * (start - truth) if where == "near" else start.copy()
    g = Z.grad(model, q, x, y, t, p, **kw)
    assert g.shape == (Z.DIMS[model],) and np.all(np.isfinite(g)) and np.abs(g).max() > 0
    assert (p > 0).any() and (p <= 0).any()
    for k, h in enumerate(STEPS[model]):
        qp, qm = q.copy(), q.copy()
        qp[k] += h
        qm[k] -= h
        mp, mm = Z.mask(model, qp, x, y, t, p, **kw), Z.mask(model, qm, x, y, t, p, **kw)
        assert np.array_equal(mp, mm) and mp.all()
        fd = (Z.loss(model, qp, x, y, t, p, **kw) - Z.loss(model, qm, x, y, t, p, **kw)) / (2 * h)
        assert abs(fd - g[k]) <= 1e-6 * np.abs(g).max(), (model, where, k, fd, g[k])


def test_gradient_without_blur_matches_central_differences():
    x, y, t, p = Z.scene(Z.LINVEL, n=6000)
    q = Z.LV_START
    g = Z.grad(Z.LINVEL, q, x, y, t, p, sigma=0)
    for k in range(2):
        e = np.zeros(2)
        e[k] = 1e-5
        fd = (Z.loss(Z.LINVEL, q + e, x, y, t, p, sigma=0) - Z.loss(Z.LINVEL, q - e, x, y, t, p, sigma=0)) / 2e-5
        assert abs(fd - g[k]) <= 1e-6 * np.abs(g).max()


@pytest.mark.parametrize("model", Z.MODELS)
def test_loss_has_its_minimum_at_the_truth(model):
    """loss(truth) < loss(truth +- delta) for every parameter: the loss is to be MINIMISED.  Upstream's negative sign fails this."""
    x, y, t, p = Z.scene(model)
    kw = dict(center=Z.CENTER[model])
    f0 = Z.loss(model, Z.TRUTH[model], x, y, t, p, **kw)
    assert f0 > 0
    for k, d in enumerate(Z.TOL[model]):
        for s in (1.0, -1.0):
            q = Z.TRUTH[model].copy()
            q[k] += s * d
            assert Z.loss(model, q, x, y, t, p, **kw) > f0, (model, k, s)


def test_masked_events_contribute_nothing():
    """Events the mask drops -- behind the camera (NaN), out of bounds, NaN polarity -- leave planes, loss and gradient as
    they are without them: nothing is piled onto pixel (0, 0)."""
    x, y, t, p = Z.scene(Z.LINVEL, n=3000)
    q = Z.LV_START
    pl = Z.planes(Z.LINVEL, q, x, y, t, p)
    xb, yb, pb = x.copy(), y.copy(), p.copy()
    xb[10:20], yb[30:40], pb[50:60] = -50.0, 400.0, np.nan
    keep = np.ones(len(x), dtype=bool)
    keep[10:20] = keep[30:40] = keep[50:60] = False
    assert np.array_equal(Z.mask(Z.LINVEL, q, xb, yb, t, pb), keep)
    plb = Z.planes(Z.LINVEL, q, xb, yb, t, pb)
    assert plb[:, 0, 0].max() == 0.0 and plb[1].sum() + plb[3].sum() == pytest.approx(keep.sum())
    assert pl[1].sum() + pl[3].sum() == pytest.approx(len(x))
    # angular velocity: an event rotated behind the camera warps to NaN and is dropped
    xa, ya, ta, pa = Z.scene(Z.ANGVEL, n=2000, duration=1.0)
    w = np.array([0.0, 3.0, 0.0])
    xw, _, _, _ = Z.warp(Z.ANGVEL, xa, ya, ta, ta[-1], w)
    m = Z.mask(Z.ANGVEL, w, xa, ya, ta, pa)
    assert np.isnan(xw).any() and not m[np.isnan(xw)].any()
    assert np.all(np.isfinite(Z.grad(Z.ANGVEL, w, xa, ya, ta, pa)))


# ---- library entry points ----------------------------------------------------------------------------------------------
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
    assert _lib.EVK_WARP_LINVEL == 0 and _lib.EVK_WARP_LINVEL not in (_lib.EVK_WARP_ROTATION, _lib.EVK_WARP_XYZTHETA,
                                                                     _lib.EVK_WARP_ANGULAR_VELOCITY, _lib.EVK_WARP_PLANAR_FLOW)


def test_prototypes_compile_from_c(tmp_path):
    """The new prototypes are plain C99 and agree with the exported symbols' names: their addresses are taken through the
    declared types."""
    from event_utils_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "use_tsobj.c"
    src.write_text(r"""
#include <dlfcn.h>
#include <stdio.h>
#include "evk.h"
int main(int argc, char **argv) {
    void *h = dlopen(argv[1], RTLD_NOW);
    if (!h) { fprintf(stderr, "%s\n", dlerror()); return 2; }
    int (*rows)(uint32_t, int, int) = (int (*)(uint32_t, int, int))dlsym(h, "evk_tsimg_band_rows");
    if (!rows) return 3;
    int (*a)(int, const float *, const float *, const float *, const float *, int64_t, double, double, double, const double *,
             double, double, int, int, uint32_t, uint64_t *, float *, void *) = evk_tsimg_warp_f32; (void)a;
    int (*b)(int, const double *, const double *, const double *, const double *, int64_t, double, double, double, const double *,
             double, double, int, int, uint32_t, uint64_t *, float *, void *) = evk_tsimg_warp_f64; (void)b;
    int (*c)(uint32_t, int, int) = evk_tsimg_band_rows; (void)c;
    int (*d)(const float *, int, int, float *, void *) = evk_tsimg_average_f32; (void)d;
    int (*e)(const float *, int, int, const double *, const double *, int, float *, float *, double *, void *, int64_t, void *) =
        evk_tsobj_post_f32; (void)e;
    int (*f)(int, const float *, const float *, const float *, const float *, int64_t, double, double, double, const double *,
             double, double, int, int, const float *, double *, void *, int64_t, void *) = evk_tsobj_grad_f32; (void)f;
    int (*g)(int, const double *, const double *, const double *, const double *, int64_t, double, double, double, const double *,
             double, double, int, int, const float *, double *, void *, int64_t, void *) = evk_tsobj_grad_f64; (void)g;
    printf("%d|%d\n", rows(0u, 481, 641), rows(EVK_IWE_DIRECT, 481, 641));
    return 0;
}
""")
    exe = tmp_path / "use_tsobj"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-ldl",
                    "-Wl,--unresolved-symbols=ignore-all"], check=True, capture_output=True)
    out = subprocess.run([str(exe), _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout.strip().split("|")
    assert [int(v) for v in out] == [7, 0]


def test_argument_errors_need_no_gpu():
    from event_utils_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused first
    hp = np.zeros(10)
    hpp = ctypes.c_void_p(hp.ctypes.data)
    big = 1 << 20
    for fn in (L.evk_tsimg_warp_f32, L.evk_tsimg_warp_f64):
        def splat(model=0, x=fake, p=fake, n=8, params=hpp, ch=181, cw=241, acc=fake, out=fake):
            return fn(model, x, fake, fake, p, n, 0.0, 0.0, 1.0, params, 240.0, 180.0, ch, cw, 0, acc, out, None)
        for bad_model in (-1, 5):
            assert splat(model=bad_model) == -1
        assert splat(n=-1) == -1 and splat(x=None) == -1 and splat(p=None) == -1 and splat(params=None) == -1
        assert splat(ch=0) == -1 and splat(cw=0) == -1 and splat(out=None) == -1 and splat(acc=None) == -1
    for fn in (L.evk_tsobj_grad_f32, L.evk_tsobj_grad_f64):
        def gather(model=0, x=fake, t=fake, n=8, params=hpp, ch=181, cw=241, adj=fake, out=fake, scratch=fake, nbytes=big):
            return fn(model, x, fake, t, fake, n, 0.0, 0.0, 1.0, params, 240.0, 180.0, ch, cw, adj, out, scratch, nbytes, None)
        for bad_model in (-1, 5):
            assert gather(model=bad_model) == -1
        assert gather(n=-1) == -1 and gather(x=None) == -1 and gather(t=None) == -1 and gather(params=None) == -1
        assert gather(ch=0) == -1 and gather(cw=0) == -1 and gather(adj=None) == -1 and gather(out=None) == -1
        assert gather(scratch=None) == -1 and gather(nbytes=8) == -2
    # a column that is not aligned to its element
    odd = ctypes.c_void_p(4098)
    assert L.evk_tsimg_warp_f32(0, odd, fake, fake, fake, 8, 0.0, 0.0, 1.0, hpp, 240.0, 180.0, 181, 241, 0, fake, fake, None) == -3
    w = np.ones(1)
    wp = ctypes.c_void_p(w.ctypes.data)

    def post(planes=fake, h=181, wd=241, host_w=wp, dev_w=None, radius=0, work=fake, out=fake, scratch=fake, nbytes=big):
        return L.evk_tsobj_post_f32(planes, h, wd, host_w, dev_w, radius, work, None, out, scratch, nbytes, None)
    assert post(planes=None) == -1 and post(h=0) == -1 and post(wd=0) == -1 and post(work=None) == -1 and post(out=None) == -1
    assert post(scratch=None) == -1 and post(host_w=None) == -1 and post(nbytes=8) == -2
    assert post(radius=_lib.EVK_MAX_RADIUS + 1) == -1          # a wide blur needs its weights on the device
    assert L.evk_tsimg_average_f32(None, 4, 4, fake, None) == -1 and L.evk_tsimg_average_f32(fake, 4, 4, None, None) == -1
    assert L.evk_tsimg_average_f32(fake, 0, 4, fake, None) == -1


def test_band_geometry():
    """Four planes of 8-byte fixed-point cells in the 160 KB of evk_iwe_param_*'s bands: 7 rows of a 641-wide canvas; the direct
    kernel for a canvas too wide for one row, for more than 24 bands per plane, and with EVK_IWE_DIRECT."""
    from event_utils_amd import _lib
    rows = _lib.lib().evk_tsimg_band_rows
    assert rows(0, 481, 641) == (160 * 1024) // (4 * 641 * 8) == 7
    assert rows(0, 181, 241) == (160 * 1024) // (4 * 241 * 8) == 21
    assert rows(0, 31, 41) == 31                       # the whole canvas in one band
    assert rows(0, 181, 5121) == 0                     # not one row fits
    assert rows(0, 2001, 641) == 0                     # 286 bands > 96
    assert rows(_lib.EVK_IWE_DIRECT, 181, 241) == 0
    assert rows(0, 1, 241) == 0 and rows(0, 181, 1) == 0


def test_existing_entries_still_refuse_the_linear_flow_id():
    from event_utils_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    hp = np.zeros(10)
    hpp = ctypes.c_void_p(hp.ctypes.data)
    assert L.evk_iwe_param_f32(0, fake, fake, fake, fake, 8, 0.0, hpp, 240.0, 180.0, 181, 241, 0, 1.0, fake, None, None) == -1
    assert L.evk_warp_param_f64(0, fake, fake, fake, 8, 0.0, hpp, fake, fake, None, None, None) == -1
    assert L.evk_iwe_param_band_rows(0, 0, 181, 241) == 0


# ---- Python surface ----------------------------------------------------------------------------------------------------
def test_python_surface():
    import inspect
    import event_utils_amd as E
    from event_utils_amd.contrast_max import objectives as O
    import event_utils_amd.lib.contrast_max.objectives as LO
    assert E.zhu_timestamp_objective is O.zhu_timestamp_objective is LO.zhu_timestamp_objective
    assert E.get_timestamp_images is O.get_timestamp_images
    obj = E.zhu_timestamp_objective()
    assert isinstance(obj, O.objective_function)
    assert (obj.name, obj.use_polarity, obj.default_blur, obj.has_derivative) == ("zhu", True, 2.0, True)
    assert obj.adaptive_lifespan is False
    for name in ("evaluate_function", "evaluate_gradient", "evaluate_function_and_gradient", "evaluate_function_batch",
                 "evaluate_function_and_numeric_gradient"):
        assert callable(getattr(obj, name)), name
    # upstream's keyword signature, `iwe` included (ignored: this objective is not a function of the IWE)
    assert list(inspect.signature(obj.evaluate_function).parameters) == \
        ["params", "xs", "ys", "ts", "ps", "warpfunc", "img_size", "blur_sigma", "showimg", "iwe"]
    assert list(inspect.signature(obj.evaluate_gradient).parameters) == \
        ["params", "xs", "ys", "ts", "ps", "warpfunc", "img_size", "blur_sigma", "showimg", "iwe", "d_iwe"]
    assert list(inspect.signature(O.get_timestamp_images).parameters)[:7] == \
        ["params", "xs", "ys", "ts", "ps", "warpfunc", "img_size"]
    assert "zhu_timestamp_objective" not in "".join(
        ln for ln in open(os.path.join(ROOT, "event_utils_amd", "contrast_max", "objectives.py")) if "Not provided" in ln)


def test_sharded_and_adaptive_lifespan_use_is_refused():
    import event_utils_amd as E
    x, y, t, p = Z.scene(Z.LINVEL, n=100)
    for warp in (E.linvel_warp(), E.xyztheta_warp()):
        q = np.zeros(warp.dims)
        obj = E.zhu_timestamp_objective()
        obj.distributed = True
        for call in (obj.evaluate_function, obj.evaluate_gradient, obj.evaluate_function_and_gradient):
            with pytest.raises(NotImplementedError):
                call(q, x, y, t, p, warp, (180, 240))
        with pytest.raises(NotImplementedError):
            obj.evaluate_function_batch([q], x, y, t, p, warp, (180, 240))
        obj = E.zhu_timestamp_objective()
        obj.process_group = object()
        with pytest.raises(NotImplementedError):
            obj.evaluate_function(q, x, y, t, p, warp, (180, 240))
        obj = E.zhu_timestamp_objective()
        obj.adaptive_lifespan = True
        with pytest.raises(NotImplementedError):
            obj.evaluate_function(q, x, y, t, p, warp, (180, 240))
