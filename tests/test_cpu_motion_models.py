"""CPU (no GPU): the rotation and xyztheta motion models -- library entry points, the compiled kernels of all four parametric
models, the Python API surface, argument errors, and the numpy restatement the GPU tests compare against (tests/_motion_models_np.py)."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.optimize as opt

import _motion_models_np as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evk_warp_param_f64", "evk_iwe_param_f32", "evk_iwe_param_f64", "evk_iwe_param_band_rows",
       "evk_objective_gradsums_planes_f32")


def test_entry_points_are_declared_exported_and_bound():
    from event_utils_amd.csrc import build
    build.build(verbose=False)
    from event_utils_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "evk.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = set(_lib.PROTOTYPES)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert name in bound, name
    assert _lib.EVK_WARP_ROTATION != _lib.EVK_WARP_XYZTHETA
    assert _lib.lib().evk_version() == 100


def test_warp_kernels_compile_without_register_spills(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    from event_utils_amd.csrc import build as B
    src = os.path.join(B.HERE, "evk_warps.hip")
    subprocess.run([hipcc] + list(B.CFLAGS) + ["-c", src, "-o", str(tmp_path / "w.o"), "-save-temps=obj"], check=True, cwd=B.HERE,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert asm, os.listdir(tmp_path)
    text = open(tmp_path / asm[0]).read()
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    seen = {n: (int(v), int(sp)) for n, v, sp in kernels}
    band = [n for n in seen if "k_iwe_param_band" in n]
    direct = [n for n in seen if "k_iwe_param_direct" in n]
    # 4 models x {f32, f64} x {value, gradient} x {aligned, unaligned}
    assert len(band) == 32 and len(direct) == 32, sorted(seen)
    assert any("k_warp_param_f64" in n for n in seen) and any("k_gradsums_planes" in n for n in seen)
    assert not {n: vs for n, vs in seen.items() if vs[1]}
    assert all(seen[n][0] <= 128 for n in band)        # 1024-thread workgroups: at most 128 VGPRs a lane
    assert text.count("cmpswap") == 0


def test_api_surface():
    import event_utils_amd as E
    from event_utils_amd.contrast_max import objectives as O
    from event_utils_amd.contrast_max import warps as W
    r, x = E.pure_rotation_warp(), E.xyztheta_warp()
    assert (r.name, r.dims, x.name, x.dims) == ("pure_rotation_warp", 3, "xyztheta_warp", 4)
    assert x.center == (0.0, 0.0) and W.xyztheta_warp(center=(3, 4)).center == (3.0, 4.0)
    sig = inspect.signature(W.linvel_warp.warp)
    assert inspect.signature(W.pure_rotation_warp.warp) == sig == inspect.signature(W.xyztheta_warp.warp)
    assert np.array_equal(r.default_params((180, 240)), [120.0, 90.0, 0.0])
    assert np.array_equal(x.default_params((480, 640)), np.zeros(4))
    assert not hasattr(E.linvel_warp(), "default_params")
    assert W.uses_fused_param(r) and W.uses_fused_param(x) and not W.uses_fused_param(E.linvel_warp())

    class Sub(W.xyztheta_warp):
        pass

    class Own(W.pure_rotation_warp):
        def warp(self, xs, ys, ts, ps, t0, params, compute_grad=False):
            return None
    assert W.uses_fused_param(Sub()) and not W.uses_fused_param(Own())
    assert callable(O.iwe_param_device)


def test_an_explicit_d_iwe_must_match_the_model():
    from event_utils_amd.contrast_max import objectives as O
    from event_utils_amd.contrast_max.warps import linvel_warp, pure_rotation_warp, xyztheta_warp
    assert O._d_iwe_planes(np.zeros((3, 4, 4)), pure_rotation_warp()) is True
    assert O._d_iwe_planes(np.zeros((4, 4, 4)), xyztheta_warp()) is True
    assert O._d_iwe_planes(np.zeros((2, 4, 4)), linvel_warp()) is False
    for d, w in ((np.zeros((2, 4, 4)), xyztheta_warp()), (np.zeros((4, 4, 4)), pure_rotation_warp()),
                 (np.zeros((3, 4, 4)), linvel_warp())):
        with pytest.raises(ValueError):
            O._d_iwe_planes(d, w)


def test_argument_errors_need_no_gpu():
    from event_utils_amd import _lib
    L = _lib.lib()
    hp = np.zeros(6)
    hpp = ctypes.c_void_p(hp.ctypes.data)
    fake = ctypes.c_void_p(4096)          # never dereferenced: every call below is refused first
    for bad_model in (0, 5, -1):
        assert L.evk_warp_param_f64(bad_model, fake, fake, fake, 8, 0.0, hpp, fake, fake, None, None, None) == -1
        assert L.evk_iwe_param_f32(bad_model, fake, fake, fake, fake, 8, 0.0, hpp, 240.0, 180.0, 181, 241, 0, 1.0, fake, None,
                                   None) == -1
        assert L.evk_iwe_param_band_rows(bad_model, 0, 181, 241) == 0
    R = _lib.EVK_WARP_ROTATION
    assert L.evk_warp_param_f64(R, None, fake, fake, 8, 0.0, hpp, fake, fake, None, None, None) == -1
    assert L.evk_warp_param_f64(R, fake, fake, fake, 8, 0.0, None, fake, fake, None, None, None) == -1
    assert L.evk_warp_param_f64(R, fake, fake, fake, 8, 0.0, hpp, fake, fake, fake, None, None) == -1
    assert L.evk_iwe_param_f32(R, fake, None, fake, fake, 8, 0.0, hpp, 240.0, 180.0, 181, 241, 0, 1.0, fake, None, None) == -1
    assert L.evk_iwe_param_f64(R, fake, fake, fake, None, 8, 0.0, hpp, 240.0, 180.0, 181, 241, 0, 1.0, fake, None, None) == -1
    assert L.evk_iwe_param_f32(R, fake, fake, fake, fake, 8, 0.0, hpp, 240.0, 180.0, 181, 241, _lib.EVK_IWE_GRADIENT, 1.0, fake,
                               None, None) == -1
    assert L.evk_iwe_param_f32(R, fake, fake, fake, fake, 8, 0.0, hpp, 240.0, 180.0, 181, 241, 0, 1.0, None, None, None) == -1
    for k in (0, 9):
        assert L.evk_objective_gradsums_planes_f32(fake, fake, k, 4, 4, 0, 0.0, fake, fake, 1 << 20, None) == -1
    assert L.evk_objective_gradsums_planes_f32(None, fake, 2, 4, 4, 0, 0.0, fake, fake, 1 << 20, None) == -1
    assert L.evk_objective_gradsums_planes_f32(fake, fake, 2, 4, 4, 0, 0.0, fake, fake, 8, None) == -2


def test_band_geometry():
    from event_utils_amd import _lib
    L = _lib.lib()
    R, X, G = _lib.EVK_WARP_ROTATION, _lib.EVK_WARP_XYZTHETA, _lib.EVK_IWE_GRADIENT
    # default canvas: value only, and with 3 / 4 derivative planes; every band fits the 160 KiB of LDS
    for model, flags, planes in ((R, 0, 1), (R, G, 4), (X, G, 5)):
        rows = L.evk_iwe_param_band_rows(model, flags, 181, 241)
        assert rows >= 1 and planes * rows * 241 * 4 <= 160 * 1024
    assert L.evk_iwe_param_band_rows(X, 0, 181, 241) == L.evk_iwe_param_band_rows(R, 0, 181, 241)
    assert L.evk_iwe_param_band_rows(X, G, 481, 641) >= 1
    assert L.evk_iwe_param_band_rows(X, G | _lib.EVK_IWE_DIRECT, 181, 241) == 0
    assert L.evk_iwe_param_band_rows(X, G, 41, 12001) == 0          # not one row of 5 planes fits: the direct kernel


# ---- the numpy restatement itself ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("model,params,center", [(M.ROTATION, (100.0, 80.0, 2.5), (0, 0)),
                                                  (M.XYZTHETA, (30.0, -12.0, 1.5, -2.0), (120.0, 90.0))])
def test_helper_jacobians_match_finite_differences(model, params, center):
    rng = np.random.default_rng(1)
    n = 200
    x, y = rng.uniform(0, 240, n), rng.uniform(0, 180, n)
    t = np.sort(rng.uniform(0, 0.2, n))
    _, _, jx, jy = M.warp(model, x, y, t, t[-1], params, center)
    for i in range(len(params)):
        h = 1e-6 * max(1.0, abs(params[i]))
        qp, qm = np.array(params, dtype=float), np.array(params, dtype=float)
        qp[i] += h
        qm[i] -= h
        xp, yp, _, _ = M.warp(model, x, y, t, t[-1], qp, center)
        xm, ym, _, _ = M.warp(model, x, y, t, t[-1], qm, center)
        np.testing.assert_allclose(jx[i], (xp - xm) / (2 * h), rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(jy[i], (yp - ym) / (2 * h), rtol=1e-6, atol=1e-7)


def test_helper_small_angle_rotation_is_xyztheta():
    rng = np.random.default_rng(2)
    x, y = rng.uniform(0, 240, 500), rng.uniform(0, 180, 500)
    t = np.sort(rng.uniform(0, 0.01, 500))
    c = (110.0, 95.0)
    for om in (1e-2, 1e-1, 1.0):
        xr, yr, jxr, jyr = M.warp(M.ROTATION, x, y, t, t[-1], (c[0], c[1], om))
        xz, yz, jxz, jyz = M.warp(M.XYZTHETA, x, y, t, t[-1], (0.0, 0.0, 0.0, om), center=c)
        ang = np.abs(om * (t - t[-1])).max()
        r = np.hypot(x - c[0], y - c[1]).max()
        # the two differ by the second-order term of cos / sin: |1 - cos| r + |theta - sin| r <= theta^2 r
        assert np.abs(xr - xz).max() <= ang ** 2 * r + 1e-9
        assert np.abs(yr - yz).max() <= ang ** 2 * r + 1e-9
        np.testing.assert_allclose(jxr[2], jxz[3], atol=ang * r * np.abs(t - t[-1]).max() + 1e-12)
    # and xyztheta at (vx, vy, 0, 0) is the linear flow exactly
    xo, yo, jx, jy = M.warp(M.XYZTHETA, x, y, t, t[-1], (30.0, -20.0, 0.0, 0.0), center=c)
    assert np.array_equal(xo, x - (t - t[-1]) * 30.0) and np.array_equal(yo, y - (t - t[-1]) * -20.0)


@pytest.mark.parametrize("model", [M.ROTATION, M.XYZTHETA])
def test_helper_scipy_bfgs_recovers_the_synthetic_scene(model):
    x, y, t, p = M.scene(model)
    truth, start = (M.ROT_TRUTH, M.ROT_START) if model == M.ROTATION else (M.XYZ_TRUTH, M.XYZ_START)
    center = (0.0, 0.0) if model == M.ROTATION else M.XYZ_CENTER
    f, g = M.objective(model, x, y, t, p, center=center, reference_exact=False)
    assert f(truth) < f(start)
    res = opt.fmin_bfgs(f, start, fprime=g, disp=False)
    assert np.all(np.abs(res - truth) <= M.TOL[model]), (res, truth)
