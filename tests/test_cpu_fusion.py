"""CPU (no GPU): the host restatement of depth fusion (tests/_fusion_np.py, the literal definition) on hand-worked cases -- the
identity case, the variance rule in its exact case, the anchor and the gate --; relative_transforms against the explicit formulas;
the restatement's fused map of a seeded slanted plane is better than the best single view; the evk_fusion_* entry points are
declared, bound and exported and refuse bad arguments before they touch the device; the Python argument errors; the public surface;
the kernels of evk_fusion.hip compile for gfx950 without register spills."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _fusion_np as N
import _header

ENTRIES = {"evk_fusion_propagate", "evk_fusion_fuse", "evk_fusion_regularise"}
PUBLIC = ("InverseDepthMap", "disparity_inverse_depth", "depth_inverse_depth", "inverse_depth_depth_map", "relative_transforms",
          "propagate_inverse_depth", "fuse_inverse_depth", "regularise_inverse_depth", "fuse_stereo_depth")
IDENTITY = N.transform12(np.eye(3), np.zeros(3))
ULP = 2.0 ** -52


def a_map(rho, var, mask=None):
    rho, var = np.asarray(rho, dtype=np.float64), np.asarray(var, dtype=np.float64)
    mask = np.ones(rho.shape, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    return rho, var, mask.astype(np.int32), np.zeros(rho.shape, dtype=np.int32), mask


def K_for(size, f=200.0):
    h, w = size
    return np.array([[f, 0.0, (w - 1) / 2], [0.0, f, (h - 1) / 2], [0.0, 0.0, 1.0]])


def candidates(pairs, at=(0, 0)):
    """hand-written candidates (rho', v') of one pixel"""
    n = len(pairs)
    return (np.full(n, at[1], dtype=np.int32), np.full(n, at[0], dtype=np.int32), np.array([p[0] for p in pairs], dtype=np.float64),
            np.array([p[1] for p in pairs], dtype=np.float64))


# ---- hand-worked cases of the restatement --------------------------------------------------------------------------------------------

def test_the_identity_case():
    """identity transforms land every pixel on itself; K maps of equal variance fuse to 1 / (K (1 / v)) and the sequential mean"""
    rng = np.random.default_rng(5)
    size, views, v = (5, 7), 6, 0.0123
    K = K_for(size, 8.0)
    maps = [a_map(rng.uniform(0.2, 0.9, size), np.full(size, v)) for _ in range(views)]
    cands = N.propagate(maps, K, np.tile(IDENTITY, (views, 1)))
    ys, xs = np.mgrid[0:size[0], 0:size[1]]
    assert np.array_equal(cands[0], np.tile(xs.reshape(-1), views)) and np.array_equal(cands[1], np.tile(ys.reshape(-1), views))
    # rho' = 1 / (1 / rho) is rho itself or a neighbour of it; v' = q^4 v with q = rho' / rho
    assert np.all(np.abs(cands[2] - np.concatenate([m[0].reshape(-1) for m in maps])) <= ULP * cands[2])
    fused = N.fuse_candidates(cands, size, gate=1e9)
    assert fused[4].all() and np.all(fused[2] == views) and not fused[3].any()
    R, V = cands[2].reshape(views, *size), cands[3].reshape(views, *size)
    for y in range(size[0]):
        for x in range(size[1]):
            W = S = 0.0
            for s in range(views):
                iw = 1.0 / V[s, y, x]
                W += iw
                S += R[s, y, x] * iw
            assert fused[0][y, x] == S / W and fused[1][y, x] == 1.0 / W
    # with rho' = rho exactly (a power of two) the variances are v itself and the claim is exact
    exact = [a_map(np.full(size, 0.5), np.full(size, v)) for _ in range(views)]
    fused = N.fuse(exact, K, np.tile(IDENTITY, (views, 1)), gate=1e9)
    W = 0.0
    for _ in range(views):
        W += 1.0 / v
    assert np.all(fused[1] == 1.0 / W) and np.all(fused[0] == 0.5)
    assert abs(1.0 / W - 1.0 / (views * (1.0 / v))) <= 4 * ULP * (1.0 / W)


def test_the_variance_rule_is_exact_for_a_translation_along_the_optical_axis():
    rng = np.random.default_rng(6)
    size = (6, 8)
    K = K_for(size, 300.0)                                  # a long lens: the shifted points stay on the sensor
    worst = 0.0
    for tz in (0.25, -0.125, 1.0):
        rho, var = rng.uniform(0.2, 1.5, size), rng.uniform(1e-4, 1e-2, size)
        cands = N.propagate([a_map(rho, var)], K, N.transform12(np.eye(3), [0.0, 0.0, tz])[None])
        assert len(cands[0]) > size[0] * size[1] // 2
        for xi, yi, rp, vp in zip(*cands):
            # which source pixel it came from: the one whose rho' it carries (rho' = 1 / (1 / rho + tz) is monotone in rho)
            src = np.argmin(np.abs(1.0 / (1.0 / rho + tz) - rp))
            r, v = rho.reshape(-1)[src], var.reshape(-1)[src]
            want = v / (1.0 + r * tz) ** 4
            worst = max(worst, abs(vp - want) / (ULP * want))
    assert worst <= 16.0, "q^4 v lies %.1f ulp from v / (1 + rho t_z)^4" % worst


def test_a_tie_in_variance_takes_the_earliest_candidate():
    # three candidates of one variance: the first is the anchor, and a gate round IT keeps the second and drops the third
    fused = N.fuse_candidates(candidates([(0.50, 0.01), (0.60, 0.01), (0.75, 0.01)]), (1, 1), gate=1.0)
    assert (fused[2][0, 0], fused[3][0, 0]) == (2, 1)       # |0.1|^2 <= 0.02 < |0.25|^2
    iw = 1.0 / 0.01
    assert fused[0][0, 0] == (0.0 + 0.50 * iw + 0.60 * iw) / (0.0 + iw + iw) and fused[1][0, 0] == 1.0 / (iw + iw)
    # were the last the anchor, the first would be out and the count the same but the mean another
    other = N.fuse_candidates(candidates([(0.75, 0.01), (0.60, 0.01), (0.50, 0.01)]), (1, 1), gate=1.0)
    assert other[2][0, 0] == 1 and other[0][0, 0] == (0.75 * iw) / iw


def test_a_gate_of_zero_keeps_only_what_equals_the_anchor():
    fused = N.fuse_candidates(candidates([(0.5, 0.02), (0.5, 0.01), (0.5000001, 0.03), (0.5, 0.04)]), (1, 1), gate=0.0)
    assert (fused[2][0, 0], fused[3][0, 0]) == (3, 1) and fused[0][0, 0] == 0.5 and fused[4][0, 0]
    assert not N.fuse_candidates(candidates([(0.5, 0.02), (0.6, 0.01)]), (1, 1), gate=0.0, min_count=2)[4][0, 0]


def test_an_outlier_of_lower_variance_becomes_the_anchor():
    """the documented consequence of anchoring on the least variance: four agreeing candidates are rejected by one confident outlier"""
    surface = [(0.50, 0.0004), (0.51, 0.0004), (0.49, 0.0004), (0.50, 0.0004)]
    fused = N.fuse_candidates(candidates(surface[:2] + [(0.90, 0.0001)] + surface[2:]), (1, 1), gate=2.0)
    assert (fused[2][0, 0], fused[3][0, 0]) == (1, 4) and fused[0][0, 0] == 0.90 and fused[1][0, 0] == 1.0 / (1.0 / 0.0001)
    # the same outlier with the surface's variance is the one rejected
    fused = N.fuse_candidates(candidates(surface[:2] + [(0.90, 0.0004)] + surface[2:]), (1, 1), gate=2.0)
    assert (fused[2][0, 0], fused[3][0, 0]) == (4, 1) and abs(fused[0][0, 0] - 0.50) < 1e-12


def test_the_options_of_the_mask_and_an_empty_pixel():
    cands = candidates([(0.5, 0.02), (0.5, 0.02)], at=(1, 2))
    fused = N.fuse_candidates(cands, (2, 3), max_variance=0.01)
    assert fused[4][1, 2] and fused[1][1, 2] == 1.0 / (1.0 / 0.02 + 1.0 / 0.02)
    assert not N.fuse_candidates(cands, (2, 3), max_variance=0.009)[4].any()
    assert not N.fuse_candidates(cands, (2, 3), min_count=3)[4].any()
    assert np.isnan(fused[0][0, 0]) and np.isnan(fused[1][0, 0]) and (fused[2][0, 0], fused[3][0, 0], fused[4][0, 0]) == (0, 0, False)


def test_no_source_is_silently_dropped_and_so_is_what_leaves_the_view():
    size = (2, 4)
    K = K_for(size, 4.0)
    rho = np.array([[0.5, np.nan, np.inf, 0.0], [-0.5, 0.5, 0.5, 0.5]])
    var = np.array([[0.01, 0.01, 0.01, 0.01], [0.01, np.nan, 0.0, -1.0]])
    cands = N.propagate([a_map(rho, var)], K, IDENTITY[None])
    assert (cands[0].tolist(), cands[1].tolist()) == ([0], [0])
    cands = N.propagate([a_map(rho, np.full(size, np.inf))], K, IDENTITY[None])
    assert len(cands[0]) == 0
    good = a_map(np.full(size, 0.5), np.full(size, 0.01), [[1, 0, 1, 1], [1, 1, 0, 1]])
    assert len(N.propagate([good], K, IDENTITY[None])[0]) == 6
    assert len(N.propagate([good], K, N.transform12(np.eye(3), [0, 0, -2.0])[None])[0]) == 0        # Z' = 0: not in front
    assert len(N.propagate([good], K, N.transform12(np.eye(3), [0, 0, -5.0])[None])[0]) == 0        # behind the camera
    assert len(N.propagate([good], K, N.transform12(np.eye(3), [100.0, 0, 0])[None])[0]) == 0       # off the sensor
    assert len(N.propagate([good], K, IDENTITY[None], process_variance=[0.5])[0]) == 6
    assert np.all(N.propagate([good], K, IDENTITY[None], process_variance=[0.5])[3] == 0.01 + 0.5)
    assert len(N.propagate([good], K, IDENTITY[None], target_size=(1, 3))[0]) == 2                  # a smaller target crops


def test_regularisation_by_hand():
    rho = np.array([[0.50, 0.52, 0.90], [0.51, 0.50, 0.50]])
    var = np.full((2, 3), 0.0001)
    mask = np.array([[1, 1, 1], [1, 0, 1]], dtype=bool)
    out = N.regularise(a_map(rho, var, mask), radius=1, gate=2.0, min_neighbours=2)
    # (0, 0): itself, (0, 1) and (1, 0) are within 2 sqrt(2) sigma = 0.028; (1, 1) is not masked
    iw = 1.0 / 0.0001
    assert out[0][0, 0] == (0.50 * iw + 0.52 * iw + 0.51 * iw) / (iw + iw + iw) and out[4][0, 0]
    assert out[0][0, 2] == (0.90 * iw) / iw and not out[4][0, 2]                    # the outlier has no compatible neighbour
    assert out[0][1, 1] == 0.50 and not out[4][1, 1]                                # not masked: as it is
    assert out[4][1, 2] == False and out[0][1, 2] == (0.52 * iw + 0.50 * iw) / (iw + iw)      # one neighbour only  # noqa: E712
    assert N.regularise(a_map(rho, var, mask), 1, 2.0, 0)[4].tolist() == mask.tolist()
    assert out[1] is not None and np.array_equal(out[1], var)                       # the variance is passed through
    assert not N.regularise(a_map(rho, var, mask), 1, 2.0, 9)[4].any()


# ---- the poses -----------------------------------------------------------------------------------------------------------------------

def test_relative_transforms_against_the_explicit_formulas():
    from event_utils_amd.depth.fusion import relative_transforms
    rng = np.random.default_rng(8)
    q = rng.normal(size=(9, 4))
    c = rng.normal(size=(9, 3)) * 3.0
    unit = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    for target in (0, 4):
        got = relative_transforms(c, q, (c[target], q[target]))                  # (any non-zero length: they are normalised)
        assert got.shape == (9, 12) and got.dtype == np.float64
        for s in range(9):
            want, mag = N.relative_transform(c[s], unit[s], c[target], unit[target])
            assert np.all(np.abs(got[s] - want) <= 4 * 2.0 ** -53 * mag), (s, np.abs(got[s] - want), mag)
        assert np.allclose(got[target], IDENTITY, atol=1e-15)
    for bad in (dict(positions=c[:, :2]), dict(quaternions=q[:8]), dict(quaternions=np.zeros((9, 4))), dict(target_pose=(c[0],)),
                dict(target_pose=(c[0, :2], q[0])), dict(target_pose=(c[0], q[0, :3])), dict(positions=np.full((9, 3), np.nan))):
        args = dict(positions=c, quaternions=q, target_pose=(c[0], q[0]))
        args.update(bad)
        with pytest.raises(ValueError):
            relative_transforms(**args)


# ---- quality: a seeded slanted plane from eight poses --------------------------------------------------------------------------------

def plane_scene(seed=11, views=8, size=(40, 60), f=200.0, baseline=0.1, sigma=0.5, fraction=0.6):
    """a plane Z = 2 + 0.3 X + 0.2 Y in the frame of view 0, seen from `views` poses with Gaussian disparity noise of `sigma` px
    -> (the maps, K, the target-from-source transforms, each view's true inverse depth)"""
    rng = np.random.default_rng(seed)
    h, w = size
    K = K_for(size, f)
    n, c = np.array([-0.3, -0.2, 1.0]), 2.0
    ys, xs = np.mgrid[0:h, 0:w]
    rays = np.stack(((xs - K[0, 2]) / f, (ys - K[1, 2]) / f, np.ones(size)), axis=-1)
    maps, transforms, truth = [], [], []
    for s in range(views):
        R = N.rodrigues(rng.normal(size=3) * (0.02 if s else 0.0))
        t = rng.normal(size=3) * (0.05 if s else 0.0)
        Z = (c - n @ t) / (rays @ (R.T @ n))                # n . (R (Z ray) + t) = c
        d = f * baseline / Z + rng.normal(size=size) * sigma
        mask = rng.random(size) < fraction
        maps.append(N.disparity_inverse_depth(d, mask, f, baseline, sigma))
        transforms.append(N.transform12(R, t))
        truth.append(1.0 / Z)
    return maps, K, np.array(transforms), truth


def test_the_fused_map_is_better_than_the_best_single_view():
    maps, K, transforms, truth = plane_scene()
    single = [(math.sqrt(np.mean((m[0][m[4]] - tr[m[4]]) ** 2)), int(m[4].sum())) for m, tr in zip(maps, truth)]
    best_rms, best_count = min(s[0] for s in single), max(s[1] for s in single)
    fused = N.fuse(maps, K, transforms, gate=2.0)
    rms = math.sqrt(np.mean((fused[0][fused[4]] - truth[0][fused[4]]) ** 2))
    count = int(fused[4].sum())
    assert rms < best_rms and count >= best_count, "fused: rms %.3e over %d pixels; best single view: rms %.3e, %d pixels" % (
        rms, count, best_rms, best_count)
    smooth = N.regularise(fused, radius=1, gate=2.0, min_neighbours=2)
    rms_s = math.sqrt(np.mean((smooth[0][smooth[4]] - truth[0][smooth[4]]) ** 2))
    assert rms_s < rms and smooth[4].sum() > 0.9 * count, (rms_s, rms, int(smooth[4].sum()), count)


# ---- the public surface and the C ABI ------------------------------------------------------------------------------------------------

def test_the_prototypes_are_bound_with_their_arguments():
    from event_utils_amd import _lib
    text = _header.TEXT
    protos = _header.prototypes("evk_fusion_")
    assert set(protos) == ENTRIES | {"evk_fusion_scratch_bytes"}
    for name, (want, ret) in protos.items():
        assert ret is (ctypes.c_int if name in ENTRIES else ctypes.c_int64), name
        assert _lib.PROTOTYPES[name] == (want, ret), name
        assert hasattr(_lib.lib(), name)
    assert (_lib.EVK_FUSION_MAX_RADIUS, _lib.EVK_FUSION_VIEW_PARAMS) == (3, 17)
    for name, value in (("EVK_FUSION_MAX_RADIUS", 3), ("EVK_FUSION_VIEW_PARAMS", 17)):
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (name, value), text, re.M)
    assert "Depth fusion (evk_fusion.hip)" in text


def test_public_surface():
    import inspect
    import event_utils_amd as E
    import event_utils_amd.lib.depth.fusion as alias
    from event_utils_amd import depth
    from event_utils_amd.depth import fusion
    assert alias is fusion
    for name in PUBLIC:
        assert getattr(E, name) is getattr(fusion, name) is getattr(depth, name)
    assert "(no reference module)           -> event_utils_amd.depth.fusion" in E.__doc__
    assert E.InverseDepthMap._fields == ("inv_depth", "variance", "count", "rejected", "mask")
    empty = inspect.Parameter.empty

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    target = [("target_camera_matrix", None), ("target_size", None)]
    assert params(E.disparity_inverse_depth) == [(n, empty) for n in ("disp", "k", "fx", "baseline")] + [("sigma_disparity", 0.5)]
    assert params(E.depth_inverse_depth) == [("depth_map", empty), ("variance", empty)]
    assert params(E.inverse_depth_depth_map) == [("idm", empty)]
    assert params(E.relative_transforms) == [(n, empty) for n in ("positions", "quaternions", "target_pose")]
    assert params(E.propagate_inverse_depth) == [(n, empty) for n in ("maps", "camera_matrix", "transforms")] + \
        [("process_variance", 0.0)] + target
    assert params(E.fuse_inverse_depth) == [(n, empty) for n in ("maps", "camera_matrix", "transforms")] + \
        [("gate", 2.0), ("process_variance", 0.0), ("min_count", 1), ("max_variance", None)] + target
    assert params(E.regularise_inverse_depth) == [("idm", empty), ("radius", 1), ("gate", 2.0), ("min_neighbours", 2)]
    assert params(E.fuse_stereo_depth)[:7] == [(n, empty) for n in ("disp", "fx", "baseline", "camera_matrix", "positions", "quaternions",
                                                                   "target")]


def test_arguments_are_refused_before_the_device_is_touched():
    from event_utils_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)                            # never dereferenced: every call below is refused first
    einval, ealign, nan, inf = -1, -3, float("nan"), float("inf")
    view = [100.0, 100.0, 4.0, 3.0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0.0]

    def propagate(rho=fake, var=fake, mask=fake, views=2, h=6, w=8, params=None, oh=6, ow=8, target=(100.0, 100.0, 4.0, 3.0), scratch=fake,
                  xi=fake, yi=fake, orho=fake, ovar=fake, result=fake, no_params=False, no_target=False):
        p = np.array(view * max(views, 1) if params is None else params, dtype=np.float64)
        t = np.array(target, dtype=np.float64)
        return L.evk_fusion_propagate(rho, var, mask, views, h, w, None if no_params else p.ctypes.data, oh, ow,
                                      None if no_target else t.ctypes.data, scratch, xi, yi, orho, ovar, result, None)
    for missing in ("rho", "var", "mask", "scratch", "xi", "yi", "orho", "ovar", "result"):
        assert propagate(**{missing: None}) == einval, missing
    assert propagate(no_params=True) == einval and propagate(no_target=True) == einval
    assert propagate(views=0) == einval and propagate(h=0) == einval and propagate(w=-1) == einval
    assert propagate(oh=0) == einval and propagate(ow=0) == einval
    assert propagate(views=1 << 12, h=1 << 10, w=1 << 10) == einval                 # views h w past 2^31 - 1
    assert propagate(oh=1 << 16, ow=1 << 15) == einval                              # the target plane past the grouping's keys
    for k in range(17):
        for bad in (nan, inf, -inf):
            assert propagate(params=view + view[:k] + [bad] + view[k + 1:]) == einval, (k, bad)
    for k, bad in ((0, 0.0), (1, -1.0), (16, -1e-9)):
        assert propagate(params=view[:k] + [bad] + view[k + 1:] + view) == einval, k
    for k in range(4):
        for bad in (nan, inf) + ((0.0, -2.0) if k < 2 else ()):
            assert propagate(target=[bad if j == k else v for j, v in enumerate((100.0, 100.0, 4.0, 3.0))]) == einval, (k, bad)
    assert propagate(scratch=ctypes.c_void_p(4096 + 128)) == ealign

    def fuse(m=10, oh=6, ow=8, scratch=fake, rho=fake, var=fake, gate2=4.0, min_count=1, use=0, max_var=0.0, orho=fake, ovar=fake, count=fake,
             rejected=fake, mask=fake):
        return L.evk_fusion_fuse(m, oh, ow, scratch, rho, var, gate2, min_count, use, max_var, orho, ovar, count, rejected, mask, None)
    for missing in ("scratch", "rho", "var", "orho", "ovar", "count", "rejected", "mask"):
        assert fuse(**{missing: None}) == einval, missing
    assert fuse(m=-1) == einval and fuse(m=1 << 31) == einval and fuse(oh=0) == einval and fuse(ow=0) == einval
    assert fuse(oh=1 << 16, ow=1 << 15) == einval
    assert fuse(gate2=-1.0) == einval and fuse(gate2=nan) == einval and fuse(min_count=0) == einval
    assert fuse(use=2) == einval and fuse(use=-1) == einval and fuse(use=1, max_var=nan) == einval
    assert fuse(scratch=ctypes.c_void_p(4096 + 64)) == ealign

    def regularise(rho=fake, var=fake, mask=fake, h=6, w=8, radius=1, gate2=4.0, mn=2, out=ctypes.c_void_p(8192), out_mask=ctypes.c_void_p(12288)):
        return L.evk_fusion_regularise(rho, var, mask, h, w, radius, gate2, mn, out, out_mask, None)
    for missing in ("rho", "var", "mask", "out", "out_mask"):
        assert regularise(**{missing: None}) == einval, missing
    assert regularise(out=fake) == einval and regularise(out_mask=fake) == einval   # in place
    assert regularise(h=0) == einval and regularise(w=0) == einval and regularise(h=1 << 16, w=1 << 15) == einval
    assert regularise(radius=0) == einval and regularise(radius=4) == einval
    assert regularise(gate2=-1.0) == einval and regularise(gate2=nan) == einval
    assert regularise(mn=-1) == einval and regularise(mn=10) == einval and regularise(radius=3, mn=50) == einval

    size = L.evk_fusion_scratch_bytes
    assert size(1, 1, 1, 1, 1) > 0 and size(1, 1, 1, 1, 1) % 256 == 0
    n = 16 * 480 * 640
    assert size(16, 480, 640, 480, 640) >= max(22 * n + L.evk_select_scratch_bytes(n), L.evk_denoise_scratch_bytes(n, 480, 640, 1))
    assert size(16, 480, 640, 480, 640) < 22 * n + L.evk_select_scratch_bytes(n) + L.evk_denoise_scratch_bytes(n, 480, 640, 1)
    assert size(0, 4, 4, 4, 4) == einval and size(1, 0, 4, 4, 4) == einval and size(1, 4, 4, 4, 0) == einval
    assert size(1 << 12, 1 << 10, 1 << 10, 4, 4) == einval and size(1, 4, 4, 1 << 16, 1 << 15) == einval
    assert size(2, 1 << 15, 1 << 15, 4, 4) == einval and size(1, 1 << 15, (1 << 16) - 1, 4, 4) > 0


def test_python_argument_errors_come_before_any_device_work():
    """every call below is refused on its arguments alone: none of them reaches the point where a missing GPU would matter"""
    import torch
    import event_utils_amd as E
    size = (4, 6)
    K = K_for(size, 5.0)

    def a(shape=size, **other):
        f = dict(inv_depth=torch.full(shape, 0.5, dtype=torch.float64), variance=torch.full(shape, 0.01, dtype=torch.float64),
                 count=torch.ones(shape, dtype=torch.int32), rejected=torch.zeros(shape, dtype=torch.int32),
                 mask=torch.ones(shape, dtype=torch.bool))
        f.update(other)
        return E.InverseDepthMap(**f)
    T = np.tile(IDENTITY, (2, 1))
    calls = (lambda maps, T=T, **kw: E.propagate_inverse_depth(maps, K, T, **kw), lambda maps, T=T, **kw: E.fuse_inverse_depth(maps, K, T, **kw))
    for f in calls:
        for wrong in (a(inv_depth=torch.zeros(size)), a(variance=torch.zeros(size, dtype=torch.float32)), a(count=torch.zeros(size)),
                      a(rejected=torch.zeros(size, dtype=torch.int64)), a(mask=torch.ones(size, dtype=torch.uint8)),
                      a(inv_depth=np.zeros(size, dtype=np.float32)), a(mask=[[True] * 6] * 4)):
            with pytest.raises(ValueError, match="must be an? (float64|int32|bool)"):
                f([a(), wrong])
        with pytest.raises(ValueError, match="of one shape"):
            f([a(), a(count=torch.ones((4, 5), dtype=torch.int32))])
        with pytest.raises(ValueError, match=r"\(H, W\)"):
            f([a((2, 4, 6)), a((2, 4, 6))])
        with pytest.raises(ValueError, match="one size"):
            f([a(), a((4, 7))])
        with pytest.raises(ValueError, match="InverseDepthMap"):
            f([a(), a()[:4]])
        with pytest.raises(ValueError, match="at least one"):
            f([], T=T[:0])
        for bad in (T[:1], np.zeros((2, 11)), np.zeros((2, 4, 4))):
            with pytest.raises(ValueError, match="transforms must be"):
                f([a(), a()], T=bad)
        for k, bad in ((0, np.nan), (11, np.inf), (5, -np.inf)):
            Tb = T.copy()
            Tb[1, k] = bad
            with pytest.raises(ValueError, match="transforms must be finite"):
                f([a(), a()], T=Tb)
        for bad in (-0.1, float("nan"), float("inf"), [0.0, -1.0], [0.0, float("nan")], [0.0, 0.0, 0.0]):
            with pytest.raises(ValueError, match="process_variance"):
                f([a(), a()], process_variance=bad)
        with pytest.raises(ValueError, match="target_size"):
            f([a(), a()], target_size=(0, 5))
        with pytest.raises(ValueError, match="target_camera_matrix"):
            f([a(), a()], target_camera_matrix=np.zeros((3, 3)))
        with pytest.raises(ValueError):
            E.propagate_inverse_depth([a(), a()], np.zeros((3, 3)), T)
    for kw, match in ((dict(gate=-1.0), "gate"), (dict(gate=float("nan")), "gate"), (dict(min_count=0), "min_count"),
                      (dict(min_count=1.5), "min_count"), (dict(max_variance=float("nan")), "max_variance")):
        with pytest.raises(ValueError, match=match):
            E.fuse_inverse_depth([a(), a()], K, T, **kw)
    for kw, match in ((dict(radius=0), "radius"), (dict(radius=4), "radius"), (dict(radius=1.5), "radius"), (dict(gate=-2.0), "gate"),
                      (dict(gate=float("nan")), "gate"), (dict(min_neighbours=-1), "min_neighbours"), (dict(min_neighbours=10), "min_neighbours"),
                      (dict(radius=2, min_neighbours=26), "min_neighbours")):
        with pytest.raises(ValueError, match=match):
            E.regularise_inverse_depth(a(), **kw)
    with pytest.raises(ValueError, match="float64"):
        E.regularise_inverse_depth(a(variance=torch.zeros(size, dtype=torch.float32)))
    with pytest.raises(ValueError, match="float64"):
        E.inverse_depth_depth_map(a(inv_depth=torch.zeros(size, dtype=torch.float32)))
    disp = E.Disparity(torch.ones((2,) + size), torch.ones((2,) + size, dtype=torch.int32), torch.ones((2,) + size, dtype=torch.int32),
                       torch.ones((2,) + size, dtype=torch.bool))
    for sigma in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma_disparity"):
            E.disparity_inverse_depth(disp, 0, 200.0, 0.1, sigma)
    for fx, b in ((0.0, 0.1), (200.0, -0.1), (float("nan"), 0.1), (200.0, float("inf"))):
        with pytest.raises(ValueError, match="fx and baseline"):
            E.disparity_inverse_depth(disp, 0, fx, b)
    for k in (2, -1, 0.5):
        with pytest.raises(IndexError, match="k must be"):
            E.disparity_inverse_depth(disp, k, 200.0, 0.1)
    with pytest.raises(ValueError, match="Disparity"):
        E.disparity_inverse_depth(disp[:3], 0, 200.0, 0.1)
    dm = E.DepthMap(torch.ones(size, dtype=torch.float64), torch.zeros(size, dtype=torch.int32), torch.ones(size), torch.ones(size, dtype=torch.bool))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="variance"):
            E.depth_inverse_depth(dm, bad)
    with pytest.raises(ValueError, match="variance"):
        E.depth_inverse_depth(dm, torch.ones((4, 5), dtype=torch.float64))
    with pytest.raises(ValueError, match="DepthMap"):
        E.depth_inverse_depth(dm[:3], 0.1)
    c, q = np.zeros((2, 3)), np.tile([0.0, 0, 0, 1.0], (2, 1))
    for kw, exc, match in ((dict(target=2), IndexError, "target"), (dict(target=0, gate=-1.0), ValueError, "gate"),
                           (dict(target=0, sigma_disparity=-1.0), ValueError, "sigma_disparity"), (dict(target=0, radius=4), ValueError, "radius"),
                           (dict(target=0, min_count=0), ValueError, "min_count"), (dict(target=0, radius=1, min_neighbours=10), ValueError,
                                                                                  "min_neighbours")):
        with pytest.raises(exc, match=match):
            E.fuse_stereo_depth(disp, 200.0, 0.1, K, c, q, **kw)
    with pytest.raises(ValueError, match="one pose per slice"):
        E.fuse_stereo_depth(disp, 200.0, 0.1, K, c[:1], q, 0)


def test_the_kernels_compile_without_register_spills(tmp_path):
    """every kernel of evk_fusion.hip compiles for gfx950 without spilling registers and without scratch memory (the per-view
    parameters are read from the kernel argument, not copied to a private array); the tile of the regularisation stays in LDS"""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    from event_utils_amd.csrc import build as B
    src = os.path.join(B.HERE, "evk_fusion.hip")
    done = subprocess.run([hipcc] + list(B.CFLAGS) + ["-c", src, "-o", str(tmp_path / "fusion.o"), "-save-temps=obj"], check=True, cwd=B.HERE,
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert b"warning" not in done.stdout, done.stdout.decode()
    asm = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert asm, os.listdir(tmp_path)
    text = open(tmp_path / asm[0]).read()
    kernels = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    seen = {n: (int(p), int(v), int(sp), int(lds)) for lds, n, p, v, sp in kernels}
    for name, count in (("k_fusion_propagate", 1), ("k_fusion_fuse", 1), ("k_fusion_regularise", 3)):
        assert sum(name in n for n in seen) == count, (name, sorted(seen))
    assert not {n: v for n, v in seen.items() if v[0] or v[2]}                   # no scratch, no spills
    assert all(v[1] <= 64 for v in seen.values())                                # eight waves per SIMD
    lds = sorted(v[3] for n, v in seen.items() if "regularise" in n)
    assert lds[0] >= 17 * 34 * 10 and lds[-1] <= 17 * 38 * 14 + 64 and lds[-1] < 16384, lds
