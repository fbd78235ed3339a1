"""GPU: depth fusion (event_utils_amd/depth/fusion.py, evk_fusion.hip) against its restatement (tests/_fusion_np.py), bit for bit:
the candidate columns of propagate_inverse_depth, the five fields of fuse_inverse_depth and of regularise_inverse_depth.  Everything
is an IEEE double in a fixed order, so no comparison here has a tolerance.  (A NaN equals a NaN: which sign and payload an invalid
operation gives is the processor's business, not the definition's.)"""
import functools

import numpy as np
import pytest
import torch

import _fusion_np as N
import _stereo_np as S

pytestmark = pytest.mark.gpu

SENSORS = ((1, 1), (2, 3), (7, 9), (33, 131), (70, 259))
VIEWS = (1, 2, 5, 16)
DEPTHS = (2.5, 3.5)
BASE_ROTATION = np.radians([1.2, -1.4, 0.8])                # about two degrees
BASE_SHIFT = np.array([0.2, -0.1, 0.15])                    # about a tenth of the depth


def camera_matrix(size, scale=0.9):
    h, w = size
    return np.array([[scale * max(w, 8), 0.0, (w - 1) / 2 + 0.3], [0.0, 0.95 * scale * max(w, 8), (h - 1) / 2 - 0.2], [0.0, 0.0, 1.0]])


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want, what):
    g, w = bits(got), bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    differ = (g != w) & ~(np.isnan(g.view(np.float64)) & np.isnan(w.view(np.float64)))
    if differ.any():
        bad = np.argwhere(differ)
        raise AssertionError("%s: %d of %d values differ, the first at %s: %r, expected %r" % (
            what, len(bad), w.size, tuple(bad[0]), np.asarray(got.cpu() if isinstance(got, torch.Tensor) else got)[tuple(bad[0])],
            np.asarray(want)[tuple(bad[0])]))


def same_ints(got, want, what):
    assert got.dtype == torch.int32 and got.is_cuda, what
    got = got.cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want), (what, int((got != want).sum()) if got.shape == want.shape else got.shape)


def same_flags(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.bool_ and np.array_equal(got, want), what


def same_map(got, want, what):
    """an InverseDepthMap on the device against the restatement's five arrays"""
    import event_utils_amd as E
    assert isinstance(got, E.InverseDepthMap) and all(t.is_cuda for t in got)
    same_bits(got.inv_depth, want[0], what + ": inv_depth")
    same_bits(got.variance, want[1], what + ": variance")
    same_ints(got.count, want[2], what + ": count")
    same_ints(got.rejected, want[3], what + ": rejected")
    same_flags(got.mask, want[4], what + ": mask")


def same_candidates(got, want, what):
    assert len(got) == 4 and all(t.is_cuda and t.dim() == 1 for t in got)
    same_ints(got[0], want[0], what + ": xi")
    same_ints(got[1], want[1], what + ": yi")
    same_bits(got[2], want[2], what + ": inv_depth")
    same_bits(got[3], want[3], what + ": variance")


def random_maps(rng, views, size, fraction, junk=True, constant_variance=None):
    """`views` maps with about `fraction` of their pixels valid, depths in DEPTHS; with junk some MASKED pixels hold what is no
    source: NaN, +-inf, 0 or a negative inv_depth, NaN, 0, a negative or an infinite variance"""
    maps = []
    for _ in range(views):
        mask = rng.random(size) < fraction
        rho = np.where(mask, 1.0 / rng.uniform(DEPTHS[0], DEPTHS[1], size), np.nan)
        var = np.where(mask, rng.uniform(1e-4, 4e-4, size) if constant_variance is None else constant_variance, np.nan)
        if junk and mask.size >= 6:
            flat = rng.permutation(mask.size)[:min(18, mask.size)]
            bad_rho = (np.nan, np.inf, -np.inf, 0.0, -0.25, 0.4, 0.4, 0.4, 0.4)
            bad_var = (2e-4, 2e-4, 2e-4, 2e-4, 2e-4, np.nan, 0.0, -1e-4, np.inf)
            for j, p in enumerate(flat):
                at = np.unravel_index(p, size)
                mask[at], rho[at], var[at] = True, bad_rho[j % 9], bad_var[j % 9]
        maps.append((rho, var, mask.astype(np.int32), np.zeros(size, dtype=np.int32), mask))
    return maps


def on_device(maps, every_other_numpy=False):
    """the restatement's maps as InverseDepthMaps: device tensors, or numpy arrays for every other one"""
    import event_utils_amd as E
    return [E.InverseDepthMap(*((np.array(a) if every_other_numpy and s % 2 else torch.from_numpy(np.array(a)).cuda()) for a in m))
            for s, m in enumerate(maps)]


def transforms_for(kind, views):
    out = []
    for s in range(views):
        f = 1.0 + 0.15 * s                                  # every view its own motion
        if kind == "identity":
            out.append(N.transform12(np.eye(3), np.zeros(3)))
        elif kind == "moved":
            out.append(N.transform12(N.rodrigues(BASE_ROTATION * f), BASE_SHIFT * f))
        elif kind == "zoom":                                # Z' = Z + 6 is about 3 Z: the image shrinks about three times
            out.append(N.transform12(np.eye(3), [0.01 * s, -0.01 * s, 6.0 + 0.02 * s]))
        elif kind == "behind":
            out.append(N.transform12(N.rodrigues(BASE_ROTATION * f), [0.0, 0.0, -10.0 - s]))
        elif kind == "off":
            out.append(N.transform12(np.eye(3), [1000.0 + s, 0.0, 0.0]))
        else:
            raise ValueError(kind)
    return np.array(out)


def check(maps, K, T, what, fuse=({},), numpy_maps=False, **target):
    """propagate and every set of fuse options against the restatement -> (the candidates, the last fused map, its restatement)"""
    import event_utils_amd as E
    dev = on_device(maps, numpy_maps)
    pv = target.pop("process_variance", 0.0)
    cands = N.propagate(maps, K, T, pv, target.get("target_camera_matrix"), target.get("target_size"))
    same_candidates(E.propagate_inverse_depth(dev, K, T, pv, **target), cands, what)
    size = target.get("target_size") or maps[0][0].shape
    got = want = None
    for opts in fuse:
        want = N.fuse_candidates(cands, size, **opts)
        got = E.fuse_inverse_depth(dev, K, T, process_variance=pv, **opts, **target)
        same_map(got, want, "%s %r" % (what, opts))
    return cands, got, want


# ---- sizes, views and motions ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("views", VIEWS)
@pytest.mark.parametrize("size", SENSORS, ids=lambda s: "%dx%d" % s)
def test_every_sensor_and_view_count(size, views):
    rng = np.random.default_rng([size[0], size[1], views])
    fraction = 0.15 if size[0] * size[1] * views > 20000 else 0.6
    maps = random_maps(rng, views, size, fraction)
    cands, _, want = check(maps, camera_matrix(size), transforms_for("moved", views), "moved", numpy_maps=views == 2)
    if size[0] * size[1] >= 63:
        assert len(cands[0]) > 0 and want[4].any()
    check(maps, camera_matrix(size), transforms_for("identity", views), "identity")


@pytest.mark.parametrize("fraction", (0.0, 0.15, 1.0))
@pytest.mark.parametrize("size,views", (((7, 9), 5), ((33, 131), 2), ((70, 259), 1)), ids=str)
def test_valid_fractions(size, views, fraction):
    rng = np.random.default_rng([size[0], views, int(fraction * 100)])
    maps = random_maps(rng, views, size, fraction, junk=fraction == 0.15)
    cands, _, want = check(maps, camera_matrix(size), transforms_for("moved", views), "fraction %g" % fraction)
    if fraction == 0.0:
        assert len(cands[0]) == 0 and not want[4].any() and np.isnan(want[0]).all()


def test_what_is_no_source_is_dropped():
    """masked pixels that hold NaN, +-inf, 0 or a negative inv_depth, or NaN, 0, a negative or an infinite variance: no candidates"""
    size = (7, 9)
    rng = np.random.default_rng(3)
    maps = random_maps(rng, 2, size, 0.0, junk=True)
    assert all(m[4].sum() == 18 for m in maps)
    cands, got, want = check(maps, camera_matrix(size), transforms_for("identity", 2), "junk")
    assert len(cands[0]) == 0 and not want[2].any()
    maps = random_maps(rng, 2, size, 1.0, junk=True)
    cands, got, want = check(maps, camera_matrix(size), transforms_for("identity", 2), "junk among sources")
    assert len(cands[0]) == 2 * (63 - 18)


@pytest.mark.parametrize("kind", ("behind", "off"))
def test_nothing_arrives(kind):
    size = (33, 131)
    maps = random_maps(np.random.default_rng(4), 5, size, 0.5)
    cands, got, want = check(maps, camera_matrix(size), transforms_for(kind, 5), kind)
    assert len(cands[0]) == 0
    assert np.isnan(want[0]).all() and np.isnan(want[1]).all() and not want[2].any() and not want[3].any() and not want[4].any()
    assert bool(torch.isnan(got.inv_depth).all()) and int(got.count.abs().sum()) == 0 and not bool(got.mask.any())


@functools.lru_cache(maxsize=None)
def zoom_case():
    size, views = (33, 131), 16
    maps = random_maps(np.random.default_rng(16), views, size, 0.45)
    K, T = camera_matrix(size), transforms_for("zoom", views)
    return maps, K, T, N.propagate(maps, K, T)


def test_a_zoom_out_crowds_pixels_beyond_one_wave():
    """16 views shrunk three times: target pixels with more than 64 candidates, runs on either side of 64"""
    maps, K, T, cands = zoom_case()
    lengths = sorted(len(c) for c in N.runs(cands, (33, 131)).values())
    assert lengths[-1] > 64 and lengths[0] < 63, (lengths[0], lengths[-1])
    assert N.longest_run(cands, (33, 131)) == lengths[-1]
    _, got, want = check(maps, K, T, "zoom", fuse=({}, dict(gate=0.5), dict(gate=1e6)))
    assert want[2].max() > 64 and int(got.count.max()) == want[2].max()


@pytest.mark.parametrize("size,target", (((7, 9), (12, 5)), ((33, 131), (40, 70)), ((33, 131), (1, 1)), ((2, 3), (70, 259)),
                                         ((70, 259), (33, 131))), ids=str)
def test_another_target_size_and_camera(size, target):
    rng = np.random.default_rng([size[0], target[0], target[1]])
    views = 2
    maps = random_maps(rng, views, size, 0.4)
    Kt = camera_matrix(target, 0.7)
    cands, _, want = check(maps, camera_matrix(size), transforms_for("moved", views), "target", target_camera_matrix=Kt, target_size=target)
    assert want[0].shape == target
    check(maps, camera_matrix(size), transforms_for("identity", views), "target, same camera", target_size=target)
    check(maps, camera_matrix(size), transforms_for("moved", views), "same size, other camera", target_camera_matrix=Kt)


def test_constant_variances_tie_everywhere():
    size, views = (33, 131), 5
    maps = random_maps(np.random.default_rng(9), views, size, 0.6, junk=False, constant_variance=2.5e-4)
    # the identity keeps rho' = rho up to an ulp, so the variances stay equal or all but equal: the earliest wins
    _, _, want = check(maps, camera_matrix(size), transforms_for("identity", views), "ties", fuse=({}, dict(gate=0.0), dict(gate=0.3)))
    assert want[3].any() and (want[2] + want[3]).max() == views
    check(maps, camera_matrix(size), transforms_for("moved", views), "ties, moved", fuse=(dict(gate=0.3),))
    # inverse depths whose reciprocals are exact: rho' = rho and v' = v to the bit, so EVERY comparison of variances is a tie and the
    # anchor is the first view that saw the pixel; with a narrow gate it decides which of the two depths the pixel gets
    rng = np.random.default_rng(19)
    exact = [(np.where(m[4], rng.choice([0.25, 0.5], size), np.nan),) + m[1:] for m in maps]
    cands, _, want = check(exact, camera_matrix(size), transforms_for("identity", views), "exact ties", fuse=(dict(gate=0.1),))
    assert set(np.unique(cands[3])) == {2.5e-4} and set(np.unique(want[0][want[4]])) == {0.25, 0.5}
    first = np.full(size, np.nan)
    for m in exact[::-1]:
        first[m[4]] = m[0][m[4]]
    assert np.array_equal(want[0], first, equal_nan=True)


def test_process_variance_per_view():
    size, views = (33, 131), 5
    maps = random_maps(np.random.default_rng(10), views, size, 0.5)
    K, T = camera_matrix(size), transforms_for("moved", views)
    pv = np.array([0.0, 1e-4, 3e-3, 0.0, 5e-5])
    cands, _, _ = check(maps, K, T, "per view", process_variance=pv, fuse=({}, dict(gate=0.7)))
    plain = N.propagate(maps, K, T)
    assert np.array_equal(cands[2], plain[2]) and (cands[3] >= plain[3]).all() and (cands[3] > plain[3]).any()
    check(maps, K, T, "scalar", process_variance=2e-4)
    check(maps, K, T, "tensor", process_variance=torch.from_numpy(pv))


# ---- the options of the fusion ---------------------------------------------------------------------------------------------------

def test_every_fusion_option():
    size, views = (33, 131), 5
    maps = random_maps(np.random.default_rng(11), views, size, 0.5)
    K, T = camera_matrix(size), transforms_for("moved", views)
    plain = N.fuse(maps, K, T)
    half = float(np.median(plain[1][plain[4]]))              # cuts about half the pixels
    options = [dict(gate=g, min_count=c, max_variance=v) for g in (0.0, 2.0, 1e6) for c in (1, 3) for v in (None, half)]
    check(maps, K, T, "options", fuse=options)
    cut = N.fuse(maps, K, T, max_variance=half)
    assert 0.3 * plain[4].sum() < cut[4].sum() < 0.7 * plain[4].sum()
    assert N.fuse(maps, K, T, gate=0.0)[3].sum() > N.fuse(maps, K, T, gate=1e6)[3].sum() == 0
    assert N.fuse(maps, K, T, min_count=3)[4].sum() < plain[4].sum()
    check(maps, K, T, "an infinite gate and limit", fuse=(dict(gate=float("inf"), max_variance=float("inf")), dict(max_variance=0.0)))


# ---- regularisation --------------------------------------------------------------------------------------------------------------

def check_regularise(idm, what, **kw):
    import event_utils_amd as E
    want = N.regularise(idm, **kw)
    got = E.regularise_inverse_depth(E.InverseDepthMap(*(torch.from_numpy(np.array(a)).cuda() for a in idm)), **kw)
    same_map(got, want, "%s %r" % (what, kw))
    return want


@functools.lru_cache(maxsize=None)
def fused_case():
    size, views = (33, 131), 5
    maps = random_maps(np.random.default_rng(12), views, size, 0.5)
    return N.fuse(maps, camera_matrix(size), transforms_for("moved", views))


@pytest.mark.parametrize("radius", (1, 2, 3))
def test_regularisation_of_a_fused_map(radius):
    full = (2 * radius + 1) ** 2
    idm = fused_case()
    kept = [int(check_regularise(idm, "fused", radius=radius, gate=2.0, min_neighbours=mn)[4].sum()) for mn in (0, 2, full - 1, full)]
    assert kept[0] == idm[4].sum() and kept[0] >= kept[1] > kept[2] >= kept[3] == 0
    check_regularise(idm, "fused", radius=radius, gate=0.0, min_neighbours=0)
    check_regularise(idm, "fused", radius=radius, gate=1e6, min_neighbours=1)


@pytest.mark.parametrize("size", SENSORS, ids=lambda s: "%dx%d" % s)
def test_regularisation_to_every_border(size):
    """dense maps, valid to every border, junk included: the window is clipped to the image, and only a full window passes
    min_neighbours = (2 r + 1)^2 - 1"""
    rng = np.random.default_rng([size[0], size[1], 13])
    dense = random_maps(rng, 1, size, 1.0, junk=False)[0]
    small = size[0] * size[1] < 10000                        # (the restatement's loops set the pace on the largest sensor)
    for radius in (1, 2, 3) if small else (3,):
        full = (2 * radius + 1) ** 2
        want = check_regularise(dense, "dense", radius=radius, gate=1e6, min_neighbours=full - 1)
        inner = np.zeros(size, dtype=bool)
        inner[radius:size[0] - radius, radius:size[1] - radius] = True
        assert np.array_equal(want[4], inner)
        if small:
            assert not check_regularise(dense, "dense", radius=radius, gate=1e6, min_neighbours=full)[4].any()
    holes = random_maps(rng, 1, size, 0.7 if small else 0.4, junk=True)[0]
    check_regularise(holes, "holes and junk", radius=1, gate=2.0, min_neighbours=0)
    check_regularise(holes, "holes and junk", radius=3, gate=2.0, min_neighbours=2)


# ---- chaining, repeatability, the pipeline ---------------------------------------------------------------------------------------

def test_a_fused_map_is_one_more_map_of_the_next_fusion():
    import event_utils_amd as E
    size = (33, 131)
    rng = np.random.default_rng(14)
    K = camera_matrix(size)
    first, second = random_maps(rng, 3, size, 0.4), random_maps(rng, 2, size, 0.4)
    T1, T2 = transforms_for("moved", 3), transforms_for("moved", 3)
    want1 = N.fuse(first, K, T1, gate=2.0)
    got1 = E.fuse_inverse_depth(on_device(first), K, T1, gate=2.0)
    same_map(got1, want1, "first")
    want2 = N.fuse([want1] + second, K, T2, gate=2.0, process_variance=[1e-5, 0.0, 0.0])
    got2 = E.fuse_inverse_depth([got1] + on_device(second), K, T2, gate=2.0, process_variance=[1e-5, 0.0, 0.0])
    same_map(got2, want2, "second")
    assert want2[2].max() > 1 and want2[4].sum() > want1[4].sum() // 2
    again = E.fuse_inverse_depth([got1] + on_device(second), K, T2, gate=2.0, process_variance=[1e-5, 0.0, 0.0])
    assert all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
               for a, b in zip(again, got2))
    smooth = E.regularise_inverse_depth(got2, radius=2)
    same_map(smooth, N.regularise(want2, radius=2), "regularised")
    twice = E.regularise_inverse_depth(got2, radius=2)
    assert torch.equal(smooth.inv_depth.view(torch.int64), twice.inv_depth.view(torch.int64)) and torch.equal(smooth.mask, twice.mask)


def test_the_conversions():
    import event_utils_amd as E
    size = (7, 9)
    rng = np.random.default_rng(15)
    depth = rng.uniform(0.5, 4.0, size)
    depth[0, 0], depth[1, 1], depth[2, 2], depth[3, 3] = np.nan, 0.0, -1.0, np.inf
    mask = rng.random(size) < 0.8
    mask[0, 0] = mask[1, 1] = mask[2, 2] = mask[3, 3] = True
    dm = E.DepthMap(torch.from_numpy(depth).cuda(), torch.zeros(size, dtype=torch.int32).cuda(), torch.ones(size).cuda(),
                    torch.from_numpy(mask).cuda())
    valid = mask & np.isfinite(depth) & (depth > 0)
    var_map = rng.uniform(1e-4, 1e-3, size)
    for variance, want_var in ((2e-4, np.full(size, 2e-4)), (var_map, var_map), (torch.from_numpy(var_map), var_map)):
        idm = E.depth_inverse_depth(dm, variance)
        with np.errstate(divide="ignore"):
            same_map(idm, (np.where(valid, 1.0 / depth, np.nan), np.where(valid, want_var, np.nan), valid.astype(np.int32),
                           np.zeros(size, dtype=np.int32), valid), "depth_inverse_depth")
    back = E.inverse_depth_depth_map(idm)
    assert isinstance(back, E.DepthMap) and back.depth.dtype == torch.float64 and back.confidence.dtype == torch.float32
    same_bits(back.depth, np.where(valid, 1.0 / (1.0 / np.where(valid, depth, 1.0)), np.nan), "depth")
    assert torch.equal(back.index, idm.count) and torch.equal(back.mask, idm.mask)
    assert np.array_equal(back.confidence.cpu().numpy(), -np.where(valid, var_map, np.nan).astype(np.float32), equal_nan=True)


def test_fuse_stereo_depth_end_to_end():
    """a seeded Disparity of four slices at (33, 131) through the whole chain; the points of the fused map are the restatement's"""
    import event_utils_amd as E
    size, nk, fx, baseline = (33, 131), 4, 0.9 * 131, 0.1
    rng = np.random.default_rng(17)
    QL, QR = S.random_pair(rng, nk, 1, size[0], size[1], density=0.6, shift=6, noise=0.1)
    disp = E.stereo_match(torch.from_numpy(QL).cuda(), torch.from_numpy(QR).cuda(), 15, radius=2, min_activity=64)
    assert int(disp.mask.sum()) > 400
    K = camera_matrix(size)
    positions = rng.normal(size=(nk, 3)) * 0.05
    rot = [N.rodrigues(rng.normal(size=3) * 0.01) for _ in range(nk)]
    from event_utils_amd.depth.tracking import _quaternion
    quaternions = np.array([_quaternion(R) for R in rot])
    host = [N.disparity_inverse_depth(disp.disparity[k].cpu().numpy(), disp.mask[k].cpu().numpy(), fx, baseline, 0.5) for k in range(nk)]
    for k in range(nk):
        same_map(E.disparity_inverse_depth(disp, k, fx, baseline), host[k], "slice %d" % k)
    target = 2
    T = E.relative_transforms(positions, quaternions, (positions[target], quaternions[target]))
    want = N.fuse(host, K, T, gate=2.0, process_variance=1e-6, min_count=2)
    got = E.fuse_stereo_depth(disp, fx, baseline, K, positions, quaternions, target, process_variance=1e-6, min_count=2)
    same_map(got, want, "fused")
    assert want[4].sum() > 50
    want_r = N.regularise(want, radius=2, gate=2.0, min_neighbours=1)
    got_r = E.fuse_stereo_depth(disp, fx, baseline, K, positions, quaternions, target, process_variance=1e-6, min_count=2, radius=2,
                                min_neighbours=1)
    same_map(got_r, want_r, "regularised")
    for g, w in ((got, want), (got_r, want_r)):
        dm, want_dm = E.inverse_depth_depth_map(g), N.depth_map(w)
        same_bits(dm.depth, want_dm[0], "depth")
        same_ints(dm.index, want_dm[1], "index")
        assert np.array_equal(dm.confidence.cpu().numpy(), want_dm[2], equal_nan=True) and dm.confidence.dtype == torch.float32
        same_flags(dm.mask, want_dm[3], "mask")
        pts = E.reference_points(dm, K)
        assert pts.is_cuda and pts.dtype == torch.float64
        same_bits(pts, N.depth_points(w, K), "points")
    assert len(N.depth_points(want_r, K)) > 20


# ---- a seeded fuzz slice ---------------------------------------------------------------------------------------------------------

FUZZ_CASES, FUZZ_PARTS = 200, 4


@pytest.mark.parametrize("part", range(FUZZ_PARTS))
def test_fuzz(part):
    """small sensors, 1 .. 6 views, random rigid motions, targets and options, each against the restatement"""
    for case in range(part, FUZZ_CASES, FUZZ_PARTS):
        rng = np.random.default_rng([2024, case])
        size = (int(rng.integers(1, 12)), int(rng.integers(1, 15)))
        views = int(rng.integers(1, 7))
        maps = random_maps(rng, views, size, float(rng.choice([0.0, 0.15, 0.5, 1.0])), junk=bool(rng.integers(2)),
                           constant_variance=None if rng.integers(3) else 2e-4)
        scale = float(rng.choice([0.0, 0.01, 0.05, 0.3]))
        T = np.array([N.transform12(N.rodrigues(rng.normal(size=3) * scale), rng.normal(size=3) * 3.0 * scale + [0, 0, rng.choice([0, 0, 6.0, -9.0])])
                      for _ in range(views)])
        target = {}
        if rng.integers(2):
            target["target_size"] = (int(rng.integers(1, 12)), int(rng.integers(1, 15)))
        if rng.integers(2):
            target["target_camera_matrix"] = camera_matrix(target.get("target_size", size), float(rng.uniform(0.3, 1.2)))
        if rng.integers(2):
            target["process_variance"] = rng.uniform(0.0, 1e-3, views) * rng.integers(0, 2, views)
        opts = dict(gate=float(rng.choice([0.0, 0.5, 2.0, 1e6])), min_count=int(rng.integers(1, 4)))
        if rng.integers(2):
            opts["max_variance"] = float(rng.uniform(5e-5, 4e-4))
        what = "case %d: %r, %d views, %r, %r" % (case, size, views, target, opts)
        _, _, fused = check(maps, camera_matrix(size), T, what, fuse=(opts,), numpy_maps=bool(rng.integers(2)), **target)
        radius = int(rng.integers(1, 4))
        check_regularise(fused, what, radius=radius, gate=float(rng.choice([0.0, 1.0, 2.0, 1e6])),
                         min_neighbours=int(rng.integers(0, (2 * radius + 1) ** 2 + 1)))
