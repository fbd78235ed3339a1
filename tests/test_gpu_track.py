"""GPU: camera tracking (event_utils_amd/depth/tracking.py, evk_track.hip) against its restatement (tests/_track_np.py).  The
per-point residuals, Jacobians and valid flags are the restatement's bits; the count is exact and every sum lies within the bound of
its own summation, n 2^-52 sum |term|, of the correctly rounded sum of the restatement's per-point products; the loop ends within
1e-3 px of the restatement's loop."""
import functools
import math

import numpy as np
import pytest
import torch

import _track_np as N

pytestmark = pytest.mark.gpu

SIZES = ((2, 2), (7, 9), (60, 80))
COUNTS = (1, 63, 64, 65, 257, 1025, 5000)


def camera(intr):
    fx, fy, cx, cy = intr
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def case(m, size, general):
    """points, surface, intrinsics and a pose.  general: a pose that is no identity and projections that spill over every side of
    the surface.  Otherwise fx = fy = 1, cx = cy = 0, the identity, Z = 1, so that (u, v) = (X, Y) exactly, and the first points
    sit on each border, behind the camera and at values that are not finite."""
    H, W = size
    rng = np.random.default_rng(1000 * m + 10 * H + int(general))
    S = rng.uniform(0.0, 255.0, (H, W)).astype(np.float32)
    if general:
        intr = (0.9 * W, 0.8 * W, 0.5 * (W - 1), 0.5 * (H - 1))
        R, t = N.se3_exp([0.05, -0.03, 0.04, 0.02, -0.03, 0.05])
        u, v, Z = rng.uniform(-1.0, W, m), rng.uniform(-1.0, H, m), rng.uniform(0.5, 4.0, m)
        X = np.stack(((u - intr[2]) / intr[0] * Z, (v - intr[3]) / intr[1] * Z, Z), axis=1)
        P = (X - t) @ R
        P[rng.uniform(size=m) < 0.05] *= -1.0               # behind the camera
    else:
        intr, R, t = (1.0, 1.0, 0.0, 0.0), np.eye(3), np.zeros(3)
        P = np.stack((rng.uniform(-0.5, W - 0.5, m), rng.uniform(-0.5, H - 0.5, m), np.ones(m)), axis=1)
        below = np.nextafter
        special = [(0.0, 0.0, 1.0), (W - 1.0, 0.5, 1.0), (below(W - 1.0, 0.0), 0.5, 1.0), (0.5, H - 1.0, 1.0), (0.5, below(H - 1.0, 0.0), 1.0),
                   (below(0.0, -1.0), 0.5, 1.0), (0.5, -1e-300, 1.0), (0.5, 0.5, 0.0), (0.5, 0.5, -1.0), (np.nan, 0.5, 1.0), (0.5, 0.5, np.nan),
                   (np.inf, 0.5, 1.0), (0.5, -np.inf, 1.0), (0.5, 0.5, np.inf), (0.25, 0.75, 1.0)]
        at = rng.permutation(m)[:len(special)]
        P[at] = special[:len(at)]
    return P, S, intr, R, t


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint8)


# ---- per-point values ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("m", COUNTS)
def test_residuals_are_the_restatements_bits(m, size):
    import event_utils_amd as E
    for general in (False, True):
        P, S, intr, R, t = case(m, size, general)
        r, J, valid = E.registration_residuals(torch.from_numpy(P).cuda(), torch.from_numpy(S).cuda(), camera(intr), N.matrix(R, t))
        assert (r.dtype, J.dtype, valid.dtype) == (torch.float64, torch.float64, torch.bool) and r.is_cuda and J.is_cuda and valid.is_cuda
        assert tuple(r.shape) == (m,) and tuple(J.shape) == (m, 6) and tuple(valid.shape) == (m,)
        wr, wJ, wv = N.residuals(P, S, intr, R, t)
        got_v, got_r, got_J = valid.cpu().numpy(), r.cpu().numpy(), J.cpu().numpy()
        assert np.array_equal(got_v, wv), ("valid", general, np.flatnonzero(got_v != wv)[:5])
        assert np.isnan(got_r[~wv]).all() and np.isnan(got_J[~wv]).all()
        assert np.array_equal(bits(got_r[wv]), bits(wr[wv])), ("r", general)
        assert np.array_equal(bits(got_J[wv]), bits(wJ[wv])), ("J", general)
        if m >= 257 and size != (2, 2):
            assert 0 < wv.sum() < m
    # numpy in, the same bits out
    P, S, intr, R, t = case(m, size, True)
    r2, J2, v2 = E.registration_residuals(P, S, camera(intr), torch.from_numpy(N.matrix(R, t)))
    assert r2.is_cuda and np.array_equal(r2.cpu().numpy(), got_r, equal_nan=True) and np.array_equal(J2.cpu().numpy(), got_J, equal_nan=True)
    assert np.array_equal(v2.cpu().numpy(), got_v)


# ---- sums ------------------------------------------------------------------------------------------------------------------------

def check_sums(got, T, what):
    """a row of 29 device sums against the per-point products T (n, 29) of the restatement"""
    n = len(T)
    assert got[28] == float(n), (what, got[28], n)
    for k in range(29):
        want = math.fsum(T[:, k])
        bound = n * 2.0 ** -52 * math.fsum(np.abs(T[:, k]))
        assert abs(got[k] - want) <= bound, (what, k, got[k], want, bound)


def sums_of(A, g, c, n):
    """(B, 29) float64 numpy, the layout of the restatement's products, from registration_terms' results"""
    A, g, c, n = (x.cpu().numpy() for x in (A, g, c, n))
    iu = np.triu_indices(6)
    assert np.array_equal(A, np.swapaxes(A, 1, 2))
    return np.concatenate((A[:, iu[0], iu[1]], g, c[:, None], n[:, None].astype(np.float64)), axis=1)


@pytest.mark.parametrize("size", SIZES[1:], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("m", COUNTS)
def test_sums_lie_within_the_bound_of_their_summation(m, size):
    import event_utils_amd as E
    for general in (False, True):
        P, S, intr, R, t = case(m, size, general)
        dP, dS, K = torch.from_numpy(P).cuda(), torch.from_numpy(S).cuda(), camera(intr)
        others = [N.left(xi, R, t) for xi in ([0.01, 0.0, -0.02, 0.0, 0.01, 0.0], [0.0, 0.03, 0.0, -0.01, 0.0, 0.02])]
        batch = np.stack([N.matrix(R, t)] + [N.matrix(*o) for o in others])
        for loss, delta in (("l2", None), ("huber", 100.0)):
            if loss == "huber" and m >= 257:                # both branches are taken
                r = N.residuals(P, S, intr, R, t)[0]
                assert (np.abs(r) > delta).sum() > 10 and (np.abs(r) <= delta).sum() > 10
            out = E.registration_terms(dP, dS, K, batch[0], loss, delta)
            assert [tuple(x.shape) for x in out] == [(1, 6, 6), (1, 6), (1,), (1,)] and all(x.is_cuda for x in out)
            assert [x.dtype for x in out] == [torch.float64] * 3 + [torch.int64]
            one = sums_of(*out)
            check_sums(one[0], N.products(P, S, intr, R, t, loss, delta), (general, loss, "single"))
            again = sums_of(*E.registration_terms(dP, dS, K, batch[0], loss, delta))
            assert np.array_equal(bits(one), bits(again)), "two runs differ"
            three = sums_of(*E.registration_terms(dP, dS, K, batch, loss, delta))
            assert three.shape == (3, 29) and np.array_equal(bits(three[0]), bits(one[0])), "row 0 of the batch is not the single call"
            for b, (Rb, tb) in enumerate(others, 1):
                check_sums(three[b], N.products(P, S, intr, Rb, tb, loss, delta), (general, loss, b))
                alone = sums_of(*E.registration_terms(dP, dS, K, batch[b], loss, delta))
                assert np.array_equal(bits(three[b]), bits(alone[0])), "row %d of the batch is not the single call" % b


def test_more_poses_than_one_launch_takes():
    import event_utils_amd as E
    P, S, intr, R, t = case(1025, (60, 80), True)
    rng = np.random.default_rng(3)
    poses = [N.left(rng.normal(size=6) * 0.01, R, t) for _ in range(19)]
    got = sums_of(*E.registration_terms(P, S, camera(intr), np.stack([N.matrix(*p) for p in poses]), "huber", 50.0))
    assert got.shape == (19, 29)
    for b in (0, 15, 16, 18):
        check_sums(got[b], N.products(P, S, intr, *poses[b], "huber", 50.0), b)


def test_no_valid_point_gives_zeros():
    import event_utils_amd as E
    for m in (1, 300, 2500):
        P, S, intr, R, t = case(5000, (60, 80), True)
        P = P[:m] * np.array([1.0, 1.0, -1.0]) - np.array([0.0, 0.0, 10.0])
        assert not N.residuals(P, S, intr, R, t)[2].any()
        A, g, c, n = E.registration_terms(P, S, camera(intr), np.stack([N.matrix(R, t)] * 2), "huber", 10.0)
        assert not A.any() and not g.any() and not c.any() and n.tolist() == [0, 0]


# ---- the surface -----------------------------------------------------------------------------------------------------------------

def test_the_tracking_surface_is_scipys_blur_of_the_inverted_surface():
    """bit for bit, as tests/test_gpu_postpass.py holds the library's blur to scipy"""
    from scipy.ndimage import gaussian_filter
    import event_utils_amd as E
    rng = np.random.default_rng(2)
    Q = rng.integers(0, 256, (3, 2, 37, 53)).astype(np.uint8)
    Q[rng.uniform(size=Q.shape) < 0.6] = 0
    inverted = (255 - Q.max(axis=1).astype(np.int64)).astype(np.float32)
    for sigma in (1.0, 2.5, 0.5):
        got = E.tracking_surface(torch.from_numpy(Q).cuda(), sigma)
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (3, 37, 53)
        want = np.stack([gaussian_filter(inverted[k], sigma, mode="reflect") for k in range(3)])
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), sigma
    assert np.array_equal(E.tracking_surface(Q).cpu().numpy(), np.stack([gaussian_filter(inverted[k], 1.0, mode="reflect") for k in range(3)]))
    for none in (None, 0, 0.0):
        assert np.array_equal(E.tracking_surface(Q, none).cpu().numpy(), inverted)
    one = E.tracking_surface(Q[:1, :1], None)
    assert np.array_equal(one.cpu().numpy(), 255.0 - Q[:1, 0].astype(np.float32))


# ---- the loop --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scene():
    sc = N.scene()
    sc["device"] = (torch.from_numpy(sc["points"]).cuda(), torch.from_numpy(sc["surface"]).cuda())
    return sc


@pytest.mark.parametrize("start", range(N.SCENE_STARTS))
def test_the_loop_ends_where_the_restatements_loop_ends(start):
    import event_utils_amd as E
    sc = scene()
    P, S, truth = sc["points"], sc["surface"], sc["pose"]
    dP, dS = sc["device"]
    K = camera(N.SCENE_INTRINSICS)
    R0, t0 = sc["starts"][start]
    reg = E.register_points(dP, dS, K, N.matrix(R0, t0))
    assert isinstance(reg, E.Registration) and isinstance(reg.pose, np.ndarray) and reg.pose.shape == (4, 4) and reg.pose.dtype == np.float64
    assert np.array_equal(reg.pose[3], [0.0, 0.0, 0.0, 1.0]) and reg.status in ("converged", "stalled", "max_evals") and reg.evaluations <= 50
    # the reported cost and count are those of the returned pose
    A, g, c, n = E.registration_terms(dP, dS, K, reg.pose, "huber", 64.0)
    assert n.item() == reg.n_valid == 400 and np.float64(c.item()).tobytes() == np.float64(reg.cost).tobytes()
    got = (reg.pose[:3, :3], reg.pose[:3, 3])
    assert np.abs(got[0] @ got[0].T - np.eye(3)).max() < 1e-13
    Rn, tn, cn, nn, evals, status = N.register(P, S, N.SCENE_INTRINSICS, R0, t0)
    apart = N.reprojection_error(P, N.SCENE_INTRINSICS, got, (Rn, tn)).max()
    end = N.reprojection_error(P, N.SCENE_INTRINSICS, got, truth).mean()
    print("start %d: %d evaluations (%s), restatement %d (%s); %.3g px apart; %.4f px from the truth" % (
        start, reg.evaluations, reg.status, evals, status, apart, end))
    assert apart <= 1e-3
    assert (reg.evaluations, reg.status, reg.n_valid) == (evals, status, nn)
    assert end <= N.SCENE_END_ERROR + 0.05


def test_the_loop_takes_numpy_l2_and_its_limits():
    import event_utils_amd as E
    sc = scene()
    P, S, truth = sc["points"], sc["surface"], sc["pose"]
    K = camera(N.SCENE_INTRINSICS)
    R0, t0 = sc["starts"][0]
    reg = E.register_points(P, S, K, N.matrix(R0, t0), loss="l2", step_tol=1e-3)
    Rn, tn, cn, nn, evals, status = N.register(P, S, N.SCENE_INTRINSICS, R0, t0, loss="l2", delta=None, step_tol=1e-3)
    assert (reg.evaluations, reg.status) == (evals, status) == (reg.evaluations, "converged")
    assert N.reprojection_error(P, N.SCENE_INTRINSICS, (reg.pose[:3, :3], reg.pose[:3, 3]), (Rn, tn)).max() <= 1e-3
    A, g, c, n = E.registration_terms(P, S, K, reg.pose)
    assert c.item() == reg.cost and n.item() == reg.n_valid
    few = E.register_points(P, S, K, N.matrix(R0, t0), max_evals=3)
    assert (few.evaluations, few.status) == (3, "max_evals")
    one = E.register_points(P, S, K, N.matrix(R0, t0), max_evals=1)
    assert (one.evaluations, one.status) == (1, "max_evals") and np.array_equal(one.pose, N.matrix(R0, t0))
    flat = np.full(N.SCENE_SIZE, 7.0, dtype=np.float32)     # no gradient: every Cholesky fails and the damping runs out
    stalled = E.register_points(P, flat, K, N.matrix(*truth), loss="l2")
    assert (stalled.evaluations, stalled.status, stalled.cost, stalled.n_valid) == (1, "stalled", 49.0 * 400, 400)
    # from the identity (pose0 None): the scene's motion is within the basin
    reg = E.register_points(P, S, K)
    assert N.reprojection_error(P, N.SCENE_INTRINSICS, (reg.pose[:3, :3], reg.pose[:3, 3]), truth).mean() <= N.SCENE_END_ERROR + 0.05


def test_lost_when_every_point_is_behind_the_camera():
    import event_utils_amd as E
    sc = scene()
    back = sc["points"] * np.array([1.0, 1.0, -1.0])
    pose0 = N.matrix(*sc["starts"][1])
    reg = E.register_points(back, sc["surface"], camera(N.SCENE_INTRINSICS), pose0)
    assert (reg.status, reg.n_valid, reg.evaluations, reg.cost) == ("lost", 0, 1, 0.0) and np.array_equal(reg.pose, pose0)
    inside = int(N.residuals(sc["points"], sc["surface"], N.SCENE_INTRINSICS, *sc["starts"][1])[2].sum())
    reg = E.register_points(sc["points"], sc["surface"], camera(N.SCENE_INTRINSICS), pose0, min_points=inside + 1)
    assert (reg.status, reg.n_valid, reg.evaluations) == ("lost", inside, 1) and np.array_equal(reg.pose, pose0)
    assert E.register_points(sc["points"], sc["surface"], camera(N.SCENE_INTRINSICS), pose0, min_points=inside, max_evals=2).status == "max_evals"
    with pytest.raises(RuntimeError, match="lost at slice 0"):
        E.track_poses(back, sc["surface"][None], camera(N.SCENE_INTRINSICS), ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)), [0.0])


# ---- a trajectory ----------------------------------------------------------------------------------------------------------------

def test_track_poses_follows_a_known_motion():
    """three slices whose basins lie under the points' projections after one, two and three steps of the scene's motion, 0.7 to
    0.9 px each; the restatement's loop ends 0.160, 0.098 and 0.041 px from the truth"""
    import event_utils_amd as E
    from event_utils_amd.depth.emvs import _rotation
    sc = scene()
    P = sc["points"]
    K = camera(N.SCENE_INTRINSICS)
    truths = [N.scene_pose(k) for k in (1, 2, 3)]
    surfaces = np.stack([N.basin(N.project(P, N.SCENE_INTRINSICS, *T)) for T in truths])
    q_ref = np.array([0.1, -0.2, 0.05, -0.9])               # (qw < 0: the first result takes this sign)
    q_ref /= np.sqrt((q_ref * q_ref).sum())
    reference_pose = (np.array([0.5, -1.0, 2.0]), q_ref)
    pose_ts = np.array([0.1, 0.2, 0.35])
    positions, quaternions = E.track_poses(sc["device"][0], torch.from_numpy(surfaces).cuda(), K, reference_pose, pose_ts)
    assert isinstance(positions, np.ndarray) and positions.shape == (3, 3) and positions.dtype == np.float64
    assert isinstance(quaternions, np.ndarray) and quaternions.shape == (3, 4) and quaternions.dtype == np.float64
    assert np.abs((quaternions * quaternions).sum(axis=1) - 1.0).max() < 1e-15
    assert ((np.concatenate((q_ref[None], quaternions[:-1])) * quaternions).sum(axis=1) >= 0.0).all()
    # the trajectory is one that the multi-view stereo takes
    table = E.packet_transforms(np.array([0.1, 0.15, 0.35]), pose_ts, positions, quaternions, K, reference_pose)
    assert table.shape == (3, 12) and np.isfinite(table).all()
    R_ref = _rotation(q_ref)
    for k, truth in enumerate(truths):
        R_wc = _rotation(quaternions[k])
        R = R_wc.T @ R_ref                                  # R_wc = R_ref R^T, c = c_ref - R_wc t
        t = R_wc.T @ (reference_pose[0] - positions[k])
        end = N.reprojection_error(P, N.SCENE_INTRINSICS, (R, t), truth).mean()
        print("slice %d: %.4f px from the truth" % (k, end))
        assert end <= N.SCENE_END_ERROR + 0.05
    # the first slice alone is register_points from the identity
    reg = E.register_points(P, surfaces[0], K)
    R_wc = R_ref @ reg.pose[:3, :3].T
    assert np.abs(_rotation(quaternions[0]) - R_wc).max() < 1e-14 and np.abs(positions[0] - (reference_pose[0] - R_wc @ reg.pose[:3, 3])).max() < 1e-14
