"""CPU (no GPU): the host restatement of camera tracking (tests/_track_np.py, the literal definition) on hand-worked cases, its
gradient and Jacobian against central differences, its loop on the seeded recovery scene; the evk_track_* entry points are declared,
bound and exported and refuse bad arguments before they touch the device; the Python argument errors; the public surface; the
kernels of evk_track.hip compile for gfx950 without scratch memory and within the register count DESIGN.md states."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import _header
import _track_np as N

ENTRIES = {"evk_track_terms", "evk_track_residuals", "evk_track_register"}
PUBLIC = ("Registration", "tracking_surface", "reference_points", "registration_terms", "registration_residuals", "register_points",
          "track_poses")
UNIT = (1.0, 1.0, 0.0, 0.0)                                 # fx = fy = 1, cx = cy = 0: with Z' = 1, (u, v) = (X', Y')
EYE, ZERO = np.eye(3), np.zeros(3)


# ---- hand-worked cases of the restatement --------------------------------------------------------------------------------------------

def test_one_point_by_hand():
    S = np.array([[0, 10], [20, 50]], dtype=np.float32)
    r, J, valid = N.residuals(np.array([[0.25, 0.5, 1.0]]), S, UNIT, EYE, ZERO)
    assert valid.tolist() == [True]
    # r = .5 (.75 0 + .25 10) + .5 (.75 20 + .25 50); gx = .5 10 + .5 30; gy = .75 20 + .25 40
    assert r[0] == 15.0
    # j3 = (gx, gy, -(gx X + gy Y)) = (20, 25, -17.5); X x j3 = (.5 -17.5 - 25, 20 + .25 17.5, .25 25 - .5 20)
    assert J[0].tolist() == [20.0, 25.0, -17.5, -33.75, 24.375, -3.75]
    # the same point twice as far away, seen through fx = 2, fy = 4 about (1, 2) on a surface shifted by (1, 2)
    S2 = np.zeros((4, 3), dtype=np.float32)
    S2[2:, 1:] = S
    r2, J2, _ = N.residuals(np.array([[0.25, 0.25, 2.0]]), S2, (2.0, 4.0, 1.0, 2.0), EYE, ZERO)
    assert r2[0] == 15.0 and J2[0, :3].tolist() == [20.0 * 2 / 2, 25.0 * 4 / 2, -(40.0 * 0.25 + 100.0 * 0.25) / 4.0]
    # a pose moves the point first: a quarter turn about z and a shift back
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    r3, J3, _ = N.residuals(np.array([[0.5, -0.25, 0.5]]), S, UNIT, Rz, np.array([0.0, 0.0, 0.5]))
    assert r3[0] == 15.0 and J3[0].tolist() == J[0].tolist()


def test_the_huber_branches_by_hand():
    r = np.array([3.0, -3.0, 5.0, -5.0, 10.0, -20.0, 0.0])
    w, rho = N.weights(r, "huber", 5.0)
    assert w.tolist() == [1.0, 1.0, 1.0, 1.0, 0.5, 0.25, 1.0]                   # |r| == delta is the quadratic branch
    assert rho.tolist() == [9.0, 9.0, 25.0, 25.0, 5.0 * (20.0 - 5.0), 5.0 * (40.0 - 5.0), 0.0]
    w, rho = N.weights(r, "l2")
    assert w.tolist() == [1.0] * 7 and rho.tolist() == (r * r).tolist()
    # the sums of two points, one on each branch
    S = np.array([[0, 0, 0], [40, 40, 40], [80, 80, 80]], dtype=np.float32)     # r = 40 v, gx = 0, gy = 40
    P = np.array([[0.5, 0.05, 1.0], [0.5, 0.5, 1.0]])                           # r = 2 and 20
    A, g, c, n = N.terms(P, S, UNIT, EYE, ZERO, "huber", 5.0)
    assert n == 2 and c == 4.0 + 5.0 * (40.0 - 5.0)
    assert A[1, 1] == 1600.0 + 0.25 * 1600.0 and g[1] == 40.0 * 2.0 + (0.25 * 40.0) * 20.0 and A[0, 0] == 0.0
    A, g, c, n = N.terms(P, S, UNIT, EYE, ZERO)
    assert (n, c, A[1, 1], g[1]) == (2, 404.0, 3200.0, 880.0) and np.array_equal(A, A.T)


def test_validity_at_the_edges():
    H, W = 4, 6
    S = np.arange(H * W, dtype=np.float32).reshape(H, W)
    below = np.nextafter
    cases = [((0.0, 0.0, 1.0), True), ((W - 1.0, 0.0, 1.0), False), ((below(W - 1.0, 0.0), 0.0, 1.0), True),
             ((0.0, H - 1.0, 1.0), False), ((0.0, below(H - 1.0, 0.0), 1.0), True), ((-1e-300, 0.0, 1.0), False),
             ((0.0, below(0.0, -1.0), 1.0), False), ((1.0, 1.0, 0.0), False), ((1.0, 1.0, -1.0), False), ((np.nan, 1.0, 1.0), False),
             ((1.0, np.nan, 1.0), False), ((1.0, 1.0, np.nan), False), ((1.0, 1.0, np.inf), False), ((np.inf, 1.0, 1.0), False),
             ((0.0, 0.0, np.inf), False), ((2.5, 1.5, 1.0), True)]
    P = np.array([c[0] for c in cases])
    r, J, valid = N.residuals(P, S, UNIT, EYE, ZERO)
    assert valid.tolist() == [c[1] for c in cases]
    assert np.isnan(r[~valid]).all() and np.isnan(J[~valid]).all() and np.isfinite(r[valid]).all() and np.isfinite(J[valid]).all()
    assert r[0] == 0.0 and r[-1] == 1.5 * W + 2.5
    assert N.terms(P, S, UNIT, EYE, ZERO)[3] == 4
    A, g, c, n = N.terms(P[[1, 3, 7]], S, UNIT, EYE, ZERO)                      # nothing valid: zeros
    assert n == 0 and c == 0.0 and not A.any() and not g.any()
    Sn = S.copy()
    Sn[1, 1] = np.nan                                                           # a sample that is not finite takes its four cells out
    assert N.residuals(np.array([[0.5, 0.5, 1.0], [1.5, 1.5, 1.0], [2.5, 1.5, 1.0]]), Sn, UNIT, EYE, ZERO)[2].tolist() == [False, False, True]


# ---- derivatives -----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def interior_case():
    """300 points whose projections lie at least a quarter pixel from every pixel boundary, under a pose that is no identity, on a
    random surface: inside a cell the interpolant is a polynomial, so central differences see no kink"""
    rng = np.random.default_rng(11)
    H, W, intr = 40, 50, (45.0, 47.0, 24.0, 19.0)
    S = rng.uniform(0.0, 255.0, (H, W)).astype(np.float32)
    R, t = N.se3_exp([0.05, -0.03, 0.04, 0.02, -0.03, 0.05])
    m = 300
    u = rng.integers(0, W - 1, m) + rng.uniform(0.25, 0.75, m)
    v = rng.integers(0, H - 1, m) + rng.uniform(0.25, 0.75, m)
    Z = rng.uniform(1.0, 4.0, m)
    Xc = np.stack(((u - intr[2]) / intr[0] * Z, (v - intr[3]) / intr[1] * Z, Z), axis=1)
    return (Xc - t) @ R, S, intr, R, t                      # P = R^T (X' - t)


def test_the_gradient_of_the_cost_is_twice_g():
    P, S, intr, R, t = interior_case()
    r = N.residuals(P, S, intr, R, t)[0]
    for loss, delta in (("l2", None), ("huber", 115.0)):
        if delta:
            assert np.abs(np.abs(r) - delta).min() > 1e-3 and (np.abs(r) > delta).sum() > 50 and (np.abs(r) < delta).sum() > 50
        A, g, c, n = N.terms(P, S, intr, R, t, loss, delta)
        assert n == len(P)
        h = 1e-6
        for k in range(6):
            xi = np.zeros(6)
            xi[k] = h
            cp = N.terms(P, S, intr, *N.left(xi, R, t), loss, delta)
            cm = N.terms(P, S, intr, *N.left(-xi, R, t), loss, delta)
            assert cp[3] == cm[3] == n
            numeric = (cp[2] - cm[2]) / (2 * h)
            assert abs(numeric - 2.0 * g[k]) <= 1e-6 * max(abs(g).max(), 1.0), (loss, k, numeric, 2.0 * g[k])


def test_the_jacobian_is_the_derivative_of_every_residual():
    P, S, intr, R, t = interior_case()
    r, J, valid = N.residuals(P, S, intr, R, t)
    assert valid.all()
    h = 1e-6
    for k in range(6):
        xi = np.zeros(6)
        xi[k] = h
        numeric = (N.residuals(P, S, intr, *N.left(xi, R, t))[0] - N.residuals(P, S, intr, *N.left(-xi, R, t))[0]) / (2 * h)
        assert np.abs(numeric - J[:, k]).max() <= 1e-6 * np.abs(J[:, k]).max(), k


def test_the_exponential():
    for xi in ([0.1, -0.2, 0.3, 0.4, -0.5, 0.6], [1.0, 2.0, 3.0, 1e-9, -2e-9, 1e-9], [0.3, 0.2, 0.1, 0.0, 0.0, 0.0]):
        R, t = N.se3_exp(xi)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and abs(np.linalg.det(R) - 1.0) < 1e-15
        Ri, ti = N.se3_exp(-np.asarray(xi))
        assert np.abs(Ri @ R - np.eye(3)).max() < 1e-15 and np.abs(Ri @ t + ti).max() < 1e-15
    R, t = N.se3_exp([0.0, 0.0, 0.0, 0.0, 0.0, np.pi / 2])
    assert np.abs(R - [[0, -1, 0], [1, 0, 0], [0, 0, 1]]).max() < 1e-15
    assert np.array_equal(N.se3_exp([1.0, 2.0, 3.0, 0.0, 0.0, 0.0])[1], [1.0, 2.0, 3.0])
    # both branches, either side of their meeting point 1e-4 too, against the matrix exponential of the twist
    from scipy.linalg import expm
    for th in (1e-12, 1e-9, 0.9e-4, 1.1e-4, 1e-3, 0.3, 3.0):
        xi = np.array([1.0, -2.0, 3.0, 0.6 * th, 0.0, -0.8 * th])
        twist = np.zeros((4, 4))
        twist[:3, :3], twist[:3, 3] = N.hat(xi[3:]), xi[:3]
        assert np.abs(N.matrix(*N.se3_exp(xi)) - expm(twist)).max() < 1e-14, th


# ---- the seeded scene ------------------------------------------------------------------------------------------------------------

def test_the_loop_recovers_the_pose_of_the_seeded_scene():
    """400 points (six lines on the plane Z = 3 + 0.4 X, the outline of a box at Z = 1.6), a 60 x 80 surface whose basin, a Gaussian
    of the distance with sigma 3 px, lies under their true projections, six starts whose mean reprojection error is 1 .. 2.5 px.
    Measured with this restatement (seed 7, loss 'huber', delta 64, 50 evaluations), start -> end in px: 1.863 -> 0.164, 1.650 ->
    0.157, 1.828 -> 0.170, 1.614 -> 0.162, 2.398 -> 0.160, 1.333 -> 0.170.  The basin's floor is the nearest-point distance
    field, not the points' own, so the minimum sits 0.16 px off the truth.  The bound is the largest end plus 0.05 px."""
    sc = N.scene()
    P, S, truth = sc["points"], sc["surface"], sc["pose"]
    assert P.shape == (400, 3) and S.shape == N.SCENE_SIZE and S.dtype == np.float32 and len(sc["starts"]) == 6
    assert N.residuals(P, S, N.SCENE_INTRINSICS, *truth)[2].all()
    for R0, t0 in sc["starts"]:
        start = N.reprojection_error(P, N.SCENE_INTRINSICS, (R0, t0), truth).mean()
        R, t, c, n, evals, status = N.register(P, S, N.SCENE_INTRINSICS, R0, t0)
        end = N.reprojection_error(P, N.SCENE_INTRINSICS, (R, t), truth).mean()
        print("start %.3f end %.3f evaluations %d %s" % (start, end, evals, status))
        assert 1.0 <= start <= 2.5 and n == 400 and evals <= 50 and status in ("converged", "stalled", "max_evals")
        assert end <= N.SCENE_END_ERROR + 0.05 and end < 0.25 * start


def test_the_loop_reports_lost_and_stops_on_its_limits():
    sc = N.scene()
    P, S = sc["points"], sc["surface"]
    back = P * np.array([1.0, 1.0, -1.0])
    R, t, c, n, evals, status = N.register(back, S, N.SCENE_INTRINSICS, EYE, ZERO)
    assert (status, n, evals, c) == ("lost", 0, 1, 0.0) and np.array_equal(R, EYE) and np.array_equal(t, ZERO)
    R0, t0 = sc["starts"][0]
    assert N.register(P, S, N.SCENE_INTRINSICS, R0, t0, max_evals=3)[4:] == (3, "max_evals")
    assert N.register(P, S, N.SCENE_INTRINSICS, R0, t0, max_evals=1)[4:] == (1, "max_evals")
    out = N.register(P, S, N.SCENE_INTRINSICS, R0, t0, step_tol=1e-3)
    assert out[5] == "converged" and out[4] < 50
    flat = np.full(N.SCENE_SIZE, 7.0, dtype=np.float32)      # no gradient anywhere: A = 0, every Cholesky fails, lambda runs out
    out = N.register(P, flat, N.SCENE_INTRINSICS, *sc["pose"])
    assert out[4:] == (1, "stalled")


# ---- the public surface and the C ABI ------------------------------------------------------------------------------------------------

def test_the_prototypes_are_bound_with_their_arguments():
    from event_utils_amd import _lib
    text = _header.TEXT
    protos = _header.prototypes("evk_track_")
    assert set(protos) == ENTRIES | {"evk_track_scratch_bytes"}
    for name, (want, ret) in protos.items():
        assert ret is (ctypes.c_int if name in ENTRIES else ctypes.c_int64), name
        assert _lib.PROTOTYPES[name] == (want, ret), name
        assert hasattr(_lib.lib(), name)
    for name, value in (("EVK_TRACK_L2", 0), ("EVK_TRACK_HUBER", 1), ("EVK_TRACK_MAX_POSES", 16), ("EVK_TRACK_SUMS", 29),
                        ("EVK_TRACK_CONVERGED", 0), ("EVK_TRACK_STALLED", 1), ("EVK_TRACK_MAX_EVALS", 2), ("EVK_TRACK_LOST", 3)):
        assert getattr(_lib, name) == value and re.search(r"^#define\s+%s\s+%d\s*$" % (name, value), text, re.M)
    assert "Camera tracking (evk_track.hip)" in text


def test_public_surface():
    import inspect
    import event_utils_amd as E
    import event_utils_amd.lib.depth.tracking as alias
    from event_utils_amd import depth
    from event_utils_amd.depth import tracking
    assert alias is tracking
    for name in PUBLIC:
        assert getattr(E, name) is getattr(tracking, name) is getattr(depth, name)
    assert "(no reference module)           -> event_utils_amd.depth.tracking" in E.__doc__
    assert E.Registration._fields == ("pose", "cost", "n_valid", "evaluations", "status")
    empty = inspect.Parameter.empty

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    loop = [("max_evals", 50), ("min_points", None), ("step_tol", 1e-10)]
    assert params(E.tracking_surface) == [("Q", empty), ("blur_sigma", 1.0)]
    assert params(E.reference_points) == [("depth_map", empty), ("camera_matrix", empty)]
    assert params(E.registration_terms) == [(n, empty) for n in ("points", "surface", "camera_matrix", "poses")] + \
        [("loss", "l2"), ("delta", None)]
    assert params(E.registration_residuals) == [(n, empty) for n in ("points", "surface", "camera_matrix", "pose")]
    assert params(E.register_points) == [(n, empty) for n in ("points", "surface", "camera_matrix")] + \
        [("pose0", None), ("loss", "huber"), ("delta", None)] + loop
    assert params(E.track_poses) == [(n, empty) for n in ("points", "surfaces", "camera_matrix", "reference_pose", "pose_ts")] + \
        [("pose0", None), ("loss", "huber"), ("delta", None)] + loop
    assert (tracking.DEFAULT_DELTA, tracking.DEFAULT_MIN_POINTS, tracking.MAX_POSES) == (64.0, 12, 16)


def test_reference_points_are_the_masked_pixels_in_the_camera_frame():
    import torch
    import event_utils_amd as E
    K = np.array([[2.0, 0.0, 1.0], [0.0, 4.0, 2.0], [0.0, 0.0, 1.0]])
    depth = np.array([[1.0, 2.0, np.nan], [4.0, np.nan, 8.0]])
    mask = np.array([[True, False, False], [True, False, True]])
    dm = E.DepthMap(depth, np.zeros((2, 3), dtype=np.int32), np.zeros((2, 3), dtype=np.float32), mask)
    P = E.reference_points(dm, K)
    assert isinstance(P, np.ndarray) and P.dtype == np.float64
    assert P.tolist() == [[-0.5, -0.5, 1.0], [-2.0, -1.0, 4.0], [4.0, -2.0, 8.0]]           # ((x - cx) / fx Z, (y - cy) / fy Z, Z)
    Pt = E.reference_points(E.DepthMap(*(torch.from_numpy(a) for a in dm)), K)
    assert isinstance(Pt, np.ndarray) or Pt.tolist() == P.tolist()


def test_the_quaternion_of_a_rotation_round_trips():
    from event_utils_amd.depth import tracking
    from event_utils_amd.depth.emvs import _rotation
    rng = np.random.default_rng(5)
    qs = list(rng.normal(size=(20, 4))) + [np.array(q, dtype=np.float64) for q in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1),
                                                                                  (1, 1, 0, 0), (0, 1, 0, 1e-9))]
    for q in qs:
        q = q / np.sqrt((q * q).sum())
        got = tracking._quaternion(_rotation(q))
        assert abs((got * got).sum() - 1.0) < 1e-15 and min(np.abs(got - q).max(), np.abs(got + q).max()) < 1e-12, (q, got)


def test_arguments_are_refused_before_the_device_is_touched():
    from event_utils_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)                            # a device pointer that is never dereferenced: every call below is refused first
    einval, nan, inf = -1, float("nan"), float("inf")
    eye = np.concatenate((np.eye(3).reshape(9), np.zeros(3)))
    host = lambda a: ctypes.c_void_p(a.ctypes.data)
    keep = []

    def poses(nb=1, bad=None):
        a = np.tile(eye, max(nb, 1))
        if bad is not None:
            a[bad[0]] = bad[1]
        keep.append(a)
        return host(a)
    outs = [np.zeros(1), np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)]

    def terms(points=fake, m=100, surface=fake, h=60, w=80, fx=70.0, fy=70.0, cx=40.0, cy=30.0, pose="eye", nb=1, loss=0, delta=0.0,
              scratch=fake, sums=fake):
        return L.evk_track_terms(points, m, surface, h, w, fx, fy, cx, cy, poses(nb) if pose == "eye" else pose, nb, loss, delta, scratch,
                                 sums, None)

    def residuals(points=fake, m=100, surface=fake, h=60, w=80, fx=70.0, fy=70.0, cx=40.0, cy=30.0, pose="eye", r=fake, jac=fake, valid=fake):
        return L.evk_track_residuals(points, m, surface, h, w, fx, fy, cx, cy, poses() if pose == "eye" else pose, r, jac, valid, None)

    def register(points=fake, m=100, surface=fake, h=60, w=80, fx=70.0, fy=70.0, cx=40.0, cy=30.0, pose="eye", loss=1, delta=64.0,
                 max_evals=50, min_points=12, step_tol=1e-10, scratch=fake, cost="out", n_valid="out", evaluations="out", status="out"):
        res = [host(o) if v == "out" else v for o, v in zip(outs, (cost, n_valid, evaluations, status))]
        return L.evk_track_register(points, m, surface, h, w, fx, fy, cx, cy, poses() if pose == "eye" else pose, loss, delta, max_evals,
                                    min_points, step_tol, scratch, *res, None)
    for f in (terms, residuals, register):
        assert f(points=None) == einval and f(surface=None) == einval and f(pose=None) == einval
        assert f(m=0) == einval and f(m=-5) == einval and f(m=1 << 31) == einval
        assert f(h=1) == einval and f(w=1) == einval and f(h=0) == einval and f(w=-3) == einval and f(h=1 << 16, w=1 << 15) == einval
        for name in ("fx", "fy", "cx", "cy"):
            for bad in (nan, inf, -inf):
                assert f(**{name: bad}) == einval, (name, bad)
        assert f(fx=0.0) == einval and f(fy=0.0) == einval and f(fx=-70.0) == einval and f(fy=-1.0) == einval
        for at in (0, 8, 9, 11):
            for bad in (nan, inf):
                assert f(pose=poses(1, (at, bad))) == einval
    assert terms(nb=0) == einval and terms(nb=-1) == einval and terms(nb=17) == einval
    assert terms(nb=3, pose=poses(3, (30, nan))) == einval
    assert terms(scratch=None) == einval and terms(sums=None) == einval
    for f in (terms, register):
        assert f(loss=2) == einval and f(loss=-1) == einval
        for bad in (0.0, -1.0, nan, inf):
            assert f(loss=1, delta=bad) == einval
    for missing in ("r", "jac", "valid"):
        assert residuals(**{missing: None}) == einval
    for missing in ("scratch", "cost", "n_valid", "evaluations", "status"):
        assert register(**{missing: None}) == einval
    assert register(max_evals=0) == einval and register(min_points=0) == einval
    assert register(step_tol=-1e-3) == einval and register(step_tol=nan) == einval
    rows = lambda m: (m + 1023) // 1024
    for m, nb in ((1, 1), (1024, 1), (1025, 2), (300_000, 16)):
        assert L.evk_track_scratch_bytes(m, nb) == (rows(m) + 1) * nb * 29 * 8
    for m, nb in ((0, 1), (1 << 31, 1), (100, 0), (100, 17)):
        assert L.evk_track_scratch_bytes(m, nb) == einval


def test_python_argument_errors_come_before_any_device_work():
    """every call below is refused on its arguments alone: none of them reaches the point where a missing GPU would matter"""
    import torch
    import event_utils_amd as E
    K = np.array([[70.0, 0.0, 39.5], [0.0, 70.0, 29.5], [0.0, 0.0, 1.0]])
    P, S, T = np.ones((5, 3)), np.zeros((6, 8), dtype=np.float32), np.eye(4)
    ref = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0))
    calls = (lambda **kw: E.registration_terms(kw.get("P", P), kw.get("S", S), kw.get("K", K), kw.get("T", T)),
             lambda **kw: E.registration_residuals(kw.get("P", P), kw.get("S", S), kw.get("K", K), kw.get("T", T)),
             lambda **kw: E.register_points(kw.get("P", P), kw.get("S", S), kw.get("K", K), kw.get("T", T)),
             lambda **kw: E.track_poses(kw.get("P", P), kw["S"][None] if "S" in kw and hasattr(kw["S"], "shape") else kw.get("S", S[None]),
                                        kw.get("K", K), ref, [0.0], kw.get("T", T)))
    for f in calls:
        for bad in (np.ones((5, 2)), np.ones(3), np.ones((0, 3)), torch.ones((2, 3, 3))):
            with pytest.raises(ValueError, match="points"):
                f(P=bad)
        for bad in ([[1.0, 2.0, 3.0]], np.ones((5, 3), dtype=complex)):
            with pytest.raises(TypeError, match="points"):
                f(P=bad)
        for bad in (S.astype(np.float64), S.astype(np.uint8), torch.zeros((6, 8), dtype=torch.float16)):
            with pytest.raises(TypeError, match="float32"):
                f(S=bad)
        for bad in (np.zeros((1, 8), dtype=np.float32), np.zeros((6, 1), dtype=np.float32), np.zeros(8, dtype=np.float32)):
            with pytest.raises(ValueError, match="surface"):
                f(S=bad)
        with pytest.raises(TypeError, match="surface"):
            f(S=[[1.0, 2.0], [3.0, 4.0]])
        for bad in (np.eye(4), np.eye(2), K * np.array([[0.0, 1, 1]] * 3), K + np.array([[0, 1.0, 0]] * 3)):
            with pytest.raises(ValueError, match="camera_matrix"):
                f(K=bad)
        nanpose, skew = np.eye(4), np.eye(4)
        nanpose[0, 3], skew[3, 0] = np.nan, 1.0
        for bad in (np.eye(3), nanpose, skew, np.ones((2, 3, 4))):
            with pytest.raises(ValueError, match="pose"):
                f(T=bad)
    for f in (E.registration_terms, E.register_points, lambda *a, **kw: E.track_poses(P, S[None], K, ref, [0.0], **kw)):
        with pytest.raises(ValueError, match="loss"):
            f(P, S, K, T, loss="cauchy")
        for bad in (0.0, -2.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="delta"):
                f(P, S, K, T, loss="huber", delta=bad)
    with pytest.raises(ValueError, match="poses"):
        E.registration_terms(P, S, K, np.zeros((0, 4, 4)))
    for f in (lambda **kw: E.register_points(P, S, K, **kw), lambda **kw: E.track_poses(P, S[None], K, ref, [0.0], **kw)):
        for kw, match in ((dict(max_evals=0), "max_evals"), (dict(max_evals=2.5), "max_evals"), (dict(min_points=0), "min_points"),
                          (dict(min_points=True), "min_points"), (dict(step_tol=-1.0), "step_tol"), (dict(step_tol=float("nan")), "step_tol")):
            with pytest.raises(ValueError, match=match):
                f(**kw)
    with pytest.raises(ValueError, match="pose_ts"):
        E.track_poses(P, np.stack((S, S)), K, ref, [0.0])
    with pytest.raises(ValueError, match="pose_ts"):
        E.track_poses(P, np.stack((S, S)), K, ref, [1.0, 1.0])
    with pytest.raises(ValueError, match="pose_ts"):
        E.track_poses(P, S[None], K, ref, [])
    with pytest.raises(ValueError, match="reference_pose"):
        E.track_poses(P, S[None], K, ((0.0, 0.0), (0.0, 0.0, 0.0, 1.0)), [0.0])
    with pytest.raises(ValueError, match="reference_pose"):
        E.track_poses(P, S[None], K, ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 0.0)), [0.0])
    with pytest.raises(ValueError, match=r"\(K, H, W\)"):
        E.track_poses(P, S, K, ref, [0.0])
    Q = torch.zeros((1, 1, 6, 8), dtype=torch.uint8)
    for bad in (Q.to(torch.float32), Q.numpy().astype(np.int8)):
        with pytest.raises(TypeError, match="uint8"):
            E.tracking_surface(bad)
    with pytest.raises(TypeError, match="uint8"):
        E.tracking_surface([[1]])
    with pytest.raises(ValueError, match=r"\(K, C, H, W\)"):
        E.tracking_surface(Q[0])
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="blur_sigma"):
            E.tracking_surface(Q, bad)


def test_the_kernels_compile_without_scratch_memory(tmp_path):
    """every kernel of evk_track.hip compiles for gfx950 with no scratch memory and no spilled registers, the sum kernel within the
    128 registers DESIGN.md states (four waves per SIMD) and the 928 bytes of LDS: read from the code object's metadata"""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    from event_utils_amd.csrc import build as B
    src = os.path.join(B.HERE, "evk_track.hip")
    subprocess.run([hipcc] + list(B.CFLAGS) + ["-c", src, "-o", str(tmp_path / "track.o"), "-save-temps=obj"], check=True, cwd=B.HERE,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert asm, os.listdir(tmp_path)
    text = open(tmp_path / asm[0]).read()
    kernels = re.findall(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n"
                         r"(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    seen = {n: dict(lds=int(l), private=int(p), sspill=int(ss), vgpr=int(v), vspill=int(vs)) for l, n, p, ss, v, vs in kernels}
    for name in ("k_track_terms", "k_track_rows", "k_track_residuals"):
        assert sum(name in n for n in seen) == 1, (name, sorted(seen))
    assert len(seen) == 3
    assert not {n: v for n, v in seen.items() if v["private"] or v["sspill"] or v["vspill"]}
    terms = next(v for n, v in seen.items() if "k_track_terms" in n)
    assert terms["vgpr"] <= 128 and terms["lds"] == 4 * 29 * 8
    assert all(v["vgpr"] <= 64 for n, v in seen.items() if "k_track_terms" not in n)
    assert next(v for n, v in seen.items() if "k_track_rows" in n)["lds"] == 8 * 29 * 8
