"""Camera tracking on the device (evk_track.hip; definition: include/evk.h, "Camera tracking", and DESIGN.md section 6): the 6-DoF pose
under which the semi-dense 3-D points of a reference view project onto the recent edges of a time surface, the tracking step of ESVO
(Zhou et al., "Event-based Stereo Visual Odometry", T-RO 2021, section V).  No reference module: upstream estimates no pose.

It closes the loop of the depth package: stereo_disparity -> disparity_depth_map -> reference_points -> track_poses -> dsi_votes.
A pose here is current-from-reference, a 4 x 4 matrix (R t; 0 1): X' = R P + t.  The surface is low where events are recent
(tracking_surface), so the points of a well-registered view sit in its valleys and the loop minimises the sum of the squared, or
Huber-weighted, surface values under the points.  Points and surfaces may be numpy or device tensors; the per-point values and the
sums stay on the device, the small pose results are numpy."""
import collections
import math

import numpy as np
import torch

from .. import _device as D
from .. import _lib
from .._checks import check_array, check_int
from ..contrast_max.objectives import gaussian_filter_device
from .emvs import _check_poses, _intrinsics, _rotation, depth_to_points

MAX_POSES = _lib.EVK_TRACK_MAX_POSES
LOSSES = {"l2": _lib.EVK_TRACK_L2, "huber": _lib.EVK_TRACK_HUBER}
STATUS = {_lib.EVK_TRACK_CONVERGED: "converged", _lib.EVK_TRACK_STALLED: "stalled", _lib.EVK_TRACK_MAX_EVALS: "max_evals",
          _lib.EVK_TRACK_LOST: "lost"}
DEFAULT_DELTA = 64.0            # a quarter of the surface's range: a point further than that from an edge pulls linearly
DEFAULT_MIN_POINTS = 12         # twice the six unknowns

Registration = collections.namedtuple("Registration", ["pose", "cost", "n_valid", "evaluations", "status"])
Registration.__doc__ = """The result of register_points: `pose` the (4, 4) float64 numpy current-from-reference transform; `cost` the sum
of rho over the `n_valid` points that project inside the surface at that pose; `evaluations` the evaluations used; `status` one of
"converged" (a step below step_tol was accepted), "stalled" (the damping passed 1e6: no better pose nearby), "max_evals", "lost"
(fewer than min_points valid points at the start; the pose is pose0)."""

_TRIU = None


# ---- arguments -------------------------------------------------------------------------------------------------------------------

def _check_loss(loss, delta):
    """-> (the loss's code, delta)"""
    if loss not in LOSSES:
        raise ValueError("loss must be 'l2' or 'huber' (got %r)" % (loss,))
    if loss == "l2":
        return LOSSES[loss], 0.0
    delta = DEFAULT_DELTA if delta is None else float(delta)
    if not (delta > 0.0 and math.isfinite(delta)):
        raise ValueError("delta must be finite and > 0 (got %r)" % delta)
    return LOSSES[loss], delta


def _check_points(points):
    if not isinstance(points, (torch.Tensor, np.ndarray)):
        raise TypeError("points must be an (M, 3) tensor or array (got %s)" % type(points).__name__)
    shape = tuple(int(v) for v in points.shape)
    if len(shape) != 2 or shape[1] != 3 or not 1 <= shape[0] <= 2 ** 31 - 1:
        raise ValueError("points must be (M, 3) with 1 <= M < 2^31 (got %r)" % (shape,))
    if not (points.is_floating_point() if isinstance(points, torch.Tensor) else points.dtype.kind in "biuf"):
        raise TypeError("points must be real (got %s)" % points.dtype)
    return shape[0]


def _check_surface(surface, what="surface", dims=2):
    shape = check_array(surface, what, torch.float32, "tracking_surface")
    if len(shape) != dims or min(shape) < 1 or shape[-2] < 2 or shape[-1] < 2 or shape[-2] * shape[-1] > 2 ** 31 - 1:
        raise ValueError("%s must be %s with H, W >= 2 and H * W < 2^31 (got %r)" % (what, "(H, W)" if dims == 2 else "(K, H, W)", shape))
    return shape


def _check_pose(pose, what):
    """a (4, 4) current-from-reference transform -> its 12 doubles (R row-major, t)"""
    T = np.asarray(pose.detach().cpu().numpy() if isinstance(pose, torch.Tensor) else pose, dtype=np.float64)
    if T.shape != (4, 4) or not np.all(np.isfinite(T)) or not np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0]):
        raise ValueError("%s must be a finite (4, 4) transform with the last row (0, 0, 0, 1)" % what)
    return np.concatenate((T[:3, :3].reshape(9), T[:3, 3]))


def _check_poses_matrix(poses):
    """(B, 4, 4) or (4, 4) -> (B, 12) float64"""
    T = np.asarray(poses.detach().cpu().numpy() if isinstance(poses, torch.Tensor) else poses, dtype=np.float64)
    if T.ndim == 2:
        T = T[None]
    if T.ndim != 3 or T.shape[1:] != (4, 4) or len(T) < 1:
        raise ValueError("poses must be (B, 4, 4) or (4, 4) with B >= 1 (got %r)" % (T.shape,))
    return np.ascontiguousarray(np.stack([_check_pose(t, "every pose of poses") for t in T]))


def _matrix(p12):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = p12[:9].reshape(3, 3), p12[9:]
    return T


def _check_loop(max_evals, min_points, step_tol):
    max_evals = check_int(max_evals, "max_evals", 1, 2 ** 31 - 1)
    min_points = check_int(DEFAULT_MIN_POINTS if min_points is None else min_points, "min_points", 1, 2 ** 31 - 1)
    step_tol = float(step_tol)
    if not step_tol >= 0.0:                    # (also NaN)
        raise ValueError("step_tol must be >= 0 (got %r)" % step_tol)
    return max_evals, min_points, step_tol


def _resident(points, surface):
    dev = D.device_of(points, surface)
    return D.resident(points, dev, torch.float64), D.resident(surface, dev), dev


def _scratch(m, nb, dev):
    return torch.empty(int(_lib.lib().evk_track_scratch_bytes(m, nb)), dtype=torch.uint8, device=dev)


# ---- surfaces and points ---------------------------------------------------------------------------------------------------------

def tracking_surface(Q, blur_sigma=1.0):
    """The surfaces tracking runs on, (K, H, W) float32 on the device: 255 - max_c Q of a quantised_time_surfaces result Q
    (K, C, H, W) uint8, so 0 at an event of this instant and 255 where nothing happened within tau, each slice through
    scipy.ndimage.gaussian_filter(mode='reflect') in float32 (gaussian_filter_device).  blur_sigma None or 0: no blur."""
    shape = check_array(Q, "Q", torch.uint8, "quantised_time_surfaces")
    if len(shape) != 4 or min(shape) < 1:
        raise ValueError("Q must be (K, C, H, W) with K, C, H, W >= 1 (got %r)" % (shape,))
    sigma = 0.0 if blur_sigma is None else float(blur_sigma)
    if not (sigma >= 0.0 and math.isfinite(sigma)):
        raise ValueError("blur_sigma must be finite and >= 0, or None (got %r)" % (blur_sigma,))
    Q = D.resident(Q, D.device_of(Q))
    S = (255.0 - Q.amax(dim=1).to(torch.float32)).contiguous()
    if sigma > 0.0:
        S = torch.stack([gaussian_filter_device(S[k], sigma) for k in range(shape[0])])
    return S


def reference_points(depth_map, camera_matrix):
    """(M, 3) float64 points of the masked pixels of a DepthMap in the camera frame of its own view, in row-major pixel order:
    depth_to_points with the identity pose.  A device tensor when the map is on the device, else numpy."""
    return depth_to_points(depth_map, camera_matrix, ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0, 1.0)))


# ---- evaluations -----------------------------------------------------------------------------------------------------------------

def registration_terms(points, surface, camera_matrix, poses, loss="l2", delta=None):
    """The normal equations of the registration at B poses in one launch -> A (B, 6, 6), g (B, 6), c (B,) float64 and n (B,) int64
    on the device: over the points that are valid at the pose, A = sum w J^T J, g = sum w J^T r, c = sum rho and their count
    (registration_residuals; loss 'l2': w = 1, rho = r^2; 'huber': w = delta / |r| and rho = delta (2 |r| - delta) beyond delta).
    poses: (B, 4, 4) or (4, 4), current-from-reference.  The sums follow one fixed tree that depends on M only: a result repeats
    bit for bit, and row b of a batch is the bits of that pose alone.  The gradient of c is 2 g."""
    global _TRIU
    K = _intrinsics(camera_matrix)
    m = _check_points(points)
    h, w = _check_surface(surface)
    p12 = _check_poses_matrix(poses)
    code, delta = _check_loss(loss, delta)
    P, S, dev = _resident(points, surface)
    nb = len(p12)
    sums = torch.empty((nb, _lib.EVK_TRACK_SUMS), dtype=torch.float64, device=dev)
    for b0 in range(0, nb, MAX_POSES):                                  # (a launch takes EVK_TRACK_MAX_POSES poses)
        part = np.ascontiguousarray(p12[b0:b0 + MAX_POSES])
        _lib.call("evk_track_terms", D.ptr(P), m, D.ptr(S), h, w, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]),
                  D.host_ptr(part), len(part), code, delta, D.ptr(_scratch(m, len(part), dev)), D.ptr(sums[b0:b0 + MAX_POSES]), D.stream())
    if _TRIU is None:
        idx = np.zeros((6, 6), dtype=np.int64)
        idx[np.triu_indices(6)] = np.arange(21)
        _TRIU = torch.from_numpy(np.maximum(idx, idx.T).reshape(-1))
    A = sums[:, :21].index_select(1, _TRIU.to(dev)).reshape(nb, 6, 6)
    return A, sums[:, 21:27], sums[:, 27], sums[:, 28].to(torch.int64)


def registration_residuals(points, surface, camera_matrix, pose):
    """The per-point values at one pose -> r (M,), J (M, 6) float64 and valid (M,) bool on the device; r and J are NaN where the
    point is not valid.  All float64, one rounding per operation.  With pose = (R, t), (fx, fy, cx, cy) of camera_matrix and the
    surface S (H, W) float32:  X' = R P + t, u = fx (X' / Z') + cx, v = fy (Y' / Z') + cy; valid iff every value is finite, Z' > 0,
    0 <= u < W - 1 and 0 <= v < H - 1; r is the bilinear value of S at (u, v) and (gx, gy) the exact derivative of that
    interpolant; j3 = (gx fx / Z', gy fy / Z', -(gx fx X' + gy fy Y') / Z'^2) and J = (j3, X' x j3), the derivative of r for a left
    increment pose <- exp(xi^) pose, xi = (upsilon, omega)."""
    K = _intrinsics(camera_matrix)
    m = _check_points(points)
    h, w = _check_surface(surface)
    p12 = np.ascontiguousarray(_check_pose(pose, "pose"))
    P, S, dev = _resident(points, surface)
    r = torch.empty(m, dtype=torch.float64, device=dev)
    J = torch.empty((m, 6), dtype=torch.float64, device=dev)
    valid = torch.empty(m, dtype=torch.uint8, device=dev)
    _lib.call("evk_track_residuals", D.ptr(P), m, D.ptr(S), h, w, float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]),
              D.host_ptr(p12), D.ptr(r), D.ptr(J), D.ptr(valid), D.stream())
    return r, J, valid.to(torch.bool)


# ---- the loop --------------------------------------------------------------------------------------------------------------------

def _register(P, S, K, p12, code, delta, max_evals, min_points, step_tol, scratch):
    m, (h, w) = int(P.shape[0]), S.shape
    pose = np.ascontiguousarray(p12, dtype=np.float64).copy()
    cost, n, out = np.zeros(1, dtype=np.float64), np.zeros(1, dtype=np.int64), np.zeros(2, dtype=np.int32)
    _lib.call("evk_track_register", D.ptr(P), m, D.ptr(S), int(h), int(w), float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]),
              D.host_ptr(pose), code, delta, max_evals, min_points, step_tol, D.ptr(scratch), D.host_ptr(cost), D.host_ptr(n),
              D.host_ptr(out[0:1]), D.host_ptr(out[1:2]), D.stream())
    return Registration(_matrix(pose), float(cost[0]), int(n[0]), int(out[0]), STATUS[int(out[1])])


def register_points(points, surface, camera_matrix, pose0=None, loss="huber", delta=None, max_evals=50, min_points=None, step_tol=1e-10):
    """The pose that registers the points to the surface, from pose0 (default: the identity) -> Registration(pose, cost, n_valid,
    evaluations, status).  Levenberg-Marquardt in the library, one read-back of 29 doubles per evaluation: with (A, g, c, n) of
    registration_terms, solve (A + lambda diag A) d = -g by Cholesky, lambda from 1e-3; the candidate exp(d^) pose is accepted iff
    it keeps n' >= min_points valid points and c' / n' < c / n; lambda <- max(lambda / 10, 1e-9) when accepted, 10 lambda when not.
    It ends when an accepted step is shorter than step_tol, lambda passes 1e6, or max_evals evaluations are used.
    delta: the Huber threshold in surface units (default 64); min_points: default 12."""
    K = _intrinsics(camera_matrix)
    _check_points(points)
    _check_surface(surface)
    p12 = _check_pose(np.eye(4) if pose0 is None else pose0, "pose0")
    code, delta = _check_loss(loss, delta)
    max_evals, min_points, step_tol = _check_loop(max_evals, min_points, step_tol)
    P, S, dev = _resident(points, surface)
    return _register(P, S, K, p12, code, delta, max_evals, min_points, step_tol, _scratch(int(P.shape[0]), 1, dev))


def _quaternion(R):
    """a rotation matrix -> the unit (qx, qy, qz, qw), by the largest of the four candidates"""
    t = np.array([R[0, 0], R[1, 1], R[2, 2]])
    c = np.array([1.0 + t[0] - t[1] - t[2], 1.0 - t[0] + t[1] - t[2], 1.0 - t[0] - t[1] + t[2], 1.0 + t.sum()])
    i = int(np.argmax(c))
    if i == 3:
        q = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1], c[3]])
    elif i == 0:
        q = np.array([c[0], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0], R[2, 1] - R[1, 2]])
    elif i == 1:
        q = np.array([R[0, 1] + R[1, 0], c[1], R[1, 2] + R[2, 1], R[0, 2] - R[2, 0]])
    else:
        q = np.array([R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], c[2], R[1, 0] - R[0, 1]])
    return q / np.sqrt((q * q).sum())


def track_poses(points, surfaces, camera_matrix, reference_pose, pose_ts, pose0=None, loss="huber", delta=None, max_evals=50,
                min_points=None, step_tol=1e-10):
    """The trajectory of the camera over the K slices of surfaces (K, H, W) -> positions (K, 3), quaternions (K, 4) float64 numpy:
    one register_points per slice, each from the result before it (the first from pose0, default the identity).  The results are
    world-from-camera, (qx, qy, qz, qw), normalised and with a non-negative dot with the one before (the first with the
    reference's): with reference_pose = (c_ref, q_ref), world-from-reference, and a slice's pose (R, t), R_wc = R_ref R^T and
    c = c_ref - R_wc t.  Together with pose_ts (K strictly increasing times, one per slice) they are the trajectory dsi_votes and
    packet_transforms take.  RuntimeError when a slice ends "lost"."""
    K = _intrinsics(camera_matrix)
    _check_points(points)
    k, h, w = _check_surface(surfaces, "surfaces", 3)
    if np.size(pose_ts) != k:
        raise ValueError("pose_ts must hold one time per slice of surfaces (got %d for %d)" % (np.size(pose_ts), k))
    # (the times and the reference pose by the rules of dsi_votes; the trajectory itself is what this call returns)
    _, _, _, (c_ref, q_ref) = _check_poses(pose_ts, np.zeros((k, 3)), np.tile([0.0, 0.0, 0.0, 1.0], (k, 1)), reference_pose)
    p12 = _check_pose(np.eye(4) if pose0 is None else pose0, "pose0")
    code, delta = _check_loss(loss, delta)
    max_evals, min_points, step_tol = _check_loop(max_evals, min_points, step_tol)
    P, S, dev = _resident(points, surfaces)
    scratch = _scratch(int(P.shape[0]), 1, dev)
    R_ref = _rotation(q_ref)
    positions, quaternions = np.empty((k, 3)), np.empty((k, 4))
    before = q_ref
    for i in range(k):
        reg = _register(P, S[i], K, p12, code, delta, max_evals, min_points, step_tol, scratch)
        if reg.status == "lost":
            raise RuntimeError("tracking lost at slice %d: %d of %d points project inside the surface" % (i, reg.n_valid, P.shape[0]))
        p12 = np.concatenate((reg.pose[:3, :3].reshape(9), reg.pose[:3, 3]))
        R_wc = R_ref @ reg.pose[:3, :3].T
        q = _quaternion(R_wc)
        before = quaternions[i] = -q if (q * before).sum() < 0.0 else q
        positions[i] = c_ref - R_wc @ reg.pose[:3, 3]
    return positions, quaternions
