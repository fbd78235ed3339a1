"""Event-based multi-view stereo on the device (evk_emvs.hip; definition: include/evk.h, "Event-based multi-view stereo", and
DESIGN.md section 6): depth from a moving event camera with known poses, after Rebecq et al., "EMVS: Event-based Multi-View Stereo"
(IJCV 2018).  No reference module: upstream estimates no depth.  Every event is back-projected as a ray through a disparity space
image (DSI), a (D, H, W) volume of depth planes in front of a reference view; a cell counts the rays through it; depth is read off
the local maxima of the volume.

Poses are world-from-camera: a position c and a quaternion (qx, qy, qz, qw), the order of the event-camera dataset's trajectories.
Events are taken as undistorted, camera matrices follow angular_velocity_warp (3x3, no skew, fx, fy > 0).  The input kinds are those
of the other event calls: numpy columns, device tensors, or a DeviceEvents in place of xs (the other columns None).  Polarity is
ignored.  The DSI stays on the device; its cells are integers, so a DSI is the same bits from run to run."""
import collections
import math

import numpy as np
import torch

from .. import _device as D
from .. import _lib
from ..contrast_max.warps import angular_velocity_warp
from ..events import DeviceEvents

VOTING = {"nearest": (_lib.EVK_EMVS_NEAREST, 1), "bilinear": (_lib.EVK_EMVS_BILINEAR, 256)}       # -> (mode, raw units per vote)
MAX_EVENTS = 2 ** 31
MAX_RADIUS = 16


class DSI(collections.namedtuple("DSI", ["raw", "scale", "depths"])):
    """A disparity space image: `raw` (D, H, W) int32 on the device, holding uint32 cells; `scale`, the raw units of one vote (1 for
    nearest voting, 256 for bilinear: one raw unit is 1 / scale vote); `depths`, the D plane depths, float64 numpy."""
    __slots__ = ()

    def votes(self):
        """(D, H, W) float32 raw / scale on the device"""
        return ((self.raw.to(torch.int64) & 0xFFFFFFFF).to(torch.float64) / float(self.scale)).to(torch.float32)


DepthMap = collections.namedtuple("DepthMap", ["depth", "index", "confidence", "mask"])
DepthMap.__doc__ = """A semi-dense depth map of the reference view, (H, W) device tensors: `depth` float64 depths[index], NaN where
masked out; `index` int32 plane index, -1 where masked out; `confidence` float32 votes of the best plane; `mask` bool."""


# ---- arguments -------------------------------------------------------------------------------------------------------------------

def _intrinsics(camera_matrix, what="camera_matrix"):
    """the 3x3 float64 matrix, by angular_velocity_warp's rules"""
    try:
        return angular_velocity_warp(camera_matrix).camera_matrix
    except ValueError as e:
        raise ValueError(str(e).replace("camera_matrix", what))


def _quaternions(q, what):
    q = np.asarray(q, dtype=np.float64)
    norm = np.sqrt((q * q).sum(axis=-1, keepdims=True))
    if q.shape[-1:] != (4,) or not np.all(np.isfinite(q)) or not np.all(norm > 0):
        raise ValueError("%s must be finite non-zero quaternions (qx, qy, qz, qw)" % what)
    return q / norm


def _rotation(q):
    """unit (qx, qy, qz, qw) -> the world-from-camera rotation matrix"""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _check_poses(pose_ts, positions, quaternions, reference_pose):
    pose_ts = np.asarray(pose_ts, dtype=np.float64).reshape(-1)
    positions = np.asarray(positions, dtype=np.float64)
    if len(pose_ts) < 1 or not np.all(np.isfinite(pose_ts)) or not np.all(np.diff(pose_ts) > 0):
        raise ValueError("pose_ts must be finite and strictly increasing")
    if positions.shape != (len(pose_ts), 3) or not np.all(np.isfinite(positions)):
        raise ValueError("positions must be finite with shape (%d, 3), one per pose time (got %r)" % (len(pose_ts), positions.shape))
    quaternions = _quaternions(quaternions, "quaternions")
    if quaternions.shape != (len(pose_ts), 4):
        raise ValueError("quaternions must have shape (%d, 4), one per pose time (got %r)" % (len(pose_ts), quaternions.shape))
    try:
        c_ref, q_ref = reference_pose
    except (TypeError, ValueError):
        raise ValueError("reference_pose must be (position, quaternion)")
    c_ref = np.asarray(c_ref, dtype=np.float64)
    if c_ref.shape != (3,) or not np.all(np.isfinite(c_ref)):
        raise ValueError("reference_pose's position must be 3 finite values")
    q_ref = _quaternions(q_ref, "reference_pose's quaternion")
    if q_ref.shape != (4,):
        raise ValueError("reference_pose's quaternion must be 4 values")
    return pose_ts, positions, quaternions, (c_ref, q_ref)


def _check_depths(depths):
    depths = np.ascontiguousarray(depths, dtype=np.float64).reshape(-1)
    if len(depths) < 1 or not np.all(np.isfinite(depths)) or not np.all(depths > 0):
        raise ValueError("depths must be at least one finite positive value")
    return depths


def _check_size(size, what):
    try:
        h, w = size
        ok = int(h) == h and int(w) == w and h >= 1 and w >= 1 and int(h) * int(w) <= 2 ** 31 - 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("%s must be (H, W) with H, W >= 1 and H * W < 2^31 (got %r)" % (what, size))
    return int(h), int(w)


def _check_packet_size(packet_size):
    if isinstance(packet_size, bool) or int(packet_size) != packet_size or packet_size < 1:
        raise ValueError("packet_size must be an integer >= 1 (got %r)" % (packet_size,))
    return min(int(packet_size), MAX_EVENTS)


def _float_column(c, dev):
    """a column as a contiguous float32 (when it is float32) or float64 device tensor"""
    if isinstance(c, torch.Tensor):
        c = c.reshape(-1)
        return D.to_device(c, torch.float32 if c.dtype == torch.float32 else torch.float64, dev)
    c = np.asarray(c).reshape(-1)
    if c.dtype.kind not in "biuf":
        raise ValueError("event columns must be real (got %s)" % c.dtype)
    return D.to_device(c if c.dtype == np.float32 else c.astype(np.float64), torch.float32 if c.dtype == np.float32 else torch.float64, dev)


def _event_count(xs, ys, ts):
    """N, from the arguments alone"""
    if isinstance(xs, DeviceEvents):
        return len(xs)
    if ys is None or ts is None:
        raise ValueError("xs, ys and ts are needed (or a DeviceEvents in place of xs)")
    lens = [int(np.prod(tuple(c.shape))) if hasattr(c, "shape") else len(c) for c in (xs, ys, ts)]
    if len(set(lens)) != 1:
        raise ValueError("event columns differ in length (%d, %d, %d)" % tuple(lens))
    return lens[0]


def _columns(xs, ys, ts):
    """-> x, y, t device columns (x and y of one width) and the absolute time of t's zero"""
    if isinstance(xs, DeviceEvents):
        x, y, t, _ = xs._columns()
        return x.contiguous(), y.contiguous(), t.contiguous(), xs.t_offset
    dev = D.require_gpu()
    x, y, t = (_float_column(c, dev) for c in (xs, ys, ts))
    if x.dtype != y.dtype:
        x, y = x.to(torch.float64), y.to(torch.float64)
    return x, y, t, 0.0


def _kind(col):
    return _lib.EVK_T_F32 if col.dtype == torch.float32 else _lib.EVK_T_F64


# ---- host: planes and per-packet transforms --------------------------------------------------------------------------------------

def depth_planes(z_min, z_max, n):
    """n depths uniform in inverse depth from z_min to z_max (float64 numpy), the usual sampling of a DSI."""
    z_min, z_max = float(z_min), float(z_max)
    if isinstance(n, bool) or int(n) != n or n < 1 or not (math.isfinite(z_min) and math.isfinite(z_max) and z_min > 0 and z_max > 0):
        raise ValueError("depth_planes needs finite z_min, z_max > 0 and n >= 1")
    if n == 1:
        return np.array([z_min])
    inv = 1.0 / z_min + (1.0 / z_max - 1.0 / z_min) * (np.arange(int(n), dtype=np.float64) / (int(n) - 1))
    return 1.0 / inv


def _slerp(q0, q1, f):
    """shortest-arc slerp of (n, 4) unit quaternions at the fractions f (n,); normalised lerp where they nearly coincide"""
    dot = (q0 * q1).sum(axis=1)
    q1 = np.where((dot < 0.0)[:, None], -q1, q1)
    dot = np.abs(dot)
    lerp = dot > 1.0 - 1e-12
    theta = np.arccos(np.where(lerp, 0.0, dot))             # (where lerp holds the angle is not used)
    w0 = np.where(lerp, 1.0 - f, np.sin((1.0 - f) * theta) / np.sin(theta))
    w1 = np.where(lerp, f, np.sin(f * theta) / np.sin(theta))
    q = w0[:, None] * q0 + w1[:, None] * q1
    return q / np.sqrt((q * q).sum(axis=1, keepdims=True))


def _rotations(q):
    """(n, 4) unit quaternions -> (n, 3, 3)"""
    return np.moveaxis(_rotation(q.T), -1, 0)


def packet_transforms(packet_ts, pose_ts, positions, quaternions, camera_matrix, reference_pose):
    """The packet table, (n_packets, 12) float64 numpy on the host: per packet time the row M = R_ref^T R_j K^-1 row-major (9
    values) followed by C = R_ref^T (c_j - c_ref) (3 values).  The pose (c_j, R_j) at a packet time is linear in position and the
    shortest-arc slerp in rotation between the two trajectory poses around it.  ValueError for a time outside
    [pose_ts[0], pose_ts[-1]]."""
    K = _intrinsics(camera_matrix)
    pose_ts, positions, quaternions, (c_ref, q_ref) = _check_poses(pose_ts, positions, quaternions, reference_pose)
    packet_ts = np.asarray(packet_ts, dtype=np.float64).reshape(-1)
    if not np.all((packet_ts >= pose_ts[0]) & (packet_ts <= pose_ts[-1])):          # (also NaN)
        raise ValueError("packet times must lie in [pose_ts[0], pose_ts[-1]] = [%r, %r]" % (pose_ts[0], pose_ts[-1]))
    Kinv = np.array([[1.0 / K[0, 0], 0.0, -K[0, 2] / K[0, 0]], [0.0, 1.0 / K[1, 1], -K[1, 2] / K[1, 1]], [0.0, 0.0, 1.0]])
    Rt = _rotation(q_ref).T
    n = len(packet_ts)
    if len(pose_ts) == 1:                                   # (every time equals the one pose time)
        lo = hi = np.zeros(n, dtype=np.int64)
        f = np.zeros(n)
    else:
        hi = np.clip(np.searchsorted(pose_ts, packet_ts, side="right"), 1, len(pose_ts) - 1)
        lo = hi - 1
        f = (packet_ts - pose_ts[lo]) / (pose_ts[hi] - pose_ts[lo])
    c = positions[lo] + f[:, None] * (positions[hi] - positions[lo])
    R = _rotations(_slerp(quaternions[lo], quaternions[hi], f))
    out = np.empty((n, 12), dtype=np.float64)
    out[:, :9] = ((Rt @ R) @ Kinv).reshape(n, 9)
    out[:, 9:] = (c - c_ref) @ Rt.T
    return out


def packet_times(xs, ys, ts, ps=None, packet_size=1024):
    """The time of every packet of dsi_votes, float64 numpy: packet j is events [j packet_size, min((j + 1) packet_size, N)) in
    stream order and its time is ts of event j packet_size + cnt_j // 2.  Gathered on the device, one read-back of N / packet_size
    doubles."""
    packet_size = _check_packet_size(packet_size)
    n = _event_count(xs, ys, ts)
    if n >= MAX_EVENTS:
        raise ValueError("%d events are more than one call takes (fewer than 2^31)" % n)
    if n == 0:
        return np.empty(0, dtype=np.float64)
    _, _, t, t_offset = _columns(xs, ys, ts)
    return _packet_times(t, t_offset, n, packet_size)


def _packet_times(t, t_offset, n, packet_size):
    size = min(packet_size, n)
    out = torch.empty((n + size - 1) // size, dtype=torch.float64, device=t.device)
    _lib.call("evk_emvs_packet_times", _kind(t), D.ptr(t), n, packet_size, D.ptr(out), D.stream())
    return out.cpu().numpy() + t_offset if t_offset else out.cpu().numpy()


# ---- device: votes and depth map -------------------------------------------------------------------------------------------------

def _votes(xs, ys, ts, camera_matrix, pose_ts, positions, quaternions, reference_pose, depths, sensor_size, packet_size, voting,
           reference_camera_matrix, dsi_size, chunks=0):
    # ---- everything that can be refused on the arguments alone
    if voting not in VOTING:
        raise ValueError("voting must be 'nearest' or 'bilinear' (got %r)" % (voting,))
    mode, scale = VOTING[voting]
    K = _intrinsics(camera_matrix)
    Kref = K if reference_camera_matrix is None else _intrinsics(reference_camera_matrix, "reference_camera_matrix")
    _check_poses(pose_ts, positions, quaternions, reference_pose)
    depths = _check_depths(depths)
    _check_size(sensor_size, "sensor_size")
    h, w = _check_size(sensor_size if dsi_size is None else dsi_size, "dsi_size")
    if len(depths) * h * w > 2 ** 40:
        raise ValueError("a DSI of %d x %d x %d cells is more than one call takes (2^40)" % (len(depths), h, w))
    packet_size = _check_packet_size(packet_size)
    n = _event_count(xs, ys, ts)
    if n >= MAX_EVENTS:
        raise ValueError("%d events are more than one call takes (fewer than 2^31)" % n)
    if voting == "bilinear" and n >= _lib.EVK_EMVS_BILINEAR_MAX_EVENTS:
        raise ValueError("%d events are more than bilinear voting takes (fewer than 2^24: a cell could wrap); vote in several calls "
                         "or use voting='nearest'" % n)
    # ---- the packet times, the table, the votes
    if n:
        x, y, t, t_offset = _columns(xs, ys, ts)
        dev = x.device
        # the caller's own poses, which packet_transforms checks and normalises itself: a quaternion normalised a second time moves
        # by an ulp, and the votes must be those of the table that packet_transforms returns for these arguments
        table = packet_transforms(_packet_times(t, t_offset, n, packet_size), pose_ts, positions, quaternions, K, reference_pose)
        dtable = torch.from_numpy(table).to(dev)
        rays = torch.empty((n, 2), dtype=torch.float64, device=dev)
    else:
        dev = xs.device if isinstance(xs, DeviceEvents) else D.require_gpu()
        x = y = dtable = rays = None
        table = np.empty((0, 12))
    planes = torch.from_numpy(np.stack((depths, 1.0 / depths))).to(dev)                  # the Z and rZ tables
    raw = torch.empty((len(depths), h, w), dtype=torch.int32, device=dev)
    _lib.call("evk_emvs_votes", _lib.EVK_T_F64 if x is None else _kind(x), D.ptr(x), D.ptr(y), n, packet_size, D.ptr(dtable), len(table),
              D.ptr(planes[0]), D.ptr(planes[1]), len(depths), float(Kref[0, 0]), float(Kref[1, 1]), float(Kref[0, 2]), float(Kref[1, 2]),
              h, w, mode, int(chunks), D.ptr(rays), D.ptr(raw), D.stream())
    return DSI(raw, scale, depths)


def dsi_votes(xs, ys, ts, ps, camera_matrix, pose_ts, positions, quaternions, reference_pose, depths, sensor_size, packet_size=1024,
              voting="nearest", reference_camera_matrix=None, dsi_size=None):
    """The ray counts of the events in a DSI in front of reference_pose -> DSI(raw, scale, depths).

    Events are cut into packets of packet_size in stream order; a packet takes the camera pose at the time of its middle event
    (packet_transforms on pose_ts, positions (P, 3), quaternions (P, 4); the times must lie inside the trajectory).  depths: D >= 1
    finite positive plane depths in any order (depth_planes).  The DSI is (D, H, W) with (H, W) = dsi_size, default sensor_size,
    seen through reference_camera_matrix, default camera_matrix.  Coordinates outside sensor_size are no error: the ray is
    wherever it is.

    All float64, one rounding per operation.  Per event (x, y) of packet j with row (M, C):  d_k = (M_k0 x + M_k1 y) + M_k2; the
    event is skipped unless d_2 > 0; a = d_0 / d_2, b = d_1 / d_2.  Per plane Z = depths[i]:  s = Z - C_2, skipped unless s > 0;
    u = (fx (C_0 + s a)) (1 / Z) + cx, v = (fy (C_1 + s b)) (1 / Z) + cy.
    voting='nearest' adds 1 at (floor(v + 0.5), floor(u + 0.5)) when that lies inside; scale = 1.
    voting='bilinear' adds rint(256 w) for the four bilinear weights w of (u, v), each corner on its own when it lies inside;
    scale = 256, and fewer than 2^24 events per call.
    ValueError for fewer than one depth, sizes that do not fit, 2^31 events or more, and packet times outside the trajectory."""
    return _votes(xs, ys, ts, camera_matrix, pose_ts, positions, quaternions, reference_pose, depths, sensor_size, packet_size, voting,
                  reference_camera_matrix, dsi_size)


def dsi_depth_map(dsi, filter_radius=2, threshold=5.0, median_size=3):
    """The semi-dense depth map of a DSI -> DepthMap(depth, index, confidence, mask); integer arithmetic on dsi.raw, so exact.

    conf = max_i raw[i] and the smallest i that attains it (-1 where conf == 0).  With S the sum of conf over the (2 r + 1)^2 window
    (zero outside the image) and area = (2 r + 1)^2 always, mask = conf area - S > floor(threshold scale) area: the pixel stands
    more than `threshold` votes above its box mean (EMVS's adaptive threshold).  median_size 3 or 5 replaces a masked pixel's index
    by the lower median of the indices of the masked pixels in its window, itself included; 0 leaves it."""
    if isinstance(filter_radius, bool) or int(filter_radius) != filter_radius or not 0 <= filter_radius <= MAX_RADIUS:
        raise ValueError("filter_radius must be 0 .. %d (got %r)" % (MAX_RADIUS, filter_radius))
    if median_size not in (0, 3, 5) or isinstance(median_size, bool):
        raise ValueError("median_size must be 0, 3 or 5 (got %r)" % (median_size,))
    threshold = float(threshold)
    if not (threshold >= 0.0 and math.isfinite(threshold)):
        raise ValueError("threshold must be finite and >= 0 (got %r)" % threshold)
    if not (isinstance(dsi, tuple) and len(dsi) == 3):
        raise ValueError("dsi must be a DSI(raw, scale, depths)")
    raw, scale, depths = dsi
    depths = _check_depths(depths)
    if int(scale) != scale or scale < 1:
        raise ValueError("dsi.scale must be an integer >= 1 (got %r)" % (scale,))
    if not isinstance(raw, torch.Tensor):
        raw = np.asarray(raw)
    shape = tuple(raw.shape)
    int32 = raw.dtype == torch.int32 if isinstance(raw, torch.Tensor) else raw.dtype in (np.dtype(np.int32), np.dtype(np.uint32))
    if len(shape) != 3 or shape[0] != len(depths) or not int32:
        raise ValueError("dsi.raw must be (D, H, W) int32 with D = len(dsi.depths) = %d (got %r, %s)" % (len(depths), shape, raw.dtype))
    nd = shape[0]
    h, w = _check_size(shape[1:], "dsi.raw's plane")
    thr = min(int(math.floor(threshold * int(scale))), 2 ** 45)
    dev = raw.device if isinstance(raw, torch.Tensor) and raw.is_cuda else D.require_gpu()
    raw = D.to_device(raw if isinstance(raw, torch.Tensor) else raw.view(np.int32), torch.int32, dev)
    ddepths = torch.from_numpy(depths).to(dev)
    conf, peak, index = (torch.empty((h, w), dtype=torch.int32, device=dev) for _ in range(3))
    mask = torch.empty((h, w), dtype=torch.uint8, device=dev)
    depth = torch.empty((h, w), dtype=torch.float64, device=dev)
    _lib.call("evk_emvs_depth_map", D.ptr(raw), D.ptr(ddepths), nd, h, w, int(filter_radius), thr, int(median_size), D.ptr(conf),
              D.ptr(peak), D.ptr(mask), D.ptr(index), D.ptr(depth), D.stream())
    confidence = ((conf.to(torch.int64) & 0xFFFFFFFF).to(torch.float64) / float(scale)).to(torch.float32)
    return DepthMap(depth, index, confidence, mask.to(torch.bool))


# ---- convenience -----------------------------------------------------------------------------------------------------------------

def emvs_depth_map(xs, ys, ts, ps, camera_matrix, pose_ts, positions, quaternions, reference_pose, depths, sensor_size, packet_size=1024,
                   voting="nearest", reference_camera_matrix=None, dsi_size=None, filter_radius=2, threshold=5.0, median_size=3):
    """dsi_votes followed by dsi_depth_map -> DepthMap."""
    dsi = dsi_votes(xs, ys, ts, ps, camera_matrix, pose_ts, positions, quaternions, reference_pose, depths, sensor_size, packet_size,
                    voting, reference_camera_matrix, dsi_size)
    return dsi_depth_map(dsi, filter_radius, threshold, median_size)


def depth_to_points(depth_map, reference_camera_matrix, reference_pose):
    """(M, 3) float64 world points of the masked pixels of a DepthMap, in row-major pixel order: X = c_ref + R_ref (Z K^-1 (x, y, 1)).
    A device tensor when the map is on the device, else numpy."""
    K = _intrinsics(reference_camera_matrix, "reference_camera_matrix")
    try:
        c_ref, q_ref = reference_pose
    except (TypeError, ValueError):
        raise ValueError("reference_pose must be (position, quaternion)")
    c_ref = np.asarray(c_ref, dtype=np.float64).reshape(3)
    R = _rotation(_quaternions(np.asarray(q_ref, dtype=np.float64).reshape(4), "reference_pose's quaternion"))
    depth, mask = depth_map.depth, depth_map.mask
    on_device = isinstance(depth, torch.Tensor)
    if not on_device:
        depth, mask = torch.from_numpy(np.asarray(depth, dtype=np.float64)), torch.from_numpy(np.asarray(mask, dtype=bool))
    ys, xs = torch.nonzero(mask, as_tuple=True)
    z = depth[ys, xs]
    cam = torch.stack(((xs.to(torch.float64) - K[0, 2]) / K[0, 0] * z, (ys.to(torch.float64) - K[1, 2]) / K[1, 1] * z, z), dim=1)
    Rt = torch.from_numpy(np.ascontiguousarray(R.T)).to(cam.device)
    points = cam @ Rt + torch.from_numpy(c_ref).to(cam.device)
    return points if on_device else points.numpy()
