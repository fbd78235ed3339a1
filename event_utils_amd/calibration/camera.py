"""Camera calibration on the device (evk_camera.hip; definition: include/evk.h, "Camera calibration", and DESIGN.md section 6): lens
undistortion and rectification of events and images, what the depth package and the rotational warps take as done.  No reference
module: upstream has nothing on the subject.

A camera is K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (no skew, the convention of angular_velocity_warp) and a lens model: "none",
"radtan" (k1, k2, p1, p2[, k3]: DAVIS240C, DSEC) or "equidistant" (k1 .. k4, Kannala-Brandt as Kalibr and OpenCV's fisheye model
define it: MVSEC).  Both usual practices are here.  Events go through a per-pixel look-up table, the forward map (raw pixel ->
rectified coordinate; rectify_events): the practice of EMVS and contrast maximisation.  Images and time surfaces are resampled through
the inverse map (rectified pixel -> raw coordinate; remap_images): the practice of ESVO.  Both maps are built once on the device
(rectification_maps) and stay there; stereo_rectify gives the two rotations and the shared new_K of a calibrated pair.

All arithmetic is float64 with one rounding per operation in a stated order: "none" and "radtan" results are the same bits as the
numpy restatement of the tests; "equidistant" calls atan and tan and agrees within 1e-9 px."""
import collections
import math

import numpy as np
import torch

from .. import _device as D
from .. import _lib
from .._checks import check_int
from ..util import event_util as U

MODELS = {"none": _lib.EVK_CAMERA_NONE, "radtan": _lib.EVK_CAMERA_RADTAN, "equidistant": _lib.EVK_CAMERA_EQUIDISTANT}
_COEFFICIENTS = {"none": (0,), "radtan": (4, 5), "equidistant": (4,)}
_MODES = {"nearest": _lib.EVK_CAMERA_NEAREST, "subpixel": _lib.EVK_CAMERA_SUBPIXEL}
_INTERPOLATIONS = {"nearest": _lib.EVK_CAMERA_NEAREST, "bilinear": _lib.EVK_CAMERA_BILINEAR}
_PLANES = {torch.uint8: _lib.EVK_CAMERA_U8, torch.float32: _lib.EVK_CAMERA_F32, torch.float64: _lib.EVK_CAMERA_F64}
_T_OF_KIND = {v: k for k, v in U._KIND.items()}
DEFAULT_ITERATIONS, DEFAULT_TOLERANCE = 20, 1e-6


# ---- arguments -------------------------------------------------------------------------------------------------------------------

def _matrix(K, what):
    """a camera matrix without skew -> (the 3 x 3 float64 array, (fx, fy, cx, cy))"""
    K = np.asarray(K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else K, dtype=np.float64)
    if K.shape != (3, 3) or not np.isfinite(K).all():
        raise ValueError("%s must be a finite 3 x 3 matrix (got shape %r)" % (what, K.shape))
    if K[0, 1] != 0.0:
        raise ValueError("%s must have no skew (K[0, 1] = %r)" % (what, K[0, 1]))
    if K[1, 0] != 0.0 or K[2, 0] != 0.0 or K[2, 1] != 0.0 or K[2, 2] != 1.0 or not (K[0, 0] > 0.0 and K[1, 1] > 0.0):
        raise ValueError("%s must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] with fx, fy > 0" % what)
    return K, (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def _rotation(R):
    if R is None:
        return np.eye(3)
    R = np.asarray(R.detach().cpu().numpy() if isinstance(R, torch.Tensor) else R, dtype=np.float64)
    if R.shape != (3, 3) or not np.isfinite(R).all():
        raise ValueError("R must be a finite 3 x 3 rotation (got shape %r)" % (R.shape,))
    if np.abs(R @ R.T - np.eye(3)).max() > 1e-6 or np.linalg.det(R) < 0.0:
        raise ValueError("R must be a rotation: R R^T = 1 and det R = 1")
    return R


def _size(size, what):
    try:
        h, w = size
    except (TypeError, ValueError):
        raise ValueError("%s must be (H, W) (got %r)" % (what, size))
    h, w = check_int(h, what + "[0]", 1, 2 ** 31 - 1), check_int(w, what + "[1]", 1, 2 ** 31 - 1)
    if h * w > 2 ** 31 - 1:
        raise ValueError("%s must hold fewer than 2^31 pixels (got %r)" % (what, (h, w)))
    return h, w


def _solver(iterations, tolerance):
    iterations = check_int(iterations, "iterations", 1, 2 ** 31 - 1)
    tolerance = float(tolerance)
    if not (tolerance >= 0.0 and math.isfinite(tolerance)):
        raise ValueError("tolerance must be finite and >= 0 pixels (got %r)" % tolerance)
    return iterations, tolerance


class CameraModel:
    """One calibrated camera: K (3 x 3, no skew), the lens model and its coefficients, and the sensor's size (H, W)."""

    def __init__(self, K, distortion=None, model="none", sensor_size=None):
        if model not in MODELS:
            raise ValueError("model must be one of 'none', 'radtan', 'equidistant' (got %r)" % (model,))
        self.K, self.intrinsics = _matrix(K, "K")
        d = np.zeros(0) if distortion is None else np.asarray(distortion, dtype=np.float64).reshape(-1)
        if len(d) not in _COEFFICIENTS[model] or not np.isfinite(d).all():
            raise ValueError("model %r takes %s finite distortion coefficients (got %d)"
                             % (model, " or ".join(str(c) for c in _COEFFICIENTS[model]), len(d)))
        if sensor_size is None:
            raise ValueError("sensor_size must be (H, W)")
        self.model, self.sensor_size = model, _size(sensor_size, "sensor_size")
        self.distortion = d
        self.coefficients = np.zeros(5)
        self.coefficients[:len(d)] = d

    def __repr__(self):
        return "CameraModel(K=%r, distortion=%r, model=%r, sensor_size=%r)" % (self.K.tolist(), self.distortion.tolist(), self.model,
                                                                                self.sensor_size)


class RectificationMaps(collections.namedtuple("RectificationMaps", ["forward", "forward_valid", "inverse", "inverse_valid", "new_K",
                                                                       "out_size"])):
    """The two look-up tables of one camera, device tensors: `forward` (2, H, W) float64, the rectified (u, v) of every raw pixel,
    NaN where `forward_valid` (H, W) bool is False; `inverse` (2, H', W') float64, the raw (x, y) of every rectified pixel, and
    `inverse_valid`; `new_K` (3 x 3 numpy) and `out_size` (H', W') of the rectified view.  rectification_maps builds them;
    from_tensors takes maps made elsewhere."""
    __slots__ = ()

    @classmethod
    def from_tensors(cls, cam, forward, inverse, forward_valid=None, inverse_valid=None, new_K=None):
        """Maps from another calibration tool, numpy or torch: forward (2, H, W) of cam's sensor, inverse (2, H', W'), which sets
        out_size.  A flag array left out counts every entry that is not NaN."""
        if not isinstance(cam, CameraModel):
            raise TypeError("cam must be a CameraModel")
        for m, valid, what in ((forward, forward_valid, "forward"), (inverse, inverse_valid, "inverse")):
            _check_map(m, valid, what)
        if tuple(forward.shape[1:]) != cam.sensor_size:
            raise ValueError("the forward map must have the camera's size %r (got %r)" % (cam.sensor_size, tuple(forward.shape[1:])))
        new_K = cam.K if new_K is None else _matrix(new_K, "new_K")[0]
        dev = D.device_of(forward, inverse)
        fwd, fv = _resident_map(forward, forward_valid, dev)
        inv, iv = _resident_map(inverse, inverse_valid, dev)
        return cls(fwd, fv, inv, iv, new_K, tuple(int(s) for s in inv.shape[1:]))


def _check_map(m, valid, what):
    if not isinstance(m, (torch.Tensor, np.ndarray)):
        raise TypeError("the %s map must be a float64 tensor or array (got %s)" % (what, type(m).__name__))
    if m.dtype not in (torch.float64, np.dtype(np.float64)):
        raise TypeError("the %s map must be float64 (got %s)" % (what, m.dtype))
    if len(m.shape) != 3 or m.shape[0] != 2:
        raise ValueError("the %s map must be (2, H, W) (got %r)" % (what, tuple(m.shape)))
    if valid is not None:
        if not isinstance(valid, (torch.Tensor, np.ndarray)):
            raise TypeError("%s_valid must be a bool tensor or array" % what)
        if tuple(valid.shape) != tuple(m.shape[1:]):
            raise ValueError("%s_valid must be %r (got %r)" % (what, tuple(m.shape[1:]), tuple(valid.shape)))


def _resident_map(m, valid, dev):
    m = D.resident(m, dev)
    return m, ((m[0] == m[0]) & (m[1] == m[1])) if valid is None else D.resident(valid, dev, torch.bool)


def _maps(maps, which):
    """the checked (map, flags, (h, w)) of a RectificationMaps for a consumer"""
    if not isinstance(maps, RectificationMaps):
        raise TypeError("maps must be a RectificationMaps (rectification_maps, RectificationMaps.from_tensors)")
    m, v = (maps.forward, maps.forward_valid) if which == "forward" else (maps.inverse, maps.inverse_valid)
    for t, dt, what in ((m, torch.float64, which), (v, torch.bool, which + "_valid")):
        if not isinstance(t, torch.Tensor) or t.dtype != dt:
            raise TypeError("maps.%s must be a %s tensor" % (what, str(dt).replace("torch.", "")))
    if m.dim() != 3 or m.shape[0] != 2 or tuple(v.shape) != tuple(m.shape[1:]) or m.shape[1] * m.shape[2] > 2 ** 31 - 1:
        raise ValueError("maps.%s must be (2, H, W) with flags (H, W) and H W < 2^31 (got %r and %r)" % (which, tuple(m.shape), tuple(v.shape)))
    return m, v, (int(m.shape[1]), int(m.shape[2]))


# ---- points --------------------------------------------------------------------------------------------------------------------------

def _points_call(cam, direction, points, n, grid, R, new_K4, iterations, tolerance, dev):
    """evk_camera_points -> (out (2, n) float64, valid (n,) bool) on dev.  points: (n, 2) device float64, or None: the pixels of `grid`"""
    out = torch.empty((2, n), dtype=torch.float64, device=dev)
    valid = torch.empty(n, dtype=torch.bool, device=dev)
    if n == 0:
        return out, valid
    M = R if direction == _lib.EVK_CAMERA_FORWARD else R.T
    params = np.ascontiguousarray(np.concatenate((cam.intrinsics, cam.coefficients, M.reshape(9), new_K4)), dtype=np.float64)
    _lib.call("evk_camera_points", MODELS[cam.model], direction, D.ptr(points), n, grid[0], grid[1], D.host_ptr(params), iterations,
              tolerance, D.ptr(out), D.ptr(valid), D.stream())
    return out, valid


def _points_in(cam, points):
    if not isinstance(cam, CameraModel):
        raise TypeError("cam must be a CameraModel")
    if not isinstance(points, (torch.Tensor, np.ndarray)):
        raise TypeError("points must be an (N, 2) tensor or array (got %s)" % type(points).__name__)
    if (points.is_complex() or points.dtype == torch.bool) if isinstance(points, torch.Tensor) else points.dtype.kind not in "fiu":
        raise TypeError("points must hold real numbers (got %s)" % points.dtype)
    if len(points.shape) != 2 or points.shape[1] != 2:
        raise ValueError("points must be (N, 2) pixel coordinates (got %r)" % (tuple(points.shape),))
    return isinstance(points, torch.Tensor)


def _points_out(out, valid, on_device, return_valid):
    pts = out.t().contiguous()
    if not on_device:
        pts, valid = pts.cpu().numpy(), valid.cpu().numpy()
    return (pts, valid) if return_valid else pts


def distort_points(cam, points):
    """Ideal (undistorted) pixel coordinates (N, 2) -> where the lens puts them on the raw sensor, (N, 2) float64: back through K,
    distort, through K again.  NaN where the result is not finite.  numpy in, numpy out; a device tensor in, a device tensor out."""
    on_device = _points_in(cam, points)
    dev = D.device_of(points)
    pts = D.to_device(points, torch.float64, dev)
    out, valid = _points_call(cam, _lib.EVK_CAMERA_INVERSE, pts, int(pts.shape[0]), (0, 0), np.eye(3), cam.intrinsics, 1, 0.0, dev)
    return _points_out(out, valid, on_device, False)


def undistort_points(cam, points, R=None, new_K=None, iterations=DEFAULT_ITERATIONS, tolerance=DEFAULT_TOLERANCE, return_valid=False):
    """Raw pixel coordinates (N, 2) -> rectified ones, (N, 2) float64: n = undistort((x - cx) / fx, (y - cy) / fy), X = R (n, 1),
    u = fx' X_x / X_z + cx' (R defaults to the identity, new_K to K).  The undistortion takes exactly `iterations` steps (radtan:
    OpenCV's fixed point; equidistant: Newton) and a point is valid iff the result is finite, distorting it again lands within
    `tolerance` pixels of the input in both coordinates, and X_z > 0: the fixed point diverges in the corners of a strongly
    distorted sensor, and such a point is NaN, not a wrong number.  return_valid: also the (N,) bool flags."""
    on_device = _points_in(cam, points)
    R = _rotation(R)
    new_K4 = cam.intrinsics if new_K is None else _matrix(new_K, "new_K")[1]
    iterations, tolerance = _solver(iterations, tolerance)
    dev = D.device_of(points)
    pts = D.to_device(points, torch.float64, dev)
    out, valid = _points_call(cam, _lib.EVK_CAMERA_FORWARD, pts, int(pts.shape[0]), (0, 0), R, new_K4, iterations, tolerance, dev)
    return _points_out(out, valid, on_device, return_valid)


def rectification_maps(cam, R=None, new_K=None, out_size=None, iterations=DEFAULT_ITERATIONS, tolerance=DEFAULT_TOLERANCE):
    """Both maps of one camera, built on the device and resident there -> RectificationMaps.  forward: undistort_points of every
    pixel of the sensor.  inverse, for every pixel (u, v) of the out_size (default: the sensor's) view: X = R^T ((u - cx') / fx',
    (v - cy') / fy', 1), not valid if X_z <= 0, then distort(X_x / X_z, X_y / X_z) through K; no iteration."""
    if not isinstance(cam, CameraModel):
        raise TypeError("cam must be a CameraModel")
    R = _rotation(R)
    new_K, new_K4 = (cam.K, cam.intrinsics) if new_K is None else _matrix(new_K, "new_K")
    out_size = cam.sensor_size if out_size is None else _size(out_size, "out_size")
    iterations, tolerance = _solver(iterations, tolerance)
    dev = D.require_gpu()
    (h, w), (oh, ow) = cam.sensor_size, out_size
    fwd, fv = _points_call(cam, _lib.EVK_CAMERA_FORWARD, None, h * w, (h, w), R, new_K4, iterations, tolerance, dev)
    inv, iv = _points_call(cam, _lib.EVK_CAMERA_INVERSE, None, oh * ow, (oh, ow), R, new_K4, 1, 0.0, dev)
    return RectificationMaps(fwd.view(2, h, w), fv.view(h, w), inv.view(2, oh, ow), iv.view(oh, ow), new_K.copy(), out_size)


# ---- events ------------------------------------------------------------------------------------------------------------------------

def rectify_events(xs, ys, ts, ps, maps, mode="nearest", return_index=False):
    """Events of the raw sensor -> events of the rectified view, through maps.forward; in stream order, in the kind they came:
    numpy columns, device tensors, or a DeviceEvents in place of xs (the other columns None).  ts and ps may be None.

    mode "nearest": the entry of the event's pixel rounded half to even; the event is kept iff the entry is valid and the rounded
    pixel lies inside maps.out_size; the new coordinates have the dtype of the old ones.  mode "subpixel": the float64 entry as it
    is (float32 columns for a float32 DeviceEvents), kept iff it is valid and inside [0, W' - 1] x [0, H' - 1]: for the bilinear
    votes of dsi_votes and the warps.  A coordinate that is no integer, is NaN or lies off the raw sensor raises ValueError (under
    EVK_ERRORS=deferred such events are dropped without a report).  return_index: also the int64 stream indices of the kept events."""
    if mode not in _MODES:
        raise ValueError("mode must be 'nearest' or 'subpixel' (got %r)" % (mode,))
    fwd, fv, (h, w) = _maps(maps, "forward")
    oh, ow = _size(maps.out_size, "maps.out_size")
    a = U._In(xs, ys, ts, ps)
    if a.cols[0] is None or a.cols[1] is None:
        raise TypeError("rectify_events needs xs and ys")
    dev = a.cols[0].device
    n = int(a.cols[0].shape[0])
    px, py, kind = a.pred_xy()
    if mode == "nearest":
        out_kind = kind
        if out_kind == _lib.EVK_SELECT_I16 and max(oh, ow) > 32768:
            raise ValueError("int16 coordinates cannot hold a rectified view of %r" % ((oh, ow),))
    else:
        out_kind = _lib.EVK_SELECT_F32 if (a.mode == "events" and a.cols[0].dtype == torch.float32) else _lib.EVK_SELECT_F64
    fwd, fv = D.resident(fwd, dev), D.resident(fv, dev)
    ox, oy = (torch.empty(n, dtype=_T_OF_KIND[out_kind], device=dev) for _ in range(2))
    have = [i for i, c in enumerate(a.cols) if c is not None]
    cols = [ox, oy] + [a.cols[i] for i in have[2:]]
    if n == 0:
        kept, index, res = cols, torch.empty(0, dtype=torch.int64, device=dev), [0]
    else:
        keep = torch.empty(n, dtype=torch.uint8, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.call("evk_camera_rectify_lookup", kind, D.ptr(px), D.ptr(py), n, D.ptr(fwd), D.ptr(fv), h, w, oh, ow, _MODES[mode], out_kind,
                  D.ptr(ox), D.ptr(oy), D.ptr(keep), D.ptr(bad), D.stream())
        if D.error_mode() == "strict" and int(bad.item()):
            raise ValueError("rectify_events needs integer pixel coordinates on the %d x %d raw sensor" % (h, w))
        kept, index, res = U._compact(_lib.EVK_SELECT_FLAGS, keep, keep, _lib.EVK_SELECT_I32, cols, image=keep, want_index=return_index,
                                      t_col=have.index(2) if 2 in have else -1)
    full = [None] * 4
    for i, k in zip(have, kept):
        full[i] = k
    if a.mode == "events":
        out = U._events_result(a.ev, full, res)
    elif a.mode == "numpy":
        out = tuple(full[i].cpu().numpy() for i in (0, 1)) + U._columns_out("numpy", full[2:], a.dts[2:])
        index = index.cpu().numpy() if return_index else None
    else:
        out = tuple(full)
    return (out, index) if return_index else out


# ---- images ------------------------------------------------------------------------------------------------------------------------

def remap_images(images, maps, interpolation="nearest", fill=0):
    """Images of the raw sensor, (..., H, W) uint8, float32 or float64 -> the rectified view (..., H', W') of the same dtype, through
    maps.inverse: the call that rectifies quantised_time_surfaces for stereo_match and frames for complementary_filter.

    interpolation "nearest": the source pixel at the half-to-even rounding of the entry.  "bilinear": the four taps around the entry
    weighted in float64, b1 (a1 v00 + a v01) + b (a1 v10 + a v11), rounded once to the dtype (uint8: half to even, then clamped);
    a tap off the sensor takes `fill`.  An entry that is not valid, or whose nearest pixel is off the sensor, gives `fill`.  numpy
    in, numpy out; a device tensor in, a device tensor out."""
    if interpolation not in _INTERPOLATIONS:
        raise ValueError("interpolation must be 'nearest' or 'bilinear' (got %r)" % (interpolation,))
    inv, iv, (oh, ow) = _maps(maps, "inverse")
    if not isinstance(images, (torch.Tensor, np.ndarray)):
        raise TypeError("images must be a uint8, float32 or float64 tensor or array (got %s)" % type(images).__name__)
    on_device = isinstance(images, torch.Tensor)
    dtype = images.dtype if on_device else U._T_OF.get(images.dtype, torch.uint8 if images.dtype == np.uint8 else None)
    if dtype not in _PLANES:
        raise TypeError("images must be uint8, float32 or float64 (got %s)" % images.dtype)
    if len(images.shape) < 2:
        raise ValueError("images must be (..., H, W) (got %r)" % (tuple(images.shape),))
    lead, (h, w) = tuple(int(s) for s in images.shape[:-2]), (int(s) for s in images.shape[-2:])
    if maps.forward is not None and (h, w) != tuple(maps.forward.shape[1:]):
        raise ValueError("the images must have the size %r of the maps' camera (got %r)" % (tuple(maps.forward.shape[1:]), (h, w)))
    if h * w > 2 ** 31 - 1:
        raise ValueError("images of %d x %d pixels are more than one call takes" % (h, w))
    fill = float(fill)
    if dtype == torch.uint8 and fill != fill:
        raise ValueError("fill must not be NaN for uint8 images")
    dev = D.device_of(images, inv)
    planes = int(np.prod(lead, dtype=np.int64))
    src = D.resident(images, dev).reshape(planes, h, w)
    inv, iv = D.resident(inv, dev), D.resident(iv, dev)
    dst = torch.empty((planes, oh, ow), dtype=dtype, device=dev)
    if planes:
        _lib.call("evk_camera_remap", D.ptr(src), _PLANES[dtype], planes, h, w, D.ptr(inv), D.ptr(iv), oh, ow, _INTERPOLATIONS[interpolation],
                  fill, D.ptr(dst), D.stream())
    dst = dst.reshape(lead + (oh, ow))
    return dst if on_device else dst.cpu().numpy()


# ---- stereo rectification (host, numpy float64: a dozen 3 x 3 products) ----------------------------------------------------------------

def _rodrigues(om):
    th = math.sqrt(float(om @ om))
    if th < 1e-12:
        return np.eye(3)
    k = om / th
    kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + math.sin(th) * kx + (1.0 - math.cos(th)) * (kx @ kx)


def _rotation_vector(R):
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s, c = 0.5 * math.sqrt(float(w @ w)), 0.5 * (np.trace(R) - 1.0)
    if s < 1e-12:
        if c < 0.0:
            raise ValueError("R turns the cameras half round: no stereo pair")
        return np.zeros(3)
    return w * (math.atan2(s, c) / (2.0 * s))


def stereo_rectify(cam_left, cam_right, R, T, out_size=None):
    """Bouguet's rectification of a calibrated pair, X_right = R X_left + T -> (R_left, R_right, new_K, baseline).  R is split in
    half between the cameras, the baseline is then turned onto the x axis, and both views share one new_K (the mean focal length,
    the mean principal point: equal principal points put zero disparity at infinity).  After rectification a point at depth Z lies
    on one row of both views, at u_left - u_right = new_K[0, 0] baseline / Z.  The rotations go to rectification_maps, new_K[0, 0]
    and baseline to disparity_depth_map.  cam_left must be the camera on the left.  out_size (default: the left sensor's) moves
    the principal point with the centre of the view."""
    for cam in (cam_left, cam_right):
        if not isinstance(cam, CameraModel):
            raise TypeError("cam_left and cam_right must be CameraModels")
    R = _rotation(np.eye(3) if R is None else R)
    T = np.asarray(T, dtype=np.float64).reshape(-1)
    if T.shape != (3,) or not np.isfinite(T).all() or not (T @ T) > 0.0:
        raise ValueError("T must be three finite numbers, not all zero")
    r_r = _rodrigues(-0.5 * _rotation_vector(R))
    t = r_r @ T
    baseline = math.sqrt(float(t @ t))
    if not t[0] < 0.0:
        raise ValueError("cam_left must be the camera on the left: the x component of the half-rotated T must be negative")
    e = np.array([-1.0, 0.0, 0.0])
    w = np.cross(t / baseline, e)
    s = math.sqrt(float(w @ w))
    turn = np.eye(3) if s < 1e-12 else _rodrigues(w * (math.atan2(s, float((t / baseline) @ e)) / s))
    h, w_ = cam_left.sensor_size
    oh, ow = (h, w_) if out_size is None else _size(out_size, "out_size")
    kl, kr = cam_left.K, cam_right.K
    f = (kl[0, 0] + kl[1, 1] + kr[0, 0] + kr[1, 1]) / 4.0
    new_K = np.array([[f, 0.0, (kl[0, 2] + kr[0, 2]) / 2.0 + (ow - w_) / 2.0], [0.0, f, (kl[1, 2] + kr[1, 2]) / 2.0 + (oh - h) / 2.0],
                      [0.0, 0.0, 1.0]])
    return turn @ r_r.T, turn @ r_r, new_K, baseline
