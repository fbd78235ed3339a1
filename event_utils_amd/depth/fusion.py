"""Depth fusion on the device (evk_fusion.hip; definition: include/evk.h, "Depth fusion", and DESIGN.md section 6): inverse-depth maps
with their variances are carried through rigid motions into one view and fused there pixel by pixel, the map update of ESVO (Zhou et
al., "Event-based Stereo Visual Odometry", T-RO 2021, section IV-C) after the inverse-depth filters of LSD-SLAM (Engel et al., ECCV
2014), then regularised over a neighbourhood as both do.  No reference module: upstream estimates no depth.

It is the link between the K slices of a Disparity and one map: stereo_disparity -> disparity_inverse_depth (each slice) ->
track_poses -> relative_transforms -> fuse_inverse_depth -> regularise_inverse_depth -> inverse_depth_depth_map -> reference_points;
fuse_stereo_depth runs it from the Disparity to the fused map.  A transform here is target-from-source, 12 doubles: R row-major,
then t, X' = R X + t.  All arithmetic is float64 with one rounding per operation and no atomics, so a result is the same bits from run
to run (a scatter written in torch is not: duplicate destination pixels make it order-dependent).

What it does not do: occlusion reasoning (no z-buffer: a surface seen through another lands on the same pixel and only the gate
separates them) and bilinear spreading of a candidate over four pixels (it goes to the nearest).  The propagated variance follows
LSD-SLAM's rule v' = (rho' / rho)^4 v + process variance, exact for a translation along the optical axis and an approximation for any
other motion.  The anchor of a pixel is its candidate of least variance, so an OUTLIER of lower variance than the surface's own
candidates becomes the anchor and rejects them: the gate trusts the variances it is given.  Inputs are numpy arrays or device tensors;
every result stays on the device."""
import collections
import math

import numpy as np
import torch

from .. import _device as D
from .. import _lib
from .._checks import check_int
from .emvs import DepthMap, _check_size, _intrinsics, _quaternions, _rotation

MAX_RADIUS = _lib.EVK_FUSION_MAX_RADIUS
_VIEW_PARAMS = _lib.EVK_FUSION_VIEW_PARAMS

InverseDepthMap = collections.namedtuple("InverseDepthMap", ["inv_depth", "variance", "count", "rejected", "mask"])
InverseDepthMap.__doc__ = """A semi-dense inverse-depth map of one view, (H, W) device tensors: `inv_depth` and `variance` float64, NaN
where there is nothing; `count` int32, the candidates fused into the pixel, and `rejected` int32, those its gate turned away; `mask`
bool.  A pixel is a source for a later fusion iff its mask is set and inv_depth and variance are finite and > 0."""

_FIELDS = (("inv_depth", torch.float64, np.float64), ("variance", torch.float64, np.float64), ("count", torch.int32, np.int32),
           ("rejected", torch.int32, np.int32), ("mask", torch.bool, np.bool_))


# ---- arguments -------------------------------------------------------------------------------------------------------------------

def _check_map(idm, what):
    """-> (H, W) of an InverseDepthMap whose five fields have their dtypes and one 2-D shape"""
    if not (isinstance(idm, tuple) and len(idm) == 5):
        raise ValueError("%s must be an InverseDepthMap(inv_depth, variance, count, rejected, mask)" % what)
    shape = None
    for (name, tdt, ndt), v in zip(_FIELDS, idm):
        if not isinstance(v, (torch.Tensor, np.ndarray)) or v.dtype not in (tdt, np.dtype(ndt)):
            raise ValueError("%s.%s must be %s %s tensor or array (got %s)" % (
                what, name, "an" if np.dtype(ndt).name[0] == "i" else "a", np.dtype(ndt).name, getattr(v, "dtype", type(v).__name__)))
        s = tuple(int(d) for d in v.shape)
        if len(s) != 2 or min(s) < 1 or s[0] * s[1] > 2 ** 31 - 1 or (shape is not None and s != shape):
            raise ValueError("the fields of %s must be (H, W) with H, W >= 1 and H * W < 2^31, all of one shape (got %r for %s)" % (
                what, s, name))
        shape = s
    return shape


def _check_maps(maps):
    """a sequence of InverseDepthMaps (or one) -> (the list, (H, W))"""
    if isinstance(maps, InverseDepthMap):
        maps = [maps]
    try:
        maps = list(maps)
    except TypeError:
        raise ValueError("maps must be a sequence of InverseDepthMaps")
    if not maps:
        raise ValueError("maps must hold at least one InverseDepthMap")
    shape = None
    for s, idm in enumerate(maps):
        got = _check_map(idm, "maps[%d]" % s)
        if shape is not None and got != shape:
            raise ValueError("maps must be of one size (got %r and %r)" % (shape, got))
        shape = got
    if len(maps) * shape[0] * shape[1] > 2 ** 31 - 1:
        raise ValueError("%d maps of %d x %d are more than one call takes (2^31 - 1 source pixels)" % (len(maps), shape[0], shape[1]))
    return maps, shape


def _check_transforms(transforms, views):
    T = np.asarray(transforms.detach().cpu().numpy() if isinstance(transforms, torch.Tensor) else transforms, dtype=np.float64)
    if T.shape == (12,) and views == 1:
        T = T[None]
    if T.shape != (views, 12):
        raise ValueError("transforms must be (%d, 12), one per map: R row-major, then t (got %r)" % (views, T.shape))
    if not np.all(np.isfinite(T)):
        raise ValueError("transforms must be finite")
    return T


def _check_gate(gate):
    gate = float(gate)
    if not gate >= 0.0:                        # (also NaN)
        raise ValueError("gate must be >= 0 (got %r)" % gate)
    return gate * gate


def _check_process_variance(process_variance, views):
    pv = np.asarray(process_variance.detach().cpu().numpy() if isinstance(process_variance, torch.Tensor) else process_variance,
                    dtype=np.float64)
    if pv.ndim == 0:
        pv = np.full(views, float(pv))
    if pv.shape != (views,):
        raise ValueError("process_variance must be a scalar or one value per map, (%d,) (got %r)" % (views, pv.shape))
    if not np.all((pv >= 0.0) & np.isfinite(pv)):
        raise ValueError("process_variance must be finite and >= 0 (got %r)" % (process_variance,))
    return pv


def _check_fuse(gate, min_count, max_variance):
    gate2 = _check_gate(gate)
    min_count = check_int(min_count, "min_count", 1, 2 ** 31 - 1)
    if max_variance is not None:
        max_variance = float(max_variance)
        if max_variance != max_variance:
            raise ValueError("max_variance must not be NaN")
    return gate2, min_count, max_variance


def _check_regularise(radius, gate, min_neighbours):
    radius = check_int(radius, "radius", 1, MAX_RADIUS)
    return radius, _check_gate(gate), check_int(min_neighbours, "min_neighbours", 0, (2 * radius + 1) ** 2)


def _focal_baseline_sigma(fx, baseline, sigma_disparity):
    fx, baseline, sigma = float(fx), float(baseline), float(sigma_disparity)
    if not (fx > 0.0 and baseline > 0.0 and math.isfinite(fx) and math.isfinite(baseline)):
        raise ValueError("fx and baseline must be finite and > 0 (got %r, %r)" % (fx, baseline))
    if not (sigma >= 0.0 and math.isfinite(sigma)):
        raise ValueError("sigma_disparity must be finite and >= 0 (got %r)" % sigma)
    return fx * baseline, sigma


def _check_disparity(disp):
    if not (isinstance(disp, tuple) and len(disp) == 4 and len(disp[0].shape) == 3 and
            all(tuple(f.shape) == tuple(disp[0].shape) for f in disp)):
        raise ValueError("disp must be a Disparity(disparity, index, cost, mask) of (K, H, W) fields")
    return int(disp[0].shape[0])


def _check_slice(k, nk, what="k"):
    if isinstance(k, bool) or int(k) != k or not 0 <= k < nk:
        raise IndexError("%s must be a slice 0 .. %d of a (K, H, W) Disparity (got %r)" % (what, nk - 1, k))
    return int(k)


# ---- conversions -----------------------------------------------------------------------------------------------------------------

def _from_values(rho, valid, variance):
    """(rho, the flags, a variance tensor) on one device -> InverseDepthMap with NaN, 0 and False where not valid"""
    nan = torch.full_like(rho, float("nan"))
    count = valid.to(torch.int32)
    return InverseDepthMap(torch.where(valid, rho, nan), torch.where(valid, variance, nan), count, torch.zeros_like(count), valid)


def disparity_inverse_depth(disp, k, fx, baseline, sigma_disparity=0.5):
    """Slice k of a Disparity as an InverseDepthMap of the left camera: rho = d / (fx baseline) and v = (sigma_disparity /
    (fx baseline))^2, the variance of rho under a disparity error of sigma_disparity pixels; valid where the slice's mask holds and
    d > 0, with count 1 and rejected 0 there.  A sigma_disparity of 0 gives variance 0, which is no source."""
    fb, sigma = _focal_baseline_sigma(fx, baseline, sigma_disparity)
    k = _check_slice(k, _check_disparity(disp))
    dev = D.device_of(disp.disparity)
    d = D.resident(disp.disparity[k], dev, torch.float64)
    mask = D.resident(disp.mask[k], dev, torch.bool)
    s = sigma / fb
    # (a tensor over a tensor: torch turns tensor / scalar into a multiply by the reciprocal, two roundings)
    return _from_values(d / torch.full_like(d, fb), mask & (d > 0.0), torch.full_like(d, s * s))


def depth_inverse_depth(depth_map, variance):
    """A DepthMap (dsi_depth_map's, emvs_depth_map's, disparity_depth_map's) as an InverseDepthMap: rho = 1 / depth where the mask
    holds and the depth is finite and > 0, count 1 and rejected 0 there.  variance: in inverse-depth units, a scalar > 0 or an (H, W)
    map."""
    if not (isinstance(depth_map, tuple) and len(depth_map) == 4 and len(depth_map[0].shape) == 2):
        raise ValueError("depth_map must be a DepthMap(depth, index, confidence, mask) of (H, W) fields")
    shape = tuple(int(v) for v in depth_map[0].shape)
    if isinstance(variance, (torch.Tensor, np.ndarray)) and len(variance.shape):
        if tuple(int(v) for v in variance.shape) != shape:
            raise ValueError("variance must be a scalar or have the map's shape %r (got %r)" % (shape, tuple(variance.shape)))
        scalar = None
    else:
        scalar = float(variance)
        if not (scalar > 0.0 and math.isfinite(scalar)):
            raise ValueError("variance must be finite and > 0 (got %r)" % scalar)
    dev = D.device_of(depth_map.depth)
    z = D.resident(depth_map.depth, dev, torch.float64)
    mask = D.resident(depth_map.mask, dev, torch.bool)
    v = torch.full_like(z, scalar) if scalar is not None else D.resident(variance, dev, torch.float64)
    return _from_values(torch.ones_like(z) / z, mask & (z > 0.0) & torch.isfinite(z), v)


def inverse_depth_depth_map(idm):
    """An InverseDepthMap as a DepthMap (depth_to_points and reference_points take it): depth = 1 / inv_depth where the mask holds,
    NaN elsewhere; index = count; confidence = -(float32)variance, the surer the higher; the mask."""
    _check_map(idm, "idm")
    if isinstance(idm.inv_depth, torch.Tensor):
        rho, mask = idm.inv_depth, idm.mask
        depth = torch.where(mask, torch.ones_like(rho) / rho, torch.full_like(rho, float("nan")))
        return DepthMap(depth, idm.count, -idm.variance.to(torch.float32), mask)
    with np.errstate(divide="ignore", invalid="ignore"):
        depth = np.where(idm.mask, 1.0 / idm.inv_depth, np.nan)
    return DepthMap(depth, idm.count, -idm.variance.astype(np.float32), idm.mask)


def relative_transforms(positions, quaternions, target_pose):
    """(K, 12) float64 numpy target-from-source transforms (R row-major, then t) of K world-from-camera poses, positions (K, 3) and
    quaternions (K, 4) as (qx, qy, qz, qw) -- what track_poses returns --, into the view target_pose = (position, quaternion):
    R = R_t^T R_s and t = R_t^T (c_s - c_t)."""
    positions = np.asarray(positions, dtype=np.float64)
    if positions.ndim != 2 or positions.shape[1] != 3 or len(positions) < 1 or not np.all(np.isfinite(positions)):
        raise ValueError("positions must be finite with shape (K, 3), K >= 1 (got %r)" % (positions.shape,))
    quaternions = _quaternions(quaternions, "quaternions")
    if quaternions.shape != (len(positions), 4):
        raise ValueError("quaternions must have shape (%d, 4), one per position (got %r)" % (len(positions), quaternions.shape))
    try:
        c_t, q_t = target_pose
    except (TypeError, ValueError):
        raise ValueError("target_pose must be (position, quaternion)")
    c_t = np.asarray(c_t, dtype=np.float64)
    if c_t.shape != (3,) or not np.all(np.isfinite(c_t)):
        raise ValueError("target_pose's position must be 3 finite values")
    q_t = _quaternions(q_t, "target_pose's quaternion")
    if q_t.shape != (4,):
        raise ValueError("target_pose's quaternion must be 4 values")
    Rt_T = _rotation(q_t).T
    out = np.empty((len(positions), 12))
    for s in range(len(positions)):
        out[s, :9] = (Rt_T @ _rotation(quaternions[s])).reshape(9)
        out[s, 9:] = Rt_T @ (positions[s] - c_t)
    return out


# ---- the device calls ------------------------------------------------------------------------------------------------------------

def _candidates(maps, camera_matrix, transforms, process_variance, target_camera_matrix, target_size):
    """every check, then evk_fusion_propagate -> (xi, yi, rho', v') of the m candidates, the scratch for their grouping, (h', w')"""
    maps, (h, w) = _check_maps(maps)
    views = len(maps)
    K = _intrinsics(camera_matrix)
    Kt = K if target_camera_matrix is None else _intrinsics(target_camera_matrix, "target_camera_matrix")
    oh, ow = (h, w) if target_size is None else _check_size(target_size, "target_size")
    T = _check_transforms(transforms, views)
    pv = _check_process_variance(process_variance, views)
    params = np.empty((views, _VIEW_PARAMS))
    params[:, :4] = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    params[:, 4:16], params[:, 16] = T, pv
    target = np.array([Kt[0, 0], Kt[1, 1], Kt[0, 2], Kt[1, 2]])
    if not (np.all(np.isfinite(params)) and np.all(np.isfinite(target))):
        raise ValueError("camera_matrix and target_camera_matrix must be finite")
    if oh * ow > 2 ** 31 - 2:
        raise ValueError("target_size must have H * W < 2^31 - 1 (got %r)" % ((oh, ow),))
    dev = D.device_of(*(m.inv_depth for m in maps))
    rho = torch.stack([D.resident(m.inv_depth, dev) for m in maps])
    var = torch.stack([D.resident(m.variance, dev) for m in maps])
    mask = torch.stack([D.resident(m.mask, dev) for m in maps]).to(torch.uint8)
    n = views * h * w
    nbytes = int(_lib.lib().evk_fusion_scratch_bytes(views, h, w, oh, ow))
    if nbytes < 0:
        raise ValueError("%d maps of %d x %d into %d x %d are more than one call takes" % (views, h, w, oh, ow))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    xi, yi = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    orho, ovar = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(2))
    result = torch.zeros(3, dtype=torch.int64, device=dev)
    _lib.call("evk_fusion_propagate", D.ptr(rho), D.ptr(var), D.ptr(mask), views, h, w, D.host_ptr(params), oh, ow, D.host_ptr(target),
              D.ptr(scratch), D.ptr(xi), D.ptr(yi), D.ptr(orho), D.ptr(ovar), D.ptr(result), D.stream())
    m = int(result[0].item())
    return (xi[:m], yi[:m], orho[:m], ovar[:m]), scratch, (oh, ow)


def _fuse(cols, scratch, size, gate2, min_count, max_variance):
    xi, yi, rho, var = cols
    (oh, ow), m, dev = size, int(xi.shape[0]), xi.device
    _lib.call("evk_denoise_group", D.ptr(xi), D.ptr(yi), None, m, oh, ow, 1, D.ptr(scratch), int(scratch.numel()), None, D.stream())
    inv_depth, variance = (torch.empty((oh, ow), dtype=torch.float64, device=dev) for _ in range(2))
    count, rejected = (torch.empty((oh, ow), dtype=torch.int32, device=dev) for _ in range(2))
    mask = torch.empty((oh, ow), dtype=torch.uint8, device=dev)
    _lib.call("evk_fusion_fuse", m, oh, ow, D.ptr(scratch), D.ptr(rho), D.ptr(var), gate2, min_count, 0 if max_variance is None else 1,
              0.0 if max_variance is None else max_variance, D.ptr(inv_depth), D.ptr(variance), D.ptr(count), D.ptr(rejected),
              D.ptr(mask), D.stream())
    return InverseDepthMap(inv_depth, variance, count, rejected, mask.to(torch.bool))


def propagate_inverse_depth(maps, camera_matrix, transforms, process_variance=0.0, target_camera_matrix=None, target_size=None):
    """The candidates of a fusion -> (xi, yi, inv_depth, variance), device columns int32, int32, float64, float64: every source
    pixel of every map carried through its transform into the target view (include/evk.h, "Depth fusion": back-projection at
    1 / rho, X' = R X + t, projection, the nearest pixel floor(u + 0.5); v' = (rho' / rho)^4 v + process_variance), without those
    that fall behind the camera or off the target.  They are ordered by map, then by source pixel in row-major order.
    maps: a sequence of InverseDepthMaps of one size; transforms (K, 12), target-from-source, as relative_transforms returns them;
    process_variance: a scalar or one value per map; the target's camera matrix and (H, W) size default to the source's."""
    cols, _, _ = _candidates(maps, camera_matrix, transforms, process_variance, target_camera_matrix, target_size)
    return cols


def fuse_inverse_depth(maps, camera_matrix, transforms, gate=2.0, process_variance=0.0, min_count=1, max_variance=None,
                       target_camera_matrix=None, target_size=None):
    """The maps fused in the target view -> InverseDepthMap.  Per target pixel, over its candidates (propagate_inverse_depth) in
    their order: the anchor is the one of least variance, the earliest on ties; a candidate is an inlier iff (rho_i - rho_a)^2 <=
    gate^2 (v_i + v_a); inv_depth = sum(rho_i / v_i) / sum(1 / v_i) and variance = 1 / sum(1 / v_i) over the inliers, summed one after
    the other; count the inliers, rejected the others; mask = count >= min_count and (max_variance is None or variance <=
    max_variance).  A pixel nothing lands on is NaN, NaN, 0, 0, False.  A previous fused map is simply one more of the maps, with the
    transform from its view."""
    gate2, min_count, max_variance = _check_fuse(gate, min_count, max_variance)
    cols, scratch, size = _candidates(maps, camera_matrix, transforms, process_variance, target_camera_matrix, target_size)
    return _fuse(cols, scratch, size, gate2, min_count, max_variance)


def regularise_inverse_depth(idm, radius=1, gate=2.0, min_neighbours=2):
    """The neighbourhood regularisation of ESVO / LSD-SLAM -> InverseDepthMap.  For a masked pixel p, its compatible neighbours are
    the masked pixels q of the (2 radius + 1)^2 window, clipped to the image, with (rho_q - rho_p)^2 <= gate^2 (v_q + v_p), p
    included: inv_depth = sum(rho_q / v_q) / sum(1 / v_q) over them in row-major order; mask = at least min_neighbours of them
    besides p.  A pixel that is not masked keeps its value.  variance, count and rejected are the input's own tensors: smoothing
    adds no information.  radius 1 .. 3."""
    radius, gate2, min_neighbours = _check_regularise(radius, gate, min_neighbours)
    h, w = _check_map(idm, "idm")
    dev = D.device_of(idm.inv_depth)
    rho, var = D.resident(idm.inv_depth, dev), D.resident(idm.variance, dev)
    mask = D.resident(idm.mask, dev).to(torch.uint8)
    out, out_mask = torch.empty_like(rho), torch.empty_like(mask)
    _lib.call("evk_fusion_regularise", D.ptr(rho), D.ptr(var), D.ptr(mask), h, w, radius, gate2, min_neighbours, D.ptr(out), D.ptr(out_mask),
              D.stream())
    return InverseDepthMap(out, var, D.resident(idm.count, dev), D.resident(idm.rejected, dev), out_mask.to(torch.bool))


def fuse_stereo_depth(disp, fx, baseline, camera_matrix, positions, quaternions, target, sigma_disparity=0.5, gate=2.0,
                      process_variance=0.0, min_count=1, max_variance=None, radius=None, min_neighbours=2):
    """The K slices of a Disparity fused in the view of slice `target` -> InverseDepthMap: disparity_inverse_depth on every slice,
    relative_transforms of the K world-from-camera poses (positions (K, 3), quaternions (K, 4): track_poses) into pose `target`,
    fuse_inverse_depth, and with a radius regularise_inverse_depth (radius None: none) under the same gate."""
    nk = _check_disparity(disp)
    target = _check_slice(target, nk, "target")
    _focal_baseline_sigma(fx, baseline, sigma_disparity)
    _check_fuse(gate, min_count, max_variance)
    if radius is not None:
        _check_regularise(radius, gate, min_neighbours)
    positions, quaternions = np.asarray(positions, dtype=np.float64), np.asarray(quaternions, dtype=np.float64)
    if positions.shape != (nk, 3) or quaternions.shape != (nk, 4):
        raise ValueError("positions and quaternions must be (%d, 3) and (%d, 4), one pose per slice (got %r and %r)" % (
            nk, nk, positions.shape, quaternions.shape))
    transforms = relative_transforms(positions, quaternions, (positions[target], quaternions[target]))
    maps = [disparity_inverse_depth(disp, k, fx, baseline, sigma_disparity) for k in range(nk)]
    fused = fuse_inverse_depth(maps, camera_matrix, transforms, gate, process_variance, min_count, max_variance)
    return fused if radius is None else regularise_inverse_depth(fused, radius, gate, min_neighbours)
