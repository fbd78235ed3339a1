"""Event stereo on the device (evk_stereo.hip; definition: include/evk.h, "Event stereo", and DESIGN.md section 6): disparity from two
rectified, time-synchronised event cameras by block matching on quantised time surfaces, the mapping step of ESVO (Zhou et al.,
"Event-based Stereo Visual Odometry", T-RO 2021) and of the time-surface stereo before it.  No reference module: upstream estimates
no depth.  No trajectory is needed.

Rectified means that epipolar lines are image rows: a scene point seen at (x, y) on the left lies at (x - d, y) on the right, d >= 0;
both sensors have one size.  The surfaces are the exact float64 ages of time_surfaces(decay=None) under a linear decay quantised to
8 bits, so every matching cost is an integer and a result is the same bits from run to run and from tiling to tiling.  The input
kinds are those of the other event calls: numpy columns, device tensors, or a DeviceEvents in place of xs (the other columns None);
every result stays on the device.  A raw, distorted pair becomes a rectified one in calibration.camera: stereo_rectify, then
rectify_events on the events or remap_images on the surfaces."""
import collections
import math

import numpy as np
import torch

from .. import _device as D
from .. import _lib
from .._checks import check_array, check_decay, check_int, check_polarity
from ..events import DeviceEvents
from ..representations.time_surface import _surfaces
from .emvs import DepthMap

MAX_DISPARITIES = _lib.EVK_STEREO_MAX_DISPARITIES
MAX_RADIUS = _lib.EVK_STEREO_MAX_RADIUS
MAX_MIN_DISPARITY = 1 << 30

Disparity = collections.namedtuple("Disparity", ["disparity", "index", "cost", "mask"])
Disparity.__doc__ = """A semi-dense disparity map of the left view, (K, H, W) device tensors: `disparity` float32, sub-pixel when asked
for, NaN where not valid; `index` int32 the winning disparity, -1 where not valid; `cost` int32 its cost, -1 where the pixel is no
candidate; `mask` bool."""


# ---- arguments (semi-global matching, sgm.py, takes the names without an underscore from here) ------------------------------------

def check_range(max_disparity, min_disparity, radius):
    """-> (d_min, D, radius)"""
    d_min = check_int(min_disparity, "min_disparity", 0, MAX_MIN_DISPARITY)
    if isinstance(max_disparity, bool) or int(max_disparity) != max_disparity:
        raise ValueError("max_disparity must be an integer (got %r)" % (max_disparity,))
    nd = int(max_disparity) - d_min + 1
    if not 1 <= nd <= MAX_DISPARITIES:
        raise ValueError("max_disparity - min_disparity + 1 must be 1 .. %d disparities (got %d)" % (MAX_DISPARITIES, nd))
    return d_min, nd, check_int(radius, "radius", 1, MAX_RADIUS)


def check_surfaces(QL, QR):
    """-> (K, C, H, W) of two uint8 surfaces of one shape"""
    shape = check_array(QL, "QL", torch.uint8, "quantised_time_surfaces")
    other = check_array(QR, "QR", torch.uint8, "quantised_time_surfaces")
    if shape != other:
        raise ValueError("QL and QR must have one shape (got %r and %r)" % (shape, other))
    if len(shape) != 4 or shape[1] not in (1, 2) or min(shape) < 1 or shape[2] * shape[3] > 2 ** 31 - 1:
        raise ValueError("the surfaces must be (K, C, H, W) with K, H, W >= 1, C 1 or 2 and H * W < 2^31 (got %r)" % (shape,))
    return shape


def check_tests(min_activity, uniqueness, max_cost, lr_tolerance, window=None):
    """-> (min_activity, uniqueness, the cost limit or -1, the tolerance or -1).  max_cost is the integer limit itself (window
    None: match_cost_volume) or the limit of the mean cost over a window of `window` = C (2 radius + 1)^2 bytes (stereo_match)."""
    min_activity = check_int(min_activity, "min_activity", 1, 255)
    uniqueness = check_int(uniqueness, "uniqueness", 0, 99)
    limit = -1
    if max_cost is not None and window is None:
        limit = check_int(max_cost, "max_cost", 0, 2 ** 62, must="an integer >= 0 or None")
    elif max_cost is not None:
        max_mean_cost = float(max_cost)
        if not (max_mean_cost >= 0.0 and math.isfinite(max_mean_cost)):
            raise ValueError("max_mean_cost must be finite and >= 0, or None (got %r)" % max_mean_cost)
        limit = min(int(math.floor(max_mean_cost * window)), 2 ** 40)
    tolerance = -1 if lr_tolerance is None else check_int(lr_tolerance, "lr_tolerance", 0, 2 ** 30, must="an integer >= 0 or None")
    return min_activity, uniqueness, limit, tolerance


def _check_volume(shape, nd):
    if shape[0] * nd * shape[2] * shape[3] > 2 ** 40:
        raise ValueError("a cost volume of %d x %d x %d x %d cells is more than one call takes (2^40)" % (shape[0], nd, shape[2], shape[3]))


def resident_pair(QL, QR):
    """-> both surfaces on the device of QL, and that device"""
    dev = D.device_of(QL)
    return D.resident(QL, dev), D.resident(QR, dev), dev


def event_stream(events, what):
    """(xs, ys, ts, ps) of one camera: a DeviceEvents, or four columns"""
    if isinstance(events, DeviceEvents):
        return events, None, None, None
    try:
        xs, ys, ts, ps = events
    except (TypeError, ValueError):
        raise TypeError("%s must be (xs, ys, ts, ps) or a DeviceEvents" % what)
    return xs, ys, ts, ps


# ---- surfaces --------------------------------------------------------------------------------------------------------------------

def _quantised(xs, ys, ts, ps, tau, sensor_size, t_refs, polarity, indices=None):
    if indices is not None:
        raise TypeError("event counts (indices) mean nothing across two streams: query the surfaces by time, with t_refs")
    if t_refs is None:
        raise TypeError("quantised_time_surfaces needs t_refs")
    _, tau = check_decay(None, tau)
    if not math.isfinite(tau):
        raise ValueError("tau must be finite (got %r)" % tau)
    check_polarity(polarity, ("ignore", "split"))
    _, ages = _surfaces(xs, ys, ts, ps, tau, sensor_size, t_refs, None, None, polarity)
    q = torch.empty(ages.shape, dtype=torch.uint8, device=ages.device)
    _lib.call("evk_stereo_quantise", D.ptr(ages), ages.numel(), tau, D.ptr(q), D.stream())
    return q


def quantised_pair(left, right, tau, sensor_size, t_refs, polarity, indices):
    """the surfaces of two event_stream results at the same times t_refs"""
    return tuple(_quantised(*cam, tau, sensor_size, t_refs, polarity, indices) for cam in (left, right))


def quantised_time_surfaces(xs, ys, ts, ps, tau, sensor_size, t_refs, polarity="ignore"):
    """The surfaces block matching runs on, (K, C, H, W) uint8 on the device: with a the float64 age of time_surfaces(decay=None)
    at the K times t_refs (polarity "ignore", C = 1, or "split", C = 2), v = 1.0 - a / tau and q = 0 unless v > 0, else
    min(255, floor(256.0 v)); no earlier event gives 0.  All float64, one rounding per operation.  ts must be non-decreasing."""
    return _quantised(xs, ys, ts, ps, tau, sensor_size, t_refs, polarity)


# ---- cost volume and matcher -----------------------------------------------------------------------------------------------------

def match_call(entry, head, tests, subpixel, scratch, k, h, w, dev):
    """entry(*head, *tests, subpixel, scratch, the four (K, H, W) outputs, the stream) -> Disparity: the arguments evk_stereo_match
    and evk_sgm_match_volume end on"""
    disparity = torch.empty((k, h, w), dtype=torch.float32, device=dev)
    index, cost = (torch.empty((k, h, w), dtype=torch.int32, device=dev) for _ in range(2))
    mask = torch.empty((k, h, w), dtype=torch.uint8, device=dev)
    _lib.call(entry, *head, *tests, 1 if subpixel else 0, D.ptr(scratch), D.ptr(disparity), D.ptr(index), D.ptr(cost), D.ptr(mask),
              D.stream())
    return Disparity(disparity, index, cost, mask.to(torch.bool))


def stereo_cost_volume(QL, QR, max_disparity, radius=3, min_disparity=0):
    """The matching costs, (K, D, H, W) int32 on the device, of the disparities d = min_disparity + i, D = max_disparity -
    min_disparity + 1 in 1 .. 256: cost[k, i, y, x] = the sum over c, |dy| <= radius, |dx| <= radius of
    |QL[k, c, y + dy, x + dx] - QR[k, c, y + dy, x + dx - d]| with Q = 0 off the sensor; -1 where d is not admissible, which it is
    iff 0 <= x - d.  QL, QR: (K, C, H, W) uint8, C 1 or 2; radius 1 .. 7."""
    d_min, nd, radius = check_range(max_disparity, min_disparity, radius)
    shape = check_surfaces(QL, QR)
    _check_volume(shape, nd)
    QL, QR, dev = resident_pair(QL, QR)
    k, c, h, w = shape
    volume = torch.empty((k, nd, h, w), dtype=torch.int32, device=dev)
    _lib.call("evk_stereo_cost_volume", D.ptr(QL), D.ptr(QR), k, c, h, w, d_min, nd, radius, D.ptr(volume), D.stream())
    return volume


def stereo_match(QL, QR, max_disparity, radius=3, min_disparity=0, min_activity=128, uniqueness=10, max_mean_cost=None, lr_tolerance=1,
                 subpixel=True):
    """Winner-takes-all block matching on two quantised surfaces -> Disparity(disparity, index, cost, mask), (K, H, W) each, without
    writing the cost volume.

    A left pixel is a candidate iff max_c QL[k, c, y, x] >= min_activity (1 .. 255) and some d is admissible.  d* is its admissible
    d of least cost (stereo_cost_volume), the smallest on ties; c1 that cost; c2 the least cost over admissible d with
    |d - d*| > 1, if there is one.  A candidate is valid iff all of these integer tests pass:
      uniqueness (0 .. 99; 0: off)   there is no c2, or c2 (100 - uniqueness) >= 100 c1;
      max_mean_cost (None: off)      c1 <= floor(max_mean_cost C (2 radius + 1)^2);
      lr_tolerance (None: off)       |dR - d*| <= lr_tolerance, dR the right image's own winner at x' = x - d*: the d with
                                     x' + d <= W - 1 of least cost[k, d - min_disparity, y, x' + d], the smallest on ties.
    subpixel: where d* - 1 and d* + 1 are in the range and admissible, with costs cm, cp and den = cm - 2 c1 + cp > 0, the
    disparity is (float)(d* + (cm - cp) / (2 den)) in float64; else (float)d*."""
    d_min, nd, radius = check_range(max_disparity, min_disparity, radius)
    shape = check_surfaces(QL, QR)
    tests = check_tests(min_activity, uniqueness, max_mean_cost, lr_tolerance, shape[1] * (2 * radius + 1) ** 2)
    QL, QR, dev = resident_pair(QL, QR)
    k, c, h, w = shape
    nbytes = int(_lib.lib().evk_stereo_scratch_bytes(k, h, w, tests[3]))
    if nbytes < 0:
        raise ValueError("%d surfaces of %d x %d are more than one call takes" % (k, h, w))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    return match_call("evk_stereo_match", (D.ptr(QL), D.ptr(QR), k, c, h, w, d_min, nd, radius), tests, subpixel, scratch, k, h, w, dev)


def stereo_disparity(left, right, tau, sensor_size, t_refs, max_disparity, radius=3, min_disparity=0, polarity="ignore", min_activity=128,
                     uniqueness=10, max_mean_cost=None, lr_tolerance=1, subpixel=True, indices=None):
    """quantised_time_surfaces of both cameras at the same K times t_refs, then stereo_match -> Disparity.  left, right: (xs, ys,
    ts, ps) or a DeviceEvents each, in one time base, with non-decreasing time stamps (ValueError otherwise).  indices is refused:
    event counts mean nothing across two streams."""
    left, right = event_stream(left, "left"), event_stream(right, "right")
    check_range(max_disparity, min_disparity, radius)
    check_polarity(polarity, ("ignore", "split"))
    check_tests(min_activity, uniqueness, max_mean_cost, lr_tolerance, 1)         # (the refusals only: no window changes them)
    QL, QR = quantised_pair(left, right, tau, sensor_size, t_refs, polarity, indices)
    return stereo_match(QL, QR, max_disparity, radius, min_disparity, min_activity, uniqueness, max_mean_cost, lr_tolerance, subpixel)


# ---- depth -----------------------------------------------------------------------------------------------------------------------

def _focal_baseline(fx, baseline):
    fx, baseline = float(fx), float(baseline)
    if not (fx > 0.0 and baseline > 0.0 and math.isfinite(fx) and math.isfinite(baseline)):
        raise ValueError("fx and baseline must be finite and > 0 (got %r, %r)" % (fx, baseline))
    return fx, baseline


def disparity_to_depth(disparity, fx, baseline):
    """float64 depth (fx baseline) / d of a rectified pair; NaN where d is NaN or <= 0.  A tensor in, a tensor on its device out;
    else numpy."""
    fx, baseline = _focal_baseline(fx, baseline)
    if isinstance(disparity, torch.Tensor):
        d = disparity.to(torch.float64)
        # (a tensor over a tensor: torch turns scalar / tensor into a reciprocal and a multiply, two roundings)
        return torch.where(d > 0.0, torch.full_like(d, fx * baseline) / d, torch.full_like(d, float("nan")))
    d = np.asarray(disparity, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(d > 0.0, (fx * baseline) / d, np.nan)


def disparity_depth_map(disp, k, fx, baseline):
    """Slice k of a Disparity as a DepthMap of the left camera (depth_to_points takes it): depth = disparity_to_depth, index the
    winning disparity, confidence = -cost as float32 (the better match the higher), mask the valid pixels with a depth."""
    fx, baseline = _focal_baseline(fx, baseline)
    if not (isinstance(disp, tuple) and len(disp) == 4):
        raise ValueError("disp must be a Disparity(disparity, index, cost, mask)")
    nk = int(disp.disparity.shape[0]) if len(disp.disparity.shape) == 3 else 0
    if isinstance(k, bool) or int(k) != k or not 0 <= k < nk:
        raise IndexError("k must be a slice 0 .. %d of a (K, H, W) Disparity (got %r)" % (nk - 1, k))
    depth = disparity_to_depth(disp.disparity[k], fx, baseline)
    confidence = -(disp.cost[k].to(torch.float32) if isinstance(disp.cost, torch.Tensor) else np.asarray(disp.cost[k], dtype=np.float32))
    return DepthMap(depth, disp.index[k], confidence, disp.mask[k] & (depth == depth))
