"""Semi-global matching on the device (evk_sgm.hip; definition: include/evk.h, "Semi-global matching", and DESIGN.md section 6): path
aggregation of the cost volume of event stereo after Hirschmueller ("Stereo Processing by Semiglobal Matching and Mutual
Information", PAMI 2008), and the winner of any cost volume under the tests of stereo_match.  No reference module: upstream
estimates no depth.

stereo_match takes the winner of every pixel on its own; sgm_aggregate adds, along up to eight directions, a penalty P1 for a
disparity step of one between neighbouring pixels and P2 for a larger one, which carries evidence along continuous contours.  All
of it is integers: a result is the same bits from run to run.  Every result stays on the device."""
import torch

from .. import _device as D
from .. import _lib
from .._checks import check_array, check_int, check_polarity
from .stereo import Disparity  # noqa: F401  (the result's type, under this module's name too)
from .stereo import MAX_DISPARITIES, MAX_MIN_DISPARITY, check_range, check_surfaces, check_tests, event_stream, match_call, \
    quantised_pair, resident_pair, stereo_cost_volume

MAX_COST = _lib.EVK_SGM_MAX_COST
MAX_PENALTY = _lib.EVK_SGM_MAX_PENALTY
DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))


# ---- arguments -------------------------------------------------------------------------------------------------------------------

def _check_penalties(p1, p2):
    p1 = check_int(p1, "p1", 0, MAX_PENALTY)
    p2 = check_int(p2, "p2", 0, MAX_PENALTY)
    if p1 > p2:
        raise ValueError("p1 must not exceed p2 (got %d and %d)" % (p1, p2))
    return p1, p2


def _check_paths(paths):
    """-> the mask of the directions: bit j is DIRECTIONS[j]"""
    if isinstance(paths, (tuple, list)):
        mask = 0
        for r in paths:
            r = tuple(r) if isinstance(r, (tuple, list)) else r
            if r not in DIRECTIONS:
                raise ValueError("a direction must be one of %r (got %r)" % (DIRECTIONS, r))
            mask |= 1 << DIRECTIONS.index(r)
        if not mask:
            raise ValueError("paths must name at least one direction")
        return mask
    if isinstance(paths, bool) or paths not in (4, 8):
        raise ValueError("paths must be 4, 8 or a tuple of directions (dx, dy) (got %r)" % (paths,))
    return 15 if paths == 4 else 255


def _check_cost_volume(volume):
    """-> (K, D, H, W) of an int32 volume"""
    shape = check_array(volume, "volume", torch.int32, "stereo_cost_volume")
    if len(shape) != 4 or min(shape) < 1 or shape[1] > MAX_DISPARITIES or shape[2] * shape[3] > 2 ** 31 - 1:
        raise ValueError("volume must be (K, D, H, W) with K, H, W >= 1, D 1 .. %d and H * W < 2^31 (got %r)" % (MAX_DISPARITIES, shape))
    if shape[0] * shape[1] * shape[2] * shape[3] > 2 ** 40 or shape[0] * (shape[2] + shape[3]) > 2 ** 31 - 1:
        raise ValueError("a cost volume of %d x %d x %d x %d cells is more than one call takes" % shape)
    return shape


def _scratch(call, k, nd, h, w, dev):
    nbytes = int(_lib.lib().evk_sgm_scratch_bytes(call, k, nd, h, w))
    if nbytes < 0:
        raise ValueError("a cost volume of %d x %d x %d x %d cells is more than one call takes" % (k, nd, h, w))
    return torch.empty(nbytes, dtype=torch.uint8, device=dev)


# ---- aggregation -----------------------------------------------------------------------------------------------------------------

def sgm_aggregate(volume, p1, p2, paths=8):
    """The summed path costs S, (K, D, H, W) int32 on the device, of a cost volume (K, D, H, W) int32, D in 1 .. 256.  A cell is
    present iff its value is >= 0 (a volume with holes is legal) and a present cost counts as C = min(value, 2^22).  For a direction
    r = (dx, dy), a pixel p and q = p - r: L_r(p, i) = C(p, i) if q is off the sensor or has no present cell; else, with m the least
    L_r(q, j) over the present j of q, L_r(p, i) = C(p, i) + min(L_r(q, i), L_r(q, i - 1) + p1, L_r(q, i + 1) + p1, m + p2) - m, each
    of the first three terms only where that cell of q exists and is present.  S is the sum of L_r over the directions where the cell
    is present and -1 elsewhere.  0 <= p1 <= p2 <= 2^20.  paths: 4 (the first four of DIRECTIONS), 8 (all), or a tuple of
    directions."""
    shape = _check_cost_volume(volume)
    p1, p2 = _check_penalties(p1, p2)
    mask = _check_paths(paths)
    dev = D.device_of(volume)
    volume = D.resident(volume, dev)
    k, nd, h, w = shape
    scratch = _scratch(_lib.EVK_SGM_AGGREGATE, k, nd, h, w, dev)
    out = torch.empty(shape, dtype=torch.int32, device=dev)
    _lib.call("evk_sgm_aggregate", D.ptr(volume), k, nd, h, w, p1, p2, mask, D.ptr(scratch), D.ptr(out), D.stream())
    return out


# ---- the winner of a volume ------------------------------------------------------------------------------------------------------

def _check_match(volume, activity, min_disparity, min_activity, uniqueness, max_cost, lr_tolerance):
    """-> (K, D, H, W), C, d_min and the tests as check_tests returns them"""
    shape = _check_cost_volume(volume)
    ashape = check_array(activity, "activity", torch.uint8, "quantised_time_surfaces")
    if len(ashape) != 4 or ashape[1] not in (1, 2) or (ashape[0],) + ashape[2:] != (shape[0],) + shape[2:]:
        raise ValueError("activity must be (K, C, H, W) with C 1 or 2 and the volume's K, H, W (got %r for a volume %r)" % (ashape, shape))
    d_min = check_int(min_disparity, "min_disparity", 0, MAX_MIN_DISPARITY)
    return shape, ashape[1], d_min, check_tests(min_activity, uniqueness, max_cost, lr_tolerance)


def match_cost_volume(volume, activity, min_disparity=0, min_activity=128, uniqueness=10, max_cost=None, lr_tolerance=1, subpixel=True):
    """The winner of stereo_match taken from a cost volume in memory -> Disparity(disparity, index, cost, mask), (K, H, W) each.
    volume: (K, D, H, W) int32, cell i the disparity d = min_disparity + i, admissible iff its value is >= 0 and 0 <= x - d;
    activity: (K, C, H, W) uint8, C 1 or 2, a pixel a candidate iff max_c activity >= min_activity and one of its cells is
    admissible.  The winner, the smallest d on ties, c2, uniqueness, the left-right test and the parabola are those of stereo_match;
    max_cost (None: off) is the integer limit of the winner's value.  `cost` is the winner's value in this volume."""
    shape, nc, d_min, tests = _check_match(volume, activity, min_disparity, min_activity, uniqueness, max_cost, lr_tolerance)
    dev = D.device_of(volume)
    volume, activity = D.resident(volume, dev), D.resident(activity, dev)
    k, nd, h, w = shape
    scratch = _scratch(_lib.EVK_SGM_MATCH, k, nd, h, w, dev) if tests[3] >= 0 else None
    return match_call("evk_sgm_match_volume", (D.ptr(volume), D.ptr(activity), k, nc, nd, h, w, d_min), tests, subpixel, scratch, k, h, w,
                      dev)


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------

def _check_pipeline(max_disparity, min_disparity, radius, p1, p2, paths, min_activity, uniqueness, max_cost, lr_tolerance):
    check_range(max_disparity, min_disparity, radius)
    _check_penalties(p1, p2)
    _check_paths(paths)
    check_tests(min_activity, uniqueness, max_cost, lr_tolerance)


def sgm_match(QL, QR, max_disparity, p1, p2, paths=8, radius=3, min_disparity=0, min_activity=128, uniqueness=10, max_cost=None,
              lr_tolerance=1, subpixel=True):
    """stereo_cost_volume, sgm_aggregate and match_cost_volume (with QL as the activity) in sequence -> Disparity.  QL, QR:
    (K, C, H, W) uint8 surfaces; `cost` and max_cost speak of the aggregated sums S."""
    _check_pipeline(max_disparity, min_disparity, radius, p1, p2, paths, min_activity, uniqueness, max_cost, lr_tolerance)
    check_surfaces(QL, QR)
    QL, QR, _ = resident_pair(QL, QR)
    volume = stereo_cost_volume(QL, QR, max_disparity, radius, min_disparity)
    volume = sgm_aggregate(volume, p1, p2, paths)
    return match_cost_volume(volume, QL, min_disparity, min_activity, uniqueness, max_cost, lr_tolerance, subpixel)


def sgm_disparity(left, right, tau, sensor_size, t_refs, max_disparity, p1, p2, paths=8, radius=3, min_disparity=0, polarity="ignore",
                  min_activity=128, uniqueness=10, max_cost=None, lr_tolerance=1, subpixel=True, indices=None):
    """quantised_time_surfaces of both cameras at the same K times t_refs, then sgm_match -> Disparity, which disparity_depth_map
    takes as it is.  left, right: (xs, ys, ts, ps) or a DeviceEvents each, as for stereo_disparity; indices is refused."""
    left, right = event_stream(left, "left"), event_stream(right, "right")
    check_polarity(polarity, ("ignore", "split"))
    _check_pipeline(max_disparity, min_disparity, radius, p1, p2, paths, min_activity, uniqueness, max_cost, lr_tolerance)
    QL, QR = quantised_pair(left, right, tau, sensor_size, t_refs, polarity, indices)
    return sgm_match(QL, QR, max_disparity, p1, p2, paths, radius, min_disparity, min_activity, uniqueness, max_cost, lr_tolerance, subpixel)
