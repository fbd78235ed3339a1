"""Event-based optical flow on the device (evk_planeflow.hip; definitions: include/evk.h, "Plane-fit flow", and DESIGN.md section 6):
the local plane fit on the surface of active events (Benosman et al., "Event-based visual flow", TNNLS 2014; "LocalPlanes" in
Rueckauer & Delbruck 2016) with the event lifetime of Mueggler et al. (ICRA 2015), event by event, and its per-pixel average as the
dense (2, H, W) field that the flow-field losses and warps take.  No reference module: upstream estimates no flow.  Both run on the
grouping of the denoising filters (_grouping.py, Grouped) and take the input kinds of the corner detectors: numpy in ->
numpy out, device tensors in -> device tensors out, a DeviceEvents in place of xs (the other columns None) -> device tensors.

polarity: "same" two classes (p > 0 and p <= 0), an event only sees its own; "ignore" one class, ps may be None.  "Earlier" means
a smaller stream index; the times may be unsorted.  The flow is in pixels per unit of ts, the lifetime in units of ts per pixel.
The window is clipped to the sensor: an event on the border is fitted on the samples it has.  The time stamps must be finite;
what a NaN or an infinite stamp gives is not part of the contract."""
import torch

from .. import _device as D
from .. import _lib
from .._checks import check_int, check_polarity, check_positive, check_time
from .._grouping import Grouped, result
from ..util.event_util import _In


def _check_fit(dt, radius, min_samples, outlier_threshold, iterations, max_speed):
    """-> the fit arguments of evk_planeflow_fit, in its order"""
    dt, radius = check_time(dt, "dt"), check_int(radius, "radius", 1, _lib.EVK_PLANEFLOW_MAX_RADIUS)
    most = (2 * radius + 1) ** 2
    min_samples = check_int(min_samples, "min_samples", 3, most, must="3 .. %d for radius %d" % (most, radius))
    iterations = check_int(iterations, "iterations", 0, _lib.EVK_PLANEFLOW_MAX_ITERATIONS)
    return (radius, dt, min_samples) + check_positive(outlier_threshold, "outlier_threshold") + (iterations,) + \
        check_positive(max_speed, "max_speed")


def _fit(g, fit, sel, rows, want_lifetime):
    flow = torch.empty((rows, 2), dtype=torch.float32, device=g.dev)
    valid = torch.empty(rows, dtype=torch.uint8, device=g.dev)
    lifetime = torch.empty(rows, dtype=torch.float32, device=g.dev) if want_lifetime else None
    if rows:
        _lib.call("evk_planeflow_fit", *g.args(), *fit, D.ptr(sel), rows, D.ptr(g.scratch),
                  D.ptr(flow), D.ptr(lifetime), D.ptr(valid), D.stream())
    return flow, valid, lifetime


def local_plane_flow(xs, ys, ts, ps, dt, sensor_size=(180, 240), radius=2, polarity="same", min_samples=5, outlier_threshold=None,
                     iterations=2, max_speed=None, select=None, return_valid=False, return_lifetime=False):
    """The normal flow of every event, float32 (M, 2) as (vx, vy), NaN where the fit is invalid.  The samples of event i are the
    times tau = t_j - t_i of the last earlier event j of its class at the pixels of the (2 radius + 1)^2 window around it, where
    t_i - t_j <= dt, and tau = 0 at the centre for the event itself.  The least-squares plane tau ~ a dx + b dy + c over them
    needs at least min_samples samples that are not collinear.  With outlier_threshold, up to `iterations` rounds drop every
    sample whose residual exceeds it and refit.  v = (a, b) / (a^2 + b^2); with max_speed a faster flow is invalid.
    return_valid appends the bool (M,) validity, return_lifetime the float32 (M,) lifetime sqrt(a^2 + b^2), the time the edge
    takes to move one pixel."""
    two, _ = check_polarity(polarity, ("same", "ignore"))
    fit = _check_fit(dt, radius, min_samples, outlier_threshold, iterations, max_speed)
    a = _In(xs, ys, ts, ps)
    g = Grouped(a, sensor_size, two, "local_plane_flow")
    sel, rows = g.selection(select)
    flow, valid, lifetime = _fit(g, fit, sel, rows, return_lifetime)
    out = (flow,) + ((valid.to(torch.bool),) if return_valid else ()) + ((lifetime,) if return_lifetime else ())
    out = tuple(result(a, o) for o in out)
    return out if len(out) > 1 else out[0]


def plane_flow_field(xs, ys, ts, ps, dt, sensor_size=(180, 240), radius=2, polarity="same", min_samples=5, outlier_threshold=None,
                     iterations=2, max_speed=None, return_count=False):
    """The dense flow field, float32 (2, H, W) as (vx plane, vy plane): at every pixel the mean of the valid flows of
    local_plane_flow of the events there, 0 where there is none -- what flow_field_contrast_loss, flow_field_timestamp_loss,
    flow_field_iwe and warp_events_flow_torch take.  One grouping serves both passes.  return_count appends the int32 (H, W)
    number of valid events per pixel."""
    two, _ = check_polarity(polarity, ("same", "ignore"))
    fit = _check_fit(dt, radius, min_samples, outlier_threshold, iterations, max_speed)
    a = _In(xs, ys, ts, ps)
    g = Grouped(a, sensor_size, two, "plane_flow_field")
    if g.n:
        field = torch.empty((2, g.h, g.w), dtype=torch.float32, device=g.dev)
        count = torch.empty((g.h, g.w), dtype=torch.int32, device=g.dev)
        flow, valid, _ = _fit(g, fit, None, g.n, False)
        _lib.call("evk_planeflow_field", *g.args()[2:], D.ptr(g.scratch), D.ptr(flow), D.ptr(valid), D.ptr(field),
                  D.ptr(count), D.stream())
    else:                                      # (no events: no grouping to walk)
        field = torch.zeros((2, g.h, g.w), dtype=torch.float32, device=g.dev)
        count = torch.zeros((g.h, g.w), dtype=torch.int32, device=g.dev)
    return (result(a, field), result(a, count)) if return_count else result(a, field)
