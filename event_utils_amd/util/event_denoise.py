"""Spatio-temporal event denoising on the device (evk_denoise.hip; definitions: include/evk.h, "Event denoising", and DESIGN.md
section 6): the background-activity filter (keep an event whose neighbourhood fired shortly before it; with support > 1,
Guo & Delbruck's STCF) and the refractory-period filter.  The input and output conventions are those of the filters of
event_util.py: numpy in -> numpy out (same dtypes), device tensors in -> device tensors out, a DeviceEvents in place of xs
(the other columns None) -> a new DeviceEvents.  The kept events keep their stream order.  The time stamps must be finite: the
definitions compare differences of times, and what a NaN or an infinite stamp gives is not part of the contract."""
from .. import _lib
from .._checks import check_int, check_time
from .._grouping import Grouped, kept, result
from .event_util import _In


def _check_support(support, radius, include_self):
    most = (2 * radius + 1) ** 2 - (0 if include_self else 1)
    if int(support) != support or not 1 <= int(support) <= most:
        raise ValueError("support must be 1 .. %d for radius %d (got %r)" % (most, radius, support))
    return int(support)


def neighbour_support(xs, ys, ts, ps, dt, sensor_size=(180, 240), radius=1, include_self=False, same_polarity=False):
    """support_i of every event (uint8, (N,)): the number of pixels of the (2 radius + 1)^2 window around the event's pixel --
    clipped to the sensor, without the centre unless include_self -- whose last earlier event (smaller stream index; of the same
    polarity class p > 0 with same_polarity) lies within dt: t_i - t_last <= dt in float64.  numpy in -> numpy out, else a device
    tensor.  ps may be None unless same_polarity."""
    dt, radius = check_time(dt, "dt"), check_int(radius, "radius", 1, _lib.EVK_DENOISE_MAX_RADIUS)
    a = _In(xs, ys, ts, ps)
    g = Grouped(a, sensor_size, same_polarity, "neighbour_support")
    sup, _ = g.support(dt, radius, include_self)
    return result(a, sup)


def background_activity_filter(xs, ys, ts, ps, dt, sensor_size=(180, 240), radius=1, support=1, include_self=False,
                               same_polarity=False, return_support=False):
    """Keeps the events with neighbour_support >= support, in stream order.  Returns the four columns (a DeviceEvents for a
    DeviceEvents); return_support=True appends the uint8 support of every INPUT event."""
    dt, radius = check_time(dt, "dt"), check_int(radius, "radius", 1, _lib.EVK_DENOISE_MAX_RADIUS)
    support = _check_support(support, radius, include_self)
    a = _In(xs, ys, ts, ps)
    g = Grouped(a, sensor_size, same_polarity, "background_activity_filter")
    sup, keep = g.support(dt, radius, include_self, support, want_keep=True)
    out = kept(a, keep)
    if not return_support:
        return out
    sup = result(a, sup)
    return (out, sup) if a.mode == "events" else tuple(out) + (sup,)


def refractory_filter(xs, ys, ts, ps, refractory, sensor_size=(180, 240), per_polarity=False):
    """Per pixel (per pixel and polarity class p > 0 with per_polarity): the first event is kept, a later one iff its time is at
    least `refractory` after the last KEPT earlier event of that pixel (float64 differences).  Stream order is kept.  ps may be
    None unless per_polarity."""
    refractory = check_time(refractory, "refractory")
    a = _In(xs, ys, ts, ps)
    g = Grouped(a, sensor_size, per_polarity, "refractory_filter")
    return kept(a, g.refractory(refractory))
