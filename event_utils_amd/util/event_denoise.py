"""Spatio-temporal event denoising on the device (evk_denoise.hip; definitions: include/evk.h, "Event denoising", and DESIGN.md
section 6): the background-activity filter (keep an event whose neighbourhood fired shortly before it; with support > 1,
Guo & Delbruck's STCF) and the refractory-period filter.  The input and output conventions are those of the filters of
event_util.py: numpy in -> numpy out (same dtypes), device tensors in -> device tensors out, a DeviceEvents in place of xs
(the other columns None) -> a new DeviceEvents.  The kept events keep their stream order.  The time stamps must be finite: the
definitions compare differences of times, and what a NaN or an infinite stamp gives is not part of the contract."""
import numpy as np
import torch

from .. import _device as D
from .. import _lib
from .event_util import _In, _columns_out, _compact, _events_result


def _check_radius(radius):
    if int(radius) != radius or not 1 <= int(radius) <= _lib.EVK_DENOISE_MAX_RADIUS:
        raise ValueError("radius must be 1 .. %d (got %r)" % (_lib.EVK_DENOISE_MAX_RADIUS, radius))
    return int(radius)


def _check_time(value, what):
    value = float(value)
    if not value >= 0.0:                       # (also NaN)
        raise ValueError("%s must be >= 0 (got %r)" % (what, value))
    return value


def _check_support(support, radius, include_self):
    most = (2 * radius + 1) ** 2 - (0 if include_self else 1)
    if int(support) != support or not 1 <= int(support) <= most:
        raise ValueError("support must be 1 .. %d for radius %d (got %r)" % (most, radius, support))
    return int(support)


class _Grouped:
    """The events of a call grouped by pixel (and polarity class): the int32 pixel columns, the time column and its kind, and
    the scratch that holds keys, order[] and the run table (evk_denoise_group)."""

    def __init__(self, a, sensor_size, use_polarity, what):
        self.h, self.w = int(sensor_size[0]), int(sensor_size[1])
        if self.h <= 0 or self.w <= 0:
            raise ValueError("sensor_size must be positive (got %r)" % (tuple(sensor_size),))
        if any(a.cols[i] is None for i in (0, 1, 2)):
            raise TypeError("%s needs xs, ys and ts" % what)
        if use_polarity and a.cols[3] is None:
            raise TypeError("%s needs ps when a polarity option is on" % what)
        self.classes = 2 if use_polarity else 1
        self.n = n = int(a.cols[0].shape[0])
        self.dev = dev = a.cols[0].device
        if n == 0:
            return
        xi, yi = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        for i, dst in ((0, xi), (1, yi)):
            pc, kind = a.pred(i)
            _lib.call("evk_select_to_i32", kind, D.ptr(pc), n, D.ptr(dst), D.ptr(bad), D.stream())
        if any(np.dtype(a.dts[i]).kind == "f" for i in (0, 1)) and int(bad.item()):
            raise TypeError("only integer pixel coordinates permitted: the coordinates are not integers")
        cls = None
        if use_polarity:                       # polarity class: p > 0 (a negative p_scale of a DeviceEvents turns it round)
            pc = a.pred(3)[0]
            cls = ((pc < 0) if (a.ev is not None and a.ev.p_scale < 0) else (pc > 0)).to(torch.uint8)
        self.t, self.t_kind = a.pred(2)
        L = _lib.lib()
        nbytes = int(L.evk_denoise_scratch_bytes(n, self.h, self.w, self.classes))
        if nbytes < 0:
            raise ValueError("%s: %d events on a %d x %d sensor are more than one grouping holds" % (what, n, self.h, self.w))
        self.scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        oob = D.OobCounter(dev)
        _lib.call("evk_denoise_group", D.ptr(xi), D.ptr(yi), D.ptr(cls), n, self.h, self.w, self.classes, D.ptr(self.scratch),
                  nbytes, oob.ptr, D.stream())
        oob.raise_if_set(ValueError, "events outside the %d x %d sensor" % (self.h, self.w))

    def support(self, dt, radius, include_self, min_support=0, want_keep=False, walk=_lib.EVK_DENOISE_WALK_DEFAULT):
        sup = torch.empty(self.n, dtype=torch.uint8, device=self.dev)
        keep = torch.empty(self.n, dtype=torch.uint8, device=self.dev) if want_keep else None
        if self.n:
            _lib.call("evk_denoise_support", self.t_kind, D.ptr(self.t), self.n, self.h, self.w, self.classes, dt, radius,
                      1 if include_self else 0, min_support, walk, D.ptr(self.scratch), D.ptr(sup), D.ptr(keep), D.stream())
        return sup, keep

    def refractory(self, refractory, wave_run=0):
        keep = torch.empty(self.n, dtype=torch.uint8, device=self.dev)
        if self.n:
            _lib.call("evk_denoise_refractory", self.t_kind, D.ptr(self.t), self.n, self.h, self.w, self.classes, refractory,
                      int(wave_run), D.ptr(self.scratch), D.ptr(keep), D.stream())
        return keep


def _kept(a, keep, want_index=False):
    """The columns of `a` compacted under the uint8 flags `keep`, in the caller's kind (None columns stay None); with want_index
    also the int64 stream indices of the kept events, on the device."""
    if int(a.cols[0].shape[0]) == 0:
        out = _events_result(a.ev, a.cols, [0]) if a.mode == "events" else _columns_out(a.mode, a.cols, a.dts)
        return (out, torch.empty(0, dtype=torch.int64, device=a.cols[0].device)) if want_index else out
    have = [i for i, c in enumerate(a.cols) if c is not None]
    kept, index, res = _compact(_lib.EVK_SELECT_FLAGS, keep, keep, _lib.EVK_SELECT_I32, [a.cols[i] for i in have], image=keep,
                                want_index=want_index, t_col=have.index(2))
    full = [None] * 4
    for i, k in zip(have, kept):
        full[i] = k
    out = _events_result(a.ev, full, res) if a.mode == "events" else _columns_out(a.mode, full, a.dts)
    return (out, index) if want_index else out


def neighbour_support(xs, ys, ts, ps, dt, sensor_size=(180, 240), radius=1, include_self=False, same_polarity=False):
    """support_i of every event (uint8, (N,)): the number of pixels of the (2 radius + 1)^2 window around the event's pixel --
    clipped to the sensor, without the centre unless include_self -- whose last earlier event (smaller stream index; of the same
    polarity class p > 0 with same_polarity) lies within dt: t_i - t_last <= dt in float64.  numpy in -> numpy out, else a device
    tensor.  ps may be None unless same_polarity."""
    dt, radius = _check_time(dt, "dt"), _check_radius(radius)
    a = _In(xs, ys, ts, ps)
    g = _Grouped(a, sensor_size, same_polarity, "neighbour_support")
    sup, _ = g.support(dt, radius, include_self)
    return sup.cpu().numpy() if a.mode == "numpy" else sup


def background_activity_filter(xs, ys, ts, ps, dt, sensor_size=(180, 240), radius=1, support=1, include_self=False,
                               same_polarity=False, return_support=False):
    """Keeps the events with neighbour_support >= support, in stream order.  Returns the four columns (a DeviceEvents for a
    DeviceEvents); return_support=True appends the uint8 support of every INPUT event."""
    dt, radius = _check_time(dt, "dt"), _check_radius(radius)
    support = _check_support(support, radius, include_self)
    a = _In(xs, ys, ts, ps)
    g = _Grouped(a, sensor_size, same_polarity, "background_activity_filter")
    sup, keep = g.support(dt, radius, include_self, support, want_keep=True)
    out = _kept(a, keep)
    if not return_support:
        return out
    sup = sup.cpu().numpy() if a.mode == "numpy" else sup
    return (out, sup) if a.mode == "events" else tuple(out) + (sup,)


def refractory_filter(xs, ys, ts, ps, refractory, sensor_size=(180, 240), per_polarity=False):
    """Per pixel (per pixel and polarity class p > 0 with per_polarity): the first event is kept, a later one iff its time is at
    least `refractory` after the last KEPT earlier event of that pixel (float64 differences).  Stream order is kept.  ps may be
    None unless per_polarity."""
    refractory = _check_time(refractory, "refractory")
    a = _In(xs, ys, ts, ps)
    g = _Grouped(a, sensor_size, per_polarity, "refractory_filter")
    return _kept(a, g.refractory(refractory))
