"""The per-pixel grouping on the host: "all events of one pixel (and polarity class), in stream order" (evk_denoise_group; csrc/
evk_group.h) and what every feature on it shares -- the argument prefix of the per-event entry points, the
selection of events, the sortedness check, query times as cuts, the polarity flags, and the kind of the result.  Its users:
util/event_denoise.py, representations/time_surface.py and reconstruction.py, features/corners.py and plane_flow.py."""
import numpy as np
import torch

from . import _device as D
from . import _lib
from ._checks import in_range, int_vector


def sensor_hw(sensor_size):
    h, w = int(sensor_size[0]), int(sensor_size[1])
    if h <= 0 or w <= 0:
        raise ValueError("sensor_size must be positive (got %r)" % (tuple(sensor_size),))
    return h, w


def polarity_flags(a):
    """uint8 (N,): the polarity class p > 0 of every event (a negative p_scale of a DeviceEvents turns it round)"""
    pc = a.pred(3)[0]
    return ((pc < 0) if (a.ev is not None and a.ev.p_scale < 0) else (pc > 0)).to(torch.uint8)


def result(a, out):
    return out.cpu().numpy() if a.mode == "numpy" else out


class Grouped:
    """The events of a call grouped by pixel (and polarity class): the int32 pixel columns, the time column and its kind, and
    the scratch that holds keys, order[] and the run table (evk_denoise_group)."""

    def __init__(self, a, sensor_size, use_polarity, what):
        self.h, self.w = sensor_hw(sensor_size)
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
        cls = polarity_flags(a) if use_polarity else None
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

    def args(self):
        """the arguments every per-event entry point begins with (n > 0)"""
        return self.t_kind, D.ptr(self.t), self.n, self.h, self.w, self.classes

    def selection(self, select):
        """-> (device int64 indices or None, the rows of the output)"""
        if select is None:
            return None, self.n
        sel = int_vector(select, "select", IndexError)
        if not in_range(sel, 0, self.n - 1):
            raise IndexError("select must hold event indices in [0, %d)" % self.n)
        return sel.to(self.dev), int(sel.shape[0])

    def require_sorted(self, what):
        if self.n < 2:
            return
        bad = torch.zeros(1, dtype=torch.int32, device=self.dev)
        _lib.call("evk_tsurf_check_sorted", self.t_kind, D.ptr(self.t), self.n, D.ptr(bad), D.stream())
        if int(bad.item()):
            raise ValueError("%s needs non-decreasing time stamps" % what)

    def cuts_before(self, keys):
        """int64 (K,): the number of events with t < keys[k] (device float64, the column's time base); ts non-decreasing.  An
        integer column is searched as float64."""
        cuts = torch.zeros(int(keys.shape[0]), dtype=torch.int64, device=self.dev)
        if self.n:
            col = self.t if self.t_kind in (_lib.EVK_SELECT_F32, _lib.EVK_SELECT_F64) else self.t.to(torch.float64)
            _lib.call("evk_searchsorted_left", D.ptr(col), col.element_size(), self.n, D.ptr(keys), int(keys.shape[0]), D.ptr(cuts),
                      D.stream())
        return cuts

    def support(self, dt, radius, include_self, min_support=0, want_keep=False, walk=_lib.EVK_DENOISE_WALK_DEFAULT):
        sup = torch.empty(self.n, dtype=torch.uint8, device=self.dev)
        keep = torch.empty(self.n, dtype=torch.uint8, device=self.dev) if want_keep else None
        if self.n:
            _lib.call("evk_denoise_support", *self.args(), dt, radius, 1 if include_self else 0, min_support, walk,
                      D.ptr(self.scratch), D.ptr(sup), D.ptr(keep), D.stream())
        return sup, keep

    def refractory(self, refractory, wave_run=0):
        keep = torch.empty(self.n, dtype=torch.uint8, device=self.dev)
        if self.n:
            _lib.call("evk_denoise_refractory", *self.args(), refractory, int(wave_run), D.ptr(self.scratch), D.ptr(keep), D.stream())
        return keep


def kept(a, keep, want_index=False):
    """The columns of `a` compacted under the uint8 flags `keep`, in the caller's kind (None columns stay None); with want_index
    also the int64 stream indices of the kept events, on the device."""
    from .util.event_util import _columns_out, _compact, _events_result      # (util imports this module: event_denoise.py)
    if int(a.cols[0].shape[0]) == 0:
        out = _events_result(a.ev, a.cols, [0]) if a.mode == "events" else _columns_out(a.mode, a.cols, a.dts)
        return (out, torch.empty(0, dtype=torch.int64, device=a.cols[0].device)) if want_index else out
    have = [i for i, c in enumerate(a.cols) if c is not None]
    cols, index, res = _compact(_lib.EVK_SELECT_FLAGS, keep, keep, _lib.EVK_SELECT_I32, [a.cols[i] for i in have], image=keep,
                                want_index=want_index, t_col=have.index(2))
    full = [None] * 4
    for i, k in zip(have, cols):
        full[i] = k
    out = _events_result(a.ev, full, res) if a.mode == "events" else _columns_out(a.mode, full, a.dts)
    return (out, index) if want_index else out
