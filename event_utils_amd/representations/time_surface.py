"""Time surfaces on the device (evk_tsurf.hip; definitions: include/evk.h, "Time surfaces", and DESIGN.md section 6): the decayed
surface of active events at one or more queries, the per-event local time surfaces of HOTS (Lagorce et al., PAMI 2017) and the
cell-averaged histograms of HATS (Sironi et al., CVPR 2018).  No reference module: upstream has none of them.  All three run on
the grouping of the denoising filters (util/event_denoise.py, _Grouped) and take their input kinds: numpy in -> numpy out, device
tensors in -> device tensors out, a DeviceEvents in place of xs (the other columns None) -> device tensors.

decay: "exp" (float)exp(-age / tau), "linear" (float)max(0, 1 - age / tau), None the float64 age itself; an age is +inf where no
earlier event exists or the pixel lies off the sensor (values 0, 0 and inf).  polarity: "ignore" one class; "same" two classes
and only the event's own (one channel); "split" two classes, channel 0 p <= 0 and channel 1 p > 0.  The time stamps must be
finite (an infinite age is the mark of "no earlier event"); what a NaN or an infinite stamp gives is not part of the contract."""
import numpy as np
import torch

from .. import _device as D
from .. import _lib
from ..util.event_denoise import _Grouped, _check_time
from ..util.event_util import _In

_DECAY = {"exp": _lib.EVK_TSURF_EXP, "linear": _lib.EVK_TSURF_LINEAR, None: _lib.EVK_TSURF_AGE}
_POLARITY = {"ignore": (False, 0), "same": (True, 0), "split": (True, 1)}      # -> (two classes in the grouping, split channels)


def _check_decay(decay, tau):
    if decay not in _DECAY:
        raise ValueError("decay must be 'exp', 'linear' or None (got %r)" % (decay,))
    tau = float(tau)
    if not tau > 0.0:                          # (also NaN)
        raise ValueError("tau must be > 0 (got %r)" % tau)
    return _DECAY[decay], tau


def _check_polarity(polarity, allowed):
    if polarity not in allowed:
        raise ValueError("polarity must be one of %s (got %r)" % (", ".join(repr(p) for p in allowed), polarity))
    return _POLARITY[polarity]


def _check_radius(radius):
    if int(radius) != radius or not 1 <= int(radius) <= _lib.EVK_TSURF_MAX_RADIUS:
        raise ValueError("radius must be 1 .. %d (got %r)" % (_lib.EVK_TSURF_MAX_RADIUS, radius))
    return int(radius)


def _out_dtype(decay):
    return torch.float64 if decay == _lib.EVK_TSURF_AGE else torch.float32


def _empty_value(decay):
    return float("inf") if decay == _lib.EVK_TSURF_AGE else 0.0


def _result(a, out):
    return out.cpu().numpy() if a.mode == "numpy" else out


def _require_sorted(g, what):
    if g.n < 2:
        return
    bad = torch.zeros(1, dtype=torch.int32, device=g.dev)
    _lib.call("evk_tsurf_check_sorted", g.t_kind, D.ptr(g.t), g.n, D.ptr(bad), D.stream())
    if int(bad.item()):
        raise ValueError("%s needs non-decreasing time stamps" % what)


def _int_vector(v, what, exc):
    """A caller's index vector as a 1-D int64 tensor (on the host or the device, wherever it was)."""
    if not isinstance(v, torch.Tensor):
        v = np.asarray(v)
        v = torch.from_numpy(np.ascontiguousarray(v if v.size else v.astype(np.int64)))
    if v.dim() > 1 or (v.numel() and (v.is_floating_point() or v.is_complex() or v.dtype == torch.bool)):
        raise exc("%s must be a vector of integers" % what)
    return v.reshape(-1).to(torch.int64)


def _in_range(v, lo, hi):
    return v.numel() == 0 or (int(v.min()) >= lo and int(v.max()) <= hi)


def time_surfaces(xs, ys, ts, ps, tau, sensor_size=(180, 240), t_refs=None, indices=None, decay="exp", polarity="split"):
    """The surface of active events at K queries, (K, C, H, W): S[k, c, y, x] = value(T_k - t of the last event of class c at
    (x, y) among the first m_k events).  Exactly one of:
      t_refs   K absolute times (the caller's time base): T_k = t_refs[k], m_k = the number of events with t < T_k; ts must be
               non-decreasing (ValueError otherwise);
      indices  K cuts m_k in 0 .. n: T_k = ts[m_k - 1]; the times may be unsorted; m_k = 0 gives an empty surface.
    polarity "split" (C = 2) or "ignore" (C = 1, ps may be None)."""
    decay, tau = _check_decay(decay, tau)
    two, _ = _check_polarity(polarity, ("split", "ignore"))
    if (t_refs is None) == (indices is None):
        raise TypeError("time_surfaces takes exactly one of t_refs and indices")
    a = _In(xs, ys, ts, ps)
    g = _Grouped(a, sensor_size, two, "time_surfaces")
    n, dev = g.n, g.dev
    refs = None
    if indices is not None:
        cuts = _int_vector(indices, "indices", TypeError)
        if not _in_range(cuts, 0, n):
            raise IndexError("indices must lie in 0 .. %d" % n)
        cuts = cuts.to(dev)
    else:
        host = t_refs.detach().cpu().numpy() if isinstance(t_refs, torch.Tensor) else np.asarray(t_refs)
        keys = host.astype(np.float64).reshape(-1) - (a.ev.t_offset if a.ev is not None else 0.0)
        refs = torch.from_numpy(np.ascontiguousarray(keys)).to(dev)
        cuts = torch.zeros(len(keys), dtype=torch.int64, device=dev)
        if n:
            _require_sorted(g, "time_surfaces with t_refs")
            col = g.t if g.t_kind in (_lib.EVK_SELECT_F32, _lib.EVK_SELECT_F64) else g.t.to(torch.float64)
            _lib.call("evk_searchsorted_left", D.ptr(col), col.element_size(), n, D.ptr(refs), len(keys), D.ptr(cuts), D.stream())
    nq = int(cuts.shape[0])
    if nq < 1:
        raise ValueError("time_surfaces needs at least one query")
    shape = (nq, g.classes, g.h, g.w)
    if n == 0:
        return _result(a, torch.full(shape, _empty_value(decay), dtype=_out_dtype(decay), device=dev))
    out = torch.empty(shape, dtype=_out_dtype(decay), device=dev)
    _lib.call("evk_tsurf_global", g.t_kind, D.ptr(g.t), n, g.h, g.w, g.classes, nq, D.ptr(cuts), D.ptr(refs), decay, tau,
              D.ptr(g.scratch), D.ptr(out), D.stream())
    return _result(a, out)


def local_time_surfaces(xs, ys, ts, ps, tau, sensor_size=(180, 240), radius=3, decay="exp", polarity="same", include_self=True,
                        select=None):
    """The local time surface of every event (HOTS), (M, C, 2 radius + 1, 2 radius + 1): element (c, dy, dx) of event i is the
    value of t_i - t of the last EARLIER event (smaller stream index) of class c at (x_i + dx, y_i + dy).  include_self puts age
    0 (value 1) at the centre of the event's own class; without it the centre is the pixel's previous event.  select: int64
    indices of the M events wanted (any order, repeats allowed; IndexError outside [0, n)); every event still forms the history.
    float32, float64 for decay=None.  The times may be unsorted."""
    decay, tau = _check_decay(decay, tau)
    two, split = _check_polarity(polarity, ("same", "split", "ignore"))
    radius = _check_radius(radius)
    a = _In(xs, ys, ts, ps)
    g = _Grouped(a, sensor_size, two, "local_time_surfaces")
    n, dev = g.n, g.dev
    sel = None
    if select is not None:
        sel = _int_vector(select, "select", IndexError)
        if not _in_range(sel, 0, n - 1):
            raise IndexError("select must hold event indices in [0, %d)" % n)
        sel = sel.to(dev)
    rows = n if sel is None else int(sel.shape[0])
    p = 2 * radius + 1
    out = torch.empty((rows, 2 if split else 1, p, p), dtype=_out_dtype(decay), device=dev)
    if rows:
        _lib.call("evk_tsurf_local", g.t_kind, D.ptr(g.t), n, g.h, g.w, g.classes, radius, decay, tau, split,
                  1 if include_self else 0, D.ptr(sel), rows, D.ptr(g.scratch), D.ptr(out), D.stream())
    return _result(a, out)


def averaged_time_surfaces(xs, ys, ts, ps, tau, dt, sensor_size=(180, 240), cell_size=10, radius=3, normalise=True,
                           return_counts=False):
    """The HATS histograms, (Cy, Cx, 2, 2 radius + 1, 2 radius + 1) float32 with Cy = ceil(H / cell_size), Cx = ceil(W / cell_size):
    h[g, q, z] = the sum over the events i of class q (p > 0) in cell g of the sum of exp(-(t_i - t_j) / tau) over the earlier
    events j of class q at pixel_i + z -- a pixel of the sensor and of the SAME cell -- with t_i - t_j <= dt; with normalise
    divided by the number of events of (g, q).  ts must be non-decreasing (ValueError).  return_counts appends the (Cy, Cx, 2)
    int32 event counts."""
    _, tau = _check_decay("exp", tau)
    dt, radius = _check_time(dt, "dt"), _check_radius(radius)
    if int(cell_size) != cell_size or int(cell_size) < 1:
        raise ValueError("cell_size must be a positive integer (got %r)" % (cell_size,))
    a = _In(xs, ys, ts, ps)
    g = _Grouped(a, sensor_size, True, "averaged_time_surfaces")
    n, dev = g.n, g.dev
    cell = min(int(cell_size), max(g.h, g.w))
    cy, cx, p = -(-g.h // cell), -(-g.w // cell), 2 * radius + 1
    if n == 0:
        out = torch.zeros((cy, cx, 2, p, p), dtype=torch.float32, device=dev)
        counts = torch.zeros((cy, cx, 2), dtype=torch.int32, device=dev)
    else:
        _require_sorted(g, "averaged_time_surfaces")
        out = torch.empty((cy, cx, 2, p, p), dtype=torch.float32, device=dev)
        counts = torch.empty((cy, cx, 2), dtype=torch.int32, device=dev)
        nbytes = int(_lib.lib().evk_tsurf_scratch_bytes(n))
        t_run = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        _lib.call("evk_tsurf_hats", g.t_kind, D.ptr(g.t), n, g.h, g.w, cell, radius, tau, dt, 1 if normalise else 0,
                  D.ptr(g.scratch), D.ptr(t_run), nbytes, D.ptr(out), D.ptr(counts), D.stream())
    return (_result(a, out), _result(a, counts)) if return_counts else _result(a, out)
