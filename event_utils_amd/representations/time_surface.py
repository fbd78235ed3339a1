"""Time surfaces on the device (evk_tsurf.hip; definitions: include/evk.h, "Time surfaces", and DESIGN.md section 6): the decayed
surface of active events at one or more queries, the per-event local time surfaces of HOTS (Lagorce et al., PAMI 2017) and the
cell-averaged histograms of HATS (Sironi et al., CVPR 2018).  No reference module: upstream has none of them.  All three run on
the grouping of the denoising filters (_grouping.py, Grouped) and take their input kinds: numpy in -> numpy out, device
tensors in -> device tensors out, a DeviceEvents in place of xs (the other columns None) -> device tensors.

decay: "exp" (float)exp(-age / tau), "linear" (float)max(0, 1 - age / tau), None the float64 age itself; an age is +inf where no
earlier event exists or the pixel lies off the sensor (values 0, 0 and inf).  polarity: "ignore" one class; "same" two classes
and only the event's own (one channel); "split" two classes, channel 0 p <= 0 and channel 1 p > 0.  The time stamps must be
finite (an infinite age is the mark of "no earlier event"); what a NaN or an infinite stamp gives is not part of the contract."""
import numpy as np
import torch

from .. import _device as D
from .. import _lib
from .._checks import check_decay, check_int, check_polarity, check_time, in_range, int_vector
from .._grouping import Grouped, result
from ..util.event_util import _In


def _out_dtype(decay):
    return torch.float64 if decay == _lib.EVK_TSURF_AGE else torch.float32


def _empty_value(decay):
    return float("inf") if decay == _lib.EVK_TSURF_AGE else 0.0


def time_surfaces(xs, ys, ts, ps, tau, sensor_size=(180, 240), t_refs=None, indices=None, decay="exp", polarity="split"):
    """The surface of active events at K queries, (K, C, H, W): S[k, c, y, x] = value(T_k - t of the last event of class c at
    (x, y) among the first m_k events).  Exactly one of:
      t_refs   K absolute times (the caller's time base): T_k = t_refs[k], m_k = the number of events with t < T_k; ts must be
               non-decreasing (ValueError otherwise);
      indices  K cuts m_k in 0 .. n: T_k = ts[m_k - 1]; the times may be unsorted; m_k = 0 gives an empty surface.
    polarity "split" (C = 2) or "ignore" (C = 1, ps may be None)."""
    return result(*_surfaces(xs, ys, ts, ps, tau, sensor_size, t_refs, indices, decay, polarity))


def _surfaces(xs, ys, ts, ps, tau, sensor_size, t_refs, indices, decay, polarity):
    """time_surfaces up to the kind of its result -> (the call's inputs, the surfaces on the device)"""
    decay, tau = check_decay(decay, tau)
    two, _ = check_polarity(polarity, ("split", "ignore"))
    if (t_refs is None) == (indices is None):
        raise TypeError("time_surfaces takes exactly one of t_refs and indices")
    a = _In(xs, ys, ts, ps)
    g = Grouped(a, sensor_size, two, "time_surfaces")
    n, dev = g.n, g.dev
    refs = None
    if indices is not None:
        cuts = int_vector(indices, "indices", TypeError)
        if not in_range(cuts, 0, n):
            raise IndexError("indices must lie in 0 .. %d" % n)
        cuts = cuts.to(dev)
    else:
        host = t_refs.detach().cpu().numpy() if isinstance(t_refs, torch.Tensor) else np.asarray(t_refs)
        keys = host.astype(np.float64).reshape(-1) - (a.ev.t_offset if a.ev is not None else 0.0)
        refs = torch.from_numpy(np.ascontiguousarray(keys)).to(dev)
        g.require_sorted("time_surfaces with t_refs")
        cuts = g.cuts_before(refs)
    nq = int(cuts.shape[0])
    if nq < 1:
        raise ValueError("time_surfaces needs at least one query")
    shape = (nq, g.classes, g.h, g.w)
    if n == 0:
        return a, torch.full(shape, _empty_value(decay), dtype=_out_dtype(decay), device=dev)
    out = torch.empty(shape, dtype=_out_dtype(decay), device=dev)
    _lib.call("evk_tsurf_global", *g.args(), nq, D.ptr(cuts), D.ptr(refs), decay, tau, D.ptr(g.scratch), D.ptr(out), D.stream())
    return a, out


def local_time_surfaces(xs, ys, ts, ps, tau, sensor_size=(180, 240), radius=3, decay="exp", polarity="same", include_self=True,
                        select=None):
    """The local time surface of every event (HOTS), (M, C, 2 radius + 1, 2 radius + 1): element (c, dy, dx) of event i is the
    value of t_i - t of the last EARLIER event (smaller stream index) of class c at (x_i + dx, y_i + dy).  include_self puts age
    0 (value 1) at the centre of the event's own class; without it the centre is the pixel's previous event.  select: int64
    indices of the M events wanted (any order, repeats allowed; IndexError outside [0, n)); every event still forms the history.
    float32, float64 for decay=None.  The times may be unsorted."""
    decay, tau = check_decay(decay, tau)
    two, split = check_polarity(polarity, ("same", "split", "ignore"))
    radius = check_int(radius, "radius", 1, _lib.EVK_TSURF_MAX_RADIUS)
    a = _In(xs, ys, ts, ps)
    g = Grouped(a, sensor_size, two, "local_time_surfaces")
    n, dev = g.n, g.dev
    sel, rows = g.selection(select)
    p = 2 * radius + 1
    out = torch.empty((rows, 2 if split else 1, p, p), dtype=_out_dtype(decay), device=dev)
    if rows:
        _lib.call("evk_tsurf_local", *g.args(), radius, decay, tau, split,
                  1 if include_self else 0, D.ptr(sel), rows, D.ptr(g.scratch), D.ptr(out), D.stream())
    return result(a, out)


def averaged_time_surfaces(xs, ys, ts, ps, tau, dt, sensor_size=(180, 240), cell_size=10, radius=3, normalise=True,
                           return_counts=False):
    """The HATS histograms, (Cy, Cx, 2, 2 radius + 1, 2 radius + 1) float32 with Cy = ceil(H / cell_size), Cx = ceil(W / cell_size):
    h[g, q, z] = the sum over the events i of class q (p > 0) in cell g of the sum of exp(-(t_i - t_j) / tau) over the earlier
    events j of class q at pixel_i + z -- a pixel of the sensor and of the SAME cell -- with t_i - t_j <= dt; with normalise
    divided by the number of events of (g, q).  ts must be non-decreasing (ValueError).  return_counts appends the (Cy, Cx, 2)
    int32 event counts."""
    _, tau = check_decay("exp", tau)
    dt, radius = check_time(dt, "dt"), check_int(radius, "radius", 1, _lib.EVK_TSURF_MAX_RADIUS)
    cell_size = check_int(cell_size, "cell_size", 1, must="a positive integer")
    a = _In(xs, ys, ts, ps)
    g = Grouped(a, sensor_size, True, "averaged_time_surfaces")
    n, dev = g.n, g.dev
    cell = min(int(cell_size), max(g.h, g.w))
    cy, cx, p = -(-g.h // cell), -(-g.w // cell), 2 * radius + 1
    if n == 0:
        out = torch.zeros((cy, cx, 2, p, p), dtype=torch.float32, device=dev)
        counts = torch.zeros((cy, cx, 2), dtype=torch.int32, device=dev)
    else:
        g.require_sorted("averaged_time_surfaces")
        out = torch.empty((cy, cx, 2, p, p), dtype=torch.float32, device=dev)
        counts = torch.empty((cy, cx, 2), dtype=torch.int32, device=dev)
        nbytes = int(_lib.lib().evk_tsurf_scratch_bytes(n))
        t_run = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=dev)
        _lib.call("evk_tsurf_hats", *g.args()[:5], cell, radius, tau, dt, 1 if normalise else 0,
                  D.ptr(g.scratch), D.ptr(t_run), nbytes, D.ptr(out), D.ptr(counts), D.stream())
    return (result(a, out), result(a, counts)) if return_counts else result(a, out)
