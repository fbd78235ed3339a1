"""Intensity reconstruction on the device (evk_reconstruct.hip; definitions: include/evk.h, "Intensity reconstruction", and
DESIGN.md section 6): the leaky event integrator (high-pass filter) and the complementary filter of Scheerlinck, Barnes & Mahony,
"Continuous-time Intensity Estimation Using Event Cameras" (ACCV 2018) -- a per-pixel estimate of the log intensity from the
events alone, or from the events and the latest frame.  No reference module: upstream reconstructs nothing.  Both run on the
grouping of the denoising filters (_grouping.py, Grouped, one class) and take the input kinds of the time surfaces: numpy
in -> numpy out, device tensors in -> device tensors out, a DeviceEvents in place of xs (the other columns None) -> device tensors.

Per pixel: L(t_start) = initial; between events dL/dt = -alpha (L - F(t)) with F the latest frame (0 without frames); at an event
with ts >= t_start, L += c_on if p > 0 else L -= c_off.  alpha is in 1 / unit of ts; alpha = 0 integrates without decay.  t_refs,
frame_ts and t_start are in the caller's time base (absolute times also for a DeviceEvents that stores its times relative to an
offset).  ts must be non-decreasing and finite (t_refs, frame_ts and t_start are refused unless finite; what a NaN or an infinite
event time gives is not part of the contract)."""
import math

import numpy as np
import torch

from .. import _device as D
from .. import _lib
from .._checks import check_gain, check_image, check_times, in_range, int_vector
from .._grouping import Grouped, polarity_flags, result, sensor_hw
from ..util.event_util import _In


def _reconstruct(what, xs, ys, ts, ps, alpha, sensor_size, t_refs, indices, c_on, c_off, initial, t_start, frames, frame_ts,
                 wave_run=0):
    # ---- everything that can be refused on the arguments alone
    alpha = check_gain(alpha, "alpha", True)
    c_on, c_off = check_gain(c_on, "c_on", False), check_gain(c_off, "c_off", False)
    h, w = sensor_hw(sensor_size)
    if (t_refs is None) == (indices is None):
        raise ValueError("%s takes exactly one of t_refs and indices" % what)
    if (frames is None) != (frame_ts is None):
        raise ValueError("%s takes frames and frame_ts together" % what)
    fts = None
    if frames is not None:
        frames = frames if isinstance(frames, torch.Tensor) else np.asarray(frames)
        fts = check_times(frame_ts, "frame_ts", True)
        if frames.ndim != 3 or len(fts) < 1:
            raise ValueError("frames must have shape (F, %d, %d) with F >= 1 (got %r)" % (h, w, tuple(frames.shape)))
        check_image(frames, (len(fts), h, w), "frames")
    if initial is not None:
        initial = check_image(initial if isinstance(initial, torch.Tensor) else np.asarray(initial), (h, w), "initial")
    if t_start is not None:
        t_start = float(t_start)
        if not math.isfinite(t_start):
            raise ValueError("t_start must be finite (got %r)" % t_start)
    elif fts is not None:
        t_start = float(fts[0])
    refs = cuts = None
    if t_refs is not None:
        refs = check_times(t_refs, "t_refs", False)
        if len(refs) < 1:
            raise ValueError("%s needs at least one query" % what)
        if t_start is not None and refs[0] < t_start:
            raise ValueError("a query lies before t_start (%r < %r)" % (float(refs[0]), t_start))
    else:
        cuts = int_vector(indices, "indices", ValueError)
        if cuts.numel() < 1:
            raise ValueError("%s needs at least one query" % what)
        if cuts.numel() > 1 and bool((cuts[1:] < cuts[:-1]).any()):
            raise ValueError("indices must be non-decreasing")
    # ---- the events
    a = _In(xs, ys, ts, ps)
    if a.cols[3] is None:
        raise TypeError("%s needs ps" % what)
    g = Grouped(a, (h, w), False, what)
    n, dev = g.n, g.dev
    g.require_sorted(what)
    off = a.ev.t_offset if a.ev is not None else 0.0       # the column's zero in the caller's time base
    if t_start is not None:
        t_start -= off
    if fts is not None:
        fts = fts - off
    first = None
    if n and t_start is None:                      # the default start of the high-pass filter: the first event
        first = a.ev.t_at(0) if a.ev is not None else float(g.t[0].item())
    if refs is not None:
        refs = refs - off
        if t_start is None:                        # (no frames) the first event, else the first query
            t_start = first if n else float(refs[0])
            if refs[0] < t_start:
                raise ValueError("a query lies before the first event, the default t_start (%r < %r)" % (float(refs[0] + off),
                                                                                                       t_start + off))
        keys = torch.from_numpy(np.append(refs, t_start)).to(dev)       # the cuts of the queries and of t_start in one search
        found = g.cuts_before(keys)
        cuts, start_cut = found[:-1].contiguous(), int(found[-1].item())
        t_k = keys[:-1].contiguous()
    else:
        if not in_range(cuts, 0, n):
            raise IndexError("indices must lie in 0 .. %d" % n)
        if t_start is None:
            t_start = first if n else 0.0
        cuts = cuts.to(dev)
        start_cut = 0
        if n:
            key = torch.tensor([t_start], dtype=torch.float64, device=dev)
            start_cut = int(g.cuts_before(key).item())
            t_k = torch.where(cuts > 0, g.t[(cuts - 1).clamp(min=0)].to(torch.float64), key)      # T_k = ts[m_k - 1]; t_start at 0
        else:
            t_k = torch.full((int(cuts.shape[0]),), t_start, dtype=torch.float64, device=dev)
        if float(t_k.min().item()) < t_start:
            raise ValueError("a query lies before t_start")
    # ---- polarity (a negative p_scale of a DeviceEvents turns it round), frames and the start state
    pos = polarity_flags(a) if n else None
    nf, dframes, dfts = 0, None, None
    if frames is not None:
        nf, dframes, dfts = len(fts), D.resident(frames, dev, torch.float64), torch.from_numpy(np.ascontiguousarray(fts)).to(dev)
    dinitial = D.resident(initial, dev, torch.float64) if initial is not None else (dframes[0] if nf else None)
    scratch = g.scratch if n else torch.empty(256, dtype=torch.uint8, device=dev)
    nq = int(cuts.shape[0])
    out = torch.empty((nq, h, w), dtype=torch.float32, device=dev)
    _lib.call("evk_reconstruct", g.t_kind if n else _lib.EVK_SELECT_F64, D.ptr(g.t) if n else None, D.ptr(pos), n, h, w, alpha,
              c_on, c_off, t_start, D.ptr(dinitial), nf, D.ptr(dframes), D.ptr(dfts), nq, D.ptr(cuts), D.ptr(t_k), start_cut,
              int(wave_run), D.ptr(scratch), D.ptr(out), D.stream())
    return result(a, out)


def leaky_integrator(xs, ys, ts, ps, alpha, sensor_size=(180, 240), t_refs=None, indices=None, c_on=0.1, c_off=0.1, initial=None,
                     t_start=None):
    """The high-pass filter: the leaky integral of the events at K queries, float32 (K, H, W).  L[k, y, x] = initial[y, x]
    exp(-alpha (T_k - t_start)) + the sum of c_j exp(-alpha (T_k - ts_j)) over the events j of the pixel with ts_j >= t_start
    before the query's cut, c_j = c_on for p_j > 0 and -c_off otherwise.  Exactly one of:
      t_refs   K non-decreasing absolute times T_k >= t_start: the events with ts < T_k count (an event at exactly T_k does not);
      indices  K non-decreasing cuts m_k in 0 .. n: the first m_k events count and T_k = ts[m_k - 1] (t_start for m_k = 0).
    initial: (H, W), default zeros; t_start: default ts[0] (the first query when there are no events).  ValueError for a negative
    alpha, a contrast that is not positive, unsorted ts or queries, a query before t_start or a wrong shape.
    Streaming: a reconstruction continues across windows when the next call gets initial=out[-1] and t_start=the last query
    time T_K of this one; the hand-over through float32 adds at most 2^-24 |out[-1]|, decayed like the state itself."""
    return _reconstruct("leaky_integrator", xs, ys, ts, ps, alpha, sensor_size, t_refs, indices, c_on, c_off, initial, t_start,
                        None, None)


def complementary_filter(xs, ys, ts, ps, alpha, frames, frame_ts, sensor_size=(180, 240), t_refs=None, indices=None, c_on=0.1,
                         c_off=0.1, initial=None, t_start=None):
    """The complementary filter: the leaky integrator pulled towards the latest frame with the same time constant, float32
    (K, H, W).  frames: (F, H, W) in the LOG domain (log_intensity), converted to float64 on the device; frame_ts: F strictly
    increasing absolute times.  The target is frames[f] from frame_ts[f] until frame_ts[f + 1]; frames[0] also holds before
    frame_ts[0].  Between events dL/dt = -alpha (L - target); alpha = 0 leaves the frames without influence.  initial defaults
    to frames[0] and t_start to frame_ts[0]; the other arguments, the errors and the streaming hand-over (initial=out[-1],
    t_start=T_K, the same frames) are those of leaky_integrator."""
    if frames is None or frame_ts is None:
        raise ValueError("complementary_filter needs frames and frame_ts")
    return _reconstruct("complementary_filter", xs, ys, ts, ps, alpha, sensor_size, t_refs, indices, c_on, c_off, initial,
                        t_start, frames, frame_ts)


def log_intensity(frames, eps=1e-3):
    """log(I + eps) in float64: intensity frames (8-bit frames of the datasets included) -> the log domain the filters work in.
    numpy in -> numpy out, a tensor in -> a tensor on its device."""
    if isinstance(frames, torch.Tensor):
        return torch.log(frames.to(torch.float64) + eps)
    return torch.log(torch.from_numpy(np.ascontiguousarray(frames)).to(torch.float64) + eps).numpy()


def to_intensity(log_image, eps=1e-3):
    """The inverse of log_intensity: exp(L) - eps, in the floating dtype of the input (float64 for other dtypes)."""
    if isinstance(log_image, torch.Tensor):
        v = log_image if log_image.is_floating_point() else log_image.to(torch.float64)
        return torch.exp(v) - eps
    v = torch.from_numpy(np.ascontiguousarray(log_image))
    return (torch.exp(v if v.is_floating_point() else v.to(torch.float64)) - eps).numpy()
