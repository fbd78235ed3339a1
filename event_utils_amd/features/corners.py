"""Event corner detection on the device (evk_corner.hip; definitions: include/evk.h, "Corner detection", and DESIGN.md section 6):
the eFAST arc test (Mueggler, Bartolozzi, Scaramuzza, BMVC 2017) and the Harris score of a binary 9 x 9 patch (Vasco, Glover,
Bartolozzi, IROS 2016), event by event.  No reference module: upstream has no detector.  Both run on the grouping of the
denoising filters (_grouping.py, Grouped) and take the input kinds of the time surfaces: numpy in -> numpy out, device
tensors in -> device tensors out, a DeviceEvents in place of xs (the other columns None) -> device tensors.

polarity: "same" two classes (p > 0 and p <= 0), an event only sees its own; "ignore" one class, ps may be None.  "Earlier" means
a smaller stream index; the times may be unsorted.  An event closer than 4 pixels to the border of the sensor is never a corner
and has the Harris score NaN.  select: int64 indices of the M events wanted (any order, repeats allowed; IndexError outside
[0, n)); every event still forms the history.  The time stamps must be finite (-inf is the time of a pixel that has not fired);
what a NaN or an infinite stamp gives is not part of the contract."""
import torch

from .. import _device as D
from .. import _lib
from .._checks import check_int, check_number, check_polarity, check_time
from .._grouping import Grouped, kept, result
from ..util.event_util import _In


def _check_window(n_last, dt, what):
    """-> (window kind, n_last, dt) of evk_corner_harris; the parameter of the other window is a valid placeholder"""
    if (n_last is None) == (dt is None):
        raise TypeError("%s takes exactly one of n_last and dt" % what)
    if dt is not None:
        return _lib.EVK_CORNER_WINDOW_TIME, 1, check_time(dt, "dt")
    return _lib.EVK_CORNER_WINDOW_COUNT, check_int(n_last, "n_last", 1, must="an integer >= 1"), 0.0


def _fast_flags(g, sel, rows):
    out = torch.empty(rows, dtype=torch.uint8, device=g.dev)
    if rows:
        _lib.call("evk_corner_fast", *g.args(), D.ptr(sel), rows, D.ptr(g.scratch), D.ptr(out), D.stream())
    return out


def _harris(g, window, k, sel, rows):
    out = torch.empty(rows, dtype=torch.float32, device=g.dev)
    if rows:
        _lib.call("evk_corner_harris", *g.args(), *window, k, D.ptr(sel), rows, D.ptr(g.scratch), D.ptr(out), D.stream())
    return out


def fast_corners(xs, ys, ts, ps, sensor_size=(180, 240), polarity="same", select=None):
    """eFAST, bool (M,): event i is a corner iff it is off the border and, on the times v(q) of the last earlier event of its
    class at the pixels q of the two Bresenham circles around it (16 pixels at radius 3, 20 at radius 4; -inf where nothing
    fired), the inner circle has a contiguous arc of 3 .. 6 pixels and the outer one an arc of 4 .. 8 pixels whose values are all
    STRICTLY newer than every other pixel of the circle.  Exact: only comparisons of float64 times."""
    two, _ = check_polarity(polarity, ("same", "ignore"))
    a = _In(xs, ys, ts, ps)
    g = Grouped(a, sensor_size, two, "fast_corners")
    sel, rows = g.selection(select)
    return result(a, _fast_flags(g, sel, rows).to(torch.bool))


def harris_scores(xs, ys, ts, ps, sensor_size=(180, 240), n_last=None, dt=None, polarity="same", k=0.04, select=None):
    """The Harris score of every event, float32 (M,), NaN on the border: det(M) - k trace(M)^2 of the Gaussian-weighted structure
    tensor of 5 x 5 Sobel gradients (scaled by 1 / 12) of the binary 9 x 9 patch around the event: the centre is 1, another
    pixel is 1 iff the last earlier event of the event's class there is recent.  Exactly one of (TypeError otherwise):
      n_last  an integer >= 1: recent iff it is among the last n_last events of the stream (index >= i - n_last).  Vasco et al.
              keep one queue per polarity: with balanced polarities n_last here corresponds to about n_last / 2 there;
      dt      >= 0: recent iff t_i - t_j <= dt in float64."""
    two, _ = check_polarity(polarity, ("same", "ignore"))
    window = _check_window(n_last, dt, "harris_scores")
    k = check_number(k, "k")
    a = _In(xs, ys, ts, ps)
    g = Grouped(a, sensor_size, two, "harris_scores")
    sel, rows = g.selection(select)
    return result(a, _harris(g, window, k, sel, rows))


def harris_corners(xs, ys, ts, ps, sensor_size=(180, 240), n_last=None, dt=None, polarity="same", k=0.04, select=None,
                   threshold=8.0):
    """bool (M,): harris_scores(...) > threshold (NaN, the border, gives False)."""
    threshold = check_number(threshold, "threshold")
    scores = harris_scores(xs, ys, ts, ps, sensor_size=sensor_size, n_last=n_last, dt=dt, polarity=polarity, k=k, select=select)
    return scores > threshold


def corner_events(xs, ys, ts, ps, detector="fast", return_index=False, **detector_kwargs):
    """The events that are corners, in stream order, in the output kind of the denoising filters (the four columns; a DeviceEvents
    for a DeviceEvents).  detector "fast" (the arguments of fast_corners) or "harris" (those of harris_corners); neither takes
    `select` here.  return_index appends the int64 stream indices of the corners -- what local_time_surfaces(select=...) takes."""
    if detector not in ("fast", "harris"):
        raise ValueError("detector must be 'fast' or 'harris' (got %r)" % (detector,))
    allowed = ("sensor_size", "polarity") + (("n_last", "dt", "k", "threshold") if detector == "harris" else ())
    for name in detector_kwargs:
        if name not in allowed:
            raise TypeError("corner_events(detector=%r) got an unexpected argument %r" % (detector, name))
    kw = dict(detector_kwargs)
    two, _ = check_polarity(kw.get("polarity", "same"), ("same", "ignore"))
    size = kw.get("sensor_size", (180, 240))
    if detector == "harris":
        window = _check_window(kw.get("n_last"), kw.get("dt"), "corner_events(detector='harris')")
        k, threshold = check_number(kw.get("k", 0.04), "k"), check_number(kw.get("threshold", 8.0), "threshold")
    a = _In(xs, ys, ts, ps)
    g = Grouped(a, size, two, "corner_events")
    if detector == "fast":
        keep = _fast_flags(g, None, g.n)
    else:
        keep = (_harris(g, window, k, None, g.n) > threshold).to(torch.uint8)
    if not return_index:
        return kept(a, keep)
    out, index = kept(a, keep, want_index=True)
    index = result(a, index)
    return (out, index) if a.mode == "events" else tuple(out) + (index,)
