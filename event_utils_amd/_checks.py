"""Argument checks of the per-pixel grouping family (denoising, time surfaces, corners, plane-fit flow, reconstruction), of the
simulator and of the depth package: pure functions of the caller's values that need neither the library nor the events, so
that every refusal comes before any device work."""
import math

import numpy as np
import torch

from . import _lib

_DECAY = {"exp": _lib.EVK_TSURF_EXP, "linear": _lib.EVK_TSURF_LINEAR, None: _lib.EVK_TSURF_AGE}
_ARRAY = {torch.uint8: np.dtype(np.uint8), torch.int32: np.dtype(np.int32), torch.float32: np.dtype(np.float32)}
_POLARITY = {"ignore": (False, 0), "same": (True, 0), "split": (True, 1)}      # -> (two classes in the grouping, split channels)


def check_time(value, what):
    value = float(value)
    if not value >= 0.0:                       # (also NaN)
        raise ValueError("%s must be >= 0 (got %r)" % (what, value))
    return value


def check_int(value, what, lo, hi=None, must=None):
    """An integer in lo .. hi (hi None: no upper limit, and `must` words the rule); a bool is not one.  must: default 'lo .. hi'."""
    if isinstance(value, bool) or int(value) != value or int(value) < lo or (hi is not None and int(value) > hi):
        raise ValueError("%s must be %s (got %r)" % (what, must or "%d .. %d" % (lo, hi), value))
    return int(value)


def check_polarity(polarity, allowed):
    if polarity not in allowed:
        raise ValueError("polarity must be one of %s (got %r)" % (", ".join(repr(p) for p in allowed), polarity))
    return _POLARITY[polarity]


def check_decay(decay, tau):
    if decay not in _DECAY:
        raise ValueError("decay must be 'exp', 'linear' or None (got %r)" % (decay,))
    tau = float(tau)
    if not tau > 0.0:                          # (also NaN)
        raise ValueError("tau must be > 0 (got %r)" % tau)
    return _DECAY[decay], tau


def check_positive(value, what):
    """-> (used, value) of an optional parameter that is > 0 when given"""
    if value is None:
        return 0, 0.0
    value = float(value)
    if not value > 0.0:                        # (also NaN)
        raise ValueError("%s must be > 0 or None (got %r)" % (what, value))
    return 1, value


def check_gain(value, what, zero_ok):
    value = float(value)
    if not (math.isfinite(value) and (value >= 0.0 if zero_ok else value > 0.0)):
        raise ValueError("%s must be finite and %s 0 (got %r)" % (what, ">=" if zero_ok else ">", value))
    return value


def check_number(value, what):
    value = float(value)
    if value != value:
        raise ValueError("%s must not be NaN" % what)
    return value


def int_vector(v, what, exc):
    """A caller's index vector as a 1-D int64 tensor (on the host or the device, wherever it was)."""
    if not isinstance(v, torch.Tensor):
        v = np.asarray(v)
        v = torch.from_numpy(np.ascontiguousarray(v if v.size else v.astype(np.int64)))
    if v.dim() > 1 or (v.numel() and (v.is_floating_point() or v.is_complex() or v.dtype == torch.bool)):
        raise exc("%s must be a vector of integers" % what)
    return v.reshape(-1).to(torch.int64)


def in_range(v, lo, hi):
    return v.numel() == 0 or (int(v.min()) >= lo and int(v.max()) <= hi)


def host_f64(v):
    return (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float64)


def check_times(v, what, strict):
    """A caller's vector of times as float64 on the host: finite and non-decreasing (increasing with `strict`)."""
    v = host_f64(v).reshape(-1)
    if not np.isfinite(v).all():
        raise ValueError("%s must be finite" % what)
    d = np.diff(v)
    if (d <= 0).any() if strict else (d < 0).any():
        raise ValueError("%s must be %s" % (what, "strictly increasing" if strict else "non-decreasing"))
    return v


def check_image(v, shape, what):
    """A caller's image stack: its shape checked on the host; -> float64 on the device by _device.resident."""
    if tuple(v.shape) != tuple(shape):
        raise ValueError("%s must have shape %r (got %r)" % (what, tuple(shape), tuple(v.shape)))
    return v


def check_array(v, what, dtype, source):
    """A tensor or numpy array of `dtype` (a torch dtype), as the call `source` returns it -> its shape.  The shape's rules are
    the caller's."""
    if not isinstance(v, (torch.Tensor, np.ndarray)):
        name = _ARRAY[dtype].name
        raise TypeError("%s must be %s %s tensor or array (got %s)" % (what, "an" if name[0] == "i" else "a", name, type(v).__name__))
    if v.dtype not in (dtype, _ARRAY[dtype]):
        raise TypeError("%s must be %s, as %s returns it (got %s)" % (what, _ARRAY[dtype].name, source, v.dtype))
    return tuple(v.shape)
