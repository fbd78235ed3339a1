"""Reference: lib/augmentation/event_augmentation.py.  The ten public functions with the reference's names, positional order and
defaults; the functions that draw random numbers take a trailing keyword-only `seed`.  Inputs follow the filters
(util/event_util.py): numpy columns in -> numpy columns out, device tensors in -> device tensors out, a DeviceEvents in place of
xs (the other columns None) -> a new DeviceEvents.

add_random_events, remove_events and add_correlated_events run on the device (evk_augment.hip, evk_select.hip).  Their per-event
draws come from a counter-based Philox4x32-10 generator keyed by `seed` (seed=None takes one 63-bit integer from np.random, so
np.random.seed makes a run repeatable), so their results match the reference IN DISTRIBUTION, not value for value: numpy's
Mersenne stream is not reproduced.  The same seed gives the same generated events for every sort / return_merged combination.
Everything else is exact: the dtypes, the sizes, the order of every merged or sorted result (numpy's
view('i8,i8,i8,i8').sort(order=['f2']): by the int64 bit patterns of t, then x, y, p), and the host scalars of sample and
rotate_events, drawn with the reference's numpy calls in the reference's order.  flip_*, crop_events, rotate_events,
events_to_block, merge_events and sample are element-wise numpy / torch plumbing."""
import numpy as np
import torch

from .. import _device as D
from .. import _lib
from ..events import DeviceEvents
from ..util import event_util as EU
from ..util.event_util import clip_events_to_bounds

_U32 = 1 << 32


def _seed(seed):
    if seed is None:
        return int(np.random.randint(0, 2 ** 63, dtype=np.int64))
    return int(seed) % (1 << 64)


# ---- columns ---------------------------------------------------------------------------------------------------------------

class _Cols:
    """The four columns of a call (event_util._In), with their native-kind views and absolute float64 copies on demand."""

    def __init__(self, xs, ys, ts, ps):
        self.a = EU._In(xs, ys, ts, ps)
        if any(c is None for c in self.a.cols):
            raise TypeError("xs, ys, ts and ps are all needed")
        self.mode, self.ev = self.a.mode, self.a.ev
        self.dev = self.a.cols[0].device
        self.n = int(self.a.cols[0].shape[0])
        self._f64 = None

    def native(self, i):
        """(column, EVK_SELECT_* kind) holding the values of column i (a DeviceEvents' time absolute)."""
        if self.mode == "events":
            return self.f64()[i], _lib.EVK_SELECT_F64
        return self.a.pred(i)

    def f64(self):
        """The four columns as float64, as numpy's astype(float64) gives them (DeviceEvents: absolute t, p times p_scale)."""
        if self._f64 is None:
            if self.mode == "events":
                ev = self.ev
                t = ev.t.to(torch.float64)
                if ev.t_offset != 0.0:
                    t = t + ev.t_offset
                p = ev.p.to(torch.float64)
                if ev.p_scale != 1.0:
                    p = p * ev.p_scale
                self._f64 = [ev.x.to(torch.float64), ev.y.to(torch.float64), t, p]
            else:
                self._f64 = [self.a.pred(i)[0].to(torch.float64) for i in range(4)]
        return self._f64


def _out(mode, cols):
    """Device columns -> the caller's kind: numpy arrays, tensors, or a DeviceEvents (float64)."""
    if mode == "numpy":
        return tuple(c.cpu().numpy() for c in cols)
    if mode == "events":
        return DeviceEvents(*[c.to(torch.float64).contiguous() for c in cols])
    return tuple(cols)


def _empty4(dev, n=0):
    return [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(4)]


# ---- device steps -------------------------------------------------------------------------------------------------------------

def _bounds(c):
    """max(xs), max(ys), min(ts), max(ts) as a device float64[4] (one reduction).  numpy's max of an empty array raises."""
    if c.n == 0:
        raise ValueError("zero-size array to reduction operation maximum which has no identity")
    (px, kx), (py, ky), (pt, kt) = c.native(0), c.native(1), c.native(2)
    out = torch.empty(4, dtype=torch.float64, device=c.dev)
    L = _lib.lib()
    sb = int(L.evk_augment_bounds_scratch_bytes())
    scratch = torch.empty(sb, dtype=torch.uint8, device=c.dev)
    _lib.call("evk_augment_bounds", kx, D.ptr(px), ky, D.ptr(py), kt, D.ptr(pt), c.n, D.ptr(out), D.ptr(scratch), sb, D.stream())
    return out


def _check_bounds(bounds, m):
    """Raise where numpy's randint(max + 1, size=m) / uniform(min(ts), max(ts), size=m) raise (bounds read back once)."""
    mx, my, tlo, thi = (float(v) for v in bounds.cpu().tolist())
    for v in (mx, my):
        h = v + 1.0
        if m <= 0:
            break                      # numpy's randint(high, size=0) checks nothing: randint(-2, size=0) is []
        if h != h:
            raise ValueError("cannot convert float NaN to integer")
        elif h in (float("inf"), float("-inf")):
            raise OverflowError("cannot convert float infinity to integer")
        elif int(h) <= 0:
            raise ValueError("high <= 0")
        elif int(h) > 2 ** 63:
            raise ValueError("high is out of bounds for int64")
    if not np.isfinite(thi - tlo):
        raise OverflowError("Range exceeds valid bounds")


def _random_into(seed, bounds, m, cols):
    """m random events into the four device columns `cols` (int64 x, y, p or float64 x, y, p; float64 t)."""
    kind = _lib.EVK_SELECT_I64 if cols[0].dtype == torch.int64 else _lib.EVK_SELECT_F64
    _lib.call("evk_random_events", seed, D.ptr(bounds), m, kind, *(D.ptr(o) for o in cols), D.stream())


def _sort(cols):
    """Four float64 device columns -> the same events in numpy's view('i8,i8,i8,i8').sort(order=['f2']) order."""
    cols = [c.contiguous() for c in cols]
    n = int(cols[0].shape[0])
    dev = cols[0].device
    outs = _empty4(dev, n)
    L = _lib.lib()
    sb = int(L.evk_sort_events_scratch_bytes(n))
    if sb < 0:
        raise ValueError("the sort takes fewer than 2^31 events (%d)" % n)
    scratch = torch.empty(max(sb, 1), dtype=torch.uint8, device=dev)
    bits = np.zeros(1, dtype=np.int32)
    _lib.call("evk_sort_events_f64", *(D.ptr(c) for c in cols), n, *(D.ptr(o) for o in outs), D.ptr(scratch), sb,
              D.host_ptr(bits), D.stream())
    return outs


def _subset(seed, purpose, n, k, dev, payload=(), want_index=False, t_col=-1):
    """A uniform k-subset of n candidates in stream order: (kept payload columns, kept indices or None, compaction result)."""
    if n >= _U32:
        raise ValueError("a uniform subset takes fewer than 2^32 candidates (%d)" % n)
    L = _lib.lib()
    hb = int(L.evk_hot_pixels_scratch_bytes())
    state = torch.empty(hb, dtype=torch.uint8, device=dev)
    _lib.call("evk_random_subset", seed, purpose, n, k, D.ptr(state), hb, D.stream())
    outs = [torch.empty(max(k, 1), dtype=c.dtype, device=dev) for c in payload]   # (EVK_SELECT_RANDOM writes no position >= k)
    index = torch.empty(max(k, 1), dtype=torch.int64, device=dev) if want_index else None
    nbytes = int(L.evk_select_scratch_bytes(n))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    result = torch.zeros(3, dtype=torch.int64, device=dev)
    src = np.array([c.data_ptr() for c in payload], dtype=np.uint64)
    dst = np.array([o.data_ptr() for o in outs], dtype=np.uint64)
    eb = np.array([c.element_size() for c in payload], dtype=np.int32)
    _lib.call("evk_select_compact", _lib.EVK_SELECT_RANDOM, _lib.EVK_SELECT_I64, None, None, n, None, D.ptr(state), 0, 0,
              len(payload), D.host_ptr(src) if payload else None, D.host_ptr(dst) if payload else None,
              D.host_ptr(eb) if payload else None, t_col, D.ptr(index), D.ptr(result), D.ptr(scratch), nbytes, None, D.stream())
    return [o[:k] for o in outs], (None if index is None else index[:k]), result


# ---- the public functions ----------------------------------------------------------------------------------------------------

def sample(cdf, ts, *, seed=None):
    """Reference :8-22.  rnd = np.random.uniform(cdf[0], cdf[-1]) on the host (exactly the reference's draw; a given `seed` seeds a
    private numpy RandomState instead of the global one), then the index of searchsorted(ts, rnd) (torch.searchsorted for a
    tensor, compared in the dtype numpy compares in)."""
    rng = np.random if seed is None else np.random.RandomState(seed % (1 << 32))
    c0, c1 = (float(cdf[0]), float(cdf[-1])) if isinstance(cdf, torch.Tensor) else (cdf[0], cdf[-1])
    rnd = rng.uniform(c0, c1)
    if isinstance(ts, torch.Tensor):
        # numpy compares in np.result_type(ts, rnd): float32 for float32 stamps, float64 for integer ones
        rt = _T_OF_NP[np.dtype(np.result_type(np.empty(0, dtype=EU._NP_OF[ts.dtype]), rnd))]
        return int(torch.searchsorted(ts.to(rt), torch.tensor([rnd], dtype=rt, device=ts.device))[0])
    return np.searchsorted(ts, rnd)


def events_to_block(xs, ys, ts, ps):
    """Reference :24-40: the (N, 4) block [x, y, t, p] in the promoted dtype (numpy or torch)."""
    if isinstance(xs, torch.Tensor):
        cols = (xs, ys, ts, ps)
        dt = cols[0].dtype
        for c in cols[1:]:
            dt = torch.promote_types(dt, c.dtype)
        return torch.stack([c.to(dt) for c in cols], dim=1)
    return np.concatenate((xs[:, np.newaxis], ys[:, np.newaxis], ts[:, np.newaxis], ps[:, np.newaxis]), axis=1)


def merge_events(event_sets):
    """Reference :42-60: the event sets concatenated into one (N, 4) block."""
    cols = [[e[k] for e in event_sets] for k in range(4)]
    if isinstance(cols[0][0], torch.Tensor):
        return events_to_block(*[torch.cat(c) for c in cols])
    return events_to_block(*[np.concatenate(c) for c in cols])


def _merged(parts, dev):
    """Concatenation of column sets (each four device columns) as four float64 columns."""
    return [torch.cat([p[k].to(torch.float64) for p in parts]) if parts else torch.empty(0, dtype=torch.float64, device=dev)
            for k in range(4)]


def add_random_events(xs, ys, ts, ps, to_add, sensor_resolution=None, sort=True, return_merged=True, *, seed=None):
    """Reference :62-92.  to_add events with x uniform in [0, max(xs)], y in [0, max(ys)] (sensor_resolution is ignored, as
    there), t uniform in [min(ts), max(ts)), p = +-1 -- drawn on the device (in distribution, see the module doc).
    return_merged: the new events followed by the originals, float64; sort: in the reference's order (float64).  Neither: the
    new events alone as int64 x, y, p and float64 t.  Errors as numpy's (empty input, NaN bounds)."""
    c = _Cols(xs, ys, ts, ps)
    s = _seed(seed)
    m = int(to_add)
    bounds = _bounds(c)
    if m < 0:
        raise ValueError("negative dimensions are not allowed")
    typed = not sort and not return_merged
    new = [torch.empty(m, dtype=torch.float64 if (typed and k == 2) or not typed else torch.int64, device=c.dev)
           for k in range(4)]
    _random_into(s, bounds, m, new)
    _check_bounds(bounds, m)
    if typed:
        return _out(c.mode, new)
    cols = _merged([new, c.f64()], c.dev) if return_merged else new
    return _out(c.mode, _sort(cols) if sort else cols)


def remove_events(xs, ys, ts, ps, to_remove, add_noise=0, *, seed=None):
    """Reference :94-116.  Keeps a uniform subset of exactly n - to_remove events in stream order, in the input dtypes (the
    device's radix select of the n - to_remove smallest Philox keys, then an order-preserving compaction).  to_remove > n gives
    four empty float64 arrays; to_remove < 0 raises ValueError as numpy does.  add_noise > 0: that many random events drawn from
    the whole input are merged in and the result is sorted, float64."""
    c = _Cols(xs, ys, ts, ps)
    s = _seed(seed)
    n, to_remove, add_noise = c.n, int(to_remove), int(add_noise)
    if to_remove > n:
        e = _empty4(c.dev)
        return (DeviceEvents(*e) if c.mode == "events" else _out(c.mode, e))
    k = n - to_remove
    if k > n:
        raise ValueError("Cannot take a larger sample than population when 'replace=False'")
    if add_noise <= 0:
        kept, _, result = _subset(s, _lib.EVK_PHILOX_SUBSET, n, k, c.dev, payload=c.a.cols, t_col=2)
        if c.mode == "events":
            return EU._events_result(c.ev, kept, [int(v) for v in result.cpu().tolist()])
        return EU._columns_out(c.mode, kept, c.a.dts)
    kept, _, _ = _subset(s, _lib.EVK_PHILOX_SUBSET, n, k, c.dev, payload=c.f64())
    bounds = _bounds(c)
    noise = _empty4(c.dev, add_noise)
    _random_into(s, bounds, add_noise, noise)
    _check_bounds(bounds, add_noise)
    return _out(c.mode, _sort(_merged([kept, noise], c.dev)))


def add_correlated_events(xs, ys, ts, ps, to_add, sort=True, return_merged=True, xy_std=1.5, ts_std=0.001, add_noise=0, *,
                          seed=None):
    """Reference :118-157.  iters = int(to_add / n) + 1 jittered copies of the stream are the candidates; to_add of them are
    chosen without replacement (a uniform subset of the iters * n candidates, fewer than 2^32), each one's x, y moved by a
    normal(xy_std) truncated toward zero and clipped to [0, max(xs)] / [0, max(ys)], t by a normal(ts_std), p kept.
    return_merged: followed by add_noise random events (the originals are NOT included, as in the reference); sort: the
    reference's order.  Always float64.  Unsorted, the chosen events come in candidate order (copy, then stream position)
    where the reference's come in random order.  A NaN coordinate (or bound) gives NaN, as np.clip does."""
    c = _Cols(xs, ys, ts, ps)
    s = _seed(seed)
    n, to_add, add_noise = c.n, int(to_add), int(add_noise)
    iters = int(to_add / n) + 1
    if to_add < 0:
        raise ValueError("negative dimensions are not allowed")
    bounds = _bounds(c)
    f = c.f64()
    _, sel, _ = _subset(s, _lib.EVK_PHILOX_CORR_CHOICE, iters * n, to_add, c.dev, want_index=True)
    new = _empty4(c.dev, to_add)
    _lib.call("evk_correlated_events", s, *(D.ptr(x) for x in f), n, D.ptr(sel), to_add, float(xy_std), float(ts_std),
              D.ptr(bounds), *(D.ptr(o) for o in new), D.stream())
    noise = _empty4(c.dev, add_noise)
    _random_into(s, bounds, add_noise, noise)
    _check_bounds(bounds, add_noise)
    cols = _merged([new, noise], c.dev) if return_merged else new
    return _out(c.mode, _sort(cols) if sort else cols)


def flip_events_x(xs, ys, ts, ps, sensor_resolution=(180, 240)):
    """Reference :159-170: xs = W - xs (not W - 1 - xs)."""
    if isinstance(xs, DeviceEvents):
        return _replace(xs, x=sensor_resolution[1] - xs.x)
    return sensor_resolution[1] - xs, ys, ts, ps


def flip_events_y(xs, ys, ts, ps, sensor_resolution=(180, 240)):
    """Reference :172-183: ys = H - ys."""
    if isinstance(xs, DeviceEvents):
        return _replace(xs, y=sensor_resolution[0] - xs.y)
    return xs, sensor_resolution[0] - ys, ts, ps


def _replace(ev, x=None, y=None):
    out = DeviceEvents(ev.x if x is None else x, ev.y if y is None else y, ev.t, ev.p)
    out.t_offset, out.p_scale, out._t_ends = ev.t_offset, ev.p_scale, ev._t_ends
    return out


def crop_events(xs, ys, sensor_resolution, new_resolution):
    """Reference :185-193: clip_events_to_bounds(xs, ys, None, None, new_resolution) -> xs, ys (a DeviceEvents: the cropped
    DeviceEvents)."""
    clip = clip_events_to_bounds(xs, ys, None, None, new_resolution)
    if isinstance(clip, DeviceEvents):
        return clip
    return clip[0], clip[1]


_T_OF_NP = {np.dtype(k): v for k, v in ((np.float16, torch.float16), (np.float32, torch.float32), (np.float64, torch.float64),
                                         (np.int8, torch.int8), (np.int16, torch.int16), (np.int32, torch.int32),
                                         (np.int64, torch.int64), (np.uint8, torch.uint8))}


def rotate_events(xs, ys, sensor_resolution=(180, 240), theta_radians=None, center_of_rotation=None, clip_to_range=False):
    """Reference :195-222, formula kept as written: new = (cx cos - cy sin) + cx with cx = x - centre (a true rotation would add
    the centre back).  theta (when None), corx and cory are drawn from np.random exactly as there -- all three always, both
    centre coordinates from sensor_resolution[1] -- so the result is bit-exact with the reference under np.random.seed.  Device
    tensors: the same float64 operations, each rounded as numpy rounds it.  clip_to_range: clip_events_to_bounds to the sensor.
    A DeviceEvents gives (DeviceEvents with the rotated float64 x, y, theta, centre)."""
    theta_radians = np.random.uniform(0, 2 * 3.14159265359) if theta_radians is None else theta_radians
    corx = int(np.random.uniform(0, sensor_resolution[1]) + 1)
    cory = int(np.random.uniform(0, sensor_resolution[1]) + 1)
    center_of_rotation = (corx, cory) if center_of_rotation is None else center_of_rotation
    cos, sin = np.cos(theta_radians), np.sin(theta_radians)
    ev = xs if isinstance(xs, DeviceEvents) else None
    if ev is not None:
        xs, ys = ev.x, ev.y
    if isinstance(xs, torch.Tensor):
        def centred(col, c):
            rt = np.result_type(np.empty(0, dtype=EU._NP_OF[col.dtype]), c)     # numpy's dtype of col - c (NEP 50)
            d = col.to(_T_OF_NP[np.dtype(rt)]) - c
            return d, d.to(torch.float64)
        _, cxd = centred(xs, center_of_rotation[0])
        _, cyd = centred(ys, center_of_rotation[1])
        cd, sd = float(cos), float(sin)
        new_xs = ((cxd * cd) - (cyd * sd)) + cxd
        new_ys = ((cxd * sd) + (cyd * cd)) + cyd
    else:
        cxs = xs - center_of_rotation[0]
        cys = ys - center_of_rotation[1]
        new_xs = (cxs * cos - cys * sin) + cxs
        new_ys = (cxs * sin + cys * cos) + cys
    if ev is not None:
        t = ev.t.to(torch.float64)
        out = DeviceEvents(new_xs, new_ys, t, ev.p.to(torch.float64))
        out.t_offset, out.p_scale = ev.t_offset, ev.p_scale
        if clip_to_range:
            out = clip_events_to_bounds(out, None, None, None, sensor_resolution)
        return out, theta_radians, center_of_rotation
    if clip_to_range:
        clip = clip_events_to_bounds(new_xs, new_ys, None, None, sensor_resolution)
        new_xs, new_ys = clip[0], clip[1]
    return new_xs, new_ys, theta_radians, center_of_rotation
