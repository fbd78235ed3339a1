"""Reference: lib/util/event_util.py.  events_bounds_mask is on the hot path (it is fused into the IWE kernel); this standalone
version keeps the reference function available.  The filters clip_events_to_bounds, get_events_from_mask and remove_hot_pixels
run as one order-preserving stream compaction on the device (evk_select.hip): numpy in -> numpy out (same dtypes), device
tensors in -> device tensors out, a DeviceEvents in place of xs (the other columns None) -> a new DeviceEvents."""
import numpy as np
import torch

from .. import _device as D
from .. import _lib
from ..events import DeviceEvents

_KIND = {torch.int16: _lib.EVK_SELECT_I16, torch.int32: _lib.EVK_SELECT_I32, torch.int64: _lib.EVK_SELECT_I64,
         torch.float32: _lib.EVK_SELECT_F32, torch.float64: _lib.EVK_SELECT_F64}
_NP_OF = {torch.int16: np.int16, torch.int32: np.int32, torch.int64: np.int64, torch.float32: np.float32,
          torch.float64: np.float64, torch.float16: np.float16, torch.int8: np.int8, torch.uint8: np.uint8, torch.bool: np.bool_}
_INT_OF_SIZE = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}


def events_bounds_mask(xs, ys, x_min, x_max, y_min, y_max):
    """mask = 0.0 where x<=x_min or x>x_max or y<=y_min or y>y_max, else 1.0 (reference: event_util.py:15-28; note the
    asymmetry: x == x_min is rejected, x == x_max kept).  numpy in -> float64 numpy out; device tensors in ->
    device tensor out."""
    dev = D.require_gpu()
    on_device = isinstance(xs, torch.Tensor)
    xd, yd = D.to_device(xs, torch.float64, dev), D.to_device(ys, torch.float64, dev)
    mask = torch.empty_like(xd)
    _lib.call("evk_bounds_mask_f64", D.ptr(xd), D.ptr(yd), xd.shape[0], float(x_min), float(x_max), float(y_min),
              float(y_max), D.ptr(mask), D.stream())
    return mask if on_device else mask.cpu().numpy()


# ---- columns in and out ---------------------------------------------------------------------------------------------------

def _np_dtype(col):
    return _NP_OF.get(col.dtype) if isinstance(col, torch.Tensor) else np.asarray(col).dtype


def _upload(a, dev):
    """numpy column -> device tensor holding the same bytes (a dtype torch lacks travels as the integer of its size)."""
    a = np.ascontiguousarray(a).reshape(-1)
    if a.dtype.itemsize not in _INT_OF_SIZE:
        raise TypeError("unsupported column dtype %s" % a.dtype)
    return torch.from_numpy(a.view(_INT_OF_SIZE[a.dtype.itemsize])).to(dev)


def _device_col(a, dev):
    if isinstance(a, torch.Tensor):
        return a.to(dev).contiguous().reshape(-1)
    return _upload(a, dev)


_T_OF = {np.dtype(np.int16): torch.int16, np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64,
         np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}


def _pred_col(col, np_dtype, host=None):
    """(device column, EVK_SELECT_* kind) of a coordinate column whose values are those of `np_dtype` (`col` holds its bytes;
    `host`: the numpy array it came from, if any).  Other dtypes than the five kinds are widened to int64 / float64."""
    np_dtype = np.dtype(np_dtype)
    t = _T_OF.get(np_dtype)
    if t is not None:
        return (col if col.dtype == t else col.view(t)), _KIND[t]
    wide = np.float64 if np_dtype.kind == "f" or np_dtype == np.uint64 else np.int64
    if host is not None:
        return _upload(np.asarray(host).astype(wide), col.device), _KIND[_T_OF[np.dtype(wide)]]
    return col.to(_T_OF[np.dtype(wide)]), _KIND[_T_OF[np.dtype(wide)]]


def _bits_value(bits, elem_bytes):
    if elem_bytes == 4:
        return float(np.array([bits & 0xFFFFFFFF], dtype=np.uint32).view(np.float32)[0])
    return float(np.array([bits], dtype=np.int64).view(np.float64)[0])


def _compact(pred, xp, yp, kind, payload, params=None, image=None, h=0, w=0, want_index=False, t_col=-1, oob=None):
    """evk_select_compact: (kept payload columns, kept indices or None, [K, t bits first, t bits last]).  The outputs are views
    of length K of n-element buffers; the three result words are the call's only read-back (after the error counter's)."""
    dev = xp.device
    n = int(xp.shape[0])
    L = _lib.lib()
    outs = [torch.empty(n, dtype=c.dtype, device=dev) for c in payload]
    index = torch.empty(n, dtype=torch.int64, device=dev) if want_index else None
    nbytes = int(L.evk_select_scratch_bytes(n))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    result = torch.zeros(3, dtype=torch.int64, device=dev)
    src = np.array([c.data_ptr() for c in payload], dtype=np.uint64)
    dst = np.array([o.data_ptr() for o in outs], dtype=np.uint64)
    eb = np.array([c.element_size() for c in payload], dtype=np.int32)
    hp = None if params is None else np.ascontiguousarray(params, dtype=np.float64)
    _lib.call("evk_select_compact", pred, kind, D.ptr(xp), D.ptr(yp), n, None if hp is None else D.host_ptr(hp), D.ptr(image),
              h, w, len(payload), D.host_ptr(src) if payload else None, D.host_ptr(dst) if payload else None,
              D.host_ptr(eb) if payload else None, t_col, D.ptr(index), D.ptr(result), D.ptr(scratch), nbytes,
              None if oob is None else oob.ptr, D.stream())
    if oob is not None:
        oob.raise_if_set(IndexError, "index out of bounds for the mask (event_util.py:106)")
    res = [int(v) for v in result.cpu().tolist()]
    k = res[0]
    return [o[:k] for o in outs], (None if index is None else index[:k]), res


def _events_result(ev, cols, res, t_col=2):
    out = DeviceEvents(*cols)
    out.t_offset, out.p_scale = ev.t_offset, ev.p_scale
    if res[0] > 0:
        eb = cols[t_col].element_size()
        out._t_ends = (_bits_value(res[1], eb), _bits_value(res[2], eb))
    return out


class _In:
    """The columns of a call: mode ('numpy' | 'torch' | 'events'), device columns, their numpy dtypes, the host arrays (numpy
    mode), the DeviceEvents (events mode); a column the caller passed as None stays None."""

    def __init__(self, xs, ys, ts, ps):
        self.ev, self.hosts = None, [None] * 4
        if isinstance(xs, DeviceEvents):
            self.mode, self.ev, self.cols = "events", xs, list(xs._columns())
        elif isinstance(xs, torch.Tensor):
            dev = D.require_gpu()
            self.mode, self.cols = "torch", [None if c is None else _device_col(c, dev) for c in (xs, ys, ts, ps)]
        else:
            dev = D.require_gpu()
            self.hosts = [None if c is None else np.asarray(c) for c in (xs, ys, ts, ps)]
            self.mode, self.cols = "numpy", [None if a is None else _upload(a, dev) for a in self.hosts]
        self.dts = [None if c is None else (h.dtype if h is not None else _NP_OF.get(c.dtype))
                    for c, h in zip(self.cols, self.hosts)]

    def pred(self, i):
        return _pred_col(self.cols[i], self.dts[i], self.hosts[i])

    def pred_xy(self):
        """x, y as predicate columns of one kind (the wider one when they differ)."""
        (px, kx), (py, ky) = self.pred(0), self.pred(1)
        if kx != ky:
            return px.to(torch.float64), py.to(torch.float64), _lib.EVK_SELECT_F64
        return px, py, kx


def _columns_out(mode, cols, dtypes):
    if mode == "numpy":
        return tuple(None if c is None else c.cpu().numpy().view(dt) for c, dt in zip(cols, dtypes))
    return tuple(cols)


def _round_bound(np_dtype, bound):
    """The bound as numpy >= 2 compares it with a column of `np_dtype` (NEP 50): rounded to np.result_type(column, bound)
    when that is a floating type (a float32 column against a python float compares in float32), as a double."""
    rt = np.result_type(np.empty(0, dtype=np_dtype), bound)
    return float(rt.type(bound)) if rt.kind == "f" else float(bound)


# ---- the filters --------------------------------------------------------------------------------------------------------

def clip_events_to_bounds(xs, ys, ts, ps, bounds, set_zero=False):
    """Reference: event_util.py:61-94.  bounds = [miny, maxy, minx, maxx], or [maxy, maxx] with the lower bounds 0; ts / ps may be
    None.  set_zero=False keeps the events of the half-open box minx <= x < maxx, miny <= y < maxy in stream order;
    set_zero=True returns every column multiplied by events_bounds_mask (float64; that mask rejects x == minx and keeps
    x == maxx).  Bounds are compared as numpy >= 2 does: rounded to the result type of column and bound, then in double."""
    if len(bounds) == 2:
        bounds = [0, bounds[0], 0, bounds[1]]
    elif len(bounds) != 4:
        raise Exception("Bounds must be of length 2 or 4 (not {})".format(len(bounds)))
    miny, maxy, minx, maxx = bounds
    a = _In(xs, ys, ts, ps)
    bx = [_round_bound(a.dts[0], minx), _round_bound(a.dts[0], maxx)]
    by = [_round_bound(a.dts[1], miny), _round_bound(a.dts[1], maxy)]
    if set_zero:
        n = a.cols[0].shape[0]
        dev = a.cols[0].device
        xd, yd = (a.pred(i)[0].to(torch.float64) for i in (0, 1))
        mask = torch.empty(n, dtype=torch.float64, device=dev)
        _lib.call("evk_bounds_mask_f64", D.ptr(xd), D.ptr(yd), n, bx[0], bx[1], by[0], by[1], D.ptr(mask), D.stream())
        out = [None] * 4
        for i, c in enumerate(a.cols):
            if c is None:
                continue
            pc, kind = a.pred(i)
            out[i] = torch.empty(n, dtype=torch.float64, device=dev)
            off = a.ev.t_offset if (a.ev is not None and i == 2) else 0.0      # the reference's absolute time stamps
            _lib.call("evk_mask_multiply_f64", kind, D.ptr(pc), n, off, D.ptr(mask), D.ptr(out[i]), D.stream())
        if a.mode == "events":
            r = DeviceEvents(*out)
            r.p_scale = a.ev.p_scale
            return r
        return tuple(None if o is None else (o.cpu().numpy() if a.mode == "numpy" else o) for o in out)
    px, py, kind = a.pred_xy()
    keep = [i for i, c in enumerate(a.cols) if c is not None]
    kept, _, res = _compact(_lib.EVK_SELECT_BOX, px, py, kind, [a.cols[i] for i in keep], params=[bx[0], bx[1], by[0], by[1]],
                            t_col=keep.index(2) if 2 in keep else -1)
    full = [None] * 4
    for i, k in zip(keep, kept):
        full[i] = k
    if a.mode == "events":
        return _events_result(a.ev, full, res)
    return _columns_out(a.mode, full, a.dts)


def get_events_from_mask(mask, xs, ys):
    """Reference: event_util.py:96-109.  int64 indices of the events whose mask value mask[int(y), int(x)] is >= 0.01 (0.01
    rounded to the mask's dtype when that is a float type, as numpy >= 2 compares); coordinates are truncated toward zero,
    negative indices wrap as numpy's do, others outside the mask raise IndexError.  One hit gives a 0-d result (.squeeze())."""
    a = _In(xs, ys, None, None)
    dev = a.cols[0].device
    mdt = np.dtype(_np_dtype(mask))
    thr = float(mdt.type(0.01)) if mdt.kind == "f" else 0.01
    if isinstance(mask, torch.Tensor):
        md = mask.to(device=dev, dtype=torch.float64).contiguous()
    else:
        md = D.to_device(np.asarray(mask), torch.float64, dev)
    if md.dim() != 2:
        raise IndexError("get_events_from_mask indexes a 2-D mask (this one has %d dimensions)" % md.dim())
    h, w = int(md.shape[0]), int(md.shape[1])
    n = int(a.cols[0].shape[0])
    if n and (h == 0 or w == 0):
        raise IndexError("index out of bounds for an empty mask")
    if n == 0:
        idx = torch.empty(0, dtype=torch.int64, device=dev)
    else:
        px, py, kind = a.pred_xy()
        _, idx, _ = _compact(_lib.EVK_SELECT_MASK, px, py, kind, [], params=[thr], image=md, h=h, w=w, want_index=True,
                             oob=D.OobCounter(dev))
    if idx.shape[0] == 1:
        idx = idx.reshape(())
    return idx.cpu().numpy() if a.mode == "numpy" else idx


def remove_hot_pixels(xs, ys, ts, ps, sensor_size=(180, 240), num_hot=50):
    """Reference: event_util.py:166-187, with the deletion by integer indices (upstream's float index array no longer works
    with numpy >= 1.19).  The event image is events_to_image's: int32 on the device for integer weights (bit-exact), float64
    otherwise; integer coordinates are required (TypeError), coordinates outside the (H+1, W+1) canvas raise ValueError.
    The num_hot pixels the reference's "argmax, set to 0" loop would pick are selected on the device (evk_hot_pixels), every
    event on one of them is removed, the others keep their order."""
    H, W = int(sensor_size[0]), int(sensor_size[1])
    a = _In(xs, ys, ts, ps)
    if any(c is None for c in a.cols):
        raise TypeError("remove_hot_pixels needs xs, ys, ts and ps")
    if a.mode == "numpy" and not (np.issubdtype(a.dts[0], np.integer) and np.issubdtype(a.dts[1], np.integer)):
        raise TypeError("only int indices permitted")      # np.ravel_multi_index, image.py:31
    x = a.cols[0]
    dev, n = x.device, int(x.shape[0])
    if n == 0:
        return _events_result(a.ev, a.cols, [0]) if a.mode == "events" else _columns_out(a.mode, a.cols, a.dts)
    xi, yi = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    for i, dst in ((0, xi), (1, yi)):
        pc, kind = a.pred(i)
        _lib.call("evk_select_to_i32", kind, D.ptr(pc), n, D.ptr(dst), D.ptr(bad), D.stream())
    if any(np.dtype(a.dts[i]).kind == "f" for i in (0, 1)) and int(bad.item()):
        raise TypeError("only int indices permitted: the coordinates are not integers")
    img_size = (H + 1, W + 1)
    oob = D.OobCounter(dev)
    int_w = a.mode == "numpy" and (np.issubdtype(a.dts[3], np.integer) or a.dts[3] == np.bool_)
    if int_w:                                 # events_to_image's rule for its int32 image
        pa = a.hosts[3]
        int_w = float(max(abs(int(pa.min())), abs(int(pa.max())))) * n < 2 ** 31
    if int_w:
        from .. import tiled
        wcol = D.to_device(a.hosts[3], torch.int32, dev)
        canvas = None
        if tiled.can_tile_image((xi, yi, wcol), tiled.default_impl()):
            canvas = torch.empty(img_size, dtype=torch.int32, device=dev)
            if not tiled.image2("i32", xi, yi, wcol, n, img_size[0], img_size[1], 0.0, 0.0, canvas, oob, fresh=True):
                canvas = None
        if canvas is None:
            canvas = torch.zeros(img_size, dtype=torch.int32, device=dev)
            _lib.call("evk_image_nearest_i32", D.ptr(xi), D.ptr(yi), D.ptr(wcol), n, img_size[0], img_size[1], D.ptr(canvas),
                      oob.ptr, D.stream())
        img_kind = _lib.EVK_SELECT_I32
    else:
        wcol = a.pred(3)[0].to(torch.float64)
        if a.ev is not None and a.ev.p_scale != 1.0:
            wcol = wcol * a.ev.p_scale
        canvas = torch.zeros(img_size, dtype=torch.float64, device=dev)
        _lib.call("evk_image_nearest_f64", D.ptr(xi), D.ptr(yi), D.ptr(wcol), n, img_size[0], img_size[1], D.ptr(canvas),
                  oob.ptr, D.stream())
        img_kind = _lib.EVK_SELECT_F64
    oob.raise_if_set(ValueError, "events outside the (H+1, W+1) canvas %s" % (img_size,))
    L = _lib.lib()
    hot = torch.empty(H * W, dtype=torch.uint8, device=dev)
    sb = int(L.evk_hot_pixels_scratch_bytes())
    hs = torch.empty(sb, dtype=torch.uint8, device=dev)
    _lib.call("evk_hot_pixels", D.ptr(canvas), img_kind, H, W, W + 1, int(num_hot), D.ptr(hot), D.ptr(hs), sb, D.stream())
    kept, _, res = _compact(_lib.EVK_SELECT_NOT_HOT, xi, yi, _lib.EVK_SELECT_I32, a.cols, image=hot, h=H, w=W, t_col=2)
    if a.mode == "events":
        return _events_result(a.ev, kept, res)
    return _columns_out(a.mode, kept, a.dts)
