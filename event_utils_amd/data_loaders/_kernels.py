"""The device side of the datasets: a resident event stream, the voxel grids of a table of windows (evk_voxel_windows_f32),
the (N, 4) event rows of return_events (evk_pack_window_events_f32) and RobustNorm (evk_robust_norm_f32)."""
import numpy as np
import torch

from .. import _device as D
from .. import _lib
from ..events import DeviceEvents

# A call for ONE window of at least this many events (a __getitem__) takes the one-pass voxel path (partition + LDS tiles)
# instead of the window kernel, whose workgroups each stream the whole window and which, for one window, fills only 43-88
# workgroups at 240x180 / 346x260: from 100 k events on the one-pass path is 1.2-1.6x faster at 240x180, within 15 % either
# way at 346x260.  A batch of windows always takes the window kernel: with 16 windows it is 9-15x faster than the one-pass
# path window by window at every length measured, 10 k to 1.5 M events (tools/window_crossover.py,
# profiles/window_crossover.txt).
LONG_WINDOW_EVENTS = 100_000


class ResidentStream:
    """One event stream uploaded once: int16 coordinates, float64 / float32 time stamps and {0, 1} polarities in their
    on-disk dtypes (DeviceEvents.from_native), or float32 coordinates / polarities (the npy format's float columns,
    widened on the host as the reference's loaders widen them)."""

    def __init__(self, xy=None, xs=None, ys=None, ts=None, ps=None, p_pm1=True, device=None):
        device = device or D.require_gpu()
        ts = np.asarray(ts)
        self.n = int(ts.shape[0])
        native = None
        if p_pm1 and xy is not None and np.asarray(xy).dtype == np.int16 and np.asarray(ps).dtype in (np.uint8, np.bool_) \
                and ts.dtype in (np.float64, np.float32):
            native = DeviceEvents.from_native(xy, None, ts, ps, polarity="pm1", device=device).native
        elif p_pm1 and xy is None and np.asarray(xs).dtype == np.int16 and np.asarray(ys).dtype == np.int16 \
                and np.asarray(ps).dtype in (np.uint8, np.bool_) and ts.dtype in (np.float64, np.float32):
            native = DeviceEvents.from_native(xs, ys, ts, ps, polarity="pm1", device=device).native
        if native is not None:
            self.x, self.y, self.t, self.p = native.x, native.y, native.t, native.p
            self.xy_kind, self.xy_stride = _lib.EVK_SELECT_I16, native.xy_stride
            self.t_kind, self.p_kind = native.t_kind, _lib.EVK_P_U8_PM1
        else:
            # memmap_dataset.py:21-24 / npy_dataset.py:24: coordinates .astype(float32), p * 2.0 - 1.0 (oracle
            # widen_native_events); the time stamps stay float64 (each window subtracts its own ts[0] first)
            if xy is not None:
                xy = np.asarray(xy)
                xs, ys = xy[:, 0], xy[:, 1]
            f32 = lambda a: D.to_device(np.asarray(a).astype(np.float32), torch.float32, device)
            self.x, self.y = f32(xs), f32(ys)
            p = np.asarray(ps)
            self.p = f32(p * 2.0 - 1.0 if p_pm1 else p)
            self.t = D.to_device(ts if ts.dtype == np.float32 else ts.astype(np.float64),
                                 torch.float32 if ts.dtype == np.float32 else torch.float64, device)
            self.xy_kind, self.xy_stride = _lib.EVK_SELECT_F32, 1
            self.t_kind = _lib.EVK_T_F32 if ts.dtype == np.float32 else _lib.EVK_T_F64
            self.p_kind = _lib.EVK_P_F32
        self.device = device

    def _table(self, windows):
        w = np.asarray(windows, dtype=np.int64).reshape(-1, 2)
        if len(w) and (w.min() < 0 or w.max() > self.n):
            raise IndexError("event window outside the stream of %d events" % self.n)
        return w

    def src_args(self):
        return (D.ptr(self.x), D.ptr(self.y) if self.y is not None else None, self.xy_kind, self.xy_stride, D.ptr(self.t),
                self.t_kind, D.ptr(self.p), self.p_kind)

    def pack_events(self, windows):
        """(sum of window lengths, 4) float32 rows [x, y, (float)(t - t[a]), p] of every window, in order, and the row offsets."""
        w = self._table(windows)
        lens = np.maximum(w[:, 1] - w[:, 0], 0)
        rows = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.int64)
        out = torch.empty((int(lens.sum()), 4), dtype=torch.float32, device=self.device)
        if len(w) and out.shape[0]:
            wd = torch.from_numpy(np.ascontiguousarray(w)).to(self.device)
            rd = torch.from_numpy(rows).to(self.device)
            _lib.call("evk_pack_window_events_f32", *self.src_args(), D.ptr(wd), D.ptr(rd), len(w), D.ptr(out), D.stream())
        return out, rows, lens

    def voxel_windows(self, windows, B, sensor_size, split):
        """(nw, C, H, W) float32 grids of the windows [a, b) (C = 2B when split)."""
        H, W = int(sensor_size[0]), int(sensor_size[1])
        w = self._table(windows)
        nw, C = len(w), (2 * B if split else B)
        out = torch.empty((nw, C, H, W), dtype=torch.float32, device=self.device)
        if nw == 0:
            return out
        if nw == 1 and w[0, 1] - w[0, 0] >= LONG_WINDOW_EVENTS:
            from ..representations.voxel_grid import events_to_neg_pos_voxel_torch, events_to_voxel_torch
            rows = self.pack_events(w)[0]
            x, y, t, p = (rows[:, c].contiguous() for c in range(4))
            if split:
                pos, neg = events_to_neg_pos_voxel_torch(x, y, t, p, B, sensor_size=(H, W))
                out[0, :B], out[0, B:] = pos, neg
            else:
                out[0] = events_to_voxel_torch(x, y, t, p, B, sensor_size=(H, W))
            return out
        oob = D.OobCounter(self.device)
        for c0 in range(0, nw, 65535):                      # (blockIdx.y holds at most 65535 windows)
            part = w[c0:c0 + 65535]
            wd = torch.from_numpy(np.ascontiguousarray(part)).to(self.device)
            _lib.call("evk_voxel_windows_f32", *self.src_args(), D.ptr(wd), len(part), B, H, W, int(bool(split)),
                      D.ptr(out[c0:c0 + len(part)]), oob.ptr, D.stream())
        oob.raise_if_set(IndexError, "index out of range for voxel grid of size %s" % ((C, H, W),))
        return out


def percentile_rank(q, m):
    """1-based rank of RobustNorm.percentile (data_augmentation.py:115): 1 + round(.01 * float(q) * (m - 1)), Python's
    round (half to even)."""
    return 1 + round(.01 * float(q) * (m - 1))


def _item_view(x, batch_dims):
    """(n, item_stride, (d0, d1, d2), (s0, s1, s2)) of a tensor whose leading `batch_dims` dims index items, or None when the
    item is not expressible as a strided 3-D view."""
    n = 1 if batch_dims == 0 else int(x.shape[0])
    shape, strides = list(x.shape[batch_dims:]), list(x.stride()[batch_dims:])
    item_stride = 0 if batch_dims == 0 else int(x.stride(0))
    if len(shape) > 3:
        return None
    while len(shape) < 3:
        shape.insert(0, 1)
        strides.insert(0, 0)
    return n, item_stride, shape, strides


def robust_norm(x, low_perc, top_perc, batch_dims=0):
    """RobustNorm of every item of a float32 tensor (batch_dims=1: x[k] is item k; 0: x is one item) on the GPU ->
    (normalised tensor of x's shape, contiguous, on x's device; (n, 2) float32 percentile pairs [low, top] on the GPU)."""
    if x.dtype != torch.float32:
        raise TypeError("RobustNorm runs on float32 tensors (voxel grids); got %s" % x.dtype)
    home = x.device
    dev = x.device if x.is_cuda else D.require_gpu()
    xd = x if x.is_cuda else x.to(dev)
    v = _item_view(xd, batch_dims)
    if v is None:
        xd = xd.contiguous()
        v = _item_view(xd.reshape((xd.shape[0], -1) if batch_dims else (-1,)), batch_dims)
    n, item_stride, (d0, d1, d2), (s0, s1, s2) = v
    m = d0 * d1 * d2
    out = torch.empty(x.shape, dtype=torch.float32, device=dev)
    stats = torch.empty((n, 4), dtype=torch.float32, device=dev)      # [t_min, t_max, min, max of the clamped item]
    if m == 0 or n == 0:
        raise RuntimeError("kthvalue(): selected number k out of range for an empty tensor")
    k_lo, k_hi = percentile_rank(low_perc, m), percentile_rank(top_perc, m)
    _lib.call("evk_robust_norm_f32", D.ptr(xd), n, item_stride, d0, d1, d2, s0, s1, s2, k_lo, k_hi, D.ptr(out), D.ptr(stats),
              D.stream())
    return (out if home == dev else out.to(home)), stats[:, :2]
