"""Motion segmentation by motion compensation: per-cluster weighted images of warped events and the soft assignment of events
to clusters, after Stoffregen, Gallego, Drummond, Kleeman and Scaramuzza, "Event-Based Motion Segmentation by Motion
Compensation" (ICCV 2019).  Upstream only hints at it (segmentation_mask_from_d_iwe thresholds a derivative image).

L motion models of one kind with parameters theta_l, and an association P (L, N) of every event with every model.  Definition
(include/evk.h, "Motion segmentation"): each cluster has its image of warped events I_l, every event
weighted by P_kl (times the sign of its polarity with use_polarity=True); B_l = gaussian_filter(I_l); the loss, to be
MINIMISED, is -sum_l Var(B_l); the gradient with respect to every theta_l is exact (by the adjoint, as zhu_timestamp_objective);
the assignment step sets P'_kl proportional to max(0, B_l at the event's place under theta_l).  Everything per event runs in
three fused kernels (csrc/evk_segment.hip: splat, adjoint gather, assignment); the image-sized steps are the post pass of the
dense-flow contrast loss, once per plane.  Planes, loss and gradient are the same bits from call to call.

Events are given as everywhere in the package: numpy columns, CUDA tensors, or a DeviceEvents in place of xs (ys, ts, ps are then
ignored).  warpfunc is linvel_warp or one of the four fused parametric warps; img_size (H, W) gives the canvas (H + 1, W + 1) and
the bounds, and the reference time is the last time stamp.  Out of scope: choosing L, initialising the motions, different models
per cluster."""
from collections import namedtuple

import numpy as np
import torch

from .. import _device as D
from .. import _lib
from .objectives import _as_device_events, _blur_kernel, _ts_model, _ts_polarities, _wide, gaussian_filter_device

__all__ = ["cluster_iwes", "segmentation_loss", "update_assignments", "segment_events", "SegmentationResult"]

MAX_CLUSTERS = _lib.EVK_SEG_MAX_CLUSTERS
_SUPPORTED = "linvel_warp, pure_rotation_warp, xyztheta_warp, angular_velocity_warp, planar_flow_warp"

SegmentationResult = namedtuple("SegmentationResult", ["params", "probs", "labels", "loss", "history"])


def _check_probs(probs):
    """0 <= P <= 1 and no NaN: one reduction on the device."""
    if probs.numel() and not bool(((probs >= 0) & (probs <= 1)).all().item()):
        raise ValueError("probs must lie in [0, 1] and hold no NaN")


class _Setup:
    """What the three kernels share: the resident events, the (L, nparams) block of the clusters' parameters, the associations on
    the device and the head of the argument lists."""

    def __init__(self, params, probs, xs, ys, ts, ps, warpfunc, img_size, use_polarity, validate=True):
        if _ts_model(warpfunc, np.zeros(getattr(warpfunc, "dims", 2))) is None:
            raise NotImplementedError("motion segmentation runs fused kernels only: warpfunc must be one of " + _SUPPORTED)
        params = np.asarray(params, dtype=np.float64)
        if params.ndim != 2 or params.shape[1] != warpfunc.dims:
            raise ValueError("params must have shape (L, %d) for %s, got %r" % (warpfunc.dims, warpfunc.name, params.shape))
        self.L, self.dims = int(params.shape[0]), int(warpfunc.dims)
        if not 1 <= self.L <= MAX_CLUSTERS:
            raise ValueError("1 to %d clusters are supported, got %d" % (MAX_CLUSTERS, self.L))
        self.device = D.require_gpu()
        self.ev = ev = _as_device_events(xs, ys, ts, ps)
        self.n = len(ev)
        self.warpfunc, self.img_size = warpfunc, (int(img_size[0]), int(img_size[1]))
        self.ch, self.cw = self.img_size[0] + 1, self.img_size[1] + 1
        self.flags = _lib.EVK_SEG_POLARITY if use_polarity else 0
        self.suffix = "f32" if ev.dtype == torch.float32 else "f64"
        self.pcol = _ts_polarities(ev)
        self.t_ref = float(ev.t_at(-1)) if self.n else 0.0
        self.set_params(params)
        self.probs = self._probs(probs, validate)

    def _probs(self, probs, validate):
        if probs is None:
            return torch.full((self.L, self.n), 1.0 / self.L, dtype=torch.float32, device=self.device)
        if not isinstance(probs, torch.Tensor):
            probs = np.asarray(probs)
        if tuple(probs.shape) != (self.L, self.n):
            raise ValueError("probs must have shape (L, N) = (%d, %d), got %r" % (self.L, self.n, tuple(probs.shape)))
        probs = D.to_device(probs, torch.float32, self.device)
        if validate:
            _check_probs(probs)
        return probs

    def set_params(self, params):
        model = None
        rows = []
        for q in np.asarray(params, dtype=np.float64).reshape(self.L, self.dims):
            model, hp = _ts_model(self.warpfunc, q)
            rows.append(hp)
        self.model, self.host_params = model, np.ascontiguousarray(np.stack(rows), dtype=np.float64)

    def head(self, probs=None, impl=None):
        ev = self.ev
        flags = self.flags | (_lib.EVK_IWE_DIRECT if impl == "direct" else 0)
        return (self.model, D.ptr(ev.x), D.ptr(ev.y), D.ptr(ev.t), D.ptr(self.pcol), self.n, self.t_ref,
                D.host_ptr(self.host_params), self.L, D.ptr(self.probs if probs is None else probs), float(self.img_size[1]),
                float(self.img_size[0]), self.ch, self.cw, flags)

    def planes(self, impl=None):
        """Steps 1-3 -> (L, H+1, W+1) float32."""
        shape = (self.L, self.ch, self.cw)
        acc = torch.zeros(shape, dtype=torch.int64, device=self.device)     # fixed point: the sums do not depend on their order
        out = torch.empty(shape, dtype=torch.float32, device=self.device)
        _lib.call("evk_seg_splat_" + self.suffix, *self.head(impl=impl), D.ptr(acc), D.ptr(out), D.stream())
        return out

    def post(self, planes, blur_sigma, want_adjoint):
        """Step 4, evk_flowcm_post_f32 plane by plane -> (loss, adjoint images (L, H+1, W+1) | None); the L values are summed
        in cluster order."""
        dev, ch, cw = self.device, self.ch, self.cw
        w, radius = _blur_kernel(blur_sigma)
        wd = torch.from_numpy(w).to(dev) if _wide(radius) else None
        losses = torch.empty(self.L, dtype=torch.float64, device=dev)
        work = torch.empty((3, ch, cw), dtype=torch.float32, device=dev)
        adj = torch.empty((self.L, ch, cw), dtype=torch.float32, device=dev) if want_adjoint else None
        scratch, nbytes = D.reduce_scratch(dev)
        for l in range(self.L):
            _lib.call("evk_flowcm_post_f32", D.ptr(planes[l]), ch, cw, D.host_ptr(w) if w is not None else None, D.ptr(wd), radius,
                      _lib.EVK_FLOWCM_VARIANCE, D.ptr(work), D.ptr(adj[l]) if want_adjoint else None, D.ptr(losses[l:]),
                      D.ptr(scratch), nbytes, D.stream())
        total = 0.0
        for v in losses.cpu().numpy():
            total += float(v)
        return total, adj

    def gradient(self, adj):
        """Step 5 -> (L, dims) float64 ndarray."""
        out = torch.empty((self.L, self.dims), dtype=torch.float64, device=self.device)
        scratch, nbytes = _grad_scratch(self.device)
        _lib.call("evk_seg_grad_" + self.suffix, *self.head(), D.ptr(adj), D.ptr(out), D.ptr(scratch), nbytes, D.stream())
        return out.cpu().numpy()

    def evaluate(self, blur_sigma, want_grad):
        loss, adj = self.post(self.planes(), blur_sigma, want_grad)
        return (loss, self.gradient(adj)) if want_grad else (loss, None)

    def assign(self, blur_sigma):
        """Step 6 with the B_l of the current associations -> (P' (L, N) float32, labels (N,) int32)."""
        planes = self.planes()
        if blur_sigma > 0:
            planes = torch.stack([gaussian_filter_device(planes[l], blur_sigma) for l in range(self.L)])
        out = torch.empty((self.L, self.n), dtype=torch.float32, device=self.device)
        labels = torch.empty(self.n, dtype=torch.int32, device=self.device)
        _lib.call("evk_seg_assign_" + self.suffix, *self.head(), D.ptr(planes), D.ptr(out), D.ptr(labels), D.stream())
        return out, labels


def _grad_scratch(device):
    key = (device.index, D.stream_id(device), "segment")
    if key not in D._scratch:
        nbytes = int(_lib.lib().evk_seg_grad_scratch_bytes())
        D._scratch[key] = (torch.empty(nbytes // 8, dtype=torch.float64, device=device), nbytes)
    return D._scratch[key]


def cluster_iwes(params, probs, xs, ys, ts, ps, warpfunc, img_size, use_polarity=False, impl=None):
    """The L images of warped events, event k weighted by probs[l, k] in image l (times the sign of its polarity with
    use_polarity=True) -> (L, H+1, W+1) float32 device tensor, the same bits on every call.  params (L, dims); probs (L, N) numpy
    or device tensor in [0, 1].  One fused pass (LDS bands holding all L planes; impl='direct': global atomics, same bits)."""
    return _Setup(params, probs, xs, ys, ts, ps, warpfunc, img_size, use_polarity).planes(impl)


def segmentation_loss(params, probs, xs, ys, ts, ps, warpfunc, img_size, blur_sigma=1.0, use_polarity=False,
                      compute_gradient=False):
    """-sum_l Var(gaussian_filter(I_l, blur_sigma)) over the cluster images of cluster_iwes, to be minimised -> loss (float);
    with compute_gradient=True -> (loss, dloss/dparams as an (L, dims) float64 ndarray), exact and bitwise repeatable."""
    loss, grad = _Setup(params, probs, xs, ys, ts, ps, warpfunc, img_size, use_polarity).evaluate(blur_sigma, compute_gradient)
    return (loss, grad) if compute_gradient else loss


def update_assignments(params, probs, xs, ys, ts, ps, warpfunc, img_size, blur_sigma=1.0, use_polarity=False):
    """The assignment step: P'[l, k] = c_kl / sum_l c_kl with c_kl = max(0, the blurred image of cluster l at the place of event
    k under params[l]) (0 where the event leaves the canvas; times the sign of the polarity with use_polarity=True); an event
    with no positive c keeps its row.  The images are those of the given probs.  -> (P' (L, N) float32, labels (N,) int32 =
    argmax over the clusters, lowest index on ties), device tensors."""
    return _Setup(params, probs, xs, ys, ts, ps, warpfunc, img_size, use_polarity).assign(blur_sigma)


def segment_events(xs, ys, ts, ps, warpfunc, x0, img_size, n_outer=6, inner_maxiter=10, blur_sigma=1.0, use_polarity=False,
                   probs0=None, callback=None):
    """Alternating optimisation: every outer iteration improves the L motions with the associations fixed (scipy BFGS with the
    analytic gradient on the stacked L x dims vector, at most inner_maxiter iterations) and then re-estimates the associations
    (update_assignments).  x0 (L, dims) starts the motions, probs0 the associations (default: uniform 1 / L).  The events are
    uploaded once and the associations never leave the device.  callback(outer, params, loss) after every outer iteration.
    -> SegmentationResult(params (L, dims), probs (L, N) device, labels (N,) device, loss, history): history holds the loss after
    every outer iteration (the new motions with the new associations), loss its last entry."""
    import scipy.optimize as opt
    if n_outer < 1:
        raise ValueError("n_outer must be at least 1")
    x0 = np.asarray(x0, dtype=np.float64)
    s = _Setup(x0, probs0, xs, ys, ts, ps, warpfunc, img_size, use_polarity)
    params, shape = x0.copy(), x0.shape

    def fun(v):
        s.set_params(v.reshape(shape))
        loss, grad = s.evaluate(blur_sigma, True)
        return loss, grad.reshape(-1)

    history, labels = [], None
    for outer in range(n_outer):
        res = opt.minimize(fun, params.reshape(-1), jac=True, method="BFGS", options={"maxiter": int(inner_maxiter)})
        params = np.asarray(res.x, dtype=np.float64).reshape(shape)
        s.set_params(params)
        s.probs, labels = s.assign(blur_sigma)
        loss = s.evaluate(blur_sigma, False)[0]
        history.append(loss)
        if callback is not None:
            callback(outer, params.copy(), loss)
    return SegmentationResult(params, s.probs, labels, history[-1], history)
