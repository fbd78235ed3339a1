"""The average-timestamp loss of Zhu et al. (CVPR 2019) as a function of a dense flow field, with dloss/dflow at every pixel
(include/evk.h, "Average-timestamp objective", steps 1' and 8'; csrc/evk_flowloss.hip).  It joins the two
halves the package already has -- warp_events_flow_torch and zhu_timestamp_objective -- in one pass over the events, and adds
what their composition cannot give: the gradient with respect to the field.

The contrast (focus) loss of the same field -- the variance or mean square of the blurred image of warped events (include/evk.h,
"Contrast loss of a flow field") -- is its peer: flow_field_iwe, flow_field_contrast_loss and flow_contrast_loss run on the same
setup, with one plane in place of four."""
import numpy as np
import torch

from .. import _device as D
from .. import _lib
from ..contrast_max.objectives import _blur_kernel, _ts_polarities, _wide
from ..events import DeviceEvents

_DIRECTIONS = {"forward": (_lib.EVK_FLOWTS_FORWARD,), "backward": (_lib.EVK_FLOWTS_BACKWARD,),
               "both": (_lib.EVK_FLOWTS_FORWARD, _lib.EVK_FLOWTS_BACKWARD)}


class _Setup:
    """The checked, device-resident inputs of one call: flow (B, 2, H, W) float32, the four float32 columns, offsets (B + 1,)
    int64 on the device, and whether the caller passed a batch."""

    def __init__(self, flow, xs, ys, ts, ps, direction, offsets):
        if direction not in _DIRECTIONS:
            raise ValueError("direction must be 'forward', 'backward' or 'both', got %r" % (direction,))
        self.directions = _DIRECTIONS[direction]
        if not isinstance(flow, torch.Tensor):
            flow = torch.as_tensor(np.asarray(flow))
        self.batched = flow.dim() == 4
        if flow.dim() not in (3, 4) or flow.shape[-3] != 2 or flow.shape[-2] < 2 or flow.shape[-1] < 2:
            raise ValueError("flow must be (2, H, W) or (B, 2, H, W) with H, W >= 2, got shape %s" % (tuple(flow.shape),))
        if self.batched and not 1 <= flow.shape[0] <= 65535:
            raise ValueError("flow holds %d samples; 1 to 65535 are supported" % flow.shape[0])
        if self.batched != (offsets is not None):
            raise ValueError("a (B, 2, H, W) field needs offsets of shape (B + 1,), a (2, H, W) field takes none")
        dev = D.require_gpu()
        self.flow = D.to_device(flow.detach(), torch.float32, dev)
        self.B, (self.H, self.W) = (int(flow.shape[0]) if self.batched else 1), (int(flow.shape[-2]), int(flow.shape[-1]))
        if isinstance(xs, DeviceEvents):
            ev = xs
            if ev.dtype != torch.float32:
                raise ValueError("flow_field_timestamp_loss takes float32 event columns")
            cols = (ev.x, ev.y, ev.t, _ts_polarities(ev))
            self.weights = (ev.p, float(ev.p_scale))                        # the contrast loss multiplies on the device
        else:
            cols = tuple(D.to_device(a, torch.float32, dev).reshape(-1) for a in (xs, ys, ts, ps))
            self.weights = (cols[3], 1.0)
        self.n = int(cols[0].shape[0])
        if any(int(c.shape[0]) != self.n for c in cols):
            raise ValueError("the event columns differ in length: %s" % ([int(c.shape[0]) for c in cols],))
        self.cols = cols
        self.offsets = self._offsets(offsets, dev)
        self.device = dev

    def _offsets(self, offsets, dev):
        if offsets is None:
            return torch.tensor([0, self.n], dtype=torch.int64, device=dev)
        off = offsets if isinstance(offsets, torch.Tensor) else torch.as_tensor(np.asarray(offsets))
        if off.dim() != 1 or off.shape[0] != self.B + 1 or off.dtype.is_floating_point:
            raise ValueError("offsets must be %d integers (B + 1), got shape %s %s" % (self.B + 1, tuple(off.shape), off.dtype))
        off = off.to(torch.int64)
        # one check per call (not per sample): a host tensor is read where it is, a device tensor costs one small transfer
        first, last, steps = torch.stack((off[0], off[-1], (off[1:] - off[:-1]).min())).tolist()
        if first != 0 or last != self.n or steps < 0:
            raise ValueError("offsets must rise from 0 to the event count %d, got %d .. %d" % (self.n, first, last))
        return off.to(dev).contiguous()

    def head(self):
        """The argument prefix shared by evk_flowts_warp_f32 and evk_flowts_grad_f32."""
        return tuple(D.ptr(c) for c in self.cols) + (D.ptr(self.offsets), self.B, self.n, D.ptr(self.flow), self.H, self.W)

    def time_constants(self, direction):
        tc = torch.empty((self.B, 3), dtype=torch.float32, device=self.device)
        _lib.call("evk_flowts_time_constants_f32", D.ptr(self.cols[2]), D.ptr(self.offsets), self.B, self.n, direction,
                  D.ptr(tc), D.stream())
        return tc

    def planes(self, tc):
        """(B, 4, H+1, W+1) float32 [T+, C+, T-, C-] per sample: one pass over the events."""
        shape = (self.B, 4, self.H + 1, self.W + 1)
        acc = torch.zeros(shape, dtype=torch.int64, device=self.device)     # fixed point: the sums do not depend on their order
        planes = torch.empty(shape, dtype=torch.float32, device=self.device)
        _lib.call("evk_flowts_warp_f32", *self.head(), D.ptr(tc), D.ptr(acc), D.ptr(planes), D.stream())
        return planes

    def post(self, planes, blur_sigma, want_adjoint):
        """evk_tsobj_post_f32 sample by sample -> losses (B,) float64 and adj4 (B, 4, H+1, W+1) | None, on the device."""
        dev, (ch, cw) = self.device, (self.H + 1, self.W + 1)
        w, radius = _blur_kernel(blur_sigma)
        wd = torch.from_numpy(w).to(dev) if _wide(radius) else None         # a wide blur reads its taps from device memory
        losses = torch.empty(self.B, dtype=torch.float64, device=dev)
        work = torch.empty((6, ch, cw), dtype=torch.float32, device=dev)
        adj = torch.empty((self.B, 4, ch, cw), dtype=torch.float32, device=dev) if want_adjoint else None
        scratch, nbytes = D.reduce_scratch(dev)
        for b in range(self.B):
            _lib.call("evk_tsobj_post_f32", D.ptr(planes[b]), ch, cw, D.host_ptr(w) if w is not None else None, D.ptr(wd), radius,
                      D.ptr(work), D.ptr(adj[b]) if want_adjoint else None, D.ptr(losses[b:]), D.ptr(scratch), nbytes, D.stream())
        return losses, adj

    def gradient(self, tc, adj):
        """(B, 2, H, W) float32 = dloss/dflow: the one gather / scatter pass over the events."""
        shape = (self.B, 2, self.H, self.W)
        gacc = torch.zeros(shape, dtype=torch.int64, device=self.device)
        absmax = torch.empty(self.B, dtype=torch.int32, device=self.device)
        grad = torch.empty(shape, dtype=torch.float32, device=self.device)
        _lib.call("evk_flowts_grad_f32", *self.head(), D.ptr(tc), D.ptr(adj), D.ptr(absmax), D.ptr(gacc), D.ptr(grad), D.stream())
        return grad

    def evaluate(self, blur_sigma, want_adjoint):
        """-> losses (B,) float64 (summed over the directions) and, per direction, (tc, adj4 | None)."""
        total, saved = None, []
        for direction in self.directions:
            tc = self.time_constants(direction)
            losses, adj = self.post(self.planes(tc), blur_sigma, want_adjoint)
            total = losses if total is None else total + losses
            saved.append((tc, adj))
        return total, saved

    def gradients(self, saved):
        total = None
        for tc, adj in saved:
            g = self.gradient(tc, adj)
            total = g if total is None else total + g
        return total

    def shaped(self, a):
        """A per-sample result in the caller's shape: the batch axis only where the caller passed one."""
        return a if self.batched else a[0]


_OBJECTIVES = {"variance": _lib.EVK_FLOWCM_VARIANCE, "mean_square": _lib.EVK_FLOWCM_MEAN_SQUARE}


class _ContrastSetup(_Setup):
    """_Setup for the contrast loss: one weighted plane in place of the four, its own post-pass and gather / scatter entries.
    evaluate() and gradients() are the base class's: what travels between the steps is (iwe | adj, qmax) in place of a tensor."""

    def __init__(self, flow, xs, ys, ts, ps, direction, offsets, objective, use_polarity):
        if objective not in _OBJECTIVES:
            raise ValueError("objective must be 'variance' or 'mean_square', got %r" % (objective,))
        _Setup.__init__(self, flow, xs, ys, ts, ps, direction, offsets)
        self.objective = _OBJECTIVES[objective]
        self.flags = 0 if use_polarity else _lib.EVK_FLOWCM_ABS
        self.cols = self.cols[:3] + (self.weights[0],)

    def tail(self, tc):
        return (D.ptr(tc), self.weights[1], self.flags)

    def planes(self, tc):
        """(iwe (B, H+1, W+1) float32, qmax (B,): the bit pattern of max |q| per sample): one pass over the events."""
        shape = (self.B, self.H + 1, self.W + 1)
        acc = torch.zeros(shape, dtype=torch.int64, device=self.device)
        qmax = torch.empty(self.B, dtype=torch.int32, device=self.device)
        iwe = torch.empty(shape, dtype=torch.float32, device=self.device)
        _lib.call("evk_flowcm_warp_f32", *self.head(), *self.tail(tc), D.ptr(qmax), D.ptr(acc), D.ptr(iwe), D.stream())
        return iwe, qmax

    def post(self, planes, blur_sigma, want_adjoint):
        """evk_flowcm_post_f32 sample by sample -> losses (B,) float64 and (adj (B, H+1, W+1) | None, qmax)."""
        (iwe, qmax), dev, (ch, cw) = planes, self.device, (self.H + 1, self.W + 1)
        w, radius = _blur_kernel(blur_sigma)
        wd = torch.from_numpy(w).to(dev) if _wide(radius) else None
        losses = torch.empty(self.B, dtype=torch.float64, device=dev)
        work = torch.empty((3, ch, cw), dtype=torch.float32, device=dev)
        adj = torch.empty((self.B, ch, cw), dtype=torch.float32, device=dev) if want_adjoint else None
        scratch, nbytes = D.reduce_scratch(dev)
        for b in range(self.B):
            _lib.call("evk_flowcm_post_f32", D.ptr(iwe[b]), ch, cw, D.host_ptr(w) if w is not None else None, D.ptr(wd), radius,
                      self.objective, D.ptr(work), D.ptr(adj[b]) if want_adjoint else None, D.ptr(losses[b:]), D.ptr(scratch),
                      nbytes, D.stream())
        return losses, (adj, qmax)

    def gradient(self, tc, saved):
        adj, qmax = saved
        shape = (self.B, 2, self.H, self.W)
        gacc = torch.zeros(shape, dtype=torch.int64, device=self.device)
        absmax = torch.empty(self.B, dtype=torch.int32, device=self.device)
        grad = torch.empty(shape, dtype=torch.float32, device=self.device)
        _lib.call("evk_flowcm_grad_f32", *self.head(), *self.tail(tc), D.ptr(adj), D.ptr(qmax), D.ptr(absmax), D.ptr(gacc),
                  D.ptr(grad), D.stream())
        return grad


def flow_field_timestamp_images(flow, xs, ys=None, ts=None, ps=None, direction="forward", offsets=None):
    """The pair of average-timestamp images A_c = T_c / (1 + C_c) (c = positive, non-positive events) of the events warped by
    the dense field `flow`: (2, H, W) -> (2, H+1, W+1), or (B, 2, H, W) with the samples' events concatenated and `offsets`
    (B + 1,) -> (B, 2, H+1, W+1); float32 device tensor.  The field's (H, W) is the sensor size.  One pass over the events: what
    get_timestamp_images gives on the output of warp_events_flow_torch, without materialising the warped columns.  direction:
    'forward' (warp to the sample's last timestamp, tau = (t - t_first) / tdiv) or 'backward' (to its first, tau =
    (t_last - t) / tdiv); 'both' has no single pair of images and is refused.  xs may be a DeviceEvents."""
    if direction == "both":
        raise ValueError("direction 'both' is a sum of two losses and has no single pair of images: ask for each direction")
    s = _Setup(flow, xs, ys, ts, ps, direction, offsets)
    planes = s.planes(s.time_constants(s.directions[0]))
    out = torch.empty((s.B, 2, s.H + 1, s.W + 1), dtype=torch.float32, device=s.device)
    for b in range(s.B):
        _lib.call("evk_tsimg_average_f32", D.ptr(planes[b]), s.H + 1, s.W + 1, D.ptr(out[b]), D.stream())
    return s.shaped(out)


def flow_field_timestamp_loss(flow, xs, ys=None, ts=None, ps=None, blur_sigma=2.0, direction="forward", offsets=None,
                              compute_gradient=False):
    """The average-timestamp loss of Zhu et al. (CVPR 2019) of a dense flow field (definition: include/evk.h, steps 1', 2-7, 8'):
    every event is moved by the bilinear sample of `flow` at its position times (t - t_ref), the moved events are splatted per
    polarity class into sum-of-tau and count images, A_c = T_c / (1 + C_c), blurred with `blur_sigma` (<= 0: no blur), and the
    loss is sum B_+^2 + sum B_-^2, to be minimised.  direction 'forward' / 'backward' / 'both' (their sum: the paper's loss).
      flow (2, H, W)                     -> loss: 0-dim float64 device tensor
      flow (B, 2, H, W), offsets (B + 1,) -> losses: (B,) float64 device tensor; the samples' events are concatenated, every
                                            sample has its own time constants (read on the device: no host round trip per sample).
    With compute_gradient the result is (loss, gradient): dloss/dflow in the shape of flow, float32, exact (the adjoint) and, like
    the loss, the same bits from call to call.  xs may be a DeviceEvents (its p_scale decides the polarity classes).  Events are
    expected in stream order per sample; an empty sample has loss 0 and a zero gradient."""
    s = _Setup(flow, xs, ys, ts, ps, direction, offsets)
    losses, saved = s.evaluate(blur_sigma, compute_gradient)
    if not compute_gradient:
        return s.shaped(losses)
    return s.shaped(losses), s.shaped(s.gradients(saved))


class _FlowTimestampLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, flow, setup, blur_sigma):
        losses, saved = setup.evaluate(blur_sigma, ctx.needs_input_grad[0])
        ctx.setup, ctx.saved = setup, saved
        return setup.shaped(losses)

    @staticmethod
    def backward(ctx, grad_out):
        s = ctx.setup
        g = s.gradients(ctx.saved)                                          # the only event pass of backward (one per direction)
        return s.shaped(g * grad_out.reshape(-1, 1, 1, 1).to(torch.float32)), None, None


def flow_timestamp_loss(flow, xs, ys=None, ts=None, ps=None, blur_sigma=2.0, direction="forward", offsets=None):
    """flow_field_timestamp_loss as a differentiable function of `flow` (a float32 device tensor, usually the output of a
    network): the same value, and loss.backward() / loss.sum().backward() adds dloss/dflow -- scaled per sample by the incoming
    gradient -- to flow.grad.  The forward pass keeps the adjoint images; backward runs the one gather / scatter kernel over the
    events (per direction) and nothing else."""
    if not isinstance(flow, torch.Tensor) or flow.dtype != torch.float32 or not flow.is_cuda:
        raise ValueError("flow_timestamp_loss takes a float32 device tensor (for host data: flow_field_timestamp_loss)")
    s = _Setup(flow, xs, ys, ts, ps, direction, offsets)
    return _FlowTimestampLoss.apply(flow, s, blur_sigma)


def flow_field_iwe(flow, xs, ys=None, ts=None, ps=None, direction="forward", offsets=None, use_polarity=True):
    """The image of the events warped by the dense field `flow`, I = sum_e q_e (four bilinear weights of (x', y')) with q = p (or
    |p| without use_polarity): (2, H, W) -> (H+1, W+1), or (B, 2, H, W) with `offsets` -> (B, H+1, W+1); float32 device tensor.
    What events_to_image_torch(bilinear, padding) gives on the output of warp_events_flow_torch, in one pass, without the warped
    columns and -- summed in fixed point -- the same bits from call to call.  direction 'forward' / 'backward' as for
    flow_field_timestamp_images; 'both' has no single image and is refused.  xs may be a DeviceEvents (p_scale multiplies p)."""
    if direction == "both":
        raise ValueError("direction 'both' is a sum of two losses and has no single image: ask for each direction")
    s = _ContrastSetup(flow, xs, ys, ts, ps, direction, offsets, "variance", use_polarity)
    return s.shaped(s.planes(s.time_constants(s.directions[0]))[0])


def flow_field_contrast_loss(flow, xs, ys=None, ts=None, ps=None, objective="variance", blur_sigma=1.0, direction="forward",
                             offsets=None, use_polarity=True, compute_gradient=False):
    """The contrast (focus) loss of a dense flow field (definition: include/evk.h, "Contrast loss of a flow field"): the events,
    moved as in flow_field_timestamp_loss, are splatted with their polarities (|p| without use_polarity) into one image, blurred
    with `blur_sigma` (<= 0: no blur) to B, and the loss -- to be minimised -- is
      objective 'variance'     -mean((B - mean B)^2)   (variance_objective with reference_exact=False, over the padded image)
      objective 'mean_square'  -mean(B^2)
    direction 'forward' / 'backward' / 'both' (their sum).  Shapes, batches (`offsets`), DeviceEvents and compute_gradient as for
    flow_field_timestamp_loss: (loss, dloss/dflow) with the gradient float32 in the shape of flow, exact (the adjoint) and, like
    the loss, the same bits from call to call.  An empty sample has loss 0 and a zero gradient."""
    s = _ContrastSetup(flow, xs, ys, ts, ps, direction, offsets, objective, use_polarity)
    losses, saved = s.evaluate(blur_sigma, compute_gradient)
    if not compute_gradient:
        return s.shaped(losses)
    return s.shaped(losses), s.shaped(s.gradients(saved))


def flow_contrast_loss(flow, xs, ys=None, ts=None, ps=None, objective="variance", blur_sigma=1.0, direction="forward",
                       offsets=None, use_polarity=True):
    """flow_field_contrast_loss as a differentiable function of `flow` (a float32 device tensor): the same value, and backward
    adds dloss/dflow, scaled per sample by the incoming gradient, to flow.grad.  The forward pass keeps the adjoint image;
    backward runs the one gather / scatter kernel over the events (per direction) and nothing else."""
    if not isinstance(flow, torch.Tensor) or flow.dtype != torch.float32 or not flow.is_cuda:
        raise ValueError("flow_contrast_loss takes a float32 device tensor (for host data: flow_field_contrast_loss)")
    s = _ContrastSetup(flow, xs, ys, ts, ps, direction, offsets, objective, use_polarity)
    return _FlowTimestampLoss.apply(flow, s, blur_sigma)
