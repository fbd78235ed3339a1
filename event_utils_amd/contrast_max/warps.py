"""Motion-model plugins.  Reference: lib/contrast_max/warps.py (warp_function ABC :6-42, linvel_warp :44-61)."""
from abc import ABC, abstractmethod

import numpy as np
import torch

from .. import _device as D
from .. import _lib


class warp_function(ABC):
    """Base class of warps: .name, .dims and .warp(xs, ys, ts, ps, t0, params, compute_grad=False) ->
    (xs_warped, ys_warped, jacobian_x | None, jacobian_y | None) (reference: warps.py:6-42)."""

    def __init__(self, name, dims):
        self.name = name
        self.dims = dims
        super().__init__()

    @abstractmethod
    def warp(self, xs, ys, ts, ps, t0, params, compute_grad=False):
        pass


class linvel_warp(warp_function):
    """Linear velocity (global optic flow) warp (reference: warps.py:44-61):
    x' = x-(t-t0)*vx, y' = y-(t-t0)*vy, jacobian_x = [-dt; 0], jacobian_y = [0; -dt] (float64).
    When get_iwe / the objectives see this class they use the fused warp->mask->splat kernel instead of calling
    .warp() and materialising x', y' and the two (2, N) Jacobians."""

    fused_kernel = "linvel"          # informational; dispatch goes through uses_fused_linvel()

    def __init__(self):
        warp_function.__init__(self, 'linvel_warp', 2)

    def warp(self, xs, ys, ts, ps, t0, params, compute_grad=False):
        dev = D.require_gpu()
        on_device = isinstance(xs, torch.Tensor)
        xd, yd, td = (D.to_device(a, torch.float64, dev) for a in (xs, ys, ts))
        n = xd.shape[0]
        xo, yo = torch.empty_like(xd), torch.empty_like(yd)
        jx = torch.empty((2, n), dtype=torch.float64, device=dev) if compute_grad else None
        jy = torch.empty((2, n), dtype=torch.float64, device=dev) if compute_grad else None
        _lib.call("evk_warp_linvel_f64", D.ptr(xd), D.ptr(yd), D.ptr(td), n, float(t0), float(params[0]),
                  float(params[1]), D.ptr(xo), D.ptr(yo), D.ptr(jx), D.ptr(jy), D.stream())
        if on_device:
            return xo, yo, jx, jy
        return (xo.cpu().numpy(), yo.cpu().numpy(), jx.cpu().numpy() if compute_grad else None,
                jy.cpu().numpy() if compute_grad else None)


def uses_fused_linvel(warpfunc):
    """True when `warpfunc` warps exactly like linvel_warp, so that the fused warp -> mask -> splat kernels may replace
    its warp(): the class itself, or a subclass that did NOT override warp() (a plugin that did must be called)."""
    return isinstance(warpfunc, linvel_warp) and type(warpfunc).warp is linvel_warp.warp


def warp_events(xs, ys, ts, ps, t0, params, compute_grad=False):
    """Alias named by BASELINE.json's north_star: linvel_warp().warp(...) (SURVEY.md headline facts)."""
    return linvel_warp().warp(xs, ys, ts, ps, t0, params, compute_grad=compute_grad)


def _warp_param(model, dims, xs, ys, ts, t0, host_params, compute_grad):
    """warp() of the parametric models through evk_warp_param_f64: numpy in -> numpy out, device tensors in -> device out."""
    dev = D.require_gpu()
    on_device = isinstance(xs, torch.Tensor)
    xd, yd, td = (D.to_device(a, torch.float64, dev) for a in (xs, ys, ts))
    n = xd.shape[0]
    xo, yo = torch.empty_like(xd), torch.empty_like(yd)
    jx = torch.empty((dims, n), dtype=torch.float64, device=dev) if compute_grad else None
    jy = torch.empty((dims, n), dtype=torch.float64, device=dev) if compute_grad else None
    hp = np.ascontiguousarray(host_params, dtype=np.float64)
    _lib.call("evk_warp_param_f64", model, D.ptr(xd), D.ptr(yd), D.ptr(td), n, float(t0), D.host_ptr(hp), D.ptr(xo),
              D.ptr(yo), D.ptr(jx), D.ptr(jy), D.stream())
    if on_device:
        return xo, yo, jx, jy
    return (xo.cpu().numpy(), yo.cpu().numpy(), jx.cpu().numpy() if compute_grad else None,
            jy.cpu().numpy() if compute_grad else None)


class xyztheta_warp(warp_function):
    """4-DoF x, y, z, rotation warp after Mitrokhin et al., "Event-based moving object detection and tracking" (upstream:
    an empty stub, warps.py:63-72).  First-order velocity field: translation, expansion along the optical axis and in-plane
    rotation about `center`.  params = (vx, vy, vz, omega); dt = t - t0, (u, v) = (x - center[0], y - center[1]):
      x' = x - dt*(vx + vz*u - omega*v),   y' = y - dt*(vy + vz*v + omega*u)
      J(vx) = (-dt, 0), J(vy) = (0, -dt), J(vz) = (-dt*u, -dt*v), J(omega) = (dt*v, -dt*u)
    with J(i) = (jacobian_x[i], jacobian_y[i]), (4, N) float64.  At (vx, vy, 0, 0) this is linvel_warp at (vx, vy).
    get_iwe / the objectives use the fused warp -> mask -> splat kernel (evk_iwe_param_*) for this class."""

    fused_model = _lib.EVK_WARP_XYZTHETA

    def __init__(self, center=(0.0, 0.0)):
        warp_function.__init__(self, 'xyztheta_warp', 4)
        self.center = (float(center[0]), float(center[1]))

    def host_params(self, params):
        """The model's argument block of the library calls: (vx, vy, vz, omega, centre x, centre y)."""
        return np.array([float(params[0]), float(params[1]), float(params[2]), float(params[3]), self.center[0],
                         self.center[1]], dtype=np.float64)

    def default_params(self, img_size):
        return np.zeros(4)

    def warp(self, xs, ys, ts, ps, t0, params, compute_grad=False):
        return _warp_param(self.fused_model, 4, xs, ys, ts, t0, self.host_params(params), compute_grad)


class pure_rotation_warp(warp_function):
    """Pure rotation warp (upstream: an empty stub, warps.py:74-83), params = (cx, cy, omega): centre of rotation and
    angular velocity.  theta = -omega*dt, c = cos(theta), s = sin(theta), (u, v) = (x - cx, y - cy):
      x' = cx + c*u - s*v,   y' = cy + s*u + c*v
      J(cx) = (1-c, -s), J(cy) = (s, 1-c), J(omega) = (dt*(s*u + c*v), -dt*(c*u - s*v))
    dims = 3 (upstream's code says 4 while its docstring and README name three parameters).
    get_iwe / the objectives use the fused warp -> mask -> splat kernel (evk_iwe_param_*) for this class."""

    fused_model = _lib.EVK_WARP_ROTATION

    def __init__(self):
        warp_function.__init__(self, 'pure_rotation_warp', 3)

    def host_params(self, params):
        return np.array([float(params[0]), float(params[1]), float(params[2])], dtype=np.float64)

    def default_params(self, img_size):
        """The image centre and omega = 0 (at omega = 0 the centre derivatives vanish: (0, 0) would be a poor start)."""
        return np.array([img_size[1] / 2.0, img_size[0] / 2.0, 0.0])

    def warp(self, xs, ys, ts, ps, t0, params, compute_grad=False):
        return _warp_param(self.fused_model, 3, xs, ys, ts, t0, self.host_params(params), compute_grad)


def uses_fused_param(warpfunc):
    """True when `warpfunc` warps exactly like pure_rotation_warp or xyztheta_warp, so that the fused kernels
    (evk_iwe_param_*) may replace its warp(): the classes themselves, or subclasses that did NOT override warp()."""
    for cls in (pure_rotation_warp, xyztheta_warp):
        if isinstance(warpfunc, cls) and type(warpfunc).warp is cls.warp:
            return True
    return False
