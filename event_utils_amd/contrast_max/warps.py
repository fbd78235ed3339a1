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


class angular_velocity_warp(warp_function):
    """3-DoF camera rotation through the intrinsics, after Gallego & Scaramuzza, "Accurate Angular Velocity Estimation with
    an Event Camera": params = (wx, wy, wz), the camera's body-frame angular velocity in rad/s for a static scene.
    camera_matrix K = [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (no skew; events already undistorted).  dt = t - t0:
      b = ((x - cx)/fx, (y - cy)/fy, 1),  theta = (wx, wy, wz)*dt,  R = exp([theta]x) (Rodrigues)
      P = R b,  x' = fx*P0/P2 + cx,  y' = fy*P1/P2 + cy
      dP/dw = -R [b]x Jr(theta) dt,  Jr(theta) = I - (1-cos a)/a^2 [theta]x + (a - sin a)/a^3 [theta]x^2,  a = |theta|
      J = [[fx/P2, 0, -fx*P0/P2^2], [0, fy/P2, -fy*P1/P2^2]] . dP/dw
    with J(i) = (jacobian_x[i], jacobian_y[i]), (3, N) float64.  An event with P2 <= 0 (rotated behind the camera) or a
    non-finite P warps to x' = y' = NaN; the fused IWE drops it.  With fx == fy and w = (0, 0, wz) this is
    pure_rotation_warp at (cx, cy, -wz).  get_iwe / the objectives use the fused warp -> mask -> splat kernel
    (evk_iwe_param_*) for this class."""

    fused_model = _lib.EVK_WARP_ANGULAR_VELOCITY

    def __init__(self, camera_matrix):
        warp_function.__init__(self, 'angular_velocity_warp', 3)
        K = np.asarray(camera_matrix, dtype=np.float64)
        if K.shape != (3, 3):
            raise ValueError("camera_matrix must be 3x3, got shape %s" % (K.shape,))
        if not np.all(np.isfinite(K)) or K[0, 1] != 0 or K[1, 0] != 0 or K[2, 0] != 0 or K[2, 1] != 0 or K[2, 2] != 1:
            raise ValueError("camera_matrix must be [[fx, 0, cx], [0, fy, cy], [0, 0, 1]] (no skew)")
        if not (K[0, 0] > 0 and K[1, 1] > 0):
            raise ValueError("camera_matrix needs fx > 0 and fy > 0")
        self.camera_matrix = K
        self.fx, self.fy, self.cx, self.cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])

    def host_params(self, params):
        """The model's argument block of the library calls: (wx, wy, wz, fx, fy, cx, cy)."""
        return np.array([float(params[0]), float(params[1]), float(params[2]), self.fx, self.fy, self.cx, self.cy],
                        dtype=np.float64)

    def default_params(self, img_size):
        return np.zeros(3)

    def warp(self, xs, ys, ts, ps, t0, params, compute_grad=False):
        return _warp_param(self.fused_model, 3, xs, ys, ts, t0, self.host_params(params), compute_grad)


class planar_flow_warp(warp_function):
    """8-parameter planar-surface motion field: the instantaneous (linearised) homography of "A Unifying Contrast
    Maximization Framework" (Gallego et al., CVPR 2018) -- affine terms plus two projective terms.  params = (a1, .., a8);
    dt = t - t0, (u, v) = (x - center[0], y - center[1]):
      x' = x - dt*(a1 + a2*u + a3*v + a7*u^2 + a8*u*v),   y' = y - dt*(a4 + a5*u + a6*v + a7*u*v + a8*v^2)
      J(a1) = (-dt, 0), J(a2) = (-dt*u, 0), J(a3) = (-dt*v, 0), J(a4) = (0, -dt), J(a5) = (0, -dt*u), J(a6) = (0, -dt*v)
      J(a7) = (-dt*u^2, -dt*u*v), J(a8) = (-dt*u*v, -dt*v^2)
    with J(i) = (jacobian_x[i], jacobian_y[i]), (8, N) float64.  xyztheta_warp(center) at (vx, vy, vz, w) is this at
    (vx, vz, -w, vy, w, vz, 0, 0); linvel_warp at (vx, vy) is this at (vx, 0, 0, vy, 0, 0, 0, 0).  get_iwe / the objectives
    use the fused warp -> mask -> splat kernel (evk_iwe_param_*) for this class."""

    fused_model = _lib.EVK_WARP_PLANAR_FLOW

    def __init__(self, center=(0.0, 0.0)):
        warp_function.__init__(self, 'planar_flow_warp', 8)
        self.center = (float(center[0]), float(center[1]))

    def host_params(self, params):
        """The model's argument block of the library calls: (a1, .., a8, centre x, centre y)."""
        return np.array([float(params[i]) for i in range(8)] + [self.center[0], self.center[1]], dtype=np.float64)

    def default_params(self, img_size):
        return np.zeros(8)

    def param_scale(self, img_size):
        """Units in which the eight parameters move an event at the image border alike: with L = half the larger image side,
        (1, 1/L, 1/L, 1, 1/L, 1/L, 1/L^2, 1/L^2) (optimize_contrast(optimizer='evk_bfgs') with a step-bounded loss)."""
        L = max(float(img_size[0]), float(img_size[1])) / 2.0
        return np.array([1.0, 1.0 / L, 1.0 / L, 1.0, 1.0 / L, 1.0 / L, 1.0 / (L * L), 1.0 / (L * L)])

    def warp(self, xs, ys, ts, ps, t0, params, compute_grad=False):
        return _warp_param(self.fused_model, 8, xs, ys, ts, t0, self.host_params(params), compute_grad)


def uses_fused_param(warpfunc):
    """True when `warpfunc` warps exactly like pure_rotation_warp, xyztheta_warp, angular_velocity_warp or planar_flow_warp,
    so that the fused kernels (evk_iwe_param_*) may replace its warp(): the classes themselves, or
    subclasses that did NOT override warp()."""
    for cls in (pure_rotation_warp, xyztheta_warp, angular_velocity_warp, planar_flow_warp):
        if isinstance(warpfunc, cls) and type(warpfunc).warp is cls.warp:
            return True
    return False

