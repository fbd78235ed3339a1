// The motion models of the fused kernels as the per-event code reads them: parameters, Jacobian layout and the float64 warp
// with its Jacobian; and on the host the model dispatch and the band / chunk geometry of the band splats.  Shared by the fused
// IWE (evk_warps.hip), the average-timestamp objective (evk_tsobj.hip) and the motion segmentation (evk_segment.hip), so that
// an event lands on the same pixel with the same fractions in all of them.  The model-independent helpers of these files
// (and of evk_flowloss.hip, which has no motion model) are in evk_accum.h.
#pragma once
#include <type_traits>

#include "evk_common.h"

namespace evk {

// Model id of the linear flow in the entries that take it (evk_tsimg_warp_*, evk_tsobj_grad_*); the evk_iwe_param_* entries
// refuse it (the linear flow has its own kernels there).
constexpr int kWarpLinvel = EVK_WARP_LINVEL;

// One model's parameters as the per-event code reads them: host_params as documented in evk.h.
struct WarpArgs {
    double q[10];
};

constexpr int kMaxDims = 8;
constexpr int kJac = 6;  // float Jacobian values carried per event, at most
constexpr int kBandThreads = 1024;
constexpr size_t kBandLds = (size_t)160 * 1024;

// Per model: dims, the length of host_params, the number of carried Jacobian values, and the index among them of plane k's
// (jx_k, jy_k); -1 is a structural zero.
template <int M>
struct Model;
template <>
struct Model<kWarpLinvel> {  // host_params = (vx, vy); s = -dt: jx = (s, 0), jy = (0, s)
    static constexpr int dims = 2, nparams = 2, njac = 1;
    __host__ __device__ static constexpr int jx(int k) { return k == 0 ? 0 : -1; }
    __host__ __device__ static constexpr int jy(int k) { return k == 1 ? 0 : -1; }
};
template <>
struct Model<EVK_WARP_ROTATION> {  // (jx0..2, jy0..2)
    static constexpr int dims = 3, nparams = 3, njac = 6;
    __host__ __device__ static constexpr int jx(int k) { return k; }
    __host__ __device__ static constexpr int jy(int k) { return 3 + k; }
};
template <>
struct Model<EVK_WARP_XYZTHETA> {  // s = (-dt, -dt u, -dt v, dt v): jx = (s0, 0, s1, s3), jy = (0, s0, s2, s1)
    static constexpr int dims = 4, nparams = 6, njac = 4;
    __host__ __device__ static constexpr int jx(int k) { return k == 0 ? 0 : k == 1 ? -1 : k == 2 ? 1 : 3; }
    __host__ __device__ static constexpr int jy(int k) { return k == 0 ? -1 : k == 1 ? 0 : k == 2 ? 2 : 1; }
};
template <>
struct Model<EVK_WARP_ANGULAR_VELOCITY> {  // (jx0..2, jy0..2)
    static constexpr int dims = 3, nparams = 7, njac = 6;
    __host__ __device__ static constexpr int jx(int k) { return k; }
    __host__ __device__ static constexpr int jy(int k) { return 3 + k; }
};
// c = -dt (1, u, v, u^2, uv, v^2): jx = (c0, c1, c2, 0, 0, 0, c3, c4), jy = (0, 0, 0, c0, c1, c2, c4, c5)
template <>
struct Model<EVK_WARP_PLANAR_FLOW> {
    static constexpr int dims = 8, nparams = 10, njac = 6;
    __host__ __device__ static constexpr int jx(int k) { return k < 3 ? k : k < 6 ? -1 : k - 3; }
    __host__ __device__ static constexpr int jy(int k) { return k < 3 ? -1 : k < 6 ? k - 3 : k - 2; }
};

// a x b
__device__ __forceinline__ void cross(const double *a, const double *b, double *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// v + s1 (th x v) + s2 (th x (th x v)): exp([th]x) v with (s1, s2) = (A, B)
__device__ __forceinline__ void rodrigues(const double *th, double s1, double s2, const double *v, double *o) {
    double c1[3], c2[3];
    cross(th, v, c1);
    cross(th, c1, c2);
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = v[i] + s1 * c1[i] + s2 * c2[i];
}

// x' = warp(x, y, dt) and, with JAC, the Model<M>::njac Jacobian values (layout: Model<M>::jx / jy); float64 throughout,
// separate roundings (-ffp-contract=off).  Angular velocity: an event whose P2 <= 0 (rotated behind the camera) or whose P
// is not finite gets x' = y' = NaN and a NaN Jacobian.
template <int M, bool JAC>
__device__ __forceinline__ void warp_event(const WarpArgs &w, double x, double y, double dt, double &xo, double &yo,
                                           double *j) {
    if constexpr (M == kWarpLinvel) {  // evk_iwe_linvel_*'s expressions (warps.py:52-54)
        xo = x - dt * w.q[0];
        yo = y - dt * w.q[1];
        if constexpr (JAC) j[0] = -dt;
    } else if constexpr (M == EVK_WARP_ROTATION) {
        const double cx = w.q[0], cy = w.q[1];
        const double u = x - cx, v = y - cy;
        const double theta = -w.q[2] * dt;
        double s, c;
        sincos(theta, &s, &c);
        xo = cx + c * u - s * v;
        yo = cy + s * u + c * v;
        if constexpr (JAC) {
            j[0] = 1.0 - c, j[3] = -s;
            j[1] = s, j[4] = 1.0 - c;
            j[2] = dt * (s * u + c * v), j[5] = -dt * (c * u - s * v);
        }
    } else if constexpr (M == EVK_WARP_XYZTHETA) {
        const double u = x - w.q[4], v = y - w.q[5];
        xo = x - dt * (w.q[0] + w.q[2] * u - w.q[3] * v);
        yo = y - dt * (w.q[1] + w.q[2] * v + w.q[3] * u);
        if constexpr (JAC) {
            j[0] = -dt;
            j[1] = -dt * u;
            j[2] = -dt * v;
            j[3] = dt * v;
        }
    } else if constexpr (M == EVK_WARP_ANGULAR_VELOCITY) {
        const double fx = w.q[3], fy = w.q[4], cx = w.q[5], cy = w.q[6];
        const double b[3] = {(x - cx) / fx, (y - cy) / fy, 1.0};
        const double th[3] = {w.q[0] * dt, w.q[1] * dt, w.q[2] * dt};
        const double a2 = th[0] * th[0] + th[1] * th[1] + th[2] * th[2];
        double A, B, C;  // sin a / a, (1 - cos a) / a^2, (a - sin a) / a^3
        if (a2 < 1e-4) {  // series: the next terms are below 2^-52 of each for a < 1e-2
            A = 1.0 - a2 / 6.0 + a2 * a2 / 120.0;
            B = 0.5 - a2 / 24.0 + a2 * a2 / 720.0;
            C = 1.0 / 6.0 - a2 / 120.0 + a2 * a2 / 5040.0;
        } else {
            const double a = sqrt(a2);
            double s, c;
            sincos(a, &s, &c);
            A = s / a;
            B = (1.0 - c) / a2;
            C = (a - s) / (a2 * a);
        }
        double P[3];
        rodrigues(th, A, B, b, P);
        const bool ok = P[2] > 0.0 && isfinite(P[0]) && isfinite(P[1]) && isfinite(P[2]);
        if (!ok) {
            xo = yo = __builtin_nan("");
            if constexpr (JAC) {
#pragma unroll
                for (int k = 0; k < Model<M>::njac; ++k) j[k] = __builtin_nan("");
            }
            return;
        }
        const double iz = 1.0 / P[2];
        xo = fx * P[0] * iz + cx;
        yo = fy * P[1] * iz + cy;
        if constexpr (JAC) {
            // dP/dw = -R [b]x Jr(th) dt = -[P]x Jl(th) dt (R [b]x = [R b]x R, R Jr(th) = Jl(th) = I + B [th]x + C [th]x^2),
            // so dP/dw_k = dt (Jl e_k) x P, Jl e_k = (1 - C a^2) e_k + B (th x e_k) + C th_k th;
            // J = [[fx/P2, 0, -fx P0/P2^2], [0, fy/P2, -fy P1/P2^2]] dP/dw
            const double gx = fx * iz, gy = fy * iz, hx = fx * P[0] * iz * iz, hy = fy * P[1] * iz * iz;
            const double d0 = 1.0 - C * a2;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                // th x e_k
                const double tx[3] = {k == 0 ? 0.0 : k == 1 ? -th[2] : th[1], k == 0 ? th[2] : k == 1 ? 0.0 : -th[0],
                                      k == 0 ? -th[1] : k == 1 ? th[0] : 0.0};
                double l[3], d[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) l[i] = (i == k ? d0 : 0.0) + B * tx[i] + C * th[k] * th[i];
                cross(l, P, d);
                const double e0 = d[0] * dt, e1 = d[1] * dt, e2 = d[2] * dt;
                j[k] = gx * e0 - hx * e2;
                j[3 + k] = gy * e1 - hy * e2;
            }
        }
    } else {
        static_assert(M == EVK_WARP_PLANAR_FLOW, "unknown model");
        const double u = x - w.q[8], v = y - w.q[9];
        const double uu = u * u, uv = u * v, vv = v * v;
        xo = x - dt * (w.q[0] + w.q[1] * u + w.q[2] * v + w.q[6] * uu + w.q[7] * uv);
        yo = y - dt * (w.q[3] + w.q[4] * u + w.q[5] * v + w.q[6] * uv + w.q[7] * vv);
        if constexpr (JAC) {
            const double nd = -dt;
            j[0] = nd;
            j[1] = nd * u;
            j[2] = nd * v;
            j[3] = nd * uu;
            j[4] = nd * uv;
            j[5] = nd * vv;
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------

// f(std::integral_constant<int, M>{}) for model id M; 0 for an id that names no model, and for the linear flow without LINVEL.
template <bool LINVEL, class F>
inline int with_model(int model, F f) {
    switch (model) {
    case kWarpLinvel:
        if constexpr (LINVEL) return f(std::integral_constant<int, kWarpLinvel>{});
        break;
    case EVK_WARP_ROTATION: return f(std::integral_constant<int, EVK_WARP_ROTATION>{});
    case EVK_WARP_XYZTHETA: return f(std::integral_constant<int, EVK_WARP_XYZTHETA>{});
    case EVK_WARP_ANGULAR_VELOCITY: return f(std::integral_constant<int, EVK_WARP_ANGULAR_VELOCITY>{});
    case EVK_WARP_PLANAR_FLOW: return f(std::integral_constant<int, EVK_WARP_PLANAR_FLOW>{});
    }
    return 0;
}

// 0 for an id that with_model<LINVEL> refuses: the entries' test of `model`
template <bool LINVEL>
inline int model_dims(int model) {
    return with_model<LINVEL>(model, [](auto m) { return Model<decltype(m)::value>::dims; });
}

// hp holds exactly the model's own count of doubles; the caller has tested `model` with model_dims
inline WarpArgs warp_args(int model, const double *hp) {
    WarpArgs w = {};
    const int k = with_model<true>(model, [](auto m) { return Model<decltype(m)::value>::nparams; });
    for (int i = 0; i < k; ++i) w.q[i] = hp[i];
    return w;
}

// Rows of a band: as many as kBandLds holds across `planes` planes of `cell_bytes` cells, at most the canvas.  0, the direct
// kernel: no plane, a canvas without an interior, EVK_IWE_DIRECT, not one row fits, or more than `cap` bands per plane --
// every band re-reads and re-warps the events, so beyond some count of them the direct kernel's atomics cost less.
inline int lds_band_rows(int planes, size_t cell_bytes, int cap, uint32_t flags, int canvas_h, int canvas_w) {
    if (planes < 1 || canvas_h <= 1 || canvas_w <= 1 || (flags & EVK_IWE_DIRECT)) return 0;
    const int64_t row_bytes = (int64_t)planes * canvas_w * (int64_t)cell_bytes;
    int rows = (int)((int64_t)kBandLds / row_bytes);
    if (rows < 1) return 0;
    if (rows > canvas_h) rows = canvas_h;
    const int bands = (canvas_h + rows - 1) / rows;
    if (bands > cap * planes) return 0;
    return rows;
}

// The band kernels' grid.x: about one workgroup per CU in all (each holds nearly the whole LDS), but no chunk under 16 k
// events -- below that the band's flush, not the events, is the workgroup's work; chunk is a multiple of 4 events.
struct ChunkPlan {
    int64_t chunk, chunks;
};
inline ChunkPlan chunk_plan(int64_t n, int bands) {
    int64_t chunks = EVK_NUM_CU / bands;
    const int64_t min_chunk = 16384;
    if (chunks < 1) chunks = 1;
    if (chunks > (n + min_chunk - 1) / min_chunk) chunks = (n + min_chunk - 1) / min_chunk;
    int64_t chunk = (n + chunks - 1) / chunks;
    chunk = (chunk + 3) & ~(int64_t)3;
    chunks = (n + chunk - 1) / chunk;
    return {chunk, chunks};
}

}  // namespace evk
