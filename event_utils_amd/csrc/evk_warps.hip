// Parametric motion models beyond the linear flow ("Rotation and xyztheta warps"): the elementwise warp with its
// Jacobians, the fused warp -> mask -> splat IWE with `dims` derivative planes, and the plane sums of the gradient post-pass.
//
// The fused IWE has two forms with the same per-event code (param_event):
//   band   -- each workgroup owns a band of canvas rows across all 1 + dims planes in LDS, streams one chunk of the events,
//             adds the contributions whose row falls in its band with LDS float adds and flushes the band row by row with
//             global float atomics (contiguous bytes per wave instruction).  Every band re-reads and re-warps the events.
//   direct -- one pass, every contribution a global float atomic; for canvases too wide for a useful band, and EVK_IWE_DIRECT.
#include "evk_common.h"

namespace evk {

// One model's parameters as the per-event code reads them.
struct WarpArgs {
    double a, b, c, d;  // rotation: cx, cy, omega, -; xyztheta: vx, vy, vz, omega
    double ox, oy;      // origin of (u, v): the centre of rotation / xyztheta's centre
};

constexpr int kMaxDims = 4;
constexpr int kBandThreads = 1024;
constexpr size_t kBandLds = (size_t)160 * 1024;

template <int M>
struct ModelDims;
template <>
struct ModelDims<EVK_WARP_ROTATION> {
    static constexpr int value = 3;
};
template <>
struct ModelDims<EVK_WARP_XYZTHETA> {
    static constexpr int value = 4;
};

// x' = warp(x, y, dt) and, with JAC, the (dims) Jacobian columns; float64 throughout, separate roundings (-ffp-contract=off).
template <int M, bool JAC>
__device__ __forceinline__ void warp_event(const WarpArgs &w, double x, double y, double dt, double &xo, double &yo,
                                           double *jx, double *jy) {
    const double u = x - w.ox, v = y - w.oy;
    if constexpr (M == EVK_WARP_ROTATION) {
        const double theta = -w.c * dt;
        double s, c;
        sincos(theta, &s, &c);
        xo = w.ox + c * u - s * v;
        yo = w.oy + s * u + c * v;
        if constexpr (JAC) {
            jx[0] = 1.0 - c, jy[0] = -s;
            jx[1] = s, jy[1] = 1.0 - c;
            jx[2] = dt * (s * u + c * v), jy[2] = -dt * (c * u - s * v);
        }
    } else {
        xo = x - dt * (w.a + w.c * u - w.d * v);
        yo = y - dt * (w.b + w.c * v + w.d * u);
        if constexpr (JAC) {
            jx[0] = -dt, jy[0] = 0.0;
            jx[1] = 0.0, jy[1] = -dt;
            jx[2] = -dt * u, jy[2] = -dt * v;
            jx[3] = dt * v, jy[3] = -dt * u;
        }
    }
}

template <int M>
__global__ void __launch_bounds__(EVK_BLOCK) k_warp_param_f64(const double *__restrict__ x, const double *__restrict__ y,
                                                              const double *__restrict__ t, int64_t n, double t0, WarpArgs w,
                                                              double *__restrict__ xo, double *__restrict__ yo,
                                                              double *__restrict__ jx, double *__restrict__ jy) {
    constexpr int DIMS = ModelDims<M>::value;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double dt = t[i] - t0;
        double a, b, ex[kMaxDims], ey[kMaxDims];
        warp_event<M, true>(w, x[i], y[i], dt, a, b, ex, ey);
        xo[i] = a;
        yo[i] = b;
        if (jx) {
#pragma unroll
            for (int k = 0; k < DIMS; ++k) {
                jx[(int64_t)k * n + i] = ex[k];
                jy[(int64_t)k * n + i] = ey[k];
            }
        }
    }
}

// Per-event part of the fused IWE shared by the band and the direct kernels: warp in float64, events_bounds_mask(0, bw, 0, bh)
// (Q2), p * p_scale [abs], cast to float32, the inner clip, floor / fraction.  False when the event adds nothing.  (The mask
// is written so that a NaN coordinate is rejected too: its splat indices would be meaningless.)
template <int M, bool GRAD, typename T>
__device__ __forceinline__ bool param_event(const WarpArgs &w, T x, T y, T t, T p, double t_ref, double bw, double bh,
                                            float clipx, float clipy, bool abs_p, double p_scale, int &px, int &py, float &dx,
                                            float &dy, float &mp, float *jxf, float *jyf) {
    constexpr int DIMS = ModelDims<M>::value;
    const double dt = (double)t - t_ref;
    double xw, yw, jx[kMaxDims], jy[kMaxDims];
    warp_event<M, GRAD>(w, (double)x, (double)y, dt, xw, yw, jx, jy);
    if (!(xw > 0.0 && xw <= bw && yw > 0.0 && yw <= bh)) return false;
    const double ps = (double)p * p_scale;
    const double pd = abs_p ? fabs(ps) : ps;
    const float xf = (float)xw, yf = (float)yw;
    if (xf >= clipx || yf >= clipy) return false;
    const float fx = floorf(xf), fy = floorf(yf);
    dx = xf - fx;
    dy = yf - fy;
    px = (int)fx;
    py = (int)fy;
    mp = (float)pd;
    if constexpr (GRAD) {
#pragma unroll
        for (int k = 0; k < DIMS; ++k) {
            jxf[k] = (float)jx[k];
            jyf[k] = (float)jy[k];
        }
    }
    return true;
}

// The four IWE weights and, per derivative plane, the four dIWE weights of one event (image.py:111-114, 130-135), in the
// reference's float32 order: w1 = jx * mp, w2 = jy * mp.
struct SplatRow {
    float l, r;  // columns px, px + 1
};

template <int DIMS, bool GRAD>
__device__ __forceinline__ void splat_weights(float dx, float dy, float mp, const float *jxf, const float *jyf, SplatRow *top,
                                              SplatRow *bot) {
    const float ax = 1.0f - dx, ay = 1.0f - dy;
    top[0] = {mp * ax * ay, mp * dx * ay};
    bot[0] = {mp * ax * dy, mp * dx * dy};
    if constexpr (GRAD) {
#pragma unroll
        for (int k = 0; k < DIMS; ++k) {
            const float w1 = jxf[k] * mp, w2 = jyf[k] * mp;
            top[1 + k] = {w1 * (-ay) + w2 * (-ax), w1 * ay + w2 * (-dx)};
            bot[1 + k] = {w1 * (-dy) + w2 * ax, w1 * dy + w2 * dx};
        }
    }
}

template <typename T>
__device__ __forceinline__ Vec4<T> load_quad(const T *p, int64_t base, int cnt, bool vec) {
    if (vec) return load4(p, base >> 2);
    Vec4<T> r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r.v[k] = (k < cnt) ? p[base + k] : T(0);
    return r;
}

__device__ __forceinline__ void lds_add(float *p, float v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// grid = (chunks, bands).  LDS holds planes x band_rows x cw floats; plane k of the band is rows [r0, r1) of plane k.
template <typename T, int M, bool GRAD, bool VEC>
__global__ void __launch_bounds__(kBandThreads) k_iwe_param_band(const T *__restrict__ x, const T *__restrict__ y,
                                                                 const T *__restrict__ t, const T *__restrict__ p, int64_t n,
                                                                 int64_t chunk, WarpArgs w, double t_ref, double bw, double bh,
                                                                 int ch, int cw, int band_rows, bool abs_p, double p_scale,
                                                                 float *__restrict__ iwe, float *__restrict__ diwe) {
    constexpr int DIMS = ModelDims<M>::value;
    constexpr int P = GRAD ? 1 + DIMS : 1;
    extern __shared__ float band[];
    const int r0 = blockIdx.y * band_rows, r1 = min(r0 + band_rows, ch), rows = r1 - r0;
    const int plane_lds = rows * cw;
    for (int i = threadIdx.x; i < P * plane_lds; i += blockDim.x) band[i] = 0.0f;
    __syncthreads();
    const float clipx = (float)(cw - 1), clipy = (float)(ch - 1);
    const int64_t c0 = (int64_t)blockIdx.x * chunk, c1 = min(c0 + chunk, n);
    for (int64_t base = c0 + 4 * (int64_t)threadIdx.x; base < c1; base += 4 * (int64_t)blockDim.x) {
        const int cnt = (int)min((int64_t)4, c1 - base);
        const bool vec = VEC && cnt == 4;
        const Vec4<T> xv = load_quad(x, base, cnt, vec), yv = load_quad(y, base, cnt, vec), tv = load_quad(t, base, cnt, vec),
                      pv = load_quad(p, base, cnt, vec);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= cnt) break;
            int px, py;
            float dx, dy, mp, jxf[kMaxDims], jyf[kMaxDims];
            if (!param_event<M, GRAD, T>(w, xv.v[k], yv.v[k], tv.v[k], pv.v[k], t_ref, bw, bh, clipx, clipy, abs_p, p_scale, px,
                                         py, dx, dy, mp, jxf, jyf))
                continue;
            if (py + 1 < r0 || py >= r1) continue;  // neither of its two rows is in this band
            SplatRow top[P], bot[P];
            splat_weights<DIMS, GRAD>(dx, dy, mp, jxf, jyf, top, bot);
            if (py >= r0) {
                float *q = band + (py - r0) * cw + px;
#pragma unroll
                for (int c = 0; c < P; ++c) {
                    lds_add(q + c * plane_lds, top[c].l);
                    lds_add(q + c * plane_lds + 1, top[c].r);
                }
            }
            if (py + 1 < r1) {
                float *q = band + (py + 1 - r0) * cw + px;
#pragma unroll
                for (int c = 0; c < P; ++c) {
                    lds_add(q + c * plane_lds, bot[c].l);
                    lds_add(q + c * plane_lds + 1, bot[c].r);
                }
            }
        }
    }
    __syncthreads();
    // flush: the band's rows of a plane are contiguous in global memory, so consecutive lanes add to consecutive floats
    const int64_t plane = (int64_t)ch * cw;
#pragma unroll
    for (int c = 0; c < P; ++c) {
        float *dst = (c == 0 ? iwe : diwe + (int64_t)(c - 1) * plane) + (int64_t)r0 * cw;
        const float *src = band + c * plane_lds;
        for (int i = threadIdx.x; i < plane_lds; i += blockDim.x) {
            const float v = src[i];
            if (v != 0.0f) atomic_add(dst + i, v);
        }
    }
}

template <typename T, int M, bool GRAD, bool VEC>
__global__ void __launch_bounds__(EVK_BLOCK) k_iwe_param_direct(const T *__restrict__ x, const T *__restrict__ y,
                                                                const T *__restrict__ t, const T *__restrict__ p, int64_t n,
                                                                WarpArgs w, double t_ref, double bw, double bh, int ch, int cw,
                                                                bool abs_p, double p_scale, float *__restrict__ iwe,
                                                                float *__restrict__ diwe) {
    constexpr int DIMS = ModelDims<M>::value;
    constexpr int P = GRAD ? 1 + DIMS : 1;
    const float clipx = (float)(cw - 1), clipy = (float)(ch - 1);
    const int64_t plane = (int64_t)ch * cw;
    const int64_t stride = 4 * (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = 4 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x); base < n; base += stride) {
        const int cnt = (int)min((int64_t)4, n - base);
        const bool vec = VEC && cnt == 4;
        const Vec4<T> xv = load_quad(x, base, cnt, vec), yv = load_quad(y, base, cnt, vec), tv = load_quad(t, base, cnt, vec),
                      pv = load_quad(p, base, cnt, vec);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= cnt) break;
            int px, py;
            float dx, dy, mp, jxf[kMaxDims], jyf[kMaxDims];
            if (!param_event<M, GRAD, T>(w, xv.v[k], yv.v[k], tv.v[k], pv.v[k], t_ref, bw, bh, clipx, clipy, abs_p, p_scale, px,
                                         py, dx, dy, mp, jxf, jyf))
                continue;
            SplatRow top[P], bot[P];
            splat_weights<DIMS, GRAD>(dx, dy, mp, jxf, jyf, top, bot);
            const int64_t o = (int64_t)py * cw + px;
#pragma unroll
            for (int c = 0; c < P; ++c) {
                float *q = (c == 0 ? iwe : diwe + (int64_t)(c - 1) * plane) + o;
                atomic_add(q, top[c].l);
                atomic_add(q + 1, top[c].r);
                atomic_add(q + cw, bot[c].l);
                atomic_add(q + cw + 1, bot[c].r);
            }
        }
    }
}

// Plane sums of the gradient post-pass on already blurred images: per block [sum a, sum a^2, sum g(a), sum d_i.., sum g(a) d_i..]
constexpr int kPlaneSums = 3 + 2 * kMaxDims;
constexpr int kPlaneSumBlocks = 512;

template <int K>
__device__ __forceinline__ void block_sums(double (&acc)[K], double *out) {
    __shared__ double part[EVK_BLOCK / EVK_WAVE][K];
    const int lane = threadIdx.x % EVK_WAVE, wave = threadIdx.x / EVK_WAVE;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double v = acc[k];
        for (int off = EVK_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, EVK_WAVE);
        if (lane == 0) part[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double s = 0.0;
        for (int i = 0; i < EVK_BLOCK / EVK_WAVE; ++i) s += part[i][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

__global__ void __launch_bounds__(EVK_BLOCK) k_gradsums_planes(const float *__restrict__ a, const float *__restrict__ d,
                                                               int nplanes, int64_t npix, int gfun, double gparam,
                                                               double *__restrict__ partials) {
    double acc[kPlaneSums] = {};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        const float af = a[i];
        const double av = (double)af;
        double g = av;
        if (gfun == EVK_G_EXP) g = exp(av);
        else if (gfun == EVK_G_STEP) g = (av > gparam) ? 1.0 : 0.0;
        else if (gfun == EVK_G_EXPNEG) g = exp((double)((float)(-gparam) * af));
        acc[0] += av;
        acc[1] += av * av;
        acc[2] += g;
#pragma unroll
        for (int k = 0; k < kMaxDims; ++k) {
            if (k < nplanes) {
                const double dv = (double)d[(int64_t)k * npix + i];
                acc[3 + k] += dv;
                acc[3 + kMaxDims + k] += g * dv;
            }
        }
    }
    block_sums<kPlaneSums>(acc, partials + (int64_t)blockIdx.x * kPlaneSums);
}

__global__ void __launch_bounds__(EVK_BLOCK) k_gradsums_planes_final(const double *__restrict__ partials, int nblocks,
                                                                     int nplanes, double *__restrict__ out) {
    double acc[kPlaneSums] = {};
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x)
#pragma unroll
        for (int k = 0; k < kPlaneSums; ++k) acc[k] += partials[(int64_t)b * kPlaneSums + k];
    __shared__ double tot[kPlaneSums];
    block_sums<kPlaneSums>(acc, tot);
    __syncthreads();
    // out = [sum a, sum a^2, sum g(a), sum d_0 .. sum d_{nplanes-1}, sum g(a) d_0 .. sum g(a) d_{nplanes-1}]
    if (threadIdx.x < 3) out[threadIdx.x] = tot[threadIdx.x];
    else if (threadIdx.x < 3 + nplanes) out[threadIdx.x] = tot[threadIdx.x];
    else if (threadIdx.x < 3 + 2 * nplanes) out[threadIdx.x] = tot[threadIdx.x - nplanes + kMaxDims];
}

}  // namespace evk

// =============================================================================================================
// C ABI
// =============================================================================================================
using namespace evk;

static int model_dims(int model) {
    return model == EVK_WARP_ROTATION ? 3 : model == EVK_WARP_XYZTHETA ? 4 : 0;
}

static WarpArgs warp_args(int model, const double *hp) {
    WarpArgs w;
    if (model == EVK_WARP_ROTATION) w = {hp[0], hp[1], hp[2], 0.0, hp[0], hp[1]};
    else w = {hp[0], hp[1], hp[2], hp[3], hp[4], hp[5]};
    return w;
}

extern "C" int evk_warp_param_f64(int model, const double *x, const double *y, const double *t, int64_t n, double t0,
                                  const double *host_params, double *xo, double *yo, double *jx, double *jy, void *stream) {
    if (!model_dims(model) || !host_params || n < 0 || (n > 0 && (!x || !y || !t || !xo || !yo)) ||
        ((jx == nullptr) != (jy == nullptr)))
        return EVK_EINVAL;
    if (n == 0) return EVK_OK;
    const WarpArgs w = warp_args(model, host_params);
    hipStream_t s = (hipStream_t)stream;
    if (model == EVK_WARP_ROTATION)
        k_warp_param_f64<EVK_WARP_ROTATION><<<stream_grid(n), EVK_BLOCK, 0, s>>>(x, y, t, n, t0, w, xo, yo, jx, jy);
    else
        k_warp_param_f64<EVK_WARP_XYZTHETA><<<stream_grid(n), EVK_BLOCK, 0, s>>>(x, y, t, n, t0, w, xo, yo, jx, jy);
    return launch_status();
}

// Band geometry ("Rotation and xyztheta warps: budget"): as many rows as the LDS holds across all planes; direct
// kernel when not one row fits, or when re-reading the events once per band would cost more than the direct kernel's atomics:
// a band pass costs ~5 ps per event (16 B at the Infinity-Cache rate plus the warp), a direct contribution ~48 ps (21 G float
// atomics/s), so the band form wins while bands < 10 x (4 x planes) -- capped at 4 x (4 x planes) to keep a margin.
extern "C" int evk_iwe_param_band_rows(int model, uint32_t flags, int canvas_h, int canvas_w) {
    const int dims = model_dims(model);
    if (!dims || canvas_h <= 1 || canvas_w <= 1 || (flags & EVK_IWE_DIRECT)) return 0;
    const int planes = (flags & EVK_IWE_GRADIENT) ? 1 + dims : 1;
    const int64_t row_bytes = (int64_t)planes * canvas_w * (int64_t)sizeof(float);
    int rows = (int)((int64_t)kBandLds / row_bytes);
    if (rows < 1) return 0;
    if (rows > canvas_h) rows = canvas_h;
    const int bands = (canvas_h + rows - 1) / rows;
    if (bands > 16 * planes) return 0;
    return rows;
}

template <typename T, int M, bool GRAD>
static int launch_param(const T *x, const T *y, const T *t, const T *p, int64_t n, const WarpArgs &w, double t_ref, double bw,
                        double bh, int ch, int cw, int band_rows, bool abs_p, bool vec, double p_scale, float *iwe, float *diwe,
                        hipStream_t s) {
    constexpr int P = GRAD ? 1 + ModelDims<M>::value : 1;
    if (band_rows > 0) {
        const int bands = (ch + band_rows - 1) / band_rows;
        // about one workgroup per CU in all (each holds nearly the whole LDS), but no chunk under 16 k events: below that
        // the band's flush, not the events, is the workgroup's work
        int64_t chunks = EVK_NUM_CU / bands;
        const int64_t min_chunk = 16384;
        if (chunks < 1) chunks = 1;
        if (chunks > (n + min_chunk - 1) / min_chunk) chunks = (n + min_chunk - 1) / min_chunk;
        int64_t chunk = (n + chunks - 1) / chunks;
        chunk = (chunk + 3) & ~(int64_t)3;
        chunks = (n + chunk - 1) / chunk;
        const size_t lds = (size_t)P * band_rows * cw * sizeof(float);
        if (vec) {
            (void)hipFuncSetAttribute((const void *)k_iwe_param_band<T, M, GRAD, true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)kBandLds);
            k_iwe_param_band<T, M, GRAD, true><<<dim3((unsigned)chunks, bands), kBandThreads, lds, s>>>(
                x, y, t, p, n, chunk, w, t_ref, bw, bh, ch, cw, band_rows, abs_p, p_scale, iwe, diwe);
        } else {
            (void)hipFuncSetAttribute((const void *)k_iwe_param_band<T, M, GRAD, false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)kBandLds);
            k_iwe_param_band<T, M, GRAD, false><<<dim3((unsigned)chunks, bands), kBandThreads, lds, s>>>(
                x, y, t, p, n, chunk, w, t_ref, bw, bh, ch, cw, band_rows, abs_p, p_scale, iwe, diwe);
        }
    } else if (vec) {
        k_iwe_param_direct<T, M, GRAD, true><<<stream_grid(n, 4), EVK_BLOCK, 0, s>>>(x, y, t, p, n, w, t_ref, bw, bh, ch, cw,
                                                                                       abs_p, p_scale, iwe, diwe);
    } else {
        k_iwe_param_direct<T, M, GRAD, false><<<stream_grid(n, 4), EVK_BLOCK, 0, s>>>(x, y, t, p, n, w, t_ref, bw, bh, ch, cw,
                                                                                        abs_p, p_scale, iwe, diwe);
    }
    return launch_status();
}

template <typename T>
static int iwe_param(int model, const T *x, const T *y, const T *t, const T *p, int64_t n, double t_ref, const double *host_params,
                     double bw, double bh, int ch, int cw, uint32_t flags, double p_scale, float *iwe, float *diwe, void *stream) {
    if (!model_dims(model) || !host_params || n < 0 || ch <= 1 || cw <= 1 || !iwe || (n > 0 && (!x || !y || !t || !p)))
        return EVK_EINVAL;
    const bool grad = flags & EVK_IWE_GRADIENT;
    if (grad && !diwe) return EVK_EINVAL;
    if (n == 0) return EVK_OK;
    const WarpArgs w = warp_args(model, host_params);
    const bool abs_p = flags & EVK_IWE_ABS_POLARITY;
    const bool vec = aligned16(x) && aligned16(y) && aligned16(t) && aligned16(p);
    const int rows = evk_iwe_param_band_rows(model, flags, ch, cw);
    hipStream_t s = (hipStream_t)stream;
    if (model == EVK_WARP_ROTATION)
        return grad ? launch_param<T, EVK_WARP_ROTATION, true>(x, y, t, p, n, w, t_ref, bw, bh, ch, cw, rows, abs_p, vec, p_scale, iwe, diwe, s)
                    : launch_param<T, EVK_WARP_ROTATION, false>(x, y, t, p, n, w, t_ref, bw, bh, ch, cw, rows, abs_p, vec, p_scale, iwe, diwe, s);
    return grad ? launch_param<T, EVK_WARP_XYZTHETA, true>(x, y, t, p, n, w, t_ref, bw, bh, ch, cw, rows, abs_p, vec, p_scale, iwe, diwe, s)
                : launch_param<T, EVK_WARP_XYZTHETA, false>(x, y, t, p, n, w, t_ref, bw, bh, ch, cw, rows, abs_p, vec, p_scale, iwe, diwe, s);
}

extern "C" int evk_iwe_param_f32(int model, const float *x, const float *y, const float *t, const float *p, int64_t n,
                                 double t_ref, const double *host_params, double bounds_w, double bounds_h, int canvas_h,
                                 int canvas_w, uint32_t flags, double p_scale, float *iwe, float *diwe, void *stream) {
    return iwe_param<float>(model, x, y, t, p, n, t_ref, host_params, bounds_w, bounds_h, canvas_h, canvas_w, flags, p_scale, iwe,
                            diwe, stream);
}

extern "C" int evk_iwe_param_f64(int model, const double *x, const double *y, const double *t, const double *p, int64_t n,
                                 double t_ref, const double *host_params, double bounds_w, double bounds_h, int canvas_h,
                                 int canvas_w, uint32_t flags, double p_scale, float *iwe, float *diwe, void *stream) {
    return iwe_param<double>(model, x, y, t, p, n, t_ref, host_params, bounds_w, bounds_h, canvas_h, canvas_w, flags, p_scale, iwe,
                             diwe, stream);
}

extern "C" int evk_objective_gradsums_planes_f32(const float *a, const float *d, int nplanes, int h, int w, int gfun,
                                                 double gparam, double *out, void *scratch, int64_t scratch_bytes,
                                                 void *stream) {
    if (!a || !d || nplanes < 1 || nplanes > kMaxDims || h <= 0 || w <= 0 || !out || !scratch || gfun < 0 || gfun > 3)
        return EVK_EINVAL;
    if (scratch_bytes < (int64_t)kPlaneSumBlocks * kPlaneSums * (int64_t)sizeof(double)) return EVK_ESCRATCH;
    const int64_t npix = (int64_t)h * w;
    int grid = (int)((npix + EVK_BLOCK - 1) / EVK_BLOCK);
    if (grid > kPlaneSumBlocks) grid = kPlaneSumBlocks;
    hipStream_t s = (hipStream_t)stream;
    k_gradsums_planes<<<grid, EVK_BLOCK, 0, s>>>(a, d, nplanes, npix, gfun, gparam, (double *)scratch);
    k_gradsums_planes_final<<<1, EVK_BLOCK, 0, s>>>((const double *)scratch, grid, nplanes, out);
    return launch_status();
}
