// Parametric motion models beyond the linear flow ("Rotation and xyztheta warps", "Angular-velocity and
// planar-flow warps"): the elementwise warp with its Jacobians, the fused warp -> mask -> splat IWE with up to 8 derivative
// planes, and the plane sums of the gradient post-pass over up to 8 planes, for all four models.
//
// The fused IWE has two forms with the same per-event code (param_event):
//   band   -- each workgroup owns a band of canvas rows across all 1 + dims planes in LDS, streams one chunk of the events,
//             adds the contributions whose row falls in its band with LDS float adds and flushes the band row by row with
//             global float atomics (contiguous bytes per wave instruction).  Every band re-reads and re-warps the events.
//   direct -- one pass, every contribution a global float atomic; for canvases too wide for a useful band, and EVK_IWE_DIRECT.
//
// Registers (the band kernel runs 1024-thread workgroups: at most 128 VGPRs a lane, and planar flow has 9 planes):
//   - the per-event Jacobian is carried as at most six float32 values (Model<M>::njac), each the float64 value cast to float
//     once, and each plane reads its (jx_k, jy_k) out of them through compile-time slots (a structural zero is a constant
//     0.0f);
//   - the four weights of a plane are formed right before its four LDS / global adds, not held for every plane at once.
#include "evk_accum.h"
#include "evk_warp_models.h"

namespace evk {

template <int M>
__global__ void __launch_bounds__(EVK_BLOCK) k_warp_param_f64(const double *__restrict__ x, const double *__restrict__ y,
                                                              const double *__restrict__ t, int64_t n, double t0, WarpArgs w,
                                                              double *__restrict__ xo, double *__restrict__ yo,
                                                              double *__restrict__ jx, double *__restrict__ jy) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double dt = t[i] - t0;
        double a, b, jv[kJac];
        warp_event<M, true>(w, x[i], y[i], dt, a, b, jv);
        xo[i] = a;
        yo[i] = b;
        if (jx) {
#pragma unroll
            for (int k = 0; k < Model<M>::dims; ++k) {
                const int sx = Model<M>::jx(k), sy = Model<M>::jy(k);
                jx[(int64_t)k * n + i] = sx >= 0 ? jv[sx] : 0.0;
                jy[(int64_t)k * n + i] = sy >= 0 ? jv[sy] : 0.0;
            }
        }
    }
}

// Per-event part of the fused IWE shared by the band and the direct kernels: warp in float64,
// events_bounds_mask(0, bw, 0, bh) (Q2; written so that a NaN coordinate is rejected too: its splat indices would be
// meaningless), p * p_scale [abs], cast to float32, the inner clip, floor / fraction.  False when the event adds nothing.
// jf: the carried Jacobian values, each cast to float once.
template <int M, bool GRAD, typename T>
__device__ __forceinline__ bool param_event(const WarpArgs &w, T x, T y, T t, T p, double t_ref, double bw, double bh,
                                            float clipx, float clipy, bool abs_p, double p_scale, int &px, int &py, float &dx,
                                            float &dy, float &mp, float *jf) {
    const double dt = (double)t - t_ref;
    double xw, yw, jv[kJac];
    warp_event<M, GRAD>(w, (double)x, (double)y, dt, xw, yw, jv);
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
        for (int k = 0; k < Model<M>::njac; ++k) jf[k] = (float)jv[k];
    }
    return true;
}

// The four weights of plane c (0: the IWE, 1 + k: dIWE plane k) of one event, in the reference's float32 order
// (image.py:111-114, 130-135): w1 = jx_k * mp, w2 = jy_k * mp.
struct Quad {
    float tl, tr, bl, br;  // (py, px), (py, px + 1), (py + 1, px), (py + 1, px + 1)
};

template <int M, int C>
__device__ __forceinline__ Quad plane_weights(float dx, float dy, float mp, const float *jf) {
    const float ax = 1.0f - dx, ay = 1.0f - dy;
    if constexpr (C == 0) {
        return {mp * ax * ay, mp * dx * ay, mp * ax * dy, mp * dx * dy};
    } else {
        constexpr int sx = Model<M>::jx(C - 1), sy = Model<M>::jy(C - 1);
        const float jxv = sx >= 0 ? jf[sx < 0 ? 0 : sx] : 0.0f, jyv = sy >= 0 ? jf[sy < 0 ? 0 : sy] : 0.0f;
        const float w1 = jxv * mp, w2 = jyv * mp;
        return {w1 * (-ay) + w2 * (-ax), w1 * ay + w2 * (-dx), w1 * (-dy) + w2 * ax, w1 * dy + w2 * dx};
    }
}

__device__ __forceinline__ void lds_add(float *p, float v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Adds planes C .. P-1 of one event to the LDS band.  o = (py - r0) cw + px is the offset of its top-left cell in plane 0:
// -cw + px when only its bottom row lies in the band, which is then the only one addressed.
template <int M, int C, int P>
__device__ __forceinline__ void band_planes(float *band, int o, int plane_lds, int cw, bool top, bool bot, float dx, float dy,
                                            float mp, const float *jf) {
    if constexpr (C < P) {
        const Quad g = plane_weights<M, C>(dx, dy, mp, jf);
        const int r = C * plane_lds + o;
        if (top) {
            lds_add(band + r, g.tl);
            lds_add(band + r + 1, g.tr);
        }
        if (bot) {
            lds_add(band + r + cw, g.bl);
            lds_add(band + r + cw + 1, g.br);
        }
        band_planes<M, C + 1, P>(band, o, plane_lds, cw, top, bot, dx, dy, mp, jf);
    }
}

template <int M, int C, int P>
__device__ __forceinline__ void direct_planes(float *iwe, float *diwe, int64_t plane, int64_t o, int cw, float dx, float dy,
                                              float mp, const float *jf) {
    if constexpr (C < P) {
        const Quad g = plane_weights<M, C>(dx, dy, mp, jf);
        float *q = (C == 0 ? iwe : diwe + (int64_t)(C - 1) * plane) + o;
        atomic_add(q, g.tl);
        atomic_add(q + 1, g.tr);
        atomic_add(q + cw, g.bl);
        atomic_add(q + cw + 1, g.br);
        direct_planes<M, C + 1, P>(iwe, diwe, plane, o, cw, dx, dy, mp, jf);
    }
}

// grid = (chunks, bands).  LDS holds planes x band_rows x cw floats; plane k of the band is rows [r0, r1) of plane k.
template <typename T, int M, bool GRAD, bool VEC>
__global__ void __launch_bounds__(kBandThreads) k_iwe_param_band(const T *__restrict__ x, const T *__restrict__ y,
                                                                 const T *__restrict__ t, const T *__restrict__ p, int64_t n,
                                                                 int64_t chunk, WarpArgs w, double t_ref, double bw, double bh,
                                                                 int ch, int cw, int band_rows, bool abs_p, double p_scale,
                                                                 float *__restrict__ iwe, float *__restrict__ diwe) {
    constexpr int P = GRAD ? 1 + Model<M>::dims : 1;
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
            float dx, dy, mp, jf[kJac];
            if (!param_event<M, GRAD, T>(w, xv.v[k], yv.v[k], tv.v[k], pv.v[k], t_ref, bw, bh, clipx, clipy, abs_p, p_scale, px,
                                         py, dx, dy, mp, jf))
                continue;
            if (py + 1 < r0 || py >= r1) continue;  // neither of its two rows is in this band
            band_planes<M, 0, P>(band, (py - r0) * cw + px, plane_lds, cw, py >= r0, py + 1 < r1, dx, dy, mp, jf);
        }
    }
    __syncthreads();
    // flush: the band's rows of a plane are contiguous in global memory, so consecutive lanes add to consecutive floats
    const int64_t plane = (int64_t)ch * cw;
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
    constexpr int P = GRAD ? 1 + Model<M>::dims : 1;
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
            float dx, dy, mp, jf[kJac];
            if (!param_event<M, GRAD, T>(w, xv.v[k], yv.v[k], tv.v[k], pv.v[k], t_ref, bw, bh, clipx, clipy, abs_p, p_scale, px,
                                         py, dx, dy, mp, jf))
                continue;
            direct_planes<M, 0, P>(iwe, diwe, plane, (int64_t)py * cw + px, cw, dx, dy, mp, jf);
        }
    }
}

// Plane sums of the gradient post-pass on already blurred images: per block [sum a, sum a^2, sum g(a), sum d_i.., sum g(a) d_i..]
// with D slots for each of the two plane groups.  The block reductions cost in proportion to the 3 + 2 D slots, so up to 4
// planes take D = 4 and only planar flow pays for D = 8.
constexpr int kPlaneSumBlocks = 512;

template <int D>
__global__ void __launch_bounds__(EVK_BLOCK) k_gradsums_planes(const float *__restrict__ a, const float *__restrict__ d,
                                                               int nplanes, int64_t npix, int gfun, double gparam,
                                                               double *__restrict__ partials) {
    constexpr int K = 3 + 2 * D;
    double acc[K] = {};
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
        for (int k = 0; k < D; ++k) {
            if (k < nplanes) {
                const double dv = (double)d[(int64_t)k * npix + i];
                acc[3 + k] += dv;
                acc[3 + D + k] += g * dv;
            }
        }
    }
    block_sums<K>(acc, partials + (int64_t)blockIdx.x * K);
}

template <int D>
__global__ void __launch_bounds__(EVK_BLOCK) k_gradsums_planes_final(const double *__restrict__ partials, int nblocks,
                                                                     int nplanes, double *__restrict__ out) {
    constexpr int K = 3 + 2 * D;
    double acc[K] = {};
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += partials[(int64_t)b * K + k];
    __shared__ double tot[K];
    block_sums<K>(acc, tot);
    __syncthreads();
    // out = [sum a, sum a^2, sum g(a), sum d_0 .. sum d_{nplanes-1}, sum g(a) d_0 .. sum g(a) d_{nplanes-1}]
    if (threadIdx.x < 3) out[threadIdx.x] = tot[threadIdx.x];
    else if (threadIdx.x < 3 + nplanes) out[threadIdx.x] = tot[threadIdx.x];
    else if (threadIdx.x < 3 + 2 * nplanes) out[threadIdx.x] = tot[threadIdx.x - nplanes + D];
}

}  // namespace evk

// =============================================================================================================
// C ABI
// =============================================================================================================
using namespace evk;

// These entries refuse the linear flow (model id 0): it has its own kernels here.
constexpr bool kTakesLinvel = false;

extern "C" int evk_warp_param_f64(int model, const double *x, const double *y, const double *t, int64_t n, double t0,
                                  const double *host_params, double *xo, double *yo, double *jx, double *jy, void *stream) {
    if (!model_dims<kTakesLinvel>(model) || !host_params || n < 0 || (n > 0 && (!x || !y || !t || !xo || !yo)) ||
        ((jx == nullptr) != (jy == nullptr)))
        return EVK_EINVAL;
    if (n == 0) return EVK_OK;
    const WarpArgs w = warp_args(model, host_params);
    hipStream_t s = (hipStream_t)stream;
    with_model<kTakesLinvel>(model, [&](auto m) {
        k_warp_param_f64<decltype(m)::value><<<stream_grid(n), EVK_BLOCK, 0, s>>>(x, y, t, n, t0, w, xo, yo, jx, jy);
        return 0;
    });
    return launch_status();
}

// Band geometry (lds_band_rows; DESIGN.md, "Rotation and xyztheta warps: budget"): float cells, 1 + dims planes or 1; direct
// kernel when not one row fits, or when re-reading the events once per band would cost more than the direct kernel's atomics:
// a band pass costs ~5 ps per event (16 B at the Infinity-Cache rate plus the warp), a direct contribution ~48 ps (21 G float
// atomics/s), so the band form wins while bands < 10 x (4 x planes) -- capped at 4 x (4 x planes) to keep a margin.
extern "C" int evk_iwe_param_band_rows(int model, uint32_t flags, int canvas_h, int canvas_w) {
    const int dims = model_dims<kTakesLinvel>(model);
    return lds_band_rows(!dims ? 0 : (flags & EVK_IWE_GRADIENT) ? 1 + dims : 1, sizeof(float), 16, flags, canvas_h, canvas_w);
}

template <typename T, int M, bool GRAD, bool VEC>
static void launch_band(const T *x, const T *y, const T *t, const T *p, int64_t n, int64_t chunk, int64_t chunks, int bands,
                        const WarpArgs &w, double t_ref, double bw, double bh, int ch, int cw, int band_rows, bool abs_p,
                        double p_scale, float *iwe, float *diwe, size_t lds, hipStream_t s) {
    (void)hipFuncSetAttribute((const void *)k_iwe_param_band<T, M, GRAD, VEC>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)kBandLds);
    k_iwe_param_band<T, M, GRAD, VEC><<<dim3((unsigned)chunks, bands), kBandThreads, lds, s>>>(
        x, y, t, p, n, chunk, w, t_ref, bw, bh, ch, cw, band_rows, abs_p, p_scale, iwe, diwe);
}

template <typename T, int M, bool GRAD>
static int launch_param(const T *x, const T *y, const T *t, const T *p, int64_t n, const WarpArgs &w, double t_ref, double bw,
                        double bh, int ch, int cw, int band_rows, bool abs_p, bool vec, double p_scale, float *iwe, float *diwe,
                        hipStream_t s) {
    constexpr int P = GRAD ? 1 + Model<M>::dims : 1;
    if (band_rows > 0) {
        const int bands = (ch + band_rows - 1) / band_rows;
        const auto [chunk, chunks] = chunk_plan(n, bands);
        const size_t lds = (size_t)P * band_rows * cw * sizeof(float);
        if (vec)
            launch_band<T, M, GRAD, true>(x, y, t, p, n, chunk, chunks, bands, w, t_ref, bw, bh, ch, cw, band_rows, abs_p, p_scale,
                                          iwe, diwe, lds, s);
        else
            launch_band<T, M, GRAD, false>(x, y, t, p, n, chunk, chunks, bands, w, t_ref, bw, bh, ch, cw, band_rows, abs_p,
                                           p_scale, iwe, diwe, lds, s);
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
    if (!model_dims<kTakesLinvel>(model) || !host_params || n < 0 || ch <= 1 || cw <= 1 || !iwe || (n > 0 && (!x || !y || !t || !p)))
        return EVK_EINVAL;
    const bool grad = flags & EVK_IWE_GRADIENT;
    if (grad && !diwe) return EVK_EINVAL;
    if (n == 0) return EVK_OK;
    const WarpArgs w = warp_args(model, host_params);
    const bool abs_p = flags & EVK_IWE_ABS_POLARITY;
    const bool vec = aligned16(x) && aligned16(y) && aligned16(t) && aligned16(p);
    const int rows = evk_iwe_param_band_rows(model, flags, ch, cw);
    hipStream_t s = (hipStream_t)stream;
    return with_model<kTakesLinvel>(model, [&](auto m) {
        constexpr int M = decltype(m)::value;
        return grad ? launch_param<T, M, true>(x, y, t, p, n, w, t_ref, bw, bh, ch, cw, rows, abs_p, vec, p_scale, iwe, diwe, s)
                    : launch_param<T, M, false>(x, y, t, p, n, w, t_ref, bw, bh, ch, cw, rows, abs_p, vec, p_scale, iwe, diwe, s);
    });
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
    if (scratch_bytes < (int64_t)kPlaneSumBlocks * (3 + 2 * kMaxDims) * (int64_t)sizeof(double)) return EVK_ESCRATCH;
    const int64_t npix = (int64_t)h * w;
    int grid = (int)((npix + EVK_BLOCK - 1) / EVK_BLOCK);
    if (grid > kPlaneSumBlocks) grid = kPlaneSumBlocks;
    hipStream_t s = (hipStream_t)stream;
    auto run = [&](auto dm) {
        constexpr int D = decltype(dm)::value;
        k_gradsums_planes<D><<<grid, EVK_BLOCK, 0, s>>>(a, d, nplanes, npix, gfun, gparam, (double *)scratch);
        k_gradsums_planes_final<D><<<1, EVK_BLOCK, 0, s>>>((const double *)scratch, grid, nplanes, out);
    };
    if (nplanes <= 4) run(std::integral_constant<int, 4>{});
    else run(std::integral_constant<int, kMaxDims>{});
    return launch_status();
}
