// The average-timestamp objective of Zhu et al. (CVPR 2019) with an analytic gradient ("Average-timestamp
// objective"; definition in include/evk.h):
//   evk_tsimg_warp_*   fused warp -> mask -> splat of the four planes [T+, C+, T-, C-] (sum of normalised timestamps and of
//                      weights, per polarity class), for the linear flow and the four parametric models;
//   evk_tsobj_post_f32 A_c = T_c / (1 + C_c), B_c = blur(A_c), loss = sum B_+^2 + sum B_-^2 and, when asked, the adjoint images
//                      gT_c = 2 S_c / (1 + C_c), gC_c = -2 S_c T_c / (1 + C_c)^2 with S_c = blur(B_c);
//   evk_tsobj_grad_*   the adjoint gather: one pass over the events, each reads the four corners of gT_c and gC_c of its class
//                      and adds (tau d_x gT + d_x gC) Jx_k + (tau d_y gT + d_y gC) Jy_k to dims float64 sums, reduced per
//                      wave, per workgroup and by a final kernel in a fixed order: no atomics, so the gradient is bitwise
//                      repeatable.
//
// The splat has the two forms of the fused IWE (evk_warps.hip): four planes, each event adding to the two of its own class
// (8 adds) -- in 64-bit fixed point, so that the planes do not depend on the order of the atomics.  The gather needs no planes per parameter: 4 (1 + dims) derivative planes would be 12 for
// the linear flow and 36 for planar flow, which no LDS band holds at a useful height.
#include "evk_accum.h"
#include "evk_warp_models.h"

namespace evk {

constexpr int kTsPlanes = 4;
constexpr int kGatherBlocks = 1024;  // partial sums of the adjoint gather: kGatherBlocks x kMaxDims doubles of the scratch

// Time constants of the normalised timestamp tau = (t - t_first) / tdiv, tdiv = t_last - t_first + 1e-6 formed by the caller.
// float32 columns: float32 arithmetic, as evk_timestamp_images_f32 (image.py:328); float64 columns: float64, cast once.
template <typename T>
__device__ __forceinline__ float norm_time(T t, double t_first, double tdiv) {
    if constexpr (sizeof(T) == 4) return (t - (float)t_first) / (float)tdiv;
    else return (float)((t - t_first) / tdiv);
}

// Per-event part shared by the splat and the gather: the warp in float64 (the expressions of evk_iwe_param_* / evk_iwe_linvel_*),
// events_bounds_mask(0, bw, 0, bh) written so that NaN is rejected, the cast to float32, the inner clip at the padded canvas,
// floor / fraction -- an event lands where get_iwe puts it.  cls: 0 for p > 0, 2 for p <= 0 (the first plane of the class); a
// NaN polarity belongs to neither.  False when the event contributes nothing.
template <int M, bool JAC, typename T>
__device__ __forceinline__ bool ts_event(const WarpArgs &w, T x, T y, T t, T p, double t_ref, double bw, double bh, float clipx,
                                         float clipy, int &px, int &py, float &dx, float &dy, int &cls, float *jf) {
    const bool pos = p > T(0), neg = p <= T(0);
    if (!pos && !neg) return false;
    const double dt = (double)t - t_ref;
    double xw, yw, jv[kJac];
    warp_event<M, JAC>(w, (double)x, (double)y, dt, xw, yw, jv);
    if (!(xw > 0.0 && xw <= bw && yw > 0.0 && yw <= bh)) return false;
    const float xf = (float)xw, yf = (float)yw;
    if (xf >= clipx || yf >= clipy) return false;
    const float fx = floorf(xf), fy = floorf(yf);
    dx = xf - fx;
    dy = yf - fy;
    px = (int)fx;
    py = (int)fy;
    cls = pos ? 0 : 2;
    if constexpr (JAC) {
#pragma unroll
        for (int k = 0; k < Model<M>::njac; ++k) jf[k] = (float)jv[k];
    }
    return true;
}

// The planes are accumulated in the fixed point of evk_accum.h: a contribution is tau w or w with 0 <= tau <= 1 and a bilinear
// weight 0 <= w <= 1, so it is in [-1, 1].

// grid = (chunks, bands).  LDS holds 4 planes x band_rows x cw fixed-point cells; the flush adds the band's rows, contiguous
// in each plane, with global 64-bit integer atomics.  Every band re-reads and re-warps its chunk of the events.
template <typename T, int M, bool VEC>
__global__ void __launch_bounds__(kBandThreads) k_tsimg_band(const T *__restrict__ x, const T *__restrict__ y,
                                                             const T *__restrict__ t, const T *__restrict__ p, int64_t n,
                                                             int64_t chunk, WarpArgs w, double t_ref, double t_first, double tdiv,
                                                             double bw, double bh, int ch, int cw, int band_rows,
                                                             acc64_t *__restrict__ acc4) {
    extern __shared__ acc64_t band[];
    const int r0 = blockIdx.y * band_rows, r1 = min(r0 + band_rows, ch), rows = r1 - r0;
    const int plane_lds = rows * cw;
    for (int i = threadIdx.x; i < kTsPlanes * plane_lds; i += blockDim.x) band[i] = 0;
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
            int px, py, cls;
            float dx, dy;
            if (!ts_event<M, false, T>(w, xv.v[k], yv.v[k], tv.v[k], pv.v[k], t_ref, bw, bh, clipx, clipy, px, py, dx, dy, cls,
                                       nullptr))
                continue;
            if (py + 1 < r0 || py >= r1) continue;  // neither of its two rows is in this band
            const float tau = norm_time<T>(tv.v[k], t_first, tdiv);
            const float ax = 1.0f - dx, ay = 1.0f - dy;
            // offset of the top-left cell in plane `cls`; -cw + px when only the bottom row lies in the band
            acc64_t *ts = band + cls * plane_lds + (py - r0) * cw + px, *cn = ts + plane_lds;
            if (py >= r0) {
                lds_add_fixed(ts, tau * ax * ay);
                lds_add_fixed(ts + 1, tau * dx * ay);
                lds_add_fixed(cn, ax * ay);
                lds_add_fixed(cn + 1, dx * ay);
            }
            if (py + 1 < r1) {
                lds_add_fixed(ts + cw, tau * ax * dy);
                lds_add_fixed(ts + cw + 1, tau * dx * dy);
                lds_add_fixed(cn + cw, ax * dy);
                lds_add_fixed(cn + cw + 1, dx * dy);
            }
        }
    }
    __syncthreads();
    const int64_t plane = (int64_t)ch * cw;
    for (int c = 0; c < kTsPlanes; ++c) {
        acc64_t *dst = acc4 + (int64_t)c * plane + (int64_t)r0 * cw;
        const acc64_t *src = band + c * plane_lds;
        for (int i = threadIdx.x; i < plane_lds; i += blockDim.x) {
            const acc64_t v = src[i];
            if (v != 0) global_add_fixed(dst + i, v);
        }
    }
}

template <typename T, int M, bool VEC>
__global__ void __launch_bounds__(EVK_BLOCK) k_tsimg_direct(const T *__restrict__ x, const T *__restrict__ y,
                                                            const T *__restrict__ t, const T *__restrict__ p, int64_t n,
                                                            WarpArgs w, double t_ref, double t_first, double tdiv, double bw,
                                                            double bh, int ch, int cw, acc64_t *__restrict__ acc4) {
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
            int px, py, cls;
            float dx, dy;
            if (!ts_event<M, false, T>(w, xv.v[k], yv.v[k], tv.v[k], pv.v[k], t_ref, bw, bh, clipx, clipy, px, py, dx, dy, cls,
                                       nullptr))
                continue;
            const float tau = norm_time<T>(tv.v[k], t_first, tdiv);
            const float ax = 1.0f - dx, ay = 1.0f - dy;
            acc64_t *ts = acc4 + (int64_t)cls * plane + (int64_t)py * cw + px, *cn = ts + plane;
            global_add_fixed(ts, fixed32(tau * ax * ay));
            global_add_fixed(ts + 1, fixed32(tau * dx * ay));
            global_add_fixed(ts + cw, fixed32(tau * ax * dy));
            global_add_fixed(ts + cw + 1, fixed32(tau * dx * dy));
            global_add_fixed(cn, fixed32(ax * ay));
            global_add_fixed(cn + 1, fixed32(dx * ay));
            global_add_fixed(cn + cw, fixed32(ax * dy));
            global_add_fixed(cn + cw + 1, fixed32(dx * dy));
        }
    }
}

// out4 = the fixed-point planes as float32
__global__ void __launch_bounds__(EVK_BLOCK) k_ts_planes(const acc64_t *__restrict__ acc4, int64_t elems, float *__restrict__ out4) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < elems; i += stride)
        out4[i] = unfixed32(acc4[i]);
}

// ---- post pass ---------------------------------------------------------------------------------------------------------

// avg[c] = T_c / (1 + C_c) for the two classes: the count images start at ONE upstream (image.py:269,271)
__global__ void __launch_bounds__(EVK_BLOCK) k_ts_average(const float *__restrict__ planes4, int64_t npix,
                                                          float *__restrict__ avg2) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * npix; i += stride) {
        const int64_t c = i / npix, j = i - c * npix;
        const float tsum = planes4[2 * c * npix + j], cnt = planes4[(2 * c + 1) * npix + j];
        avg2[i] = tsum / (1.0f + cnt);
    }
}

__global__ void __launch_bounds__(EVK_BLOCK) k_ts_sumsq(const float *__restrict__ b, int64_t n, double *__restrict__ partials) {
    double acc[1] = {0.0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = (double)b[i];
        acc[0] += v * v;
    }
    block_sums<1>(acc, partials + blockIdx.x);
}

// out[0..K) = sums over the blocks' partials (row-major nblocks x stride), in a fixed order
template <int K>
__global__ void __launch_bounds__(EVK_BLOCK) k_ts_final(const double *__restrict__ partials, int nblocks, int stride, int nout,
                                                        double *__restrict__ out) {
    double acc[K] = {};
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += partials[(int64_t)b * stride + k];
    __shared__ double tot[K];
    block_sums<K>(acc, tot);
    __syncthreads();
    if ((int)threadIdx.x < nout) out[threadIdx.x] = tot[threadIdx.x];
}

// adj4 = [gT+, gC+, gT-, gC-]: gT_c = 2 S_c / (1 + C_c), gC_c = -2 S_c T_c / (1 + C_c)^2 (float64, stored as float32)
__global__ void __launch_bounds__(EVK_BLOCK) k_ts_adjoint(const float *__restrict__ planes4, const float *__restrict__ s2,
                                                          int64_t npix, float *__restrict__ adj4) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * npix; i += stride) {
        const int64_t c = i / npix, j = i - c * npix;
        const double tsum = (double)planes4[2 * c * npix + j], d = 1.0 + (double)planes4[(2 * c + 1) * npix + j];
        const double gt = 2.0 * (double)s2[i] / d;
        adj4[2 * c * npix + j] = (float)gt;
        adj4[(2 * c + 1) * npix + j] = (float)(-gt * tsum / d);
    }
}

// ---- adjoint gather ----------------------------------------------------------------------------------------------------

template <typename T, int M, bool VEC>
__global__ void __launch_bounds__(EVK_BLOCK) k_tsobj_gather(const T *__restrict__ x, const T *__restrict__ y,
                                                            const T *__restrict__ t, const T *__restrict__ p, int64_t n,
                                                            WarpArgs w, double t_ref, double t_first, double tdiv, double bw,
                                                            double bh, int ch, int cw, const float *__restrict__ adj4,
                                                            double *__restrict__ partials) {
    constexpr int D = Model<M>::dims;
    const float clipx = (float)(cw - 1), clipy = (float)(ch - 1);
    const int64_t plane = (int64_t)ch * cw;
    double acc[D] = {};
    const int64_t stride = 4 * (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = 4 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x); base < n; base += stride) {
        const int cnt = (int)min((int64_t)4, n - base);
        const bool vec = VEC && cnt == 4;
        const Vec4<T> xv = load_quad(x, base, cnt, vec), yv = load_quad(y, base, cnt, vec), tv = load_quad(t, base, cnt, vec),
                      pv = load_quad(p, base, cnt, vec);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= cnt) break;
            int px, py, cls;
            float dx, dy, jf[kJac];
            if (!ts_event<M, true, T>(w, xv.v[k], yv.v[k], tv.v[k], pv.v[k], t_ref, bw, bh, clipx, clipy, px, py, dx, dy, cls, jf))
                continue;
            const double tau = (double)norm_time<T>(tv.v[k], t_first, tdiv);
            const float *gt = adj4 + (int64_t)cls * plane + (int64_t)py * cw + px;
            double tx, ty, cx, cy;
            bilinear_slopes(gt, cw, dx, dy, tx, ty);
            bilinear_slopes(gt + plane, cw, dx, dy, cx, cy);
            const double ex = tau * tx + cx, ey = tau * ty + cy;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int sx = Model<M>::jx(d), sy = Model<M>::jy(d);
                const double jxv = sx >= 0 ? (double)jf[sx < 0 ? 0 : sx] : 0.0, jyv = sy >= 0 ? (double)jf[sy < 0 ? 0 : sy] : 0.0;
                acc[d] += ex * jxv + ey * jyv;
            }
        }
    }
    block_sums<D>(acc, partials + (int64_t)blockIdx.x * kMaxDims);
}

}  // namespace evk

// =============================================================================================================
// C ABI
// =============================================================================================================
using namespace evk;

// These entries take the linear flow (model id 0) beside the four parametric models.
constexpr bool kTakesLinvel = true;

// Band geometry (lds_band_rows): four planes of 8-byte cells, at most 24 bands per plane (evk_iwe_param_band_rows puts the
// break-even at 40 bands per plane and keeps 16; the 8-byte cells halve the rows, so a 641-wide canvas has 69 bands of 7 rows).
extern "C" int evk_tsimg_band_rows(uint32_t flags, int canvas_h, int canvas_w) {
    return lds_band_rows(kTsPlanes, sizeof(acc64_t), 24, flags, canvas_h, canvas_w);
}

template <typename T, int M, bool VEC>
static void ts_launch_splat(const T *x, const T *y, const T *t, const T *p, int64_t n, const WarpArgs &w, double t_ref,
                            double t_first, double tdiv, double bw, double bh, int ch, int cw, int band_rows, acc64_t *out4,
                            hipStream_t s) {
    if (band_rows > 0) {
        const int bands = (ch + band_rows - 1) / band_rows;
        const auto [chunk, chunks] = chunk_plan(n, bands);
        const size_t lds = (size_t)kTsPlanes * band_rows * cw * sizeof(acc64_t);
        (void)hipFuncSetAttribute((const void *)k_tsimg_band<T, M, VEC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBandLds);
        k_tsimg_band<T, M, VEC><<<dim3((unsigned)chunks, bands), kBandThreads, lds, s>>>(x, y, t, p, n, chunk, w, t_ref, t_first,
                                                                                         tdiv, bw, bh, ch, cw, band_rows, out4);
    } else {
        k_tsimg_direct<T, M, VEC><<<stream_grid(n, 4), EVK_BLOCK, 0, s>>>(x, y, t, p, n, w, t_ref, t_first, tdiv, bw, bh, ch, cw,
                                                                          out4);
    }
}

template <typename T>
static int tsimg_warp(int model, const T *x, const T *y, const T *t, const T *p, int64_t n, double t_ref, double t_first,
                      double tdiv, const double *host_params, double bw, double bh, int ch, int cw, uint32_t flags, uint64_t *acc4,
                      float *out4, void *stream) {
    if (!model_dims<kTakesLinvel>(model) || !host_params || n < 0 || ch <= 1 || cw <= 1 || !acc4 || !out4 ||
        (n > 0 && (!x || !y || !t || !p)))
        return EVK_EINVAL;
    if (n > 0 && !columns_elem_aligned(x, y, t, p)) return EVK_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    acc64_t *acc = reinterpret_cast<acc64_t *>(acc4);
    if (n > 0) {
        const WarpArgs w = warp_args(model, host_params);
        const bool vec = aligned16(x) && aligned16(y) && aligned16(t) && aligned16(p);
        const int rows = evk_tsimg_band_rows(flags, ch, cw);
        with_model<kTakesLinvel>(model, [&](auto m) {
            constexpr int M = decltype(m)::value;
            if (vec) ts_launch_splat<T, M, true>(x, y, t, p, n, w, t_ref, t_first, tdiv, bw, bh, ch, cw, rows, acc, s);
            else ts_launch_splat<T, M, false>(x, y, t, p, n, w, t_ref, t_first, tdiv, bw, bh, ch, cw, rows, acc, s);
            return 1;
        });
    }
    const int64_t elems = (int64_t)kTsPlanes * ch * cw;
    k_ts_planes<<<stream_grid(elems), EVK_BLOCK, 0, s>>>(acc, elems, out4);
    return launch_status();
}

extern "C" int evk_tsimg_warp_f32(int model, const float *x, const float *y, const float *t, const float *p, int64_t n,
                                  double t_ref, double t_first, double tdiv, const double *host_params, double bounds_w,
                                  double bounds_h, int canvas_h, int canvas_w, uint32_t flags, uint64_t *acc4, float *out4,
                                  void *stream) {
    return tsimg_warp<float>(model, x, y, t, p, n, t_ref, t_first, tdiv, host_params, bounds_w, bounds_h, canvas_h, canvas_w, flags,
                             acc4, out4, stream);
}

extern "C" int evk_tsimg_warp_f64(int model, const double *x, const double *y, const double *t, const double *p, int64_t n,
                                  double t_ref, double t_first, double tdiv, const double *host_params, double bounds_w,
                                  double bounds_h, int canvas_h, int canvas_w, uint32_t flags, uint64_t *acc4, float *out4,
                                  void *stream) {
    return tsimg_warp<double>(model, x, y, t, p, n, t_ref, t_first, tdiv, host_params, bounds_w, bounds_h, canvas_h, canvas_w, flags,
                              acc4, out4, stream);
}

static int ts_image_grid(int64_t elems) {
    int grid = stream_grid(elems);
    return grid > kGatherBlocks ? kGatherBlocks : grid;
}

extern "C" int evk_tsimg_average_f32(const float *planes4, int h, int w, float *avg2, void *stream) {
    if (!planes4 || !avg2 || h <= 0 || w <= 0) return EVK_EINVAL;
    const int64_t npix = (int64_t)h * w;
    k_ts_average<<<ts_image_grid(2 * npix), EVK_BLOCK, 0, (hipStream_t)stream>>>(planes4, npix, avg2);
    return launch_status();
}

extern "C" int evk_tsobj_post_f32(const float *planes4, int h, int w, const double *host_weights, const double *dev_weights,
                                  int radius, float *work6, float *adj4, double *out, void *scratch, int64_t scratch_bytes,
                                  void *stream) {
    if (!planes4 || h <= 0 || w <= 0 || !work6 || !out || !scratch) return EVK_EINVAL;
    if (radius >= 0 && (radius <= EVK_MAX_RADIUS ? !host_weights : !dev_weights)) return EVK_EINVAL;
    if (scratch_bytes < evk_reduce_scratch_bytes()) return EVK_ESCRATCH;
    hipStream_t s = (hipStream_t)stream;
    const int64_t npix = (int64_t)h * w;
    // work6: [0, 2) the averages A (then S), [2, 4) the blurred B, [4, 6) the filter's scratch
    float *a2 = work6, *b2 = work6 + 2 * npix, *tmp = work6 + 4 * npix;
    const int dims[2] = {h, w};
    auto blur = [&](const float *src, float *dst) {
        for (int c = 0; c < 2; ++c) {
            const int rc = radius <= EVK_MAX_RADIUS
                               ? evk_gaussian_filter_f32(src + c * npix, dst + c * npix, tmp, 2, dims, host_weights, radius, stream)
                               : evk_gaussian_filter_wide_f32(src + c * npix, dst + c * npix, tmp, 2, dims, dev_weights, radius,
                                                              stream);
            if (rc != EVK_OK) return rc;
        }
        return (int)EVK_OK;
    };
    const int grid = ts_image_grid(2 * npix);
    k_ts_average<<<grid, EVK_BLOCK, 0, s>>>(planes4, npix, a2);
    const float *b = a2;
    if (radius >= 0) {
        const int rc = blur(a2, b2);
        if (rc != EVK_OK) return rc;
        b = b2;
    }
    k_ts_sumsq<<<grid, EVK_BLOCK, 0, s>>>(b, 2 * npix, (double *)scratch);
    k_ts_final<1><<<1, EVK_BLOCK, 0, s>>>((const double *)scratch, grid, 1, 1, out);
    if (adj4) {
        const float *sm = b;
        if (radius >= 0) {  // S = blur(B): the reflect-mode blur with a symmetric kernel is self-adjoint
            const int rc = blur(b2, a2);
            if (rc != EVK_OK) return rc;
            sm = a2;
        }
        k_ts_adjoint<<<grid, EVK_BLOCK, 0, s>>>(planes4, sm, npix, adj4);
    }
    return launch_status();
}

template <typename T>
static int tsobj_grad(int model, const T *x, const T *y, const T *t, const T *p, int64_t n, double t_ref, double t_first,
                      double tdiv, const double *host_params, double bw, double bh, int ch, int cw, const float *adj4, double *out,
                      void *scratch, int64_t scratch_bytes, void *stream) {
    const int dims = model_dims<kTakesLinvel>(model);
    if (!dims || !host_params || n < 0 || ch <= 1 || cw <= 1 || !adj4 || !out || !scratch || (n > 0 && (!x || !y || !t || !p)))
        return EVK_EINVAL;
    if (scratch_bytes < (int64_t)kGatherBlocks * kMaxDims * (int64_t)sizeof(double)) return EVK_ESCRATCH;
    if (n > 0 && !columns_elem_aligned(x, y, t, p)) return EVK_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const WarpArgs w = warp_args(model, host_params);
    const bool vec = aligned16(x) && aligned16(y) && aligned16(t) && aligned16(p);
    int grid = stream_grid(n, 4);  // a function of n alone: the order of the sums, and with it the result, is repeatable
    if (grid > kGatherBlocks) grid = kGatherBlocks;
    with_model<kTakesLinvel>(model, [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (vec) k_tsobj_gather<T, M, true><<<grid, EVK_BLOCK, 0, s>>>(x, y, t, p, n, w, t_ref, t_first, tdiv, bw, bh, ch, cw, adj4,
                                                                     (double *)scratch);
        else k_tsobj_gather<T, M, false><<<grid, EVK_BLOCK, 0, s>>>(x, y, t, p, n, w, t_ref, t_first, tdiv, bw, bh, ch, cw, adj4,
                                                                   (double *)scratch);
        return 1;
    });
    k_ts_final<kMaxDims><<<1, EVK_BLOCK, 0, s>>>((const double *)scratch, grid, kMaxDims, dims, out);
    return launch_status();
}

extern "C" int evk_tsobj_grad_f32(int model, const float *x, const float *y, const float *t, const float *p, int64_t n,
                                  double t_ref, double t_first, double tdiv, const double *host_params, double bounds_w,
                                  double bounds_h, int canvas_h, int canvas_w, const float *adj4, double *out, void *scratch,
                                  int64_t scratch_bytes, void *stream) {
    return tsobj_grad<float>(model, x, y, t, p, n, t_ref, t_first, tdiv, host_params, bounds_w, bounds_h, canvas_h, canvas_w, adj4,
                             out, scratch, scratch_bytes, stream);
}

extern "C" int evk_tsobj_grad_f64(int model, const double *x, const double *y, const double *t, const double *p, int64_t n,
                                  double t_ref, double t_first, double tdiv, const double *host_params, double bounds_w,
                                  double bounds_h, int canvas_h, int canvas_w, const float *adj4, double *out, void *scratch,
                                  int64_t scratch_bytes, void *stream) {
    return tsobj_grad<double>(model, x, y, t, p, n, t_ref, t_first, tdiv, host_params, bounds_w, bounds_h, canvas_h, canvas_w, adj4,
                              out, scratch, scratch_bytes, stream);
}
