// The average-timestamp loss of a DENSE flow field with its gradient with respect to the field (DESIGN.md section 6,
// "Average-timestamp loss of a flow field"; definition in include/evk.h, steps 1' and 8' of the average-timestamp objective):
//   evk_flowts_time_constants_f32  per-sample (t_ref, t_origin, signed tdiv), read on the device from `offsets` and `t`;
//   evk_flowts_warp_f32            one pass over the events (grid.y = sample): bilinear sample of the field at the event (the
//                                  expressions of k_warp_flow_field_f32, evk_scatter.hip), x' = x + u dt, mask, splat of the four
//                                  planes [T+, C+, T-, C-] in 64-bit fixed point (as evk_tsimg_warp_*: integer adds commute);
//   evk_flowts_grad_f32            one pass: re-warp, mask, gather the eight adj4 values of the event's class, form the slopes
//                                  e_x, e_y at (x', y') and scatter b_j dt e_x, b_j dt e_y to the (at most) four field cells
//                                  around (x, y), in 64-bit fixed point with a per-sample scale 2^k taken on the device from
//                                  max |adj4|: the gradient is the same bits from call to call.
// The splat is the direct (global-atomic) form only.  An LDS band kernel re-reads and re-warps its events once per band, and
// here the warp is the eight-load field sample: section 6 found the direct splat the faster one already for the warps with a
// transcendental per event, which cost less than eight dependent loads.
//
// The contrast (focus) loss of the same field (evk.h, "Contrast loss of a flow field") is a peer built from the same parts:
//   evk_flowcm_warp_f32            max |q| per sample, the splat of q times the four bilinear weights into ONE plane in 64-bit
//                                  fixed point at a per-sample scale 2^kI (from max |q| and the event count), the plane as float32;
//   evk_flowcm_post_f32            B = blur(I), the variance or mean-square loss (float64, two stages, fixed order) and the
//                                  adjoint image G = dL/dI;
//   evk_flowcm_grad_f32            the gather / scatter pass of evk_flowts_grad_f32 with e = q (slopes of G) and its own bound.
#include "evk_accum.h"

namespace evk {

// The four planes of evk_flowts_warp_f32 are accumulated in the fixed point of evk_accum.h: a contribution is tau w or w with
// 0 <= tau <= 1 and a bilinear weight 0 <= w <= 1, so it is in [-1, 1].  The field gradients and the contrast loss's plane add
// 64-bit integers at per-sample scales of their own (fl_grad_scale, fl_scale_of_bound).

// the sample's slice [o0, o1) of the concatenated columns, clamped into [0, n_total]: a bad `offsets` reads nothing out of bounds
__device__ __forceinline__ void fl_range(const int64_t *__restrict__ offsets, int b, int64_t n_total, int64_t &o0, int64_t &o1) {
    o0 = offsets[b];
    o1 = offsets[b + 1];
    o0 = o0 < 0 ? 0 : (o0 > n_total ? n_total : o0);
    o1 = o1 < o0 ? o0 : (o1 > n_total ? n_total : o1);
}

// Bilinear sample of the (2, h, wd) field at (xv, yv): k_warp_flow_field_f32's float32 expressions in its order (grid_sample,
// align_corners=True, zero padding; the coordinate is normalised to [-1, 1] and back), so that x' below is warp_events_flow_torch's.
struct FlowSample {
    float u, v;          // the sampled flow
    int x0, y0;          // top-left corner of the cell
    float w, e, nn, ss;  // fractions: w = ix - x0, e = 1 - w, nn = iy - y0, ss = 1 - nn
};

__device__ __forceinline__ FlowSample fl_sample(const float *__restrict__ flow, int h, int wd, int64_t plane, float xv, float yv) {
    const float wm1 = (float)(wd - 1), hm1 = (float)(h - 1);
    const float gx = xv / wm1 * 2.0f - 1.0f, gy = yv / hm1 * 2.0f - 1.0f;
    const float ix = (gx + 1.0f) / 2.0f * wm1, iy = (gy + 1.0f) / 2.0f * hm1;
    const float xw = floorf(ix), yn = floorf(iy);
    FlowSample s;
    s.w = ix - xw;
    s.e = 1.0f - s.w;
    s.nn = iy - yn;
    s.ss = 1.0f - s.nn;
    s.x0 = (int)xw;
    s.y0 = (int)yn;
    float f[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float *fl = flow + c * plane;
        auto at = [&](int yy, int xx) -> float {
            return (xx >= 0 && xx < wd && yy >= 0 && yy < h) ? fl[(int64_t)yy * wd + xx] : 0.0f;
        };
        float acc = at(s.y0, s.x0) * (s.e * s.ss);
        acc = acc + at(s.y0, s.x0 + 1) * (s.w * s.ss);
        acc = acc + at(s.y0 + 1, s.x0) * (s.e * s.nn);
        acc = acc + at(s.y0 + 1, s.x0 + 1) * (s.w * s.nn);
        f[c] = acc;
    }
    s.u = f[0];
    s.v = f[1];
    return s;
}

// Steps 1' and 2 for one event: sample, warp in float32, events_bounds_mask(0, W, 0, H) and the inner clip x' < W, y' < H of
// the (H + 1, W + 1) canvas -- together 0 < x' < W, 0 < y' < H, written so that NaN is rejected -- then floor / fraction.
// cls: 0 for p > 0, 2 for p <= 0 (first plane of the class); a NaN polarity belongs to neither.  False: the event adds nothing.
__device__ __forceinline__ bool fl_event(const float *__restrict__ flow, int h, int wd, int64_t plane, float xv, float yv, float tv,
                                         float pv, float t_ref, FlowSample &s, float &dt, int &px, int &py, float &dx, float &dy,
                                         int &cls) {
    const bool pos = pv > 0.0f, neg = pv <= 0.0f;
    if (!pos && !neg) return false;
    s = fl_sample(flow, h, wd, plane, xv, yv);
    dt = tv - t_ref;
    const float xw = xv + s.u * dt, yw = yv + s.v * dt;
    if (!(xw > 0.0f && xw < (float)wd && yw > 0.0f && yw < (float)h)) return false;
    const float fx = floorf(xw), fy = floorf(yw);
    dx = xw - fx;
    dy = yw - fy;
    px = (int)fx;  // 0 <= px <= wd - 1: px + 1 is a column of the (wd + 1)-wide canvas
    py = (int)fy;
    cls = pos ? 0 : 2;
    return true;
}

__global__ void __launch_bounds__(EVK_WAVE) k_flowts_time_constants(const float *__restrict__ t,
                                                                    const int64_t *__restrict__ offsets, int batch,
                                                                    int64_t n_total, int backward, float *__restrict__ tc) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    int64_t o0, o1;
    fl_range(offsets, b, n_total, o0, o1);
    float first = 0.0f, last = 0.0f;
    if (o1 > o0) {
        first = t[o0];
        last = t[o1 - 1];
    }
    const float td = (last - first) + 1e-6f;
    tc[3 * b] = backward ? first : last;
    tc[3 * b + 1] = backward ? last : first;
    tc[3 * b + 2] = backward ? -td : td;  // (t - t_last) / -td is (t_last - t) / td to the bit
}

// grid = (blocks, batch); one event per thread and trip.  A sample starts anywhere in the concatenated columns, so the loads
// are dwords; eight 64-bit atomics per counted event bound the kernel, not the loads.
__global__ void __launch_bounds__(EVK_BLOCK) k_flowts_warp(const float *__restrict__ x, const float *__restrict__ y,
                                                           const float *__restrict__ t, const float *__restrict__ p,
                                                           const int64_t *__restrict__ offsets, int64_t n_total,
                                                           const float *__restrict__ flow, int h, int wd,
                                                           const float *__restrict__ tc, acc64_t *__restrict__ acc4) {
    const int b = blockIdx.y, cw = wd + 1;
    int64_t o0, o1;
    fl_range(offsets, b, n_total, o0, o1);
    const float t_ref = tc[3 * b], t_org = tc[3 * b + 1], tdiv = tc[3 * b + 2];
    const int64_t fplane = (int64_t)h * wd, plane = (int64_t)(h + 1) * cw;
    const float *fl = flow + (int64_t)b * 2 * fplane;
    acc64_t *acc = acc4 + (int64_t)b * 4 * plane;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = o0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < o1; i += stride) {
        FlowSample s;
        float dt, dx, dy;
        int px, py, cls;
        const float tv = t[i];
        if (!fl_event(fl, h, wd, fplane, x[i], y[i], tv, p[i], t_ref, s, dt, px, py, dx, dy, cls)) continue;
        const float tau = (tv - t_org) / tdiv;
        const float ax = 1.0f - dx, ay = 1.0f - dy;
        acc64_t *ts = acc + (int64_t)cls * plane + (int64_t)py * cw + px, *cn = ts + plane;
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

// out4 = the fixed-point planes as float32
__global__ void __launch_bounds__(EVK_BLOCK) k_flowts_planes(const acc64_t *__restrict__ acc4, int64_t elems,
                                                             float *__restrict__ out4) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < elems; i += stride)
        out4[i] = unfixed32(acc4[i]);
}

// ---- gradient ------------------------------------------------------------------------------------------------------------

// absmax[b] = the bit pattern of max |adj4[b]| (non-negative floats order like their bits; a NaN is above every number)
__global__ void __launch_bounds__(EVK_BLOCK) k_flowts_absmax(const float *__restrict__ adj4, int64_t elems,
                                                             uint32_t *__restrict__ absmax) {
    const float *a = adj4 + (int64_t)blockIdx.y * elems;
    uint32_t m = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < elems; i += (int64_t)gridDim.x * blockDim.x)
        m = max(m, __float_as_uint(fabsf(a[i])));
    for (int off = EVK_WAVE / 2; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_down((int)m, off, EVK_WAVE));
    if (threadIdx.x % EVK_WAVE == 0 && m) atomicMax(absmax + blockIdx.y, m);
}

// The sample's fixed-point exponent k.  A term of the field gradient is b_j dt e with 0 <= b_j <= 1, |dt| <= D = |t_ref - t_origin|
// (events in stream order) and |e| = |tau d g_T + d g_C| <= 4 M: 0 <= tau <= 1 and a slope of the bilinear interpolant is a convex
// combination of differences of two values of magnitude <= M = max |adj4|.  A cell receives at most one term per event, so
// |sum| <= bound = 4 M D n < 2^(E + 1), E = ilogb(bound); with k = 61 - E the scaled sum stays below 2^62 and the n roundings
// (1/2 each) below 2^62 more.  Returns 0: every term is zero (M = 0, D = 0 or n = 0); -1: M is not finite; 1: k is set.
__device__ __forceinline__ int fl_grad_scale(uint32_t absmax_bits, float t_ref, float t_org, int64_t n, int &k) {
    const double m = (double)__uint_as_float(absmax_bits);
    const double bound = 4.0 * m * fabs((double)t_ref - (double)t_org) * (double)n;
    k = 0;
    if (!(bound == bound) || bound > 1.7e308) return -1;
    if (!(bound > 0.0)) return 0;
    k = 61 - ilogb(bound);
    return 1;
}

__global__ void __launch_bounds__(EVK_BLOCK) k_flowts_grad(const float *__restrict__ x, const float *__restrict__ y,
                                                           const float *__restrict__ t, const float *__restrict__ p,
                                                           const int64_t *__restrict__ offsets, int64_t n_total,
                                                           const float *__restrict__ flow, int h, int wd,
                                                           const float *__restrict__ tc, const float *__restrict__ adj4,
                                                           const uint32_t *__restrict__ absmax, acc64_t *__restrict__ gacc) {
    const int b = blockIdx.y, cw = wd + 1;
    int64_t o0, o1;
    fl_range(offsets, b, n_total, o0, o1);
    const float t_ref = tc[3 * b], t_org = tc[3 * b + 1], tdiv = tc[3 * b + 2];
    int k;
    if (fl_grad_scale(absmax[b], t_ref, t_org, o1 - o0, k) <= 0) return;
    const int64_t fplane = (int64_t)h * wd, plane = (int64_t)(h + 1) * cw;
    const float *fl = flow + (int64_t)b * 2 * fplane;
    const float *adj = adj4 + (int64_t)b * 4 * plane;
    acc64_t *gx = gacc + (int64_t)b * 2 * fplane, *gy = gx + fplane;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = o0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < o1; i += stride) {
        FlowSample s;
        float dt, dx, dy;
        int px, py, cls;
        const float tv = t[i];
        if (!fl_event(fl, h, wd, fplane, x[i], y[i], tv, p[i], t_ref, s, dt, px, py, dx, dy, cls)) continue;
        const double tau = (double)((tv - t_org) / tdiv);
        const float *gt = adj + (int64_t)cls * plane + (int64_t)py * cw + px;
        double tx, ty, cx, cy;
        bilinear_slopes(gt, cw, dx, dy, tx, ty);
        bilinear_slopes(gt + plane, cw, dx, dy, cx, cy);
        const double sx = ldexp((double)dt * (tau * tx + cx), k), sy = ldexp((double)dt * (tau * ty + cy), k);
        auto scatter = [&](int yy, int xx, float wt) {
            if (wt == 0.0f || xx < 0 || xx >= wd || yy < 0 || yy >= h) return;
            const int64_t j = (int64_t)yy * wd + xx;
            global_add_fixed(gx + j, (acc64_t)__double2ll_rn((double)wt * sx));
            global_add_fixed(gy + j, (acc64_t)__double2ll_rn((double)wt * sy));
        };
        scatter(s.y0, s.x0, s.e * s.ss);
        scatter(s.y0, s.x0 + 1, s.w * s.ss);
        scatter(s.y0 + 1, s.x0, s.e * s.nn);
        scatter(s.y0 + 1, s.x0 + 1, s.w * s.nn);
    }
}

// grad = gacc 2^-k per sample (zero where no term was added; NaN where max |adj4| is not finite)
__global__ void __launch_bounds__(EVK_BLOCK) k_flowts_grad_out(const acc64_t *__restrict__ gacc,
                                                               const int64_t *__restrict__ offsets, int64_t n_total,
                                                               int64_t elems, const float *__restrict__ tc,
                                                               const uint32_t *__restrict__ absmax, float *__restrict__ grad) {
    const int b = blockIdx.y;
    int64_t o0, o1;
    fl_range(offsets, b, n_total, o0, o1);
    int k;
    const int st = fl_grad_scale(absmax[b], tc[3 * b], tc[3 * b + 1], o1 - o0, k);
    const acc64_t *src = gacc + (int64_t)b * elems;
    float *dst = grad + (int64_t)b * elems;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < elems; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = st < 0 ? __uint_as_float(0x7fc00000u) : (float)ldexp((double)(long long)src[i], -k);
}

// ---- contrast loss ----------------------------------------------------------------------------------------------------------

// q = p * p_scale [abs], cast to float32 once (the weight get_iwe's kernels splat)
__device__ __forceinline__ float fl_weight(float pv, double p_scale, bool abs_p) {
    const double ps = (double)pv * p_scale;
    return (float)(abs_p ? fabs(ps) : ps);
}

// qmax[b] = the bit pattern of max |q| over the sample's slice; a NaN weight adds nothing anywhere and is left out here too
__global__ void __launch_bounds__(EVK_BLOCK) k_flowcm_qmax(const float *__restrict__ p, const int64_t *__restrict__ offsets,
                                                           int64_t n_total, double p_scale, uint32_t *__restrict__ qmax) {
    int64_t o0, o1;
    fl_range(offsets, blockIdx.y, n_total, o0, o1);
    uint32_t m = 0;
    for (int64_t i = o0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < o1; i += (int64_t)gridDim.x * blockDim.x) {
        const float q = fabsf(fl_weight(p[i], p_scale, true));
        if (q == q) m = max(m, __float_as_uint(q));
    }
    for (int off = EVK_WAVE / 2; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_down((int)m, off, EVK_WAVE));
    if (threadIdx.x % EVK_WAVE == 0 && m) atomicMax(qmax + blockIdx.y, m);
}

// The sample's fixed-point exponent of a sum of at most n terms, each of magnitude <= bound / n: |sum| <= bound < 2^(E + 1),
// E = ilogb(bound); with k = 61 - E the scaled sum stays below 2^62 and the n roundings (1/2 each) below 2^62 more
// (fl_grad_scale's head-room).  Returns 0: every term is zero; -1: the bound is not finite; 1: k is set.
__device__ __forceinline__ int fl_scale_of_bound(double bound, int &k) {
    k = 0;
    if (!(bound == bound) || bound > 1.7e308) return -1;
    if (!(bound > 0.0)) return 0;
    k = 61 - ilogb(bound);
    return 1;
}

// IWE: a cell receives at most one term per event, q times a bilinear weight in [0, 1]: |cell| <= Q n, Q = max |q|
__device__ __forceinline__ int fl_iwe_scale(uint32_t qmax_bits, int64_t n, int &k) {
    return fl_scale_of_bound((double)__uint_as_float(qmax_bits) * (double)n, k);
}

// Field gradient: a term is b_j dt q e with 0 <= b_j <= 1, |dt| <= D = |t_ref - t_origin|, |q| <= Q and |e| <= 2 M: a slope
// of the bilinear interpolant is a convex combination of differences of two values of magnitude <= M = max |G|
__device__ __forceinline__ int fl_cm_grad_scale(uint32_t absmax_bits, uint32_t qmax_bits, float t_ref, float t_org, int64_t n,
                                                int &k) {
    const double m = (double)__uint_as_float(absmax_bits), q = (double)__uint_as_float(qmax_bits);
    return fl_scale_of_bound(2.0 * m * fabs((double)t_ref - (double)t_org) * q * (double)n, k);
}

// grid = (blocks, batch); one event per thread and trip, dword loads (see k_flowts_warp); four 64-bit atomics per counted event
__global__ void __launch_bounds__(EVK_BLOCK) k_flowcm_splat(const float *__restrict__ x, const float *__restrict__ y,
                                                            const float *__restrict__ t, const float *__restrict__ p,
                                                            const int64_t *__restrict__ offsets, int64_t n_total,
                                                            const float *__restrict__ flow, int h, int wd,
                                                            const float *__restrict__ tc, double p_scale, bool abs_p,
                                                            const uint32_t *__restrict__ qmax, acc64_t *__restrict__ acc1) {
    const int b = blockIdx.y, cw = wd + 1;
    int64_t o0, o1;
    fl_range(offsets, b, n_total, o0, o1);
    int k;
    if (fl_iwe_scale(qmax[b], o1 - o0, k) <= 0) return;
    const float t_ref = tc[3 * b];
    const int64_t fplane = (int64_t)h * wd, plane = (int64_t)(h + 1) * cw;
    const float *fl = flow + (int64_t)b * 2 * fplane;
    acc64_t *acc = acc1 + (int64_t)b * plane;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = o0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < o1; i += stride) {
        FlowSample s;
        float dt, dx, dy;
        int px, py, cls;
        const float q = fl_weight(p[i], p_scale, abs_p);
        if (!fl_event(fl, h, wd, fplane, x[i], y[i], t[i], q, t_ref, s, dt, px, py, dx, dy, cls)) continue;
        const float ax = 1.0f - dx, ay = 1.0f - dy;
        const double qs = ldexp((double)q, k);
        acc64_t *c = acc + (int64_t)py * cw + px;
        global_add_fixed(c, (acc64_t)__double2ll_rn(qs * (double)(ax * ay)));
        global_add_fixed(c + 1, (acc64_t)__double2ll_rn(qs * (double)(dx * ay)));
        global_add_fixed(c + cw, (acc64_t)__double2ll_rn(qs * (double)(ax * dy)));
        global_add_fixed(c + cw + 1, (acc64_t)__double2ll_rn(qs * (double)(dx * dy)));
    }
}

// iwe = acc1 2^-kI per sample (zero where no term was added; NaN where max |q| is not finite)
__global__ void __launch_bounds__(EVK_BLOCK) k_flowcm_iwe_out(const acc64_t *__restrict__ acc1,
                                                              const int64_t *__restrict__ offsets, int64_t n_total,
                                                              int64_t elems, const uint32_t *__restrict__ qmax,
                                                              float *__restrict__ iwe) {
    const int b = blockIdx.y;
    int64_t o0, o1;
    fl_range(offsets, b, n_total, o0, o1);
    int k;
    const int st = fl_iwe_scale(qmax[b], o1 - o0, k);
    const acc64_t *src = acc1 + (int64_t)b * elems;
    float *dst = iwe + (int64_t)b * elems;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < elems; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = st < 0 ? __uint_as_float(0x7fc00000u) : (float)ldexp((double)(long long)src[i], -k);
}

// the workgroup's sum in a fixed order: lanes by shuffle, the four waves through LDS; valid in thread 0
__device__ __forceinline__ double fl_block_sum(double v) {
    __shared__ double part[EVK_BLOCK / EVK_WAVE];
    for (int off = EVK_WAVE / 2; off > 0; off >>= 1) v += __shfl_down(v, off, EVK_WAVE);
    if (threadIdx.x % EVK_WAVE == 0) part[threadIdx.x / EVK_WAVE] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int i = 0; i < EVK_BLOCK / EVK_WAVE; ++i) s += part[i];
    return s;
}

// partials[block] = sum (b - shift) (SQUARE: squared) over the block's pixels; shift: a device double, or NULL for 0
template <bool SQUARE>
__global__ void __launch_bounds__(EVK_BLOCK) k_flowcm_sum(const float *__restrict__ b, int64_t n, const double *__restrict__ shift,
                                                          double *__restrict__ partials) {
    const double m = shift ? shift[0] : 0.0;
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = (double)b[i] - m;
        acc += SQUARE ? v * v : v;
    }
    const double s = fl_block_sum(acc);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// out[0] = factor x the sum of the blocks' partials, in a fixed order (one workgroup)
__global__ void __launch_bounds__(EVK_BLOCK) k_flowcm_final(const double *__restrict__ partials, int nblocks, double factor,
                                                            double *__restrict__ out) {
    double acc = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x) acc += partials[b];
    const double s = fl_block_sum(acc);
    if (threadIdx.x == 0) out[0] = factor * s;
}

// G = factor (S - shift) (float64, stored as float32); shift as in k_flowcm_sum
__global__ void __launch_bounds__(EVK_BLOCK) k_flowcm_adjoint(const float *__restrict__ sm, int64_t n, const double *__restrict__ shift,
                                                              double factor, float *__restrict__ adj) {
    const double m = shift ? shift[0] : 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        adj[i] = (float)(factor * ((double)sm[i] - m));
}

__global__ void __launch_bounds__(EVK_BLOCK) k_flowcm_grad(const float *__restrict__ x, const float *__restrict__ y,
                                                           const float *__restrict__ t, const float *__restrict__ p,
                                                           const int64_t *__restrict__ offsets, int64_t n_total,
                                                           const float *__restrict__ flow, int h, int wd,
                                                           const float *__restrict__ tc, double p_scale, bool abs_p,
                                                           const float *__restrict__ adj1, const uint32_t *__restrict__ qmax,
                                                           const uint32_t *__restrict__ absmax, acc64_t *__restrict__ gacc) {
    const int b = blockIdx.y, cw = wd + 1;
    int64_t o0, o1;
    fl_range(offsets, b, n_total, o0, o1);
    const float t_ref = tc[3 * b], t_org = tc[3 * b + 1];
    int k;
    if (fl_cm_grad_scale(absmax[b], qmax[b], t_ref, t_org, o1 - o0, k) <= 0) return;
    const int64_t fplane = (int64_t)h * wd, plane = (int64_t)(h + 1) * cw;
    const float *fl = flow + (int64_t)b * 2 * fplane;
    const float *adj = adj1 + (int64_t)b * plane;
    acc64_t *gx = gacc + (int64_t)b * 2 * fplane, *gy = gx + fplane;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = o0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < o1; i += stride) {
        FlowSample s;
        float dt, dx, dy;
        int px, py, cls;
        const float q = fl_weight(p[i], p_scale, abs_p);
        if (!fl_event(fl, h, wd, fplane, x[i], y[i], t[i], q, t_ref, s, dt, px, py, dx, dy, cls)) continue;
        double ex, ey;
        bilinear_slopes(adj + (int64_t)py * cw + px, cw, dx, dy, ex, ey);
        const double dq = (double)dt * (double)q;
        const double sx = ldexp(dq * ex, k), sy = ldexp(dq * ey, k);
        auto scatter = [&](int yy, int xx, float wt) {
            if (wt == 0.0f || xx < 0 || xx >= wd || yy < 0 || yy >= h) return;
            const int64_t j = (int64_t)yy * wd + xx;
            global_add_fixed(gx + j, (acc64_t)__double2ll_rn((double)wt * sx));
            global_add_fixed(gy + j, (acc64_t)__double2ll_rn((double)wt * sy));
        };
        scatter(s.y0, s.x0, s.e * s.ss);
        scatter(s.y0, s.x0 + 1, s.w * s.ss);
        scatter(s.y0 + 1, s.x0, s.e * s.nn);
        scatter(s.y0 + 1, s.x0 + 1, s.w * s.nn);
    }
}

// grad = gacc 2^-k per sample (zero where no term was added; NaN where the bound is not finite)
__global__ void __launch_bounds__(EVK_BLOCK) k_flowcm_grad_out(const acc64_t *__restrict__ gacc,
                                                               const int64_t *__restrict__ offsets, int64_t n_total,
                                                               int64_t elems, const float *__restrict__ tc,
                                                               const uint32_t *__restrict__ qmax,
                                                               const uint32_t *__restrict__ absmax, float *__restrict__ grad) {
    const int b = blockIdx.y;
    int64_t o0, o1;
    fl_range(offsets, b, n_total, o0, o1);
    int k;
    const int st = fl_cm_grad_scale(absmax[b], qmax[b], tc[3 * b], tc[3 * b + 1], o1 - o0, k);
    const acc64_t *src = gacc + (int64_t)b * elems;
    float *dst = grad + (int64_t)b * elems;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < elems; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = st < 0 ? __uint_as_float(0x7fc00000u) : (float)ldexp((double)(long long)src[i], -k);
}

}  // namespace evk

// =============================================================================================================
// C ABI
// =============================================================================================================
using namespace evk;

// an image-sized pass per sample: grid = (blocks, batch)
static dim3 fl_image_grid(int64_t elems, int batch) {
    int gx = stream_grid(elems);
    if (gx > 256) gx = 256;
    return dim3((unsigned)gx, (unsigned)batch);
}

extern "C" int evk_flowts_time_constants_f32(const float *t, const int64_t *offsets, int batch, int64_t n_total, int direction,
                                             float *tc, void *stream) {
    if (!offsets || !tc || batch < 1 || batch > 65535 || n_total < 0 || (n_total > 0 && !t) ||
        (direction != EVK_FLOWTS_FORWARD && direction != EVK_FLOWTS_BACKWARD))
        return EVK_EINVAL;
    if ((uintptr_t)t & 3u) return EVK_EALIGN;
    k_flowts_time_constants<<<(batch + EVK_WAVE - 1) / EVK_WAVE, EVK_WAVE, 0, (hipStream_t)stream>>>(
        t, offsets, batch, n_total, direction == EVK_FLOWTS_BACKWARD, tc);
    return launch_status();
}

extern "C" int evk_flowts_warp_f32(const float *x, const float *y, const float *t, const float *p, const int64_t *offsets,
                                   int batch, int64_t n_total, const float *flow, int h, int w, const float *tc, uint64_t *acc4,
                                   float *out4, void *stream) {
    if (!offsets || !flow || !tc || !acc4 || !out4 || batch < 1 || batch > 65535 || n_total < 0 || h < 2 || w < 2 ||
        (n_total > 0 && (!x || !y || !t || !p)))
        return EVK_EINVAL;
    if (n_total > 0 && !columns_elem_aligned(x, y, t, p)) return EVK_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    acc64_t *acc = reinterpret_cast<acc64_t *>(acc4);
    if (n_total > 0)
        k_flowts_warp<<<dim3((unsigned)stream_grid(n_total), (unsigned)batch), EVK_BLOCK, 0, s>>>(x, y, t, p, offsets, n_total, flow,
                                                                                                 h, w, tc, acc);
    const int64_t elems = (int64_t)batch * 4 * (h + 1) * (w + 1);
    k_flowts_planes<<<stream_grid(elems), EVK_BLOCK, 0, s>>>(acc, elems, out4);
    return launch_status();
}

extern "C" int evk_flowts_grad_f32(const float *x, const float *y, const float *t, const float *p, const int64_t *offsets,
                                   int batch, int64_t n_total, const float *flow, int h, int w, const float *tc,
                                   const float *adj4, uint32_t *absmax, int64_t *gacc, float *grad, void *stream) {
    if (!offsets || !flow || !tc || !adj4 || !absmax || !gacc || !grad || batch < 1 || batch > 65535 || n_total < 0 || h < 2 ||
        w < 2 || (n_total > 0 && (!x || !y || !t || !p)))
        return EVK_EINVAL;
    if (n_total > 0 && !columns_elem_aligned(x, y, t, p)) return EVK_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    acc64_t *acc = reinterpret_cast<acc64_t *>(gacc);
    hipError_t e = hipMemsetAsync(absmax, 0, (size_t)batch * sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    const int64_t adj_elems = (int64_t)4 * (h + 1) * (w + 1), elems = (int64_t)2 * h * w;
    k_flowts_absmax<<<fl_image_grid(adj_elems, batch), EVK_BLOCK, 0, s>>>(adj4, adj_elems, absmax);
    if (n_total > 0)
        k_flowts_grad<<<dim3((unsigned)stream_grid(n_total), (unsigned)batch), EVK_BLOCK, 0, s>>>(x, y, t, p, offsets, n_total, flow,
                                                                                                 h, w, tc, adj4, absmax, acc);
    k_flowts_grad_out<<<fl_image_grid(elems, batch), EVK_BLOCK, 0, s>>>(acc, offsets, n_total, elems, tc, absmax, grad);
    return launch_status();
}

// ---- contrast loss ----------------------------------------------------------------------------------------------------------
constexpr int kFlReduceBlocks = 1024;  // partial sums of the loss: scratch[0 .. 1024), the mean in scratch[1024]

extern "C" int evk_flowcm_warp_f32(const float *x, const float *y, const float *t, const float *p, const int64_t *offsets,
                                   int batch, int64_t n_total, const float *flow, int h, int w, const float *tc, double p_scale,
                                   uint32_t flags, uint32_t *qmax, uint64_t *acc, float *iwe, void *stream) {
    if (!offsets || !flow || !tc || !qmax || !acc || !iwe || batch < 1 || batch > 65535 || n_total < 0 || h < 2 || w < 2 ||
        (flags & ~EVK_FLOWCM_ABS) || (n_total > 0 && (!x || !y || !t || !p)))
        return EVK_EINVAL;
    if (n_total > 0 && !columns_elem_aligned(x, y, t, p)) return EVK_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    acc64_t *a = reinterpret_cast<acc64_t *>(acc);
    hipError_t e = hipMemsetAsync(qmax, 0, (size_t)batch * sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    if (n_total > 0) {
        const dim3 grid((unsigned)stream_grid(n_total), (unsigned)batch);
        k_flowcm_qmax<<<grid, EVK_BLOCK, 0, s>>>(p, offsets, n_total, p_scale, qmax);
        k_flowcm_splat<<<grid, EVK_BLOCK, 0, s>>>(x, y, t, p, offsets, n_total, flow, h, w, tc, p_scale,
                                                  (flags & EVK_FLOWCM_ABS) != 0, qmax, a);
    }
    const int64_t elems = (int64_t)(h + 1) * (w + 1);
    k_flowcm_iwe_out<<<fl_image_grid(elems, batch), EVK_BLOCK, 0, s>>>(a, offsets, n_total, elems, qmax, iwe);
    return launch_status();
}

extern "C" int evk_flowcm_post_f32(const float *iwe, int h, int w, const double *host_weights, const double *dev_weights,
                                   int radius, int objective, float *work, float *adj, double *out, void *scratch,
                                   int64_t scratch_bytes, void *stream) {
    if (!iwe || h <= 0 || w <= 0 || !work || !out || !scratch ||
        (objective != EVK_FLOWCM_VARIANCE && objective != EVK_FLOWCM_MEAN_SQUARE))
        return EVK_EINVAL;
    if (radius >= 0 && (radius <= EVK_MAX_RADIUS ? !host_weights : !dev_weights)) return EVK_EINVAL;
    if (scratch_bytes < evk_reduce_scratch_bytes() || scratch_bytes < (int64_t)(kFlReduceBlocks + 1) * (int64_t)sizeof(double))
        return EVK_ESCRATCH;
    hipStream_t s = (hipStream_t)stream;
    const int64_t npix = (int64_t)h * w;
    // work: [0] the blurred B, [1] the filter's scratch, [2] S = blur(B)
    float *b1 = work, *tmp = work + npix, *s1 = work + 2 * npix;
    const int dims[2] = {h, w};
    auto blur = [&](const float *src, float *dst) {
        return radius <= EVK_MAX_RADIUS ? evk_gaussian_filter_f32(src, dst, tmp, 2, dims, host_weights, radius, stream)
                                        : evk_gaussian_filter_wide_f32(src, dst, tmp, 2, dims, dev_weights, radius, stream);
    };
    const float *b = iwe;
    if (radius >= 0) {
        const int rc = blur(iwe, b1);
        if (rc != EVK_OK) return rc;
        b = b1;
    }
    int grid = stream_grid(npix);
    if (grid > kFlReduceBlocks) grid = kFlReduceBlocks;
    double *partials = (double *)scratch, *mean = nullptr;
    if (objective == EVK_FLOWCM_VARIANCE) {
        mean = partials + kFlReduceBlocks;
        k_flowcm_sum<false><<<grid, EVK_BLOCK, 0, s>>>(b, npix, nullptr, partials);
        k_flowcm_final<<<1, EVK_BLOCK, 0, s>>>(partials, grid, 1.0 / (double)npix, mean);
    }
    k_flowcm_sum<true><<<grid, EVK_BLOCK, 0, s>>>(b, npix, mean, partials);
    k_flowcm_final<<<1, EVK_BLOCK, 0, s>>>(partials, grid, -1.0 / (double)npix, out);
    if (adj) {
        const float *sm = b;
        if (radius >= 0) {  // the reflect-mode blur with a symmetric normalised kernel is self-adjoint and keeps constants
            const int rc = blur(b1, s1);
            if (rc != EVK_OK) return rc;
            sm = s1;
        }
        k_flowcm_adjoint<<<grid, EVK_BLOCK, 0, s>>>(sm, npix, mean, -2.0 / (double)npix, adj);
    }
    return launch_status();
}

extern "C" int evk_flowcm_grad_f32(const float *x, const float *y, const float *t, const float *p, const int64_t *offsets,
                                   int batch, int64_t n_total, const float *flow, int h, int w, const float *tc, double p_scale,
                                   uint32_t flags, const float *adj, const uint32_t *qmax, uint32_t *absmax, int64_t *gacc,
                                   float *grad, void *stream) {
    if (!offsets || !flow || !tc || !adj || !qmax || !absmax || !gacc || !grad || batch < 1 || batch > 65535 || n_total < 0 ||
        h < 2 || w < 2 || (flags & ~EVK_FLOWCM_ABS) || (n_total > 0 && (!x || !y || !t || !p)))
        return EVK_EINVAL;
    if (n_total > 0 && !columns_elem_aligned(x, y, t, p)) return EVK_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    acc64_t *acc = reinterpret_cast<acc64_t *>(gacc);
    hipError_t e = hipMemsetAsync(absmax, 0, (size_t)batch * sizeof(uint32_t), s);
    if (e != hipSuccess) return (int)e;
    const int64_t adj_elems = (int64_t)(h + 1) * (w + 1), elems = (int64_t)2 * h * w;
    k_flowts_absmax<<<fl_image_grid(adj_elems, batch), EVK_BLOCK, 0, s>>>(adj, adj_elems, absmax);
    if (n_total > 0)
        k_flowcm_grad<<<dim3((unsigned)stream_grid(n_total), (unsigned)batch), EVK_BLOCK, 0, s>>>(
            x, y, t, p, offsets, n_total, flow, h, w, tc, p_scale, (flags & EVK_FLOWCM_ABS) != 0, adj, qmax, absmax, acc);
    k_flowcm_grad_out<<<fl_image_grid(elems, batch), EVK_BLOCK, 0, s>>>(acc, offsets, n_total, elems, tc, qmax, absmax, grad);
    return launch_status();
}
