// The model-independent helpers around the warp of the fused kernel files (evk_warps.hip, evk_tsobj.hip, evk_segment.hip,
// evk_flowloss.hip): the 4-event column load, the 64-bit fixed-point accumulation, the fixed-order block reduction and the
// slopes of the adjoint gathers.  One copy, because what these files promise rests on it being the same everywhere: sums that
// do not depend on the order of the atomics, and gradients reduced in a fixed order.  The model-dependent half is
// evk_warp_models.h.
#pragma once
#include "evk_common.h"

namespace evk {

// Events base .. base + 3 of a column: one load4 when `vec` (all four present, 16-byte aligned column), else `cnt` scalar
// loads and zeros behind them.
template <typename T>
__device__ __forceinline__ Vec4<T> load_quad(const T *p, int64_t base, int cnt, bool vec) {
    if (vec) return load4(p, base >> 2);
    Vec4<T> r;
#pragma unroll
    for (int k = 0; k < 4; ++k) r.v[k] = (k < cnt) ? p[base + k] : T(0);
    return r;
}

// 64-bit fixed point with 32 fractional bits: integer adds commute, so a plane summed in it -- and every loss and gradient
// formed from it -- is the same bits whatever order the atomics land in.  A contribution is a float32 in [-1, 1] (each user
// says why its own are); scaling by 2^32 is exact and the rounding to an integer is below 2^-33; a pixel holds up to 2^31 of
// them.
typedef unsigned long long acc64_t;
constexpr float kFixedScale = 4294967296.0f;
constexpr double kFixedUnscale = 1.0 / 4294967296.0;

__device__ __forceinline__ acc64_t fixed32(float v) { return (acc64_t)__float2ll_rn(v * kFixedScale); }
__device__ __forceinline__ float unfixed32(acc64_t a) { return (float)((double)(long long)a * kFixedUnscale); }

__device__ __forceinline__ void lds_add_fixed(acc64_t *p, float v) {
    __hip_atomic_fetch_add(p, fixed32(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void global_add_fixed(acc64_t *p, acc64_t v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// K running float64 sums of an EVK_BLOCK-thread workgroup in a fixed order: wave shuffle -> LDS -> out[0 .. K) written by
// threads 0 .. K-1.
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

// d_x g, d_y g of the bilinear interpolant of g at the event (corners a b / c d), one-sided by the floor convention
__device__ __forceinline__ void bilinear_slopes(const float *__restrict__ g, int cw, float dx, float dy, double &gx, double &gy) {
    const double a = (double)g[0], b = (double)g[1], c = (double)g[cw], d = (double)g[cw + 1];
    gx = (b - a) * (1.0 - (double)dy) + (d - c) * (double)dy;
    gy = (c - a) * (1.0 - (double)dx) + (d - b) * (double)dx;
}

// host: the four columns are aligned to their element (4 bytes; 8 for float64).  The kernels read them with dword loads unless
// all four are 16-byte aligned.
template <typename T>
inline bool columns_elem_aligned(const T *x, const T *y, const T *t, const T *p) {
    const uintptr_t m = sizeof(T) - 1;
    return !(((uintptr_t)x | (uintptr_t)y | (uintptr_t)t | (uintptr_t)p) & m);
}

}  // namespace evk
