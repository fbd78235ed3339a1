// Motion segmentation by motion compensation (Stoffregen et al., ICCV 2019; DESIGN.md section 6, "Motion segmentation";
// definition in include/evk.h): L <= 8 motion models of one kind, a soft association P (L, N) of every event with every model.
//   evk_seg_splat_*   fused warp -> mask -> weighted splat of the L cluster images I_l = sum_k q_kl (bilinear weights of the
//                     event under theta_l), in 64-bit fixed point: the planes do not depend on the order of the atomics;
//   evk_seg_grad_*    the adjoint gather: grid.y = cluster, each event reads the four corners of G_l and adds
//                     q_kl (d_x G_l Jx_d + d_y G_l Jy_d) to dims float64 sums, reduced per wave, per workgroup and by a final
//                     kernel in a fixed order: no atomics, so the gradient is bitwise repeatable;
//   evk_seg_assign_*  the re-association: per event the L blurred images are gathered at the L warped positions and
//                     normalised across the clusters; the label is the argmax.
// The image-sized steps between them (blur, variance, adjoint image) are evk_flowcm_post_f32, once per plane.
#include "evk_accum.h"
#include "evk_warp_models.h"

namespace evk {

constexpr int kSegMaxClusters = EVK_SEG_MAX_CLUSTERS;
constexpr int kSegGatherBlocks = 1024;  // partial sums of the adjoint gather per cluster: kSegGatherBlocks x kMaxDims doubles

// The parameters of every cluster, by value in the kernel arguments (8 x 80 bytes).
struct SegArgs {
    WarpArgs w[kSegMaxClusters];
};

// The parameters of the block's cluster by a chain of uniform selects over the by-value struct (scalar registers throughout).
__device__ __forceinline__ WarpArgs seg_cluster(const SegArgs &a, int l) {
    WarpArgs w = a.w[0];
#pragma unroll
    for (int i = 1; i < kSegMaxClusters; ++i)
        if (l == i) w = a.w[i];
    return w;
}

// Per-event part shared by the three kernels: ts_event of evk_tsobj.hip without the class -- the warp in float64, the bounds
// mask written so that NaN is rejected, the cast to float32, the inner clip at the padded canvas, floor / fraction: an event
// lands where get_iwe puts it.  The caller has dropped NaN polarities.  False when the event does not count under `w`.
template <int M, bool JAC>
__device__ __forceinline__ bool seg_event(const WarpArgs &w, double x, double y, double dt, double bw, double bh, float clipx,
                                          float clipy, int &px, int &py, float &dx, float &dy, float *jf) {
    double xw, yw, jv[kJac];
    warp_event<M, JAC>(w, x, y, dt, xw, yw, jv);
    if (!(xw > 0.0 && xw <= bw && yw > 0.0 && yw <= bh)) return false;
    const float xf = (float)xw, yf = (float)yw;
    if (xf >= clipx || yf >= clipy) return false;
    const float fx = floorf(xf), fy = floorf(yf);
    dx = xf - fx;
    dy = yf - fy;
    px = (int)fx;
    py = (int)fy;
    if constexpr (JAC) {
#pragma unroll
        for (int k = 0; k < Model<M>::njac; ++k) jf[k] = (float)jv[k];
    }
    return true;
}

// q_kl of one event: P_kl, with EVK_SEG_POLARITY times the sign of the polarity; 0 for P_kl == 0 or NaN (adds nothing)
__device__ __forceinline__ float seg_weight(float prob, bool pos, bool signedq) {
    if (!(prob > 0.0f || prob < 0.0f)) return 0.0f;
    return (signedq && !pos) ? -prob : prob;
}

// The planes are accumulated in the fixed point of evk_accum.h: a contribution is q times a bilinear weight in [0, 1] with
// |q| <= 1, so it is in [-1, 1].

// ---- splat -------------------------------------------------------------------------------------------------------------

// grid = (chunks, bands).  LDS holds L planes x band_rows x cw fixed-point cells; an event's four columns are loaded once and
// the clusters are looped over in registers; the flush adds the band's rows with global 64-bit integer atomics.  Every band
// re-reads and re-warps its chunk of the events.
template <typename T, int M, bool VEC>
__global__ void __launch_bounds__(kBandThreads) k_seg_band(const T *__restrict__ x, const T *__restrict__ y,
                                                           const T *__restrict__ t, const T *__restrict__ p, int64_t n,
                                                           int64_t chunk, SegArgs a, int L, const float *__restrict__ probs,
                                                           bool pvec, bool signedq, double t_ref, double bw, double bh, int ch,
                                                           int cw, int band_rows, acc64_t *__restrict__ acc) {
    extern __shared__ acc64_t seg_band[];
    const int r0 = blockIdx.y * band_rows, r1 = min(r0 + band_rows, ch), rows = r1 - r0;
    const int plane_lds = rows * cw;
    for (int i = threadIdx.x; i < L * plane_lds; i += blockDim.x) seg_band[i] = 0;
    __syncthreads();
    const float clipx = (float)(cw - 1), clipy = (float)(ch - 1);
    const int64_t c0 = (int64_t)blockIdx.x * chunk, c1 = min(c0 + chunk, n);
    for (int64_t base = c0 + 4 * (int64_t)threadIdx.x; base < c1; base += 4 * (int64_t)blockDim.x) {
        const int cnt = (int)min((int64_t)4, c1 - base);
        const bool vec = VEC && cnt == 4;
        const Vec4<T> xv = load_quad(x, base, cnt, vec), yv = load_quad(y, base, cnt, vec), tv = load_quad(t, base, cnt, vec),
                      pv = load_quad(p, base, cnt, vec);
#pragma unroll 1
        for (int l = 0; l < L; ++l) {  // rolled: a.w[l] is read from the kernel arguments as it is needed
            const Vec4<float> qv = load_quad(probs + (int64_t)l * n, base, cnt, pvec && cnt == 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= cnt) break;
                const bool pos = pv.v[k] > T(0), neg = pv.v[k] <= T(0);
                const float q = seg_weight(qv.v[k], pos, signedq);
                if ((!pos && !neg) || q == 0.0f) continue;
                int px, py;
                float dx, dy;
                if (!seg_event<M, false>(a.w[l], (double)xv.v[k], (double)yv.v[k], (double)tv.v[k] - t_ref, bw, bh, clipx, clipy,
                                         px, py, dx, dy, nullptr))
                    continue;
                if (py + 1 < r0 || py >= r1) continue;  // neither of its two rows is in this band
                const float ax = 1.0f - dx, ay = 1.0f - dy;
                // offset of the top-left cell in plane l; -cw + px when only the bottom row lies in the band
                acc64_t *c = seg_band + l * plane_lds + (py - r0) * cw + px;
                if (py >= r0) {
                    lds_add_fixed(c, q * (ax * ay));
                    lds_add_fixed(c + 1, q * (dx * ay));
                }
                if (py + 1 < r1) {
                    lds_add_fixed(c + cw, q * (ax * dy));
                    lds_add_fixed(c + cw + 1, q * (dx * dy));
                }
            }
        }
    }
    __syncthreads();
    const int64_t plane = (int64_t)ch * cw;
    for (int l = 0; l < L; ++l) {
        acc64_t *dst = acc + (int64_t)l * plane + (int64_t)r0 * cw;
        const acc64_t *src = seg_band + l * plane_lds;
        for (int i = threadIdx.x; i < plane_lds; i += blockDim.x) {
            const acc64_t v = src[i];
            if (v != 0) global_add_fixed(dst + i, v);
        }
    }
}

template <typename T, int M, bool VEC>
__global__ void __launch_bounds__(EVK_BLOCK) k_seg_direct(const T *__restrict__ x, const T *__restrict__ y,
                                                          const T *__restrict__ t, const T *__restrict__ p, int64_t n, SegArgs a,
                                                          int L, const float *__restrict__ probs, bool pvec, bool signedq,
                                                          double t_ref, double bw, double bh, int ch, int cw,
                                                          acc64_t *__restrict__ acc) {
    const float clipx = (float)(cw - 1), clipy = (float)(ch - 1);
    const int64_t plane = (int64_t)ch * cw;
    const int64_t stride = 4 * (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = 4 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x); base < n; base += stride) {
        const int cnt = (int)min((int64_t)4, n - base);
        const bool vec = VEC && cnt == 4;
        const Vec4<T> xv = load_quad(x, base, cnt, vec), yv = load_quad(y, base, cnt, vec), tv = load_quad(t, base, cnt, vec),
                      pv = load_quad(p, base, cnt, vec);
#pragma unroll 1
        for (int l = 0; l < L; ++l) {  // rolled: a.w[l] is read from the kernel arguments as it is needed
            const Vec4<float> qv = load_quad(probs + (int64_t)l * n, base, cnt, pvec && cnt == 4);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k >= cnt) break;
                const bool pos = pv.v[k] > T(0), neg = pv.v[k] <= T(0);
                const float q = seg_weight(qv.v[k], pos, signedq);
                if ((!pos && !neg) || q == 0.0f) continue;
                int px, py;
                float dx, dy;
                if (!seg_event<M, false>(a.w[l], (double)xv.v[k], (double)yv.v[k], (double)tv.v[k] - t_ref, bw, bh, clipx, clipy,
                                         px, py, dx, dy, nullptr))
                    continue;
                const float ax = 1.0f - dx, ay = 1.0f - dy;
                acc64_t *c = acc + (int64_t)l * plane + (int64_t)py * cw + px;
                global_add_fixed(c, fixed32(q * (ax * ay)));
                global_add_fixed(c + 1, fixed32(q * (dx * ay)));
                global_add_fixed(c + cw, fixed32(q * (ax * dy)));
                global_add_fixed(c + cw + 1, fixed32(q * (dx * dy)));
            }
        }
    }
}

// out = the fixed-point planes as float32
__global__ void __launch_bounds__(EVK_BLOCK) k_seg_planes(const acc64_t *__restrict__ acc, int64_t elems, float *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < elems; i += stride)
        out[i] = unfixed32(acc[i]);
}

// ---- adjoint gather ----------------------------------------------------------------------------------------------------

// grid = (blocks, L): block (b, l) sums cluster l's terms of its share of the events into partials[(l, b)][0 .. dims)
template <typename T, int M, bool VEC>
__global__ void __launch_bounds__(EVK_BLOCK) k_seg_gather(const T *__restrict__ x, const T *__restrict__ y,
                                                          const T *__restrict__ t, const T *__restrict__ p, int64_t n, SegArgs a,
                                                          const float *__restrict__ probs, bool pvec, bool signedq, double t_ref,
                                                          double bw, double bh, int ch, int cw, const float *__restrict__ adj,
                                                          double *__restrict__ partials) {
    constexpr int D = Model<M>::dims;
    const int l = blockIdx.y;
    const WarpArgs w = seg_cluster(a, l);
    const float *__restrict__ pl = probs + (int64_t)l * n;
    const float *__restrict__ g = adj + (int64_t)l * ch * cw;
    const float clipx = (float)(cw - 1), clipy = (float)(ch - 1);
    double acc[D] = {};
    const int64_t stride = 4 * (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = 4 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x); base < n; base += stride) {
        const int cnt = (int)min((int64_t)4, n - base);
        const bool vec = VEC && cnt == 4;
        const Vec4<T> xv = load_quad(x, base, cnt, vec), yv = load_quad(y, base, cnt, vec), tv = load_quad(t, base, cnt, vec),
                      pv = load_quad(p, base, cnt, vec);
        const Vec4<float> qv = load_quad(pl, base, cnt, pvec && cnt == 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (k >= cnt) break;
            const bool pos = pv.v[k] > T(0), neg = pv.v[k] <= T(0);
            const float q = seg_weight(qv.v[k], pos, signedq);
            if ((!pos && !neg) || q == 0.0f) continue;
            int px, py;
            float dx, dy, jf[kJac];
            if (!seg_event<M, true>(w, (double)xv.v[k], (double)yv.v[k], (double)tv.v[k] - t_ref, bw, bh, clipx, clipy, px, py, dx,
                                    dy, jf))
                continue;
            double ex, ey;
            bilinear_slopes(g + (int64_t)py * cw + px, cw, dx, dy, ex, ey);
            ex *= (double)q;
            ey *= (double)q;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const int sx = Model<M>::jx(d), sy = Model<M>::jy(d);
                const double jxv = sx >= 0 ? (double)jf[sx < 0 ? 0 : sx] : 0.0, jyv = sy >= 0 ? (double)jf[sy < 0 ? 0 : sy] : 0.0;
                acc[d] += ex * jxv + ey * jyv;
            }
        }
    }
    block_sums<D>(acc, partials + ((int64_t)l * kSegGatherBlocks + blockIdx.x) * kMaxDims);
}

// block l: out[l dims .. (l + 1) dims) = the sums over cluster l's partials, in a fixed order
__global__ void __launch_bounds__(EVK_BLOCK) k_seg_final(const double *__restrict__ partials, int nblocks, int dims,
                                                         double *__restrict__ out) {
    const double *mine = partials + (int64_t)blockIdx.x * kSegGatherBlocks * kMaxDims;
    double acc[kMaxDims] = {};
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x)
#pragma unroll
        for (int k = 0; k < kMaxDims; ++k) acc[k] += mine[(int64_t)b * kMaxDims + k];
    __shared__ double tot[kMaxDims];
    block_sums<kMaxDims>(acc, tot);
    __syncthreads();
    if ((int)threadIdx.x < dims) out[(int64_t)blockIdx.x * dims + threadIdx.x] = tot[threadIdx.x];
}

// ---- assignment --------------------------------------------------------------------------------------------------------

template <typename U>
__device__ __forceinline__ void seg_store(U *p, int64_t base, int cnt, bool vec, const U (&v)[4]) {
    static_assert(sizeof(U) == 4, "one dword per event");
    if (vec) {
        uint4 q;
        q.x = __builtin_bit_cast(uint32_t, v[0]);
        q.y = __builtin_bit_cast(uint32_t, v[1]);
        q.z = __builtin_bit_cast(uint32_t, v[2]);
        q.w = __builtin_bit_cast(uint32_t, v[3]);
        reinterpret_cast<uint4 *>(p)[base >> 2] = q;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < cnt) p[base + k] = v[k];
}

// One grid-stride pass, four events per thread.  c[l] = max(0, s bilinear(B_l)) at the event's place under theta_l (0 when it
// does not count there), S = sum_l c[l] in cluster order, P' = (float)(c / S) or the old row when S == 0; label = argmax of the
// row written, lowest l on ties.  Every loop over the clusters is unrolled to the bound 8 so that c[] and the rows stay in
// registers.  The stores of one cluster's four events are one 16-byte store per lane where probs_out allows it.
template <typename T, int M, bool VEC>
__global__ void __launch_bounds__(EVK_BLOCK) k_seg_assign(const T *__restrict__ x, const T *__restrict__ y,
                                                          const T *__restrict__ t, const T *__restrict__ p, int64_t n, SegArgs a,
                                                          int L, const float *__restrict__ probs, bool ovec, bool lvec,
                                                          bool signedq, double t_ref, double bw, double bh, int ch, int cw,
                                                          const float *__restrict__ blurred, float *__restrict__ probs_out,
                                                          int32_t *__restrict__ labels) {
    const float clipx = (float)(cw - 1), clipy = (float)(ch - 1);
    const int64_t plane = (int64_t)ch * cw;
    const int64_t stride = 4 * (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = 4 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x); base < n; base += stride) {
        const int cnt = (int)min((int64_t)4, n - base);
        const bool vec = VEC && cnt == 4;
        const Vec4<T> xv = load_quad(x, base, cnt, vec), yv = load_quad(y, base, cnt, vec), tv = load_quad(t, base, cnt, vec),
                      pv = load_quad(p, base, cnt, vec);
        float row[kSegMaxClusters][4];
        int32_t lab[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            lab[k] = 0;
#pragma unroll
            for (int l = 0; l < kSegMaxClusters; ++l) row[l][k] = 0.0f;
            if (k >= cnt) continue;
            const bool pos = pv.v[k] > T(0), neg = pv.v[k] <= T(0);
            const double sgn = (signedq && !pos) ? -1.0 : 1.0;
            const double dt = (double)tv.v[k] - t_ref;
            double c[kSegMaxClusters], S = 0.0;
#pragma unroll
            for (int l = 0; l < kSegMaxClusters; ++l) {
                c[l] = 0.0;
                if (l >= L || (!pos && !neg)) continue;
                int px, py;
                float dx, dy;
                if (!seg_event<M, false>(a.w[l], (double)xv.v[k], (double)yv.v[k], dt, bw, bh, clipx, clipy, px, py, dx, dy, nullptr))
                    continue;
                const float *g = blurred + (int64_t)l * plane + (int64_t)py * cw + px;
                const double fx = (double)dx, fy = (double)dy;
                const double v = (double)g[0] * ((1.0 - fx) * (1.0 - fy)) + (double)g[1] * (fx * (1.0 - fy)) +
                                 (double)g[cw] * ((1.0 - fx) * fy) + (double)g[cw + 1] * (fx * fy);
                const double sv = sgn * v;
                c[l] = sv > 0.0 ? sv : 0.0;
                S += c[l];
            }
            const bool keep_row = !(S > 0.0);
            float best = 0.0f;
#pragma unroll
            for (int l = 0; l < kSegMaxClusters; ++l) {
                if (l >= L) continue;
                const float v = keep_row ? probs[(int64_t)l * n + base + k] : (float)(c[l] / S);
                row[l][k] = v;
                if (l == 0 || v > best) {
                    best = v;
                    lab[k] = l;
                }
            }
        }
#pragma unroll
        for (int l = 0; l < kSegMaxClusters; ++l) {
            if (l >= L) break;
            seg_store(probs_out + (int64_t)l * n, base, cnt, ovec && cnt == 4, row[l]);
        }
        seg_store(labels, base, cnt, lvec && cnt == 4, lab);
    }
}

}  // namespace evk

// =============================================================================================================
// C ABI
// =============================================================================================================
using namespace evk;

// These entries take the linear flow (model id 0) beside the four parametric models.
constexpr bool kTakesLinvel = true;

// host_params: L rows of the model's nparams values
static SegArgs seg_args(int model, const double *hp, int L) {
    SegArgs a = {};
    const int k = with_model<kTakesLinvel>(model, [](auto m) { return Model<decltype(m)::value>::nparams; });
    for (int l = 0; l < L; ++l) a.w[l] = warp_args(model, hp + l * k);
    return a;
}

static bool seg_dword_ok(const void *p) { return !((uintptr_t)p & 3u); }

// a (L, n) array of dwords is read / written 16 bytes at a time when every row starts on a 16-byte boundary
static bool seg_rows16(const void *p, int L, int64_t n) { return aligned16(p) && (L == 1 || (n & 3) == 0); }

// what every entry refuses: the shared head of the argument lists
template <typename T>
static int seg_check(int model, const T *x, const T *y, const T *t, const T *p, int64_t n, const double *host_params, int L,
                     const float *probs, int ch, int cw, uint32_t flags) {
    if (!model_dims<kTakesLinvel>(model) || !host_params || n < 0 || L < 1 || L > kSegMaxClusters || ch <= 1 || cw <= 1 ||
        (flags & ~(EVK_SEG_POLARITY | EVK_IWE_DIRECT)) || (n > 0 && (!x || !y || !t || !p || !probs)))
        return EVK_EINVAL;
    if (n > 0 && (!columns_elem_aligned(x, y, t, p) || !seg_dword_ok(probs))) return EVK_EALIGN;
    return EVK_OK;
}

// Band geometry (lds_band_rows): evk_tsimg_band_rows' constants with L planes in place of its four.
extern "C" int evk_seg_band_rows(int L, uint32_t flags, int canvas_h, int canvas_w) {
    return lds_band_rows(L <= kSegMaxClusters ? L : 0, sizeof(acc64_t), 24, flags, canvas_h, canvas_w);
}

extern "C" int64_t evk_seg_grad_scratch_bytes(void) {
    return (int64_t)kSegMaxClusters * kSegGatherBlocks * kMaxDims * (int64_t)sizeof(double);
}

template <typename T, int M, bool VEC>
static void seg_launch_splat(const T *x, const T *y, const T *t, const T *p, int64_t n, const SegArgs &a, int L,
                             const float *probs, bool pvec, bool signedq, double t_ref, double bw, double bh, int ch, int cw,
                             int band_rows, acc64_t *acc, hipStream_t s) {
    if (band_rows > 0) {
        const int bands = (ch + band_rows - 1) / band_rows;
        const auto [chunk, chunks] = chunk_plan(n, bands);
        const size_t lds = (size_t)L * band_rows * cw * sizeof(acc64_t);
        (void)hipFuncSetAttribute((const void *)k_seg_band<T, M, VEC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kBandLds);
        k_seg_band<T, M, VEC><<<dim3((unsigned)chunks, bands), kBandThreads, lds, s>>>(x, y, t, p, n, chunk, a, L, probs, pvec,
                                                                                       signedq, t_ref, bw, bh, ch, cw, band_rows, acc);
    } else {
        k_seg_direct<T, M, VEC><<<stream_grid(n, 4), EVK_BLOCK, 0, s>>>(x, y, t, p, n, a, L, probs, pvec, signedq, t_ref, bw, bh, ch,
                                                                        cw, acc);
    }
}

template <typename T>
static int seg_splat(int model, const T *x, const T *y, const T *t, const T *p, int64_t n, double t_ref, const double *host_params,
                     int L, const float *probs, double bw, double bh, int ch, int cw, uint32_t flags, uint64_t *accL, float *outL,
                     void *stream) {
    const int rc = seg_check(model, x, y, t, p, n, host_params, L, probs, ch, cw, flags);
    if (rc != EVK_OK) return rc;
    if (!accL || !outL) return EVK_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    acc64_t *acc = reinterpret_cast<acc64_t *>(accL);
    if (n > 0) {
        const SegArgs a = seg_args(model, host_params, L);
        const bool vec = aligned16(x) && aligned16(y) && aligned16(t) && aligned16(p), pvec = seg_rows16(probs, L, n);
        const bool signedq = (flags & EVK_SEG_POLARITY) != 0;
        const int rows = evk_seg_band_rows(L, flags, ch, cw);
        with_model<kTakesLinvel>(model, [&](auto m) {
            constexpr int M = decltype(m)::value;
            if (vec) seg_launch_splat<T, M, true>(x, y, t, p, n, a, L, probs, pvec, signedq, t_ref, bw, bh, ch, cw, rows, acc, s);
            else seg_launch_splat<T, M, false>(x, y, t, p, n, a, L, probs, pvec, signedq, t_ref, bw, bh, ch, cw, rows, acc, s);
            return 1;
        });
    }
    const int64_t elems = (int64_t)L * ch * cw;
    k_seg_planes<<<stream_grid(elems), EVK_BLOCK, 0, s>>>(acc, elems, outL);
    return launch_status();
}

extern "C" int evk_seg_splat_f32(int model, const float *x, const float *y, const float *t, const float *p, int64_t n,
                                 double t_ref, const double *host_params, int L, const float *probs, double bounds_w,
                                 double bounds_h, int canvas_h, int canvas_w, uint32_t flags, uint64_t *accL, float *outL,
                                 void *stream) {
    return seg_splat<float>(model, x, y, t, p, n, t_ref, host_params, L, probs, bounds_w, bounds_h, canvas_h, canvas_w, flags, accL,
                            outL, stream);
}

extern "C" int evk_seg_splat_f64(int model, const double *x, const double *y, const double *t, const double *p, int64_t n,
                                 double t_ref, const double *host_params, int L, const float *probs, double bounds_w,
                                 double bounds_h, int canvas_h, int canvas_w, uint32_t flags, uint64_t *accL, float *outL,
                                 void *stream) {
    return seg_splat<double>(model, x, y, t, p, n, t_ref, host_params, L, probs, bounds_w, bounds_h, canvas_h, canvas_w, flags, accL,
                             outL, stream);
}

template <typename T>
static int seg_grad(int model, const T *x, const T *y, const T *t, const T *p, int64_t n, double t_ref, const double *host_params,
                    int L, const float *probs, double bw, double bh, int ch, int cw, uint32_t flags, const float *adjL, double *out,
                    void *scratch, int64_t scratch_bytes, void *stream) {
    const int rc = seg_check(model, x, y, t, p, n, host_params, L, probs, ch, cw, flags);
    if (rc != EVK_OK) return rc;
    if (!adjL || !out || !scratch) return EVK_EINVAL;
    if (scratch_bytes < evk_seg_grad_scratch_bytes()) return EVK_ESCRATCH;
    hipStream_t s = (hipStream_t)stream;
    const int dims = model_dims<kTakesLinvel>(model);
    int grid = 0;
    if (n > 0) {
        const SegArgs a = seg_args(model, host_params, L);
        const bool vec = aligned16(x) && aligned16(y) && aligned16(t) && aligned16(p), pvec = seg_rows16(probs, L, n);
        const bool signedq = (flags & EVK_SEG_POLARITY) != 0;
        grid = stream_grid(n, 4);  // a function of n alone: the order of the sums, and with it the result, is repeatable
        if (grid > kSegGatherBlocks) grid = kSegGatherBlocks;
        const dim3 g((unsigned)grid, (unsigned)L);
        with_model<kTakesLinvel>(model, [&](auto m) {
            constexpr int M = decltype(m)::value;
            if (vec) k_seg_gather<T, M, true><<<g, EVK_BLOCK, 0, s>>>(x, y, t, p, n, a, probs, pvec, signedq, t_ref, bw, bh, ch, cw,
                                                                    adjL, (double *)scratch);
            else k_seg_gather<T, M, false><<<g, EVK_BLOCK, 0, s>>>(x, y, t, p, n, a, probs, pvec, signedq, t_ref, bw, bh, ch, cw, adjL,
                                                                  (double *)scratch);
            return 1;
        });
    }
    k_seg_final<<<L, EVK_BLOCK, 0, s>>>((const double *)scratch, grid, dims, out);  // n == 0: no partials, zeros
    return launch_status();
}

extern "C" int evk_seg_grad_f32(int model, const float *x, const float *y, const float *t, const float *p, int64_t n, double t_ref,
                                const double *host_params, int L, const float *probs, double bounds_w, double bounds_h,
                                int canvas_h, int canvas_w, uint32_t flags, const float *adjL, double *out, void *scratch,
                                int64_t scratch_bytes, void *stream) {
    return seg_grad<float>(model, x, y, t, p, n, t_ref, host_params, L, probs, bounds_w, bounds_h, canvas_h, canvas_w, flags, adjL,
                           out, scratch, scratch_bytes, stream);
}

extern "C" int evk_seg_grad_f64(int model, const double *x, const double *y, const double *t, const double *p, int64_t n,
                                double t_ref, const double *host_params, int L, const float *probs, double bounds_w,
                                double bounds_h, int canvas_h, int canvas_w, uint32_t flags, const float *adjL, double *out,
                                void *scratch, int64_t scratch_bytes, void *stream) {
    return seg_grad<double>(model, x, y, t, p, n, t_ref, host_params, L, probs, bounds_w, bounds_h, canvas_h, canvas_w, flags, adjL,
                            out, scratch, scratch_bytes, stream);
}

template <typename T>
static int seg_assign(int model, const T *x, const T *y, const T *t, const T *p, int64_t n, double t_ref,
                      const double *host_params, int L, const float *probs, double bw, double bh, int ch, int cw, uint32_t flags,
                      const float *blurredL, float *probs_out, int32_t *labels, void *stream) {
    const int rc = seg_check(model, x, y, t, p, n, host_params, L, probs, ch, cw, flags);
    if (rc != EVK_OK) return rc;
    if (!blurredL || (n > 0 && (!probs_out || !labels || probs_out == probs))) return EVK_EINVAL;
    if (n == 0) return EVK_OK;
    if (!seg_dword_ok(probs_out) || !seg_dword_ok(labels)) return EVK_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    const SegArgs a = seg_args(model, host_params, L);
    const bool vec = aligned16(x) && aligned16(y) && aligned16(t) && aligned16(p);
    const bool ovec = seg_rows16(probs_out, L, n), lvec = aligned16(labels), signedq = (flags & EVK_SEG_POLARITY) != 0;
    const int grid = stream_grid(n, 4);
    with_model<kTakesLinvel>(model, [&](auto m) {
        constexpr int M = decltype(m)::value;
        if (vec) k_seg_assign<T, M, true><<<grid, EVK_BLOCK, 0, s>>>(x, y, t, p, n, a, L, probs, ovec, lvec, signedq, t_ref, bw, bh, ch,
                                                                   cw, blurredL, probs_out, labels);
        else k_seg_assign<T, M, false><<<grid, EVK_BLOCK, 0, s>>>(x, y, t, p, n, a, L, probs, ovec, lvec, signedq, t_ref, bw, bh, ch,
                                                                 cw, blurredL, probs_out, labels);
        return 1;
    });
    return launch_status();
}

extern "C" int evk_seg_assign_f32(int model, const float *x, const float *y, const float *t, const float *p, int64_t n,
                                  double t_ref, const double *host_params, int L, const float *probs, double bounds_w,
                                  double bounds_h, int canvas_h, int canvas_w, uint32_t flags, const float *blurredL,
                                  float *probs_out, int32_t *labels, void *stream) {
    return seg_assign<float>(model, x, y, t, p, n, t_ref, host_params, L, probs, bounds_w, bounds_h, canvas_h, canvas_w, flags,
                             blurredL, probs_out, labels, stream);
}

extern "C" int evk_seg_assign_f64(int model, const double *x, const double *y, const double *t, const double *p, int64_t n,
                                  double t_ref, const double *host_params, int L, const float *probs, double bounds_w,
                                  double bounds_h, int canvas_h, int canvas_w, uint32_t flags, const float *blurredL,
                                  float *probs_out, int32_t *labels, void *stream) {
    return seg_assign<double>(model, x, y, t, p, n, t_ref, host_params, L, probs, bounds_w, bounds_h, canvas_h, canvas_w, flags,
                              blurredL, probs_out, labels, stream);
}
