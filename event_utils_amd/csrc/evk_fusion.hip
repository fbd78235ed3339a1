// Depth fusion (include/evk.h, "Depth fusion"): inverse-depth maps with their variances are carried through rigid motions into one
// target view and everything that lands on a pixel is fused by gated inverse-variance weighting, the map update of ESVO (Zhou et
// al., T-RO 2021, section IV-C) after the inverse-depth filters of LSD-SLAM; then the neighbourhood regularisation both apply.
// A scatter with duplicate destinations is order-dependent; here it is a gather instead, on machinery the library has:
//
//   k_fusion_propagate    one thread per (view, source pixel), the view wave-uniform (blockIdx.y, so that its 17 parameters are
//                         scalar loads from the kernel argument) and consecutive lanes on consecutive pixels: a keep flag and
//                         the four candidate columns (xi, yi, rho', v'), staged in the scratch at the thread's own index
//   evk_select_compact    EVK_SELECT_FLAGS: the four columns compacted in order, which IS the candidate order of the definition
//                         (view ascending, then source pixel row-major); the count comes back in `result`
//   evk_denoise_group     the caller groups the candidates by (xi, yi), classes == 1: order[] holds the candidates of a target
//                         pixel in ascending index, i.e. in candidate order (evk_group.h)
//   k_fusion_fuse         lane = target pixel, a wave takes 64 consecutive pixels and its stores are coalesced.  Two walks over
//                         the pixel's run: the anchor (least v', the earliest on ties), then the gated sums in candidate order
//                         from 0.0.  The order of the sums is the definition, so a run is not split over lanes: a crowded pixel
//                         makes one lane slow and the pixels are not balanced (as the field pass of evk_planeflow.hip)
//   k_fusion_regularise   a 32 x 8 tile of (rho, v, mask) with its halo in LDS, one lane per pixel; a row of the tile is 32
//                         doubles = the 64 banks once, so the half-wave groups of a ds_read_b64 are conflict-free
//
// No atomics and no floating-point reassociation: every result is the same bits from run to run.  Every index a kernel forms is
// bounded: a staged element by views * h * w, a candidate by the pixel test of the propagation (and by evk_denoise_group's own
// check for columns from elsewhere: key 0), a run position by the run table, a tile element by the image test of its load.
#include "evk_common.h"
#include "evk_group.h"

namespace evk {

constexpr int FU_VIEWS = 16;                          // views per launch: their parameters travel as a kernel argument
constexpr int FU_PARAMS = EVK_FUSION_VIEW_PARAMS;     // fx fy cx cy, R row-major, t, process variance
constexpr int FU_TW = 32, FU_TH = 8;                  // the tile of the regularisation: one pixel per thread
static_assert(FU_TW * FU_TH == EVK_BLOCK, "one pixel per thread");

struct FuViews {
    double p[FU_VIEWS][FU_PARAMS];
};
struct FuTarget {
    double fx, fy, cx, cy, w, h;                      // the size as doubles: the pixel test compares doubles
};

// the staging columns of n = views * h * w (view, pixel) pairs, and the scratch of their compaction behind them
struct FuStage {
    uint8_t *keep;
    int32_t *xi, *yi;
    double *rho, *var;
    void *select;
    int64_t select_bytes, total;
};

static FuStage fu_stage(void *scratch, int64_t n) {
    char *sb = static_cast<char *>(scratch);
    FuStage S;
    int64_t off = 0;
    S.keep = reinterpret_cast<uint8_t *>(sb + off), off += dn_al(n);
    S.xi = reinterpret_cast<int32_t *>(sb + off), off += dn_al(4 * n);
    S.yi = reinterpret_cast<int32_t *>(sb + off), off += dn_al(4 * n);
    S.rho = reinterpret_cast<double *>(sb + off), off += dn_al(8 * n);
    S.var = reinterpret_cast<double *>(sb + off), off += dn_al(8 * n);
    S.select = sb + off;
    S.select_bytes = evk_select_scratch_bytes(n);
    S.total = off + dn_al(S.select_bytes);
    return S;
}

// views * h * w candidates at most, grouped on the out_h x out_w plane
static bool fu_shape_ok(int views, int h, int w, int out_h, int out_w) {
    if (views < 1 || h < 1 || w < 1 || out_h < 1 || out_w < 1 || (int64_t)h * w > DN_MAX_N) return false;
    return (int64_t)views * ((int64_t)h * w) <= DN_MAX_N && dn_shape_ok(0, out_h, out_w, 1);
}

__device__ __forceinline__ bool fu_finite(double a) { return __builtin_fabs(a) < __builtin_inf(); }     // (false for NaN)

__global__ void __launch_bounds__(EVK_BLOCK) k_fusion_propagate(const double *__restrict__ rho, const double *__restrict__ var,
                                                              const uint8_t *__restrict__ mask, uint32_t hw, uint32_t w, FuViews V,
                                                              FuTarget T, uint8_t *__restrict__ keep, int32_t *__restrict__ oxi,
                                                              int32_t *__restrict__ oyi, double *__restrict__ orho,
                                                              double *__restrict__ ovar) {
    const double *P = V.p[blockIdx.y];
    const double fx = P[0], fy = P[1], cx = P[2], cy = P[3], pv = P[16];
    const int64_t base = (int64_t)blockIdx.y * hw;
    for (uint32_t pix = blockIdx.x * EVK_BLOCK + threadIdx.x; pix < hw; pix += gridDim.x * EVK_BLOCK) {
        const int64_t i = base + pix;
        const double r = rho[i], v = var[i];
        bool ok = mask[i] != 0 && r > 0.0 && fu_finite(r) && v > 0.0 && fu_finite(v);
        if (ok) {
            const uint32_t y = pix / w, x = pix - y * w;
            const double Z = 1.0 / r, X = (((double)x - cx) / fx) * Z, Y = (((double)y - cy) / fy) * Z;
            const double Xp = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[13];
            const double Yp = ((P[7] * X + P[8] * Y) + P[9] * Z) + P[14];
            const double Zp = ((P[10] * X + P[11] * Y) + P[12] * Z) + P[15];
            const double rp = 1.0 / Zp, u = T.fx * (Xp / Zp) + T.cx, v_ = T.fy * (Yp / Zp) + T.cy;
            const double xf = __builtin_floor(u + 0.5), yf = __builtin_floor(v_ + 0.5);
            const double q = rp / r, q2 = q * q, vp = (q2 * q2) * v + pv;
            ok = Zp > 0.0 && fu_finite(Xp) && fu_finite(Yp) && fu_finite(Zp) && xf >= 0.0 && xf < T.w && yf >= 0.0 && yf < T.h &&
                 fu_finite(vp);
            if (ok) oxi[i] = (int32_t)xf, oyi[i] = (int32_t)yf, orho[i] = rp, ovar[i] = vp;
        }
        keep[i] = ok ? 1 : 0;
    }
}

struct FuGate {
    double gate2, max_variance;
    int min_count;
    bool use_max_variance;
};

__global__ void __launch_bounds__(EVK_BLOCK) k_fusion_fuse(const uint32_t *__restrict__ order, const uint32_t *__restrict__ start,
                                                         int64_t hw, const double *__restrict__ rho,
                                                         const double *__restrict__ var, FuGate G, double *__restrict__ out_rho,
                                                         double *__restrict__ out_var, int32_t *__restrict__ count,
                                                         int32_t *__restrict__ rejected, uint8_t *__restrict__ mask) {
    for (int64_t pix = (int64_t)blockIdx.x * EVK_BLOCK + threadIdx.x; pix < hw; pix += (int64_t)gridDim.x * EVK_BLOCK) {
        const uint32_t s = start[pix], e = start[pix + 1];
        double fr = __builtin_nan(""), fv = __builtin_nan("");
        int32_t c = 0;
        if (e > s) {
            uint32_t a = order[s];
            double va = var[a];
            for (uint32_t p = s + 1; p < e; ++p) {
                const uint32_t i = order[p];
                const double vi = var[i];
                if (vi < va) a = i, va = vi;
            }
            const double ra = rho[a];
            double W = 0.0, S = 0.0;
            for (uint32_t p = s; p < e; ++p) {
                const uint32_t i = order[p];
                const double ri = rho[i], vi = var[i], d = ri - ra;
                if (i == a || d * d <= G.gate2 * (vi + va)) {
                    const double iw = 1.0 / vi;
                    W += iw;
                    S += ri * iw;
                    ++c;
                }
            }
            fr = S / W, fv = 1.0 / W;
        }
        out_rho[pix] = fr, out_var[pix] = fv;
        count[pix] = c, rejected[pix] = (int32_t)(e - s) - c;
        mask[pix] = (c >= G.min_count && (!G.use_max_variance || fv <= G.max_variance)) ? 1 : 0;
    }
}

template <int R>
__global__ void __launch_bounds__(EVK_BLOCK) k_fusion_regularise(const double *__restrict__ rho, const double *__restrict__ var,
                                                               const uint8_t *__restrict__ mask, int h, int w, int tiles_x,
                                                               double gate2, int min_neighbours, double *__restrict__ out_rho,
                                                               uint8_t *__restrict__ out_mask) {
    constexpr int LW = FU_TW + 2 * R, LH = FU_TH + 2 * R;
    __shared__ double s_rho[LH][LW], s_var[LH][LW];
    __shared__ uint8_t s_mask[LH][LW];
    const int ty0 = (int)(blockIdx.x / (uint32_t)tiles_x) * FU_TH, tx0 = (int)(blockIdx.x % (uint32_t)tiles_x) * FU_TW;
    for (int k = threadIdx.x; k < LW * LH; k += EVK_BLOCK) {
        const int ly = k / LW, lx = k - ly * LW, yy = ty0 + ly - R, xx = tx0 + lx - R;
        const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;
        const int64_t g = (int64_t)yy * w + xx;
        s_rho[ly][lx] = in ? rho[g] : 0.0;
        s_var[ly][lx] = in ? var[g] : 0.0;
        s_mask[ly][lx] = in ? mask[g] : (uint8_t)0;
    }
    __syncthreads();
    const int ly = threadIdx.x / FU_TW, lx = threadIdx.x % FU_TW, y = ty0 + ly, x = tx0 + lx;
    if (y >= h || x >= w) return;
    const double rp = s_rho[ly + R][lx + R], vp = s_var[ly + R][lx + R];
    const int64_t g = (int64_t)y * w + x;
    if (!s_mask[ly + R][lx + R]) {
        out_rho[g] = rp, out_mask[g] = 0;
        return;
    }
    double W = 0.0, S = 0.0;
    int n = 0;
#pragma unroll
    for (int dy = 0; dy <= 2 * R; ++dy) {
#pragma unroll
        for (int dx = 0; dx <= 2 * R; ++dx) {
            const double rq = s_rho[ly + dy][lx + dx], vq = s_var[ly + dy][lx + dx], d = rq - rp;
            if (s_mask[ly + dy][lx + dx] && d * d <= gate2 * (vq + vp)) {
                const double iw = 1.0 / vq;
                W += iw;
                S += rq * iw;
                if (dy != R || dx != R) ++n;
            }
        }
    }
    out_rho[g] = S / W;
    out_mask[g] = n >= min_neighbours ? 1 : 0;
}

}  // namespace evk

using namespace evk;

extern "C" int64_t evk_fusion_scratch_bytes(int views, int h, int w, int out_h, int out_w) {
    if (!fu_shape_ok(views, h, w, out_h, out_w)) return EVK_EINVAL;
    const int64_t n = (int64_t)views * h * w;
    const int64_t stage = fu_stage(nullptr, n).total, group = dn_layout(nullptr, n, (int64_t)out_h * out_w).total;
    return stage > group ? stage : group;
}

extern "C" int evk_fusion_propagate(const double *inv_depth, const double *variance, const void *mask, int views, int h, int w,
                                    const double *host_views, int out_h, int out_w, const double *host_target, void *scratch,
                                    int32_t *xi, int32_t *yi, double *out_inv_depth, double *out_variance, int64_t *result,
                                    void *stream) {
    if (!fu_shape_ok(views, h, w, out_h, out_w) || !inv_depth || !variance || !mask || !host_views || !host_target || !scratch || !xi ||
        !yi || !out_inv_depth || !out_variance || !result)
        return EVK_EINVAL;
    for (int64_t k = 0; k < (int64_t)views * FU_PARAMS; ++k)
        if (!(host_views[k] - host_views[k] == 0.0)) return EVK_EINVAL;                 // (NaN and the infinities)
    for (int s = 0; s < views; ++s) {
        const double *P = host_views + (int64_t)s * FU_PARAMS;
        if (!(P[0] > 0.0 && P[1] > 0.0 && P[16] >= 0.0)) return EVK_EINVAL;
    }
    for (int k = 0; k < 4; ++k)
        if (!(host_target[k] - host_target[k] == 0.0) || (k < 2 && !(host_target[k] > 0.0))) return EVK_EINVAL;
    if ((uintptr_t)scratch & 255u) return EVK_EALIGN;
    const int64_t hw = (int64_t)h * w, n = (int64_t)views * hw;
    const FuStage S = fu_stage(scratch, n);
    const FuTarget T = {host_target[0], host_target[1], host_target[2], host_target[3], (double)out_w, (double)out_h};
    hipStream_t s = (hipStream_t)stream;
    const uint8_t *m8 = static_cast<const uint8_t *>(mask);
    for (int v0 = 0; v0 < views; v0 += FU_VIEWS) {
        const int nv = views - v0 < FU_VIEWS ? views - v0 : FU_VIEWS;
        FuViews V = {};
        for (int k = 0; k < nv * FU_PARAMS; ++k) V.p[k / FU_PARAMS][k % FU_PARAMS] = host_views[(int64_t)v0 * FU_PARAMS + k];
        const int64_t o = (int64_t)v0 * hw;
        k_fusion_propagate<<<dim3((unsigned)stream_grid(hw), (unsigned)nv), EVK_BLOCK, 0, s>>>(
            inv_depth + o, variance + o, m8 + o, (uint32_t)hw, (uint32_t)w, V, T, S.keep + o, S.xi + o, S.yi + o, S.rho + o, S.var + o);
    }
    if (const int rc = launch_status()) return rc;
    const void *src[4] = {S.xi, S.yi, S.rho, S.var};
    void *dst[4] = {xi, yi, out_inv_depth, out_variance};
    const int eb[4] = {4, 4, 8, 8};
    return evk_select_compact(EVK_SELECT_FLAGS, EVK_SELECT_I32, nullptr, nullptr, n, nullptr, S.keep, 0, 0, 4, src, dst, eb, -1, nullptr,
                              result, S.select, S.select_bytes, nullptr, stream);
}

extern "C" int evk_fusion_fuse(int64_t m, int out_h, int out_w, const void *scratch, const double *inv_depth, const double *variance,
                               double gate2, int min_count, int use_max_variance, double max_variance, double *out_inv_depth,
                               double *out_variance, int32_t *count, int32_t *rejected, void *mask, void *stream) {
    if (!out_inv_depth || !out_variance || !count || !rejected || !mask || !(gate2 >= 0.0) || min_count < 1 ||
        (use_max_variance != 0 && use_max_variance != 1) || (use_max_variance && max_variance != max_variance) ||
        (m > 0 && (!inv_depth || !variance)))
        return EVK_EINVAL;
    DnScratch L;
    if (const int rc = dn_open(scratch, m, out_h, out_w, 1, &L)) return rc;
    const int64_t hw = (int64_t)out_h * out_w;
    const FuGate G = {gate2, max_variance, min_count, use_max_variance != 0};
    k_fusion_fuse<<<stream_grid(hw), EVK_BLOCK, 0, (hipStream_t)stream>>>(L.order, L.start, hw, inv_depth, variance, G, out_inv_depth,
                                                                        out_variance, count, rejected, static_cast<uint8_t *>(mask));
    return launch_status();
}

extern "C" int evk_fusion_regularise(const double *inv_depth, const double *variance, const void *mask, int h, int w, int radius,
                                     double gate2, int min_neighbours, double *out_inv_depth, void *out_mask, void *stream) {
    if (!inv_depth || !variance || !mask || !out_inv_depth || !out_mask || out_inv_depth == inv_depth || out_mask == mask || h < 1 ||
        w < 1 || (int64_t)h * w > DN_MAX_N || radius < 1 || radius > EVK_FUSION_MAX_RADIUS || !(gate2 >= 0.0) || min_neighbours < 0 ||
        min_neighbours > (2 * radius + 1) * (2 * radius + 1))
        return EVK_EINVAL;
    const int tiles_x = (w + FU_TW - 1) / FU_TW;
    const int64_t tiles = (int64_t)tiles_x * ((h + FU_TH - 1) / FU_TH);
    hipStream_t s = (hipStream_t)stream;
    const uint8_t *m8 = static_cast<const uint8_t *>(mask);
    uint8_t *o8 = static_cast<uint8_t *>(out_mask);
    switch (radius) {
        case 1: k_fusion_regularise<1><<<(unsigned)tiles, EVK_BLOCK, 0, s>>>(inv_depth, variance, m8, h, w, tiles_x, gate2, min_neighbours, out_inv_depth, o8); break;
        case 2: k_fusion_regularise<2><<<(unsigned)tiles, EVK_BLOCK, 0, s>>>(inv_depth, variance, m8, h, w, tiles_x, gate2, min_neighbours, out_inv_depth, o8); break;
        default: k_fusion_regularise<3><<<(unsigned)tiles, EVK_BLOCK, 0, s>>>(inv_depth, variance, m8, h, w, tiles_x, gate2, min_neighbours, out_inv_depth, o8); break;
    }
    return launch_status();
}
