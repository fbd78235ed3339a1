// The device work of lib/data_loaders/ (base_dataset.py): the voxel grids of a table of event windows in one launch, the
// RobustNorm transform (data_augmentation.py:92-146) for a batch of items, and the (N, 4) event rows of return_events.
//
// Windows.  One workgroup per (window, tile), where a tile is a run of VOXWIN_LDS_BYTES / (4 C) consecutive pixels of the
// row-major H x W plane and C = B (combined) or 2B (split) channels.  The workgroup streams its window's events (from L2:
// every tile of a window reads the same events), keeps those whose pixel falls in its tile, accumulates their bin weights in
// LDS and stores the tile of all C channels once, zeros included: every output cell is written exactly once, with no memset
// and no global atomics.  The events are read one per lane with per-element loads, so a window may start at any event of
// the resident stream (the 4-event groups of evk_part.h's SrcNative need group-aligned starts).
//
// RobustNorm.  One workgroup per item: a radix select of both ranks on order-preserving keys (3 passes of 11/11/10-bit digits,
// two LDS histograms per pass, each lane's run of equal digits counted in a register), min / max of the item in the first
// pass; then a launch of many workgroups per item writes the normalised items.
#include "evk_common.h"

namespace evk {

// ---- windows ---------------------------------------------------------------------------------------------------------------

constexpr int VOXWIN_LDS_BYTES = 40 * 1024;   // 4 workgroups per CU (160 KiB of LDS)
constexpr int VOXWIN_BLOCK = 256;

struct WinSrc {
    const void *x, *y;   // EVK_SELECT_I16: int16, EVK_SELECT_F32: float32; xy_stride 2 = one interleaved (N, 2) array in x
    const void *t;       // EVK_T_F64 / EVK_T_F32
    const void *p;       // EVK_P_U8_PM1 / EVK_P_U8 / EVK_P_I8 (one byte), EVK_P_F32
    int xy_kind, xy_stride, t_kind, p_kind;

    __device__ __forceinline__ void xy(int64_t i, float &fx, float &fy, int &ix, int &iy, bool &finite) const {
        if (xy_kind == EVK_SELECT_I16) {
            const int16_t *a = static_cast<const int16_t *>(x), *b = static_cast<const int16_t *>(y);
            ix = xy_stride == 2 ? a[2 * i] : a[i];
            iy = xy_stride == 2 ? a[2 * i + 1] : b[i];
            fx = (float)ix, fy = (float)iy, finite = true;
        } else {
            const float *a = static_cast<const float *>(x), *b = static_cast<const float *>(y);
            fx = xy_stride == 2 ? a[2 * i] : a[i];
            fy = xy_stride == 2 ? a[2 * i + 1] : b[i];
            // .long(): truncation toward zero (saturating; NaN is rejected explicitly, torch gives INT64_MIN -> IndexError)
            ix = (int)fx, iy = (int)fy, finite = (fx == fx) & (fy == fy);
        }
    }
    __device__ __forceinline__ double t64(int64_t i) const {
        return t_kind == EVK_T_F64 ? static_cast<const double *>(t)[i] : (double)static_cast<const float *>(t)[i];
    }
    __device__ __forceinline__ float pv(int64_t i) const {
        if (p_kind == EVK_P_F32) return static_cast<const float *>(p)[i];
        const uint8_t b = static_cast<const uint8_t *>(p)[i];
        return p_kind == EVK_P_U8_PM1 ? (float)(2 * (int)b - 1) : (p_kind == EVK_P_I8 ? (float)(int8_t)b : (float)b);
    }
};

// torch.max(zeros, v): NaN propagates (fmaxf would drop it)
__device__ __forceinline__ float max0_nan(float v) { return v != v ? v : fmaxf(0.0f, v); }

__global__ __launch_bounds__(VOXWIN_BLOCK) void k_voxel_windows(WinSrc src, const int64_t *__restrict__ win, int B, int h,
                                                                int wd, int split, int tile_px, int vec4, float *__restrict__ vox,
                                                                uint32_t *oob) {
    extern __shared__ float acc[];                  // [C][tile_px]
    const int C = split ? 2 * B : B;
    const int64_t hw = (int64_t)h * wd;
    const int w = blockIdx.y;
    const int64_t c0 = (int64_t)blockIdx.x * tile_px;
    const int64_t a = win[2 * w], b = win[2 * w + 1];
    for (int j = threadIdx.x; j < C * tile_px; j += VOXWIN_BLOCK) acc[j] = 0.0f;
    // time of the window, normalised against its own first event: t_i = (float)(ts[i] - ts[a]) with the subtraction in
    // float64 (base_dataset.py:306 / widen_native_events); dt = t_last - t_first in float32 (voxel_grid.py:133).  An empty
    // window is one zero event (base_dataset.py:218-223): t = 0, dt = 0.
    const bool empty = b <= a;
    const double ta = empty ? 0.0 : src.t64(a);
    const float dt = empty ? 0.0f : (float)(src.t64(b - 1) - ta) - 0.0f;
    const float bm1 = (float)(B - 1);
    __syncthreads();
    const int64_t n = empty ? 1 : b - a;
    for (int64_t k = threadIdx.x; k < n; k += VOXWIN_BLOCK) {
        const int64_t i = a + k;
        float fx = 0.0f, fy = 0.0f;
        int ix = 0, iy = 0;
        bool finite = true;
        if (!empty) src.xy(i, fx, fy, ix, iy, finite);
        ix += ix < 0 ? wd : 0;                      // index_put_: a negative index wraps once
        iy += iy < 0 ? h : 0;
        const bool ok = finite & ((unsigned)ix < (unsigned)wd) & ((unsigned)iy < (unsigned)h);
        if (!ok) {
            if (blockIdx.x == 0) count_oob(oob);    // (counted by one tile of the window)
            continue;
        }
        const int64_t cell = (int64_t)iy * wd + ix - c0;
        if (cell < 0 || cell >= tile_px) continue;
        const float t = empty ? 0.0f : (float)(src.t64(i) - ta);
        const float p = empty ? 0.0f : src.pv(i);
        const float tn = (t - 0.0f) / dt * bm1;     // voxel_grid.py:134, t_first = 0 (evk_part.h time_norm)
        // split: channels [0, B) weight ps > 0, [B, 2B) weight ps <= 0 (voxel_grid.py:172-175, base_dataset.py:453)
        const float wp = split ? (p > 0.0f ? 1.0f : 0.0f) : p;
        const float wn = (p <= 0.0f) ? 1.0f : 0.0f;
        for (int bi = 0; bi < B; ++bi) {
            const float bil = max0_nan(1.0f - fabsf(tn - (float)bi));
            // adding +-0 to a cell changes nothing (a cell starts at +0 and a sum of floats is never -0): skip it
            const float v = wp * bil;
            if (v != 0.0f) atomicAdd(&acc[bi * tile_px + cell], v);
            if (split) {
                const float u = wn * bil;
                if (u != 0.0f) atomicAdd(&acc[(B + bi) * tile_px + cell], u);
            }
        }
    }
    __syncthreads();
    const int64_t len = hw - c0 < tile_px ? hw - c0 : tile_px;
    float *dst = vox + (int64_t)w * C * hw + c0;
    if (vec4) {                                     // hw, tile_px and c0 are multiples of 4, vox is 16-byte aligned
        const int q = (int)(len >> 2);
        for (int j = threadIdx.x; j < C * q; j += VOXWIN_BLOCK) {
            const int c = j / q, r = j - c * q;
            const float *s = acc + c * tile_px + 4 * r;
            reinterpret_cast<float4 *>(dst + c * hw)[r] = make_float4(s[0], s[1], s[2], s[3]);
        }
    } else {
        for (int j = threadIdx.x; j < C * (int)len; j += VOXWIN_BLOCK) {
            const int c = j / (int)len, r = j - c * (int)len;
            dst[c * hw + r] = acc[c * tile_px + r];
        }
    }
}

__global__ __launch_bounds__(VOXWIN_BLOCK) void k_pack_window_events(WinSrc src, const int64_t *__restrict__ win,
                                                                     const int64_t *__restrict__ rows, float *__restrict__ out) {
    const int w = blockIdx.x;
    const int64_t a = win[2 * w], b = win[2 * w + 1];
    if (b <= a) return;
    const double ta = src.t64(a);
    float4 *o = reinterpret_cast<float4 *>(out) + rows[w];
    for (int64_t k = threadIdx.x; k < b - a; k += VOXWIN_BLOCK) {
        float fx, fy;
        int ix, iy;
        bool finite;
        src.xy(a + k, fx, fy, ix, iy, finite);
        o[k] = make_float4(fx, fy, (float)(src.t64(a + k) - ta), src.pv(a + k));
    }
}

static int make_src(WinSrc &s, const void *x, const void *y, int xy_kind, int xy_stride, const void *t, int t_kind, const void *p,
                    int p_kind) {
    if (!x || !t || !p || (xy_kind != EVK_SELECT_I16 && xy_kind != EVK_SELECT_F32) || (xy_stride != 1 && xy_stride != 2) ||
        (xy_stride == 1 && !y) || (t_kind != EVK_T_F32 && t_kind != EVK_T_F64) ||
        (p_kind != EVK_P_U8_PM1 && p_kind != EVK_P_U8 && p_kind != EVK_P_I8 && p_kind != EVK_P_F32))
        return EVK_EINVAL;
    s = WinSrc{x, y, t, p, xy_kind, xy_stride, t_kind, p_kind};
    return EVK_OK;
}

// ---- RobustNorm ------------------------------------------------------------------------------------------------------------

constexpr int RN_BLOCK = 1024;
constexpr int RN_BINS = 2048;                      // 11-bit digits: bits 31..21, 20..10, 9..0
constexpr int RN_APPLY_BLOCK = 256;
constexpr int RN_MAX_ELEMS = 0x7FFFFFFF - 4 * RN_BLOCK;   // element loops step by RN_BLOCK in int

// order-preserving key of torch.kthvalue's order: -0.0 and 0.0 tie, every NaN sorts last
__device__ __forceinline__ uint32_t rn_key(float v) {
    if (v != v) return 0xFFFFFFFFu;
    uint32_t u = __float_as_uint(v == 0.0f ? 0.0f : v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rn_value(uint32_t k) {
    if (k == 0xFFFFFFFFu) return __uint_as_float(0x7FC00000u);
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

struct RnItem {
    int64_t item_stride, s0, s1, s2;
    int d0, d1, d2, contig;                         // contig: element j of an item is at j
    __device__ __forceinline__ int64_t off(int j) const {
        if (contig) return j;
        const int row = j / d2, col = j - row * d2;
        const int r0 = row / d1, r1 = row - r0 * d1;
        return r0 * s0 + r1 * s1 + col * s2;
    }
};

// f(v) for every element of the item this thread visits: 16-byte loads where the item is contiguous and aligned
template <typename F>
__device__ __forceinline__ void rn_for_each(const float *xi, const RnItem &it, int m, F &&f) {
    if (it.contig && (reinterpret_cast<uintptr_t>(xi) & 15u) == 0) {
        const int m4 = m >> 2;
        const float4 *q = reinterpret_cast<const float4 *>(xi);
        for (int j = threadIdx.x; j < m4; j += RN_BLOCK) {
            const float4 v = q[j];
            f(v.x), f(v.y), f(v.z), f(v.w);
        }
        for (int j = 4 * m4 + threadIdx.x; j < m; j += RN_BLOCK) f(xi[j]);
    } else {
        for (int j = threadIdx.x; j < m; j += RN_BLOCK) f(xi[it.off(j)]);
    }
}

// A lane's run of equal digits is counted in a register and added to the LDS histogram once, when the digit changes.  A
// voxel grid is mostly zeros -- one key -- and counting every element with its own LDS atomic made every lane of every wave
// add to the same histogram word, serialised: 2.4 ms per batched launch of 432 k-element items.
struct RnRun {
    uint32_t d = 0xFFFFFFFFu, c = 0;
    __device__ __forceinline__ void add(uint32_t dig, uint32_t *h) {
        if (dig == d) {
            ++c;
        } else {
            if (c) atomicAdd(&h[d], c);
            d = dig, c = 1;
        }
    }
    __device__ __forceinline__ void flush(uint32_t *h) {
        if (c) atomicAdd(&h[d], c);
    }
};

// workgroup-wide exclusive scan of one value per thread (RN_BLOCK threads)
__device__ __forceinline__ uint32_t rn_scan(uint32_t v, uint32_t *wsum) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(s, d, 64);
        if (lane >= d) s += o;
    }
    if (lane == 63) wsum[wv] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (int k = 0; k < RN_BLOCK / 64; ++k) {
            const uint32_t q = wsum[k];
            wsum[k] = run;
            run += q;
        }
    }
    __syncthreads();
    const uint32_t r = wsum[wv] + s - v;
    __syncthreads();
    return r;
}

// One workgroup per item: both ranks' values and the min / max of the clamped item -> stats[4i .. 4i+3] =
// {t_min, t_max, min(c), max(c)} (NaN where torch's min / max would give NaN).
__global__ __launch_bounds__(RN_BLOCK) void k_robust_select(const float *__restrict__ x, RnItem it, uint32_t k_lo, uint32_t k_hi,
                                                            float *__restrict__ stats) {
    __shared__ uint32_t hist[2][RN_BINS];
    __shared__ uint32_t wsum[RN_BLOCK / 64];
    __shared__ uint32_t sel[4];                      // prefix lo, prefix hi, remaining rank lo, remaining rank hi
    __shared__ float red[3][RN_BLOCK / 64];
    const int m = it.d0 * it.d1 * it.d2;
    const float *xi = x + (int64_t)blockIdx.x * it.item_stride;
    if (threadIdx.x == 0) sel[0] = 0, sel[1] = 0, sel[2] = k_lo, sel[3] = k_hi;
    float mn = __builtin_inff(), mx = -__builtin_inff(), nan = 0.0f;
    for (int pass = 0; pass < 3; ++pass) {
        const int sh = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
        const uint32_t bins = pass == 2 ? 1024u : 2048u;
        const uint32_t hi_mask = pass == 0 ? 0u : (pass == 1 ? 0xFFE00000u : 0xFFFFFC00u);
        for (int j = threadIdx.x; j < 2 * RN_BINS; j += RN_BLOCK) (&hist[0][0])[j] = 0;
        __syncthreads();
        const uint32_t pl = sel[0], ph = sel[1];
        RnRun rl, rh;
        rn_for_each(xi, it, m, [&](float v) {
            if (pass == 0) {
                if (v != v) nan = v;
                mn = fminf(mn, v), mx = fmaxf(mx, v);
            }
            const uint32_t k = rn_key(v), d = (k >> sh) & (bins - 1);
            if ((k & hi_mask) == pl) rl.add(d, hist[0]);
            if ((k & hi_mask) == ph) rh.add(d, hist[1]);
        });
        rl.flush(hist[0]);
        rh.flush(hist[1]);
        __syncthreads();
        // each thread owns two consecutive bins; find the digit in which each remaining rank falls
        for (int r = 0; r < 2; ++r) {
            const uint32_t b0 = 2 * threadIdx.x;
            const uint32_t h0 = b0 < bins ? hist[r][b0] : 0, h1 = b0 + 1 < bins ? hist[r][b0 + 1] : 0;
            const uint32_t before = rn_scan(h0 + h1, wsum);
            const uint32_t want = sel[2 + r];       // 1-based rank among the keys matching the prefix
            __syncthreads();
            if (want > before && want <= before + h0 + h1) {
                const bool first = want <= before + h0;
                const uint32_t d = first ? b0 : b0 + 1;
                sel[r] = (r == 0 ? pl : ph) | (d << sh);
                sel[2 + r] = want - before - (first ? 0 : h0);
            }
            __syncthreads();
        }
    }
    // min / max of the item (NaN propagates: torch.min / torch.max)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int d = 32; d >= 1; d >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, d, 64));
        mx = fmaxf(mx, __shfl_xor(mx, d, 64));
        const float o = __shfl_xor(nan, d, 64);
        nan = o != o ? o : nan;
    }
    if (lane == 0) red[0][wv] = mn, red[1][wv] = mx, red[2][wv] = nan;
    __syncthreads();
    if (threadIdx.x != 0) return;
    bool any_nan = false;
    for (int k = 0; k < RN_BLOCK / 64; ++k) {
        mn = fminf(mn, red[0][k]), mx = fmaxf(mx, red[1][k]);
        any_nan |= red[2][k] != red[2][k];
    }
    const float t_min = rn_value(sel[0]), t_max = rn_value(sel[1]);
    // clamp is monotone: the min and max of the clamped item are the clamped min and max of the item
    const bool nan_out = any_nan | (t_min != t_min) | (t_max != t_max);
    const float qnan = __uint_as_float(0x7FC00000u);
    float *st = stats + 4 * (int64_t)blockIdx.x;
    st[0] = t_min, st[1] = t_max;
    st[2] = nan_out ? qnan : fminf(fmaxf(mn, t_min), t_max);
    st[3] = nan_out ? qnan : fminf(fmaxf(mx, t_min), t_max);
}

// (clamp(x, t_min, t_max) - min(c)) / (max(c) + 1e-6) over every element (many workgroups per item); an item whose two
// percentiles are 0 is copied unchanged (data_augmentation.py:138-139).  NaN in x or in a bound propagates; t_min > t_max
// clamps to t_max, as torch.clamp.
__global__ __launch_bounds__(RN_APPLY_BLOCK) void k_robust_apply(const float *__restrict__ x, RnItem it, int blocks_per_item,
                                                                 const float *__restrict__ stats, float *__restrict__ out) {
    const int64_t i = blockIdx.x / blocks_per_item;
    const int part = blockIdx.x - (int)i * blocks_per_item;
    const int m = it.d0 * it.d1 * it.d2;
    const float *xi = x + i * it.item_stride;
    float *o = out + i * m;
    const float t_min = stats[4 * i], t_max = stats[4 * i + 1], cmin = stats[4 * i + 2], den = stats[4 * i + 3] + 1e-6f;
    const bool keep = t_max == 0.0f && t_min == 0.0f;
    const bool bound_nan = (t_min != t_min) | (t_max != t_max);
    const float qnan = __uint_as_float(0x7FC00000u);
    for (int j = part * RN_APPLY_BLOCK + threadIdx.x; j < m; j += blocks_per_item * RN_APPLY_BLOCK) {
        const float v = xi[it.off(j)];
        if (keep) {
            o[j] = v;
        } else {
            const float c = v != v ? v : (bound_nan ? qnan : fminf(fmaxf(v, t_min), t_max));
            o[j] = (c - cmin) / den;
        }
    }
}

}  // namespace evk

using namespace evk;

extern "C" int evk_voxel_windows_f32(const void *x, const void *y, int xy_kind, int xy_stride, const void *t, int t_kind,
                                     const void *p, int p_kind, const int64_t *windows, int nw, int B, int h, int wd, int split,
                                     float *vox, uint32_t *oob, void *stream) {
    WinSrc src;
    if (make_src(src, x, y, xy_kind, xy_stride, t, t_kind, p, p_kind) != EVK_OK || !windows || !vox || nw < 0 || nw > 65535 ||
        B < 1 || h < 1 || wd < 1 || (int64_t)h * wd >= ((int64_t)1 << 31) || (split != 0 && split != 1))
        return EVK_EINVAL;
    const int C = split ? 2 * B : B;
    const int tile_px = (VOXWIN_LDS_BYTES / (4 * C)) & ~3;
    if (tile_px < 4) return EVK_EINVAL;
    if (nw == 0) return EVK_OK;
    const int64_t hw = (int64_t)h * wd;
    const int vec4 = (hw & 3) == 0 && aligned16(vox);
    const dim3 grid((unsigned)((hw + tile_px - 1) / tile_px), (unsigned)nw);
    k_voxel_windows<<<grid, VOXWIN_BLOCK, (size_t)C * tile_px * 4, (hipStream_t)stream>>>(src, windows, B, h, wd, split, tile_px,
                                                                                           vec4, vox, oob);
    return launch_status();
}

extern "C" int evk_pack_window_events_f32(const void *x, const void *y, int xy_kind, int xy_stride, const void *t, int t_kind,
                                          const void *p, int p_kind, const int64_t *windows, const int64_t *row_offsets, int nw,
                                          float *out, void *stream) {
    WinSrc src;
    if (make_src(src, x, y, xy_kind, xy_stride, t, t_kind, p, p_kind) != EVK_OK || !windows || !row_offsets || !out || nw < 0 ||
        !aligned16(out))
        return EVK_EINVAL;
    if (nw == 0) return EVK_OK;
    k_pack_window_events<<<(unsigned)nw, VOXWIN_BLOCK, 0, (hipStream_t)stream>>>(src, windows, row_offsets, out);
    return launch_status();
}

extern "C" int evk_robust_norm_f32(const float *x, int64_t n, int64_t item_stride, int d0, int d1, int d2, int64_t s0, int64_t s1,
                                   int64_t s2, int64_t k_lo, int64_t k_hi, float *out, float *stats, void *stream) {
    const int64_t m = (int64_t)d0 * d1 * d2;
    if (!x || !out || !stats || n < 0 || n > 0x7FFFFFFF || d0 < 1 || d1 < 1 || d2 < 1 || m > RN_MAX_ELEMS || k_lo < 1 ||
        k_lo > m || k_hi < 1 || k_hi > m)
        return EVK_EINVAL;
    if (n == 0) return EVK_OK;
    const int contig = s2 == 1 && s1 == d2 && s0 == (int64_t)d1 * d2;
    const RnItem it{item_stride, s0, s1, s2, d0, d1, d2, contig};
    hipStream_t s = (hipStream_t)stream;
    k_robust_select<<<(unsigned)n, RN_BLOCK, 0, s>>>(x, it, (uint32_t)k_lo, (uint32_t)k_hi, stats);
    // the elementwise pass: ~4 k elements per workgroup, at most ~8 k workgroups in all
    int64_t bpi = (m + 4095) / 4096;
    const int64_t cap = (8192 + n - 1) / n;
    bpi = bpi < cap ? bpi : cap;
    bpi = bpi < 1 ? 1 : bpi;
    if (n * bpi > 0x7FFFFFFF) return EVK_EINVAL;
    k_robust_apply<<<(unsigned)(n * bpi), RN_APPLY_BLOCK, 0, s>>>(x, it, (int)bpi, stats, out);
    return launch_status();
}
