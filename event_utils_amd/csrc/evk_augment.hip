// Event augmentation of lib/augmentation/event_augmentation.py on the device: random events (add_random_events :60-92), jittered
// copies of chosen events (add_correlated_events :118-157) and the sort of a merged block into numpy's order (:85,89,115,156).
// Per-event draws come from Philox4x32-10 (evk_philox.h), key = the call's seed, counter = (index, purpose): independent of the
// launch shape.  The uniform subsets (remove_events, the candidate choice of add_correlated_events) are evk_random_subset +
// evk_select_compact(EVK_SELECT_RANDOM) in evk_select.hip.
#include <hipcub/hipcub.hpp>

#include "evk_common.h"
#include "evk_philox.h"

namespace evk {

// ---- raw generator words -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(EVK_BLOCK) k_philox_words(uint64_t seed, uint32_t purpose, uint64_t offset, int64_t n,
                                                          uint32_t *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const Philox4 r = philox_at(seed, purpose, offset + (uint64_t)i);
        reinterpret_cast<uint4 *>(out)[i] = make_uint4(r.v[0], r.v[1], r.v[2], r.v[3]);
    }
}

// ---- bounds: max(xs), max(ys), min(ts), max(ts) as double, NaN when a column holds one (numpy's max / min) --------------------
constexpr int BOUNDS_BLOCKS = 512;

template <typename T>
__device__ __forceinline__ double col_value(const void *c, int64_t i) {
    return (double)static_cast<const T *>(c)[i];
}

__device__ __forceinline__ double load_kind(int kind, const void *c, int64_t i) {
    switch (kind) {
        case EVK_SELECT_I16: return col_value<int16_t>(c, i);
        case EVK_SELECT_I32: return col_value<int32_t>(c, i);
        case EVK_SELECT_I64: return col_value<int64_t>(c, i);
        case EVK_SELECT_F32: return col_value<float>(c, i);
        default: return col_value<double>(c, i);
    }
}

struct Bounds4 {
    double v[4];   // max x, max y, -min t, max t: all four reduced by max
    uint32_t nan;  // bit k: column k of (x, y, t) holds a NaN
};

__device__ __forceinline__ void bounds_merge(Bounds4 &a, const Bounds4 &b) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a.v[k] = fmax(a.v[k], b.v[k]);
    a.nan |= b.nan;
}

__device__ __forceinline__ Bounds4 bounds_block(Bounds4 b) {
    __shared__ Bounds4 s_b[EVK_BLOCK / EVK_WAVE];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        Bounds4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o.v[k] = __shfl_xor(b.v[k], off, 64);
        o.nan = __shfl_xor(b.nan, off, 64);
        bounds_merge(b, o);
    }
    if ((threadIdx.x & 63) == 0) s_b[threadIdx.x >> 6] = b;
    __syncthreads();
    b = s_b[0];
    for (int w = 1; w < EVK_BLOCK / EVK_WAVE; ++w) bounds_merge(b, s_b[w]);
    return b;
}

__global__ void __launch_bounds__(EVK_BLOCK) k_bounds_partial(int kx, const void *__restrict__ x, int ky, const void *__restrict__ y,
                                                            int kt, const void *__restrict__ t, int64_t n, Bounds4 *__restrict__ part) {
    Bounds4 b;
#pragma unroll
    for (int k = 0; k < 4; ++k) b.v[k] = -__builtin_inf();
    b.nan = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double xv = load_kind(kx, x, i), yv = load_kind(ky, y, i), tv = load_kind(kt, t, i);
        b.nan |= (xv != xv ? 1u : 0u) | (yv != yv ? 2u : 0u) | (tv != tv ? 4u : 0u);
        b.v[0] = fmax(b.v[0], xv);
        b.v[1] = fmax(b.v[1], yv);
        b.v[2] = fmax(b.v[2], -tv);
        b.v[3] = fmax(b.v[3], tv);
    }
    b = bounds_block(b);
    if (threadIdx.x == 0) part[blockIdx.x] = b;
}

__global__ void __launch_bounds__(EVK_BLOCK) k_bounds_final(const Bounds4 *__restrict__ part, int nparts, double *__restrict__ out) {
    Bounds4 b;
#pragma unroll
    for (int k = 0; k < 4; ++k) b.v[k] = -__builtin_inf();
    b.nan = 0;
    for (int i = threadIdx.x; i < nparts; i += EVK_BLOCK) bounds_merge(b, part[i]);
    b = bounds_block(b);
    if (threadIdx.x == 0) {
        const double qnan = __builtin_nan("");
        out[0] = (b.nan & 1u) ? qnan : b.v[0];
        out[1] = (b.nan & 2u) ? qnan : b.v[1];
        out[2] = (b.nan & 4u) ? qnan : -b.v[2];
        out[3] = (b.nan & 4u) ? qnan : b.v[3];
    }
}

// ---- random events (add_random_events :65-68) ---------------------------------------------------------------------------
// x = uniform integer in [0, int(max(xs) + 1)), y likewise (EVK_PHILOX_RANDOM_XY: words 0-1 -> x, 2-3 -> y);
// t = min(ts) + (max(ts) - min(ts)) * (53-bit uniform of words 0-1), p = 2 * (bit 0 of word 2) - 1 (EVK_PHILOX_RANDOM_TP).
// A range that numpy rejects (NaN, <= 0, too large) writes 0: the caller raises numpy's error from the bounds it reads back.
__device__ __forceinline__ uint64_t draw_range(double maxv) {
    const double h = maxv + 1.0;
    return (h >= 1.0 && h < 18446744073709551616.0) ? (uint64_t)h : 0ull;
}

template <typename O>
__global__ void __launch_bounds__(EVK_BLOCK) k_random_events(uint64_t seed, const double *__restrict__ bounds, int64_t m,
                                                           O *__restrict__ ox, O *__restrict__ oy, double *__restrict__ ot,
                                                           O *__restrict__ op) {
    const uint64_t rx = draw_range(bounds[0]), ry = draw_range(bounds[1]);
    const double lo = bounds[2], span = bounds[3] - bounds[2];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x) {
        const Philox4 a = philox_at(seed, EVK_PHILOX_RANDOM_XY, (uint64_t)i);
        const Philox4 b = philox_at(seed, EVK_PHILOX_RANDOM_TP, (uint64_t)i);
        ox[i] = (O)(int64_t)uniform_below(words64(a.v[0], a.v[1]), rx);
        oy[i] = (O)(int64_t)uniform_below(words64(a.v[2], a.v[3]), ry);
        ot[i] = lo + span * unit53(words64(b.v[0], b.v[1]));
        op[i] = (O)(int64_t)((b.v[2] & 1u) ? 1 : -1);
    }
}

// ---- correlated events (add_correlated_events :127-144) -----------------------------------------------------------------
// candidate j of the iters * n jittered copies is (copy, event) = divmod(j, n); its jitter: two Box-Muller normals of
// EVK_PHILOX_CORR_XY for x, y (xy_std * z truncated toward zero, as .astype(int)), one of EVK_PHILOX_CORR_T for t (ts_std * z);
// x, y clipped to [0, max(xs)] / [0, max(ys)] as np.clip does (NaN propagates); p copied.
__device__ __forceinline__ void box_muller(const Philox4 &r, double &z0, double &z1) {
    const double u1 = 1.0 - unit53(words64(r.v[0], r.v[1]));    // (0, 1]
    const double u2 = unit53(words64(r.v[2], r.v[3]));
    const double rad = sqrt(-2.0 * log(u1)), a = 6.283185307179586 * u2;
    z0 = rad * cos(a);
    z1 = rad * sin(a);
}

// np.clip(v, 0, hi) = minimum(maximum(v, 0), hi): a NaN value or bound gives NaN (fmin / fmax would drop it)
__device__ __forceinline__ double np_clip(double v, double hi) {
    if (v != v || hi != hi) return v != v ? v : hi;
    return fmin(fmax(v, 0.0), hi);
}

__global__ void __launch_bounds__(EVK_BLOCK) k_correlated_events(uint64_t seed, const double *__restrict__ x, const double *__restrict__ y,
                                                               const double *__restrict__ t, const double *__restrict__ p, int64_t n,
                                                               const int64_t *__restrict__ sel, int64_t k, double xy_std,
                                                               double ts_std, const double *__restrict__ bounds,
                                                               double *__restrict__ ox, double *__restrict__ oy,
                                                               double *__restrict__ ot, double *__restrict__ op) {
    const double hx = bounds[0], hy = bounds[1];
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < k; q += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = sel[q];
        const int64_t e = j % n;
        double zx, zy, zt, unused;
        box_muller(philox_at(seed, EVK_PHILOX_CORR_XY, (uint64_t)j), zx, zy);
        box_muller(philox_at(seed, EVK_PHILOX_CORR_T, (uint64_t)j), zt, unused);
        const double dx = trunc(xy_std * zx), dy = trunc(xy_std * zy);
        ox[q] = np_clip(x[e] + dx, hx);
        oy[q] = np_clip(y[e] + dy, hy);
        ot[q] = t[e] + ts_std * zt;
        op[q] = p[e];
    }
}

// ---- sort of float64 (x, y, t, p) columns into numpy's order of view('i8,i8,i8,i8').sort(order=['f2']) -----------------
// Order: t, then x, y, p, each by its int64 bit pattern.  A field's sort key is its bits with the sign bit flipped (unsigned
// order = signed order).  LSD over the fields p, y, x, t: each stage is a stable radix sort of (key, permutation) over the bit
// range [lo, hi) in which the field varies (OR of key ^ key[0] over all events, one reduction for the four fields); a field
// that does not vary costs nothing.  The keys are shifted down by lo and sorted from bit 0: hipcub's onesweep path (more than
// a merge sort's worth of events) leaves keys that differ only in bit 63 -- +-1 polarities -- unsorted when asked for the bit
// range [63, 64).  The range is at least 8 bits wide (the bits above hi are the same in every key).  One gather writes the four
// output columns.
constexpr uint64_t SIGN = 0x8000000000000000ull;

__device__ __forceinline__ uint64_t dbits(double v) { return (uint64_t)__double_as_longlong(v); }

__global__ void __launch_bounds__(EVK_BLOCK) k_sort_varying(const double *__restrict__ x, const double *__restrict__ y,
                                                          const double *__restrict__ t, const double *__restrict__ p, int64_t n,
                                                          unsigned long long *__restrict__ mask) {
    const uint64_t r0 = dbits(x[0]), r1 = dbits(y[0]), r2 = dbits(t[0]), r3 = dbits(p[0]);
    uint64_t m0 = 0, m1 = 0, m2 = 0, m3 = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        m0 |= dbits(x[i]) ^ r0;
        m1 |= dbits(y[i]) ^ r1;
        m2 |= dbits(t[i]) ^ r2;
        m3 |= dbits(p[i]) ^ r3;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        m0 |= __shfl_xor(m0, off, 64);
        m1 |= __shfl_xor(m1, off, 64);
        m2 |= __shfl_xor(m2, off, 64);
        m3 |= __shfl_xor(m3, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (m0) atomicOr(&mask[0], (unsigned long long)m0);
        if (m1) atomicOr(&mask[1], (unsigned long long)m1);
        if (m2) atomicOr(&mask[2], (unsigned long long)m2);
        if (m3) atomicOr(&mask[3], (unsigned long long)m3);
    }
}

__global__ void __launch_bounds__(EVK_BLOCK) k_sort_keys(const double *__restrict__ col, const uint32_t *__restrict__ perm, int64_t n,
                                                       int shift, uint64_t *__restrict__ keys) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        keys[i] = (dbits(col[perm ? perm[i] : (uint32_t)i]) ^ SIGN) >> shift;
}

__global__ void __launch_bounds__(EVK_BLOCK) k_sort_iota(uint32_t *__restrict__ perm, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) perm[i] = (uint32_t)i;
}

__global__ void __launch_bounds__(EVK_BLOCK) k_sort_gather(const double *__restrict__ x, const double *__restrict__ y,
                                                         const double *__restrict__ t, const double *__restrict__ p,
                                                         const uint32_t *__restrict__ perm, int64_t n, double *__restrict__ ox,
                                                         double *__restrict__ oy, double *__restrict__ ot, double *__restrict__ op) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t j = perm ? perm[i] : (uint32_t)i;
        ox[i] = x[j];
        oy[i] = y[j];
        ot[i] = t[j];
        op[i] = p[j];
    }
}

static inline int64_t al(int64_t b) { return (b + 255) & ~(int64_t)255; }

static size_t sort_temp_bytes(int64_t n, int begin_bit, int end_bit) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr,
                                             (uint32_t *)nullptr, (int)n, begin_bit, end_bit);
    return b;
}

constexpr int64_t SORT_MAX = 0x7FFFFFFF;   // hipcub's item count is an int

}  // namespace evk

using namespace evk;

extern "C" int evk_philox4x32(uint64_t seed, uint32_t purpose, uint64_t offset, int64_t n, uint32_t *out, void *stream) {
    if (n < 0 || (n > 0 && !out) || ((uintptr_t)out & 15u)) return EVK_EINVAL;
    if (n == 0) return EVK_OK;
    k_philox_words<<<stream_grid(n), EVK_BLOCK, 0, (hipStream_t)stream>>>(seed, purpose, offset, n, out);
    return launch_status();
}

extern "C" int64_t evk_augment_bounds_scratch_bytes(void) { return (int64_t)BOUNDS_BLOCKS * sizeof(Bounds4); }

extern "C" int evk_augment_bounds(int kx, const void *x, int ky, const void *y, int kt, const void *t, int64_t n, double *bounds,
                                  void *scratch, int64_t scratch_bytes, void *stream) {
    for (int k : {kx, ky, kt})
        if (k < EVK_SELECT_I16 || k > EVK_SELECT_F64) return EVK_EINVAL;
    if (n <= 0 || !x || !y || !t || !bounds || !scratch) return EVK_EINVAL;
    if (scratch_bytes < evk_augment_bounds_scratch_bytes()) return EVK_ESCRATCH;
    hipStream_t s = (hipStream_t)stream;
    int blocks = stream_grid(n);
    if (blocks > BOUNDS_BLOCKS) blocks = BOUNDS_BLOCKS;
    Bounds4 *part = static_cast<Bounds4 *>(scratch);
    k_bounds_partial<<<blocks, EVK_BLOCK, 0, s>>>(kx, x, ky, y, kt, t, n, part);
    k_bounds_final<<<1, EVK_BLOCK, 0, s>>>(part, blocks, bounds);
    return launch_status();
}

extern "C" int evk_random_events(uint64_t seed, const double *bounds, int64_t m, int out_kind, void *x, void *y, double *t, void *p,
                                 void *stream) {
    if (m < 0 || !bounds || (out_kind != EVK_SELECT_I64 && out_kind != EVK_SELECT_F64) || (m > 0 && (!x || !y || !t || !p)))
        return EVK_EINVAL;
    if (m == 0) return EVK_OK;
    hipStream_t s = (hipStream_t)stream;
    const int g = stream_grid(m);
    if (out_kind == EVK_SELECT_I64)
        k_random_events<int64_t><<<g, EVK_BLOCK, 0, s>>>(seed, bounds, m, (int64_t *)x, (int64_t *)y, t, (int64_t *)p);
    else
        k_random_events<double><<<g, EVK_BLOCK, 0, s>>>(seed, bounds, m, (double *)x, (double *)y, t, (double *)p);
    return launch_status();
}

extern "C" int evk_correlated_events(uint64_t seed, const double *x, const double *y, const double *t, const double *p, int64_t n,
                                     const int64_t *sel, int64_t k, double xy_std, double ts_std, const double *bounds, double *ox,
                                     double *oy, double *ot, double *op, void *stream) {
    if (n <= 0 || k < 0 || !bounds || !x || !y || !t || !p || (k > 0 && (!sel || !ox || !oy || !ot || !op))) return EVK_EINVAL;
    if (k == 0) return EVK_OK;
    k_correlated_events<<<stream_grid(k), EVK_BLOCK, 0, (hipStream_t)stream>>>(seed, x, y, t, p, n, sel, k, xy_std, ts_std, bounds,
                                                                               ox, oy, ot, op);
    return launch_status();
}

extern "C" int64_t evk_sort_events_scratch_bytes(int64_t n) {
    if (n < 0 || n > SORT_MAX) return EVK_EINVAL;
    return 256 + 2 * al(8 * n) + 2 * al(4 * n) + al((int64_t)sort_temp_bytes(n, 0, 64));
}

extern "C" int evk_sort_events_f64(const double *x, const double *y, const double *t, const double *p, int64_t n, double *ox,
                                   double *oy, double *ot, double *op, void *scratch, int64_t scratch_bytes, int *host_bits,
                                   void *stream) {
    if (n < 0 || n > SORT_MAX || (n > 0 && (!x || !y || !t || !p || !ox || !oy || !ot || !op || !scratch)) ||
        ((uintptr_t)scratch & 255u))
        return EVK_EINVAL;
    if (scratch_bytes < evk_sort_events_scratch_bytes(n)) return EVK_ESCRATCH;
    if (host_bits) *host_bits = 0;
    if (n == 0) return EVK_OK;
    hipStream_t s = (hipStream_t)stream;
    char *sb = static_cast<char *>(scratch);
    unsigned long long *mask = reinterpret_cast<unsigned long long *>(sb);
    uint64_t *keys[2] = {reinterpret_cast<uint64_t *>(sb + 256), reinterpret_cast<uint64_t *>(sb + 256 + al(8 * n))};
    uint32_t *perm[2] = {reinterpret_cast<uint32_t *>(sb + 256 + 2 * al(8 * n)),
                         reinterpret_cast<uint32_t *>(sb + 256 + 2 * al(8 * n) + al(4 * n))};
    void *temp = sb + 256 + 2 * al(8 * n) + 2 * al(4 * n);
    const size_t temp_avail = (size_t)(scratch_bytes - (256 + 2 * al(8 * n) + 2 * al(4 * n)));
    const int g = stream_grid(n);
    hipError_t e = hipMemsetAsync(mask, 0, 4 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return (int)e;
    k_sort_varying<<<g, EVK_BLOCK, 0, s>>>(x, y, t, p, n, mask);
    unsigned long long m[4];
    e = hipMemcpyAsync(m, mask, sizeof(m), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return (int)e;
    const double *cols[4] = {x, y, t, p};
    const int order[4] = {3, 1, 0, 2};                 // least significant field first: p, y, x, t
    int cur = -1, bits = 0;                            // perm[cur] holds the permutation so far (-1: identity)
    for (int f : order) {
        if (!m[f]) continue;
        const int lo = __builtin_ctzll(m[f]), hi = 64 - __builtin_clzll(m[f]);
        const int width = hi - lo < 8 ? (64 - lo < 8 ? 64 - lo : 8) : hi - lo;
        k_sort_keys<<<g, EVK_BLOCK, 0, s>>>(cols[f], cur < 0 ? nullptr : perm[cur], n, lo, keys[0]);
        if (cur < 0) {
            k_sort_iota<<<g, EVK_BLOCK, 0, s>>>(perm[0], n);
            cur = 0;
        }
        size_t tb = sort_temp_bytes(n, 0, width);
        if (tb > temp_avail) return EVK_ESCRATCH;
        e = hipcub::DeviceRadixSort::SortPairs(temp, tb, keys[0], keys[1], perm[cur], perm[cur ^ 1], (int)n, 0, width, s);
        if (e != hipSuccess) return (int)e;
        cur ^= 1;
        bits += hi - lo;
    }
    if (host_bits) *host_bits = bits;
    k_sort_gather<<<g, EVK_BLOCK, 0, s>>>(x, y, t, p, cur < 0 ? nullptr : perm[cur], n, ox, oy, ot, op);
    return launch_status();
}
