// Spatio-temporal event denoising (include/evk.h, "Event denoising"): the neighbour-support count behind the background-activity
// filter (Delbruck; with a support threshold above 1, Guo & Delbruck's STCF) and the refractory-period filter.  Both are defined
// by a sequential recurrence over a per-pixel timestamp map; what makes them data-parallel is the grouping "all events of one
// pixel, in stream order":
//
//   k_dn_keys        key[i] = class * H*W + y*W + x (32 bits), index[i] = i, pixels off the sensor counted in *oob (key 0)
//   hipCUB           stable radix sort of (key, index) over the key's significant bits -> order[]: indices grouped by key,
//                    ascending inside a key
//   k_dn_runs        start[k] = first position of key k in order[] (lower bound in the sorted keys), k = 0 .. K: empty keys allowed
//   k_dn_support     one thread per event: for every pixel of the clipped window, binary search of that pixel's run for the
//                    predecessor of i, one gathered time, compared in double.  The threads take the events in stream order
//                    (coalesced key and time loads) or in pixel order (neighbouring threads search the same runs)
//   k_dn_refractory  the recurrence "kept iff t - t(last kept) >= refractory" along every run: one thread per short run, a whole
//                    wave per long run (64 consecutive times per load, the chain resolved in registers by ballots)
//
// The kept flags go through evk_select_compact (EVK_SELECT_FLAGS).  Every index a kernel forms comes from a key below K or a
// position below n: a pixel off the sensor gets key 0, so the later passes stay inside their arrays whatever the input holds.
#include <hipcub/hipcub.hpp>

#include "evk_common.h"
#include "evk_group.h"

namespace evk {

constexpr int DN_WAVE_ITEMS = 4;                      // chunks of 64 events a wave keeps in flight on a long run

size_t dn_sort_temp_bytes(int64_t n, int bits) {
    size_t b = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr,
                                             (uint32_t *)nullptr, (int)n, 0, bits);
    return b;
}

__global__ void __launch_bounds__(EVK_BLOCK) k_dn_keys(const int32_t *__restrict__ x, const int32_t *__restrict__ y,
                                                     const uint8_t *__restrict__ cls, int64_t n, int h, int w,
                                                     uint32_t *__restrict__ keys, uint32_t *__restrict__ iota,
                                                     uint32_t *__restrict__ oob) {
    const uint32_t hw = (uint32_t)h * (uint32_t)w;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t xi = x[i], yi = y[i];
        uint32_t k = 0;
        if ((uint32_t)xi < (uint32_t)w && (uint32_t)yi < (uint32_t)h)
            k = ((cls && cls[i]) ? hw : 0u) + (uint32_t)yi * (uint32_t)w + (uint32_t)xi;
        else
            count_oob(oob);
        keys[i] = k;
        iota[i] = (uint32_t)i;
    }
}

// start[k] = number of sorted keys below k: one search per key, so a sparse or a crowded key costs the same
__global__ void __launch_bounds__(EVK_BLOCK) k_dn_runs(const uint32_t *__restrict__ sorted, uint32_t n, int64_t nkeys,
                                                     uint32_t *__restrict__ start) {
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= nkeys; k += (int64_t)gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;       // (n < 2^31: no wrap)
            if (sorted[mid] < (uint32_t)k) lo = mid + 1;
            else hi = mid;
        }
        start[k] = lo;
    }
}

// support[i] = pixels q of the clipped (2R+1)^2 window whose last event before i (stream index, own class when the keys carry
// one) lies within dt: t_i - t_last <= dt in double, a negative difference included.  The pixel's run holds its events' indices
// in ascending order, so the predecessor of i is the element before the lower bound of i.
// BY_PIXEL: thread p takes event order[p] (`keys` = the sorted keys), so that the threads of a wave search the runs of the same
// few pixels -- cache hits where the stream-order walk gathers from all over order[].
template <typename T, int R, bool BY_PIXEL>
__global__ void __launch_bounds__(EVK_BLOCK) k_dn_support(const T *__restrict__ t, const uint32_t *__restrict__ keys,
                                                        const uint32_t *__restrict__ order, const uint32_t *__restrict__ start,
                                                        int64_t n, int h, int w, double dt, int include_self, int min_support,
                                                        uint8_t *__restrict__ support, uint8_t *__restrict__ keep) {
    const uint32_t hw = (uint32_t)h * (uint32_t)w;
    for (int64_t i64 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i64 < n; i64 += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t i = BY_PIXEL ? order[i64] : (uint32_t)i64;
        const uint32_t key = keys[i64];
        const DnPixel px = dn_pixel(key, hw, (uint32_t)w);
        const uint32_t cbase = px.cbase;
        const int y = px.y, x = px.x;
        const double ti = (double)t[i];
        int cnt = 0;
        for (int dy = -R; dy <= R; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= h) continue;
            const uint32_t row = cbase + (uint32_t)yy * (uint32_t)w;
#pragma unroll
            for (int dx = -R; dx <= R; ++dx) {
                const int xx = x + dx;
                if (xx < 0 || xx >= w || (dx == 0 && dy == 0 && !include_self)) continue;
                const uint32_t s = start[row + (uint32_t)xx];
                uint32_t lo = s, hi = start[row + (uint32_t)xx + 1];
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (order[mid] < i) lo = mid + 1;
                    else hi = mid;
                }
                if (lo > s && ti - (double)t[order[lo - 1]] <= dt) ++cnt;
            }
        }
        support[i] = (uint8_t)cnt;
        if (keep) keep[i] = cnt >= min_support ? 1 : 0;
    }
}

// One step of the refractory recurrence on the 64 events a wave holds (lane l: time tv, `valid`): keeps the first event of the
// run, then every event at least `refr` after the last kept one.  last / have: the wave-uniform state carried along the run.
// Each kept event costs one ballot and one broadcast, no memory access.  All 64 lanes are active.  -> the mask of kept lanes
__device__ __forceinline__ uint64_t dn_resolve64(double tv, bool valid, double refr, double &last, bool &have) {
    uint64_t rem = __ballot(valid), km = 0;
    if (!have && rem) {
        km = 1ull;
        last = __shfl(tv, 0, 64);
        rem &= ~1ull;
        have = true;
    }
    while (rem) {
        const uint64_t ok = __ballot(valid && tv - last >= refr) & rem;
        if (!ok) break;
        const int f = __builtin_ctzll(ok);
        km |= 1ull << f;
        last = __shfl(tv, f, 64);
        rem &= ~((2ull << f) - 1ull);                  // (f = 63: 2 << 63 wraps to 0, the mask to all ones)
    }
    return km;
}

// A wave takes 64 consecutive keys.  Lane l walks the run of its key by itself when that run is shorter than wave_run (four
// events loaded ahead of the chain); the longer runs are then walked by the whole wave, one after the other: 64 * DN_WAVE_ITEMS
// consecutive events per step, their indices loaded two steps and their times one step ahead of the chain, which runs in
// registers (dn_resolve64).
template <typename T>
__global__ void __launch_bounds__(EVK_BLOCK) k_dn_refractory(const T *__restrict__ t, const uint32_t *__restrict__ order,
                                                           const uint32_t *__restrict__ start, int64_t nkeys, double refr,
                                                           uint32_t wave_run, uint8_t *__restrict__ keep) {
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (EVK_BLOCK / EVK_WAVE);
    for (int64_t kb = (((int64_t)blockIdx.x * EVK_BLOCK + threadIdx.x) >> 6) * 64; kb < nkeys; kb += nwaves * 64) {
        const int64_t k = kb + lane;
        uint32_t s = 0, e = 0;
        if (k < nkeys) s = start[k], e = start[k + 1];
        const uint32_t len = e - s;
        if (len < wave_run) {
            double last = 0.0;
            bool have = false;
            for (uint32_t pos = s; pos < e; pos += 4) {
                const uint32_t m = e - pos;
                uint32_t j[4];
                double tv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) j[u] = (uint32_t)u < m ? order[pos + u] : 0u;
#pragma unroll
                for (int u = 0; u < 4; ++u) tv[u] = (uint32_t)u < m ? (double)t[j[u]] : 0.0;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if ((uint32_t)u >= m) break;
                    const bool kp = !have || tv[u] - last >= refr;
                    if (kp) last = tv[u], have = true;
                    keep[j[u]] = kp ? 1 : 0;
                }
            }
        }
        uint64_t longs = __ballot(len >= wave_run && len > 0);
        while (longs) {                                // wave-uniform from here on
            const int l = __builtin_ctzll(longs);
            longs &= longs - 1;
            const uint32_t ws = __shfl(s, l, 64), we = __shfl(e, l, 64);
            constexpr uint32_t STEP = 64 * DN_WAVE_ITEMS;
            double last = 0.0;
            bool have = false;
            uint32_t j0[DN_WAVE_ITEMS], j1[DN_WAVE_ITEMS], j2[DN_WAVE_ITEMS];
            double tv0[DN_WAVE_ITEMS], tv1[DN_WAVE_ITEMS];
            // (we < 2^31: positions past the run's end do not wrap)
#pragma unroll
            for (int u = 0; u < DN_WAVE_ITEMS; ++u) {
                const uint32_t p0 = ws + 64u * u + lane, p1 = p0 + STEP;
                j0[u] = p0 < we ? order[p0] : 0u;
                j1[u] = p1 < we ? order[p1] : 0u;
            }
#pragma unroll
            for (int u = 0; u < DN_WAVE_ITEMS; ++u) tv0[u] = ws + 64u * u + lane < we ? (double)t[j0[u]] : 0.0;
            for (uint32_t base = ws; base < we; base += STEP) {
#pragma unroll
                for (int u = 0; u < DN_WAVE_ITEMS; ++u) {
                    const uint32_t p1 = base + STEP + 64u * u + lane, p2 = p1 + STEP;
                    j2[u] = p2 < we ? order[p2] : 0u;
                    tv1[u] = p1 < we ? (double)t[j1[u]] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < DN_WAVE_ITEMS; ++u) {
                    const bool valid = base + 64u * u + lane < we;
                    const uint64_t km = dn_resolve64(tv0[u], valid, refr, last, have);
                    if (valid) keep[j0[u]] = (uint8_t)((km >> lane) & 1ull);
                }
#pragma unroll
                for (int u = 0; u < DN_WAVE_ITEMS; ++u) j0[u] = j1[u], j1[u] = j2[u], tv0[u] = tv1[u];
            }
        }
    }
}

template <typename T, bool BY_PIXEL>
static void dn_support_walk(const T *t, const DnScratch &L, int64_t n, int h, int w, double dt, int radius, int include_self,
                            int min_support, uint8_t *support, uint8_t *keep, hipStream_t s) {
    const int g = stream_grid(n);
    const uint32_t *keys = BY_PIXEL ? L.sorted : L.keys;
    if (radius == 1)
        k_dn_support<T, 1, BY_PIXEL><<<g, EVK_BLOCK, 0, s>>>(t, keys, L.order, L.start, n, h, w, dt, include_self, min_support, support, keep);
    else if (radius == 2)
        k_dn_support<T, 2, BY_PIXEL><<<g, EVK_BLOCK, 0, s>>>(t, keys, L.order, L.start, n, h, w, dt, include_self, min_support, support, keep);
    else
        k_dn_support<T, 3, BY_PIXEL><<<g, EVK_BLOCK, 0, s>>>(t, keys, L.order, L.start, n, h, w, dt, include_self, min_support, support, keep);
}

template <typename T>
static void dn_support_launch(const T *t, const DnScratch &L, int64_t n, int h, int w, double dt, int radius, int include_self,
                              int min_support, int walk, uint8_t *support, uint8_t *keep, hipStream_t s) {
    if (walk == EVK_DENOISE_WALK_STREAM) dn_support_walk<T, false>(t, L, n, h, w, dt, radius, include_self, min_support, support, keep, s);
    else dn_support_walk<T, true>(t, L, n, h, w, dt, radius, include_self, min_support, support, keep, s);
}

template <typename T>
static void dn_refractory_launch(const T *t, const DnScratch &L, int64_t nkeys, double refr, uint32_t wave_run, uint8_t *keep,
                                 hipStream_t s) {
    k_dn_refractory<T><<<stream_grid(nkeys, 4), EVK_BLOCK, 0, s>>>(t, L.order, L.start, nkeys, refr, wave_run, keep);
}

}  // namespace evk

using namespace evk;

extern "C" int64_t evk_denoise_scratch_bytes(int64_t n, int h, int w, int classes) {
    if (!dn_shape_ok(n, h, w, classes)) return EVK_EINVAL;
    return dn_layout(nullptr, n, (int64_t)classes * h * w).total;
}

extern "C" int evk_denoise_group(const int32_t *x, const int32_t *y, const uint8_t *cls, int64_t n, int h, int w, int classes,
                                 void *scratch, int64_t scratch_bytes, uint32_t *oob, void *stream) {
    if ((n > 0 && (!x || !y)) || (classes == 2 && n > 0 && !cls)) return EVK_EINVAL;
    DnScratch L;
    if (const int rc = dn_open(scratch, n, h, w, classes, &L)) return rc;
    const int64_t nkeys = (int64_t)classes * h * w;
    if (scratch_bytes < L.total) return EVK_ESCRATCH;
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) {
        k_dn_keys<<<stream_grid(n), EVK_BLOCK, 0, s>>>(x, y, classes == 2 ? cls : nullptr, n, h, w, L.keys, L.iota, oob);
        size_t tb = (size_t)L.temp_bytes;
        const hipError_t e = hipcub::DeviceRadixSort::SortPairs(L.temp, tb, (const uint32_t *)L.keys, L.sorted,
                                                                (const uint32_t *)L.iota, L.order, (int)n, 0, dn_key_bits(nkeys), s);
        if (e != hipSuccess) return (int)e;
    }
    k_dn_runs<<<stream_grid(nkeys + 1), EVK_BLOCK, 0, s>>>(L.sorted, (uint32_t)n, nkeys, L.start);
    return launch_status();
}

extern "C" int evk_denoise_support(int t_kind, const void *t, int64_t n, int h, int w, int classes, double dt, int radius,
                                   int include_self, int min_support, int walk, void *scratch, uint8_t *support,
                                   uint8_t *keep, void *stream) {
    const int window = (2 * radius + 1) * (2 * radius + 1);
    if ((n > 0 && (!t || !support)) || t_kind < EVK_SELECT_I16 || t_kind > EVK_SELECT_F64 || !(dt >= 0.0) || radius < 1 ||
        radius > EVK_DENOISE_MAX_RADIUS || min_support < 0 || min_support > window || walk < EVK_DENOISE_WALK_DEFAULT ||
        walk > EVK_DENOISE_WALK_PIXEL)
        return EVK_EINVAL;
    DnScratch L;
    if (const int rc = dn_open(scratch, n, h, w, classes, &L)) return rc;
    if (n == 0) return EVK_OK;
    hipStream_t s = (hipStream_t)stream;
    include_self = include_self ? 1 : 0;
    with_time_kind(t_kind, t, [&](auto *tt) {
        dn_support_launch(tt, L, n, h, w, dt, radius, include_self, min_support, walk, support, keep, s);
    });
    return launch_status();
}

extern "C" int evk_denoise_refractory(int t_kind, const void *t, int64_t n, int h, int w, int classes, double refractory,
                                      int wave_run, void *scratch, uint8_t *keep, void *stream) {
    if ((n > 0 && (!t || !keep)) || t_kind < EVK_SELECT_I16 || t_kind > EVK_SELECT_F64 || !(refractory >= 0.0)) return EVK_EINVAL;
    DnScratch L;
    if (const int rc = dn_open(scratch, n, h, w, classes, &L)) return rc;
    if (n == 0) return EVK_OK;
    const int64_t nkeys = (int64_t)classes * h * w;
    const uint32_t wr = wave_run > 0 ? (uint32_t)wave_run : (uint32_t)EVK_DENOISE_WAVE_RUN;
    hipStream_t s = (hipStream_t)stream;
    with_time_kind(t_kind, t, [&](auto *tt) { dn_refractory_launch(tt, L, nkeys, refractory, wr, keep, s); });
    return launch_status();
}
